// Host checks of the reversed tick's block order (csrc/zigzag_map.hpp zz_block): for every grid size 1 .. 300 the map is a
// bijection, its own inverse, keeps b % 8, starts at the last block of each class and descends within a class.
#include <cstdio>
#include <vector>

#include "../../target_estimation_amd/csrc/zigzag_map.hpp"

using namespace te;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (n = %u, b = %u)\n", __FILE__, __LINE__, #c, n, b); ++failures; } } while (0)

static_assert(ZZ_CLASSES == 8, "one class per XCD");
static_assert(zz_block(0, 1) == 0 && zz_block(0, 9) == 8 && zz_block(1, 9) == 1 && zz_block(8, 9) == 0, "usable in constant expressions");

int main() {
  for (unsigned n = 1; n <= 300; ++n) {
    std::vector<int> hit(n, 0);
    unsigned b = 0;
    for (b = 0; b < n; ++b) {
      const unsigned t = zz_block(b, n);
      CHECK(t < n);
      if (t >= n) continue;
      ++hit[t];
      CHECK(zz_block(t, n) == b);   // its own inverse
      CHECK(t % 8 == b % 8);        // a tile stays in its class
      if (b < 8) {                  // the walk starts where the forward walk ended: the largest member of each class
        CHECK(t + 8 >= n);
        unsigned largest = b;
        while (largest + 8 < n) largest += 8;
        CHECK(t == largest);
      }
      if (b + 8 < n) CHECK(zz_block(b + 8, n) + 8 == t);   // within a class the images descend, member by member
    }
    for (b = 0; b < n; ++b) CHECK(hit[b] == 1);   // a bijection of [0, n)
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("zigzag map host test ok\n");
  return 0;
}

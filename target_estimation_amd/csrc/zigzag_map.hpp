// The order of a reversed dense tick (zig-zag: StepArgs::reverse, PopulationArgs::reverse_blocks).
//
// Workgroups are observed to be dealt round-robin over the 8 XCDs, each with an L2 of its own, and plain stores leave
// their lines in the storing XCD's L2.  A plain mirror b -> n - 1 - b moves a tile from class b % 8 to class
// (n - 1 - b) % 8, for most tiles another XCD: what the forward tick wrote last sits in the wrong L2 when the backward
// tick starts.  zz_block mirrors INSIDE each residue class mod 8 instead: the walk
// still starts where the previous tick ended (blocks 0 .. 7 map to the last block of each class), at a granularity of
// 8 blocks, and every tile keeps its class.  Placement is not a contract: the map is a bijection of [0, n) for every
// n, so every tile is stepped exactly once wherever the dispatcher puts its block, and results never depend on it.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TE_ZZ_HD __host__ __device__
#else
#define TE_ZZ_HD
#endif

namespace te {

constexpr unsigned ZZ_CLASSES = 8;   // XCDs of an MI355X

// Block b of a grid of n blocks (b < n) -> the block whose work it does in a reversed tick.  Its own inverse; keeps b % 8.
TE_ZZ_HD constexpr unsigned zz_block(unsigned b, unsigned n) {
  const unsigned r = b % ZZ_CLASSES;
  const unsigned k = (n - r + ZZ_CLASSES - 1) / ZZ_CLASSES;   // blocks of class r (>= 1, since r <= b < n)
  return r + ZZ_CLASSES * (k - 1 - b / ZZ_CLASSES);
}

}  // namespace te

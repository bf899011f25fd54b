// quartic_cases_host.cpp -- te_quartic.hpp compiled for the host, run over a file of quartics (tests/test_quartic_cases.py and
// tests/golden/make_quartic_cases.py).  Test code.
//   quartic_cases_host IN OUT    IN: n x 5 doubles, c[0] .. c[4] (lowest order first);  OUT: n x 2 doubles:
//   quartic_sturm_classify of the quartic with its leading coefficient made positive (-1 if that coefficient is zero), and
//   first_crossing_quartic
#define TE_QUARTIC_HOST
#include "../../target_estimation_amd/csrc/te_quartic.hpp"

#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  std::vector<double> c;
  double row[5];
  while (fread(row, sizeof(double), 5, in) == 5) c.insert(c.end(), row, row + 5);
  fclose(in);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  for (size_t i = 0; i < c.size() / 5; ++i) {
    const double* q = &c[5 * i];
    double res[2] = {-1.0, te::first_crossing_quartic(q)};
    if (std::fabs(q[4]) > 0.0) {
      double cc[5];
      for (int k = 0; k < 5; ++k) cc[k] = q[4] < 0 ? -q[k] : q[k];
      res[0] = (double)te::quartic_sturm_classify(cc);
    }
    fwrite(res, sizeof(double), 2, out);
  }
  fclose(out);
  return 0;
}

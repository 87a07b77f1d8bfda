// det_ppnd16 (ipmc_rng.hpp) on the host, stand-alone: prints "p z" for a grid
// of p in [1e-10, 1 - 1e-10] with 17 significant digits
// (tests/test_rank_cpu.py compares the values with scipy.special.ndtri).
//   g++ -O2 -std=c++17 -ffp-contract=off ipmc_ppnd16_check.cpp -o ppnd16_check
// g++ only, no HIP; it can be built with -fsanitize=address,undefined as host-asan is.
#include <cstdio>

#include "ipmc_rng.hpp"

int main() {
  int n = 0;
  // both tails, decade by decade, with three points inside each decade
  for (int e = -10; e <= -1; ++e) {
    double d = 1.0;
    for (int i = e; i < 0; ++i) d = d / 10.0;
    const double m[3] = {1.0, 2.5, 6.0};
    for (int j = 0; j < 3; ++j) {
      const double p = m[j] * d;
      if (p >= 0.5) continue;
      std::printf("%.17g %.17g\n", p, ipmc::det_ppnd16(p));
      std::printf("%.17g %.17g\n", 1.0 - p, ipmc::det_ppnd16(1.0 - p));
      n += 2;
    }
  }
  // the central rational function, its edges |p - 0.5| = 0.425, and both sides of the
  // r = 5 switch (p = exp(-25) = 1.39e-11, below what a rank of S < 2^32 samples reaches)
  for (int i = 1; i < 400; ++i) {
    const double p = (double)i / 400.0;
    std::printf("%.17g %.17g\n", p, ipmc::det_ppnd16(p));
    ++n;
  }
  const double edges[8] = {0.075, 0.925, 0.0749999999, 0.9250000001, 1.4e-11, 1.0 - 1.4e-11, 1e-12, 1e-15};
  for (int j = 0; j < 8; ++j) {
    std::printf("%.17g %.17g\n", edges[j], ipmc::det_ppnd16(edges[j]));
    ++n;
  }
  return n > 0 ? 0 : 1;
}

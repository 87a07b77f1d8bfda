// det_exp (ipmc_exp.hpp) on the host, stand-alone: prints "x det_exp(x)" with
// 17 significant digits (tests/test_smc_cpu.py compares the values with
// numpy's long double exp):
//   a dense grid of [-708, 0], both sides of every multiple of ln 2 (and of
//   ln 2 / 2, where the reduced argument changes sign) up to 1 022 of them,
//   -708 and one ulp to either side, tiny arguments down to -2^-60, 0 and -0.
//   g++ -O2 -std=c++17 -ffp-contract=off ipmc_exp_check.cpp -o exp_check
// g++ only, no HIP; it can be built with -fsanitize=address,undefined as host-asan is.
#include <cmath>
#include <cstdio>

#include "ipmc_exp.hpp"

static int n_out = 0;

static void row(double x) {
  std::printf("%.17g %.17g\n", x, ipmc::det_exp(x));
  ++n_out;
}

int main() {
  for (int i = 0; i <= 70800; ++i) row(-(double)i / 100.0);
  for (int i = 1; i < 4000; ++i) row(-(double)i / 4000.0 * 0.7);  // the first two reduction intervals, finer
  const double ln2 = 0x1.62e42fefa39efp-1;
  for (int m = 1; m <= 2 * 1022; ++m) {
    const double x = -(double)m * (ln2 * 0.5);  // even m: a multiple of ln 2; odd m: the rounding switches
    if (x < -709.0) break;
    row(x);
    row(std::nextafter(x, 0.0));
    row(std::nextafter(x, -1000.0));
  }
  row(-708.0);
  row(std::nextafter(-708.0, 0.0));
  row(std::nextafter(-708.0, -1000.0));
  row(-709.0);
  row(-745.0);
  row(-1e300);
  for (int e = 1; e <= 60; ++e) row(-std::ldexp(1.0, -e));
  row(0.0);
  row(-0.0);
  return n_out > 0 ? 0 : 1;
}

// det_exp: exp(x) for x <= 0, the importance weight of tempered SMC
// (ipmc_smc.hip, ipmc_host.cpp).  Like det_log / det_ppnd16 of
// ipmc_rng.hpp it is built from + - * and a float -> int conversion in a fixed
// order, and both compilers run with -ffp-contract=off, so libipmc.so and
// libipmc_host.so give the same bits.  It lives in a header of its own: the
// sweep units include ipmc_rng.hpp and must not be rebuilt differently
// because of a function they do not call.
//
//   x == 0 (also -0.0)   1 exactly
//   x < -708             0 exactly (exp(-708) = 3.3e-308 is still a normal
//                        double: no subnormal scaling anywhere)
//   NaN, x > 0           NaN
//   else                 x = n ln2 + r, |r| <= ln2 / 2 (n = x / ln2 rounded,
//                        ln2 split as in det_log so that n * ln2_hi is exact),
//                        exp(r) = 1 + (r + r^2 (1/2 + r (1/6 + ... r / 14!)))
//                        (truncation below 4e-19), times 2^n built from its
//                        exponent bits (exact)
// Relative error against expl at most 2^-50 (measured: ipmc_exp_check.cpp,
// tests/test_smc_cpu.py).
#pragma once

#include <stdint.h>

#ifndef IPMC_HD
#ifdef __HIP__
#define IPMC_HD __host__ __device__ __forceinline__
#else
#define IPMC_HD inline __attribute__((always_inline))
#endif
#endif

namespace ipmc {

IPMC_HD double det_exp(double x) {
  if (x == 0.0) return 1.0;
  if (x < -708.0) return 0.0;
  if (!(x < 0.0)) return __builtin_nan("");  // NaN, and x > 0 (outside the contract): a visible NaN
  const double t = x * 0x1.71547652b82fep+0;  // x / ln 2
  const int n = (int)(t - 0.5);               // t < 0: the conversion truncates towards zero = t rounded
  const double dn = (double)n;
  const double r = (x - dn * 0x1.62e42fee00000p-1) - dn * 0x1.a39ef35793c76p-33;
  double q = 0x1.93974a8c07c9dp-37;  // 1/14!
  q = q * r + 0x1.6124613a86d09p-33;
  q = q * r + 0x1.1eed8eff8d898p-29;
  q = q * r + 0x1.ae64567f544e4p-26;
  q = q * r + 0x1.27e4fb7789f5cp-22;
  q = q * r + 0x1.71de3a556c734p-19;
  q = q * r + 0x1.a01a01a01a01ap-16;
  q = q * r + 0x1.a01a01a01a01ap-13;
  q = q * r + 0x1.6c16c16c16c17p-10;
  q = q * r + 0x1.1111111111111p-7;
  q = q * r + 0x1.5555555555555p-5;
  q = q * r + 0x1.5555555555555p-3;
  q = q * r + 0.5;
  const double e = 1.0 + (r + (r * r) * q);
  // 2^n, n in [-1022, 0]: a normal double from its exponent field
  const double scale = __builtin_bit_cast(double, (uint64_t)(n + 1023) << 52);
  return e * scale;
}

// The weight of a particle with potential phi for the temperature increment
// delta >= 0: det_exp(-(delta * (phi - phi_ref))), 0 for a potential that is
// not finite (an invalid forward map).
IPMC_HD double smc_weight(double phi, double phi_ref, double delta) {
  if (!(__builtin_fabs(phi) < __builtin_inf())) return 0.0;
  return det_exp(-(delta * (phi - phi_ref)));
}

// The ancestor of an offspring at position p of systematic resampling over the
// cumulative weights cum[0 .. n), total = cum[n - 1] finite and > 0: the
// smallest c with cum[c] > p, or, where p >= total by rounding, the first c
// that holds the total (the last at which cum rises).  mid < n always.
// libipmc_host.so calls it; ancestors_kernel (ipmc_smc.hip) keeps the same
// search written out (profiles/r16), and test_ancestors_equal_the_host_twin
// holds the two together.
IPMC_HD int64_t smc_ancestor(double p, const double* cum, int64_t n, double total) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (cum[mid] > p) hi = mid; else lo = mid + 1;
  }
  if (lo == n) {
    lo = 0, hi = n - 1;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (cum[mid] >= total) hi = mid; else lo = mid + 1;
    }
  }
  return lo;
}

}  // namespace ipmc

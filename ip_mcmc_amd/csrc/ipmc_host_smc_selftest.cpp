// The SMC entry points of include/ipmc_host.h (ipmc_host_temper_sums,
// ipmc_host_temper_cumweights, ipmc_host_systematic_ancestors), stand-alone
// with its own main, for the sanitizers (make host-smc-asan;
// tests/test_smc_cpu.py): sizes around the block edge, f32 and f64, potentials
// that are not finite, every error return.  Each result is checked against a
// plain restatement of its definition.  Prints "host smc selftest ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/ipmc.h"
#include "../../include/ipmc_host.h"
#include "ipmc_exp.hpp"

static int g_fail = 0;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++g_fail;                                                      \
    }                                                                \
  } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// a small LCG: potentials in [0, spread), reproducible
static double next_unit(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(s >> 11) / 9007199254740992.0;
}

template <typename T>
static void one_size(int64_t n, double spread, bool bad, int32_t dtype) {
  uint64_t seed = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
  std::vector<T> phi((size_t)n);
  for (int64_t c = 0; c < n; ++c) phi[(size_t)c] = (T)(3.0 + spread * next_unit(seed));
  if (bad) {
    phi[0] = std::numeric_limits<T>::infinity();
    if (n > 2) phi[(size_t)(n / 2)] = std::numeric_limits<T>::quiet_NaN();
    if (n > 1030) phi[1024] = std::numeric_limits<T>::infinity();
  }
  double ref = std::numeric_limits<double>::infinity();
  for (int64_t c = 0; c < n; ++c)
    if (std::isfinite((double)phi[(size_t)c]) && (double)phi[(size_t)c] < ref) ref = (double)phi[(size_t)c];
  const bool any = std::isfinite(ref);
  if (!any) ref = 0.0;

  const int nd = 5;
  const double deltas[nd] = {0.0, 1e-3, 0.25, 1.0, 7.5};
  std::vector<double> s1(nd, -1.0), s2(nd, -1.0);
  CHECK(ipmc_host_temper_sums(phi.data(), dtype, n, ref, deltas, nd, s1.data(), s2.data()) == IPMC_OK);
  for (int j = 0; j < nd; ++j) {
    double t1 = 0.0, t2 = 0.0;
    for (int64_t b0 = 0; b0 < n; b0 += IPMC_SMC_BLOCK) {
      double a1 = 0.0, a2 = 0.0;
      for (int64_t c = b0; c < n && c < b0 + IPMC_SMC_BLOCK; ++c) {
        const double w = ipmc::smc_weight((double)phi[(size_t)c], ref, deltas[j]);
        a1 = a1 + w;
        a2 = a2 + w * w;
      }
      t1 = t1 + a1;
      t2 = t2 + a2;
    }
    CHECK(same_bits(s1[(size_t)j], t1) && same_bits(s2[(size_t)j], t2));
  }
  int64_t finite = 0;
  for (int64_t c = 0; c < n; ++c) finite += std::isfinite((double)phi[(size_t)c]) ? 1 : 0;
  CHECK(s1[0] == (double)finite && s2[0] == (double)finite);  // delta = 0: every valid particle weighs 1

  std::vector<double> cum((size_t)n, -1.0);
  const double delta = 0.25;
  CHECK(ipmc_host_temper_cumweights(phi.data(), dtype, n, ref, delta, cum.data()) == IPMC_OK);
  double offset = 0.0;
  for (int64_t b0 = 0; b0 < n; b0 += IPMC_SMC_BLOCK) {
    double within = 0.0;
    for (int64_t c = b0; c < n && c < b0 + IPMC_SMC_BLOCK; ++c) {
      within = within + ipmc::smc_weight((double)phi[(size_t)c], ref, delta);
      CHECK(same_bits(cum[(size_t)c], offset + within));
    }
    offset = offset + within;
  }
  for (int64_t c = 1; c < n; ++c) CHECK(cum[(size_t)c] >= cum[(size_t)(c - 1)]);
  CHECK(same_bits(cum[(size_t)(n - 1)], s1[2]));  // the total is the sum of the same blocks in the same order

  const int64_t outs[3] = {1, n, 3 * n};
  const double us[3] = {0.0, 0.5, 0.999999};
  for (int64_t n_out : outs)
    for (double u : us) {
      std::vector<int64_t> anc((size_t)n_out, -7);
      CHECK(ipmc_host_systematic_ancestors(cum.data(), n, u, n_out, anc.data()) == IPMC_OK);
      const double total = cum[(size_t)(n - 1)];
      if (!(total > 0.0)) {
        for (int64_t a : anc) CHECK(a == -1);
        continue;
      }
      const double step = total / (double)n_out;
      int64_t prev = 0;
      for (int64_t i = 0; i < n_out; ++i) {
        const int64_t a = anc[(size_t)i];
        CHECK(a >= prev && a < n);
        if (a < 0 || a >= n) break;
        prev = a;
        const double p = ((double)i + u) * step;
        CHECK(cum[(size_t)a] > (a > 0 ? cum[(size_t)(a - 1)] : 0.0));  // a parent has weight
        if (p < total) {
          CHECK(cum[(size_t)a] > p && (a == 0 || cum[(size_t)(a - 1)] <= p));
        } else {
          CHECK(cum[(size_t)a] == total);
        }
      }
    }
}

static void errors() {
  const double phi[4] = {1.0, 2.0, 3.0, 4.0};
  const double d1[1] = {0.5};
  double deltas[65];
  for (double& d : deltas) d = 0.1;
  double s1[65], s2[65], cum[4];
  int64_t anc[4];
  const int INV = IPMC_ERR_INVALID;
  CHECK(ipmc_host_temper_sums(phi, IPMC_F64, -1, 1.0, d1, 1, s1, s2) == INV);
  CHECK(ipmc_host_temper_sums(phi, IPMC_F64, 4, 1.0, d1, -1, s1, s2) == INV);
  CHECK(ipmc_host_temper_sums(phi, IPMC_F64, 4, 1.0, d1, 0, s1, s2) == INV);
  CHECK(ipmc_host_temper_sums(phi, IPMC_F64, 4, 1.0, deltas, 65, s1, s2) == INV);
  CHECK(std::strstr(ipmc_host_last_error(), "outside [1, 64]") != nullptr);
  CHECK(ipmc_host_temper_sums(phi, IPMC_F64, 4, 1.0, deltas, 64, s1, s2) == IPMC_OK);
  CHECK(ipmc_host_temper_sums(phi, 7, 4, 1.0, d1, 1, s1, s2) == INV);
  CHECK(ipmc_host_temper_sums(nullptr, IPMC_F64, 4, 1.0, d1, 1, s1, s2) == INV);
  CHECK(ipmc_host_temper_sums(phi, IPMC_F64, 4, 1.0, nullptr, 1, s1, s2) == INV);
  CHECK(ipmc_host_temper_sums(phi, IPMC_F64, 4, 1.0, d1, 1, nullptr, s2) == INV);
  CHECK(ipmc_host_temper_sums(phi, IPMC_F64, 4, 1.0, d1, 1, s1, nullptr) == INV);
  const double neg[1] = {-0.5}, nan[1] = {std::nan("")};
  CHECK(ipmc_host_temper_sums(phi, IPMC_F64, 4, 1.0, neg, 1, s1, s2) == INV);
  CHECK(ipmc_host_temper_sums(phi, IPMC_F64, 4, 1.0, nan, 1, s1, s2) == INV);
  CHECK(ipmc_host_temper_sums(nullptr, IPMC_F64, 0, 1.0, nullptr, 1, nullptr, nullptr) == IPMC_OK);

  CHECK(ipmc_host_temper_cumweights(phi, IPMC_F64, -1, 1.0, 0.5, cum) == INV);
  CHECK(ipmc_host_temper_cumweights(phi, 7, 4, 1.0, 0.5, cum) == INV);
  CHECK(ipmc_host_temper_cumweights(nullptr, IPMC_F64, 4, 1.0, 0.5, cum) == INV);
  CHECK(ipmc_host_temper_cumweights(phi, IPMC_F64, 4, 1.0, 0.5, nullptr) == INV);
  CHECK(ipmc_host_temper_cumweights(phi, IPMC_F64, 4, 1.0, -0.5, cum) == INV);
  CHECK(ipmc_host_temper_cumweights(phi, IPMC_F64, 4, 1.0, INFINITY, cum) == INV);
  CHECK(ipmc_host_temper_cumweights(nullptr, IPMC_F64, 0, 1.0, 0.5, nullptr) == IPMC_OK);
  CHECK(ipmc_host_temper_cumweights(phi, IPMC_F64, 4, 1.0, 0.5, cum) == IPMC_OK);

  CHECK(ipmc_host_systematic_ancestors(cum, -1, 0.5, 4, anc) == INV);
  CHECK(ipmc_host_systematic_ancestors(cum, 4, 0.5, -4, anc) == INV);
  CHECK(ipmc_host_systematic_ancestors(cum, 4, 1.0, 4, anc) == INV);
  CHECK(ipmc_host_systematic_ancestors(cum, 4, -0.1, 4, anc) == INV);
  CHECK(ipmc_host_systematic_ancestors(cum, 4, std::nan(""), 4, anc) == INV);
  CHECK(ipmc_host_systematic_ancestors(nullptr, 4, 0.5, 4, anc) == INV);
  CHECK(ipmc_host_systematic_ancestors(cum, 4, 0.5, 4, nullptr) == INV);
  CHECK(ipmc_host_systematic_ancestors(nullptr, 0, 0.5, 4, nullptr) == IPMC_OK);
  CHECK(ipmc_host_systematic_ancestors(cum, 4, 0.5, 0, nullptr) == IPMC_OK);
  // a total that is zero, NaN or infinite: no parent
  const double zero[3] = {0.0, 0.0, 0.0}, bad[3] = {1.0, 2.0, std::nan("")}, inf[3] = {1.0, 2.0, INFINITY};
  for (const double* c : {zero, bad, inf}) {
    anc[0] = anc[1] = 5;
    CHECK(ipmc_host_systematic_ancestors(c, 3, 0.5, 2, anc) == IPMC_OK && anc[0] == -1 && anc[1] == -1);
  }
  // one parent holds all the weight
  const double single[5] = {0.0, 0.0, 1.0, 1.0, 1.0};
  CHECK(ipmc_host_systematic_ancestors(single, 5, 0.999, 4, anc) == IPMC_OK);
  for (int i = 0; i < 4; ++i) CHECK(anc[i] == 2);
}

int main() {
  CHECK(ipmc::det_exp(0.0) == 1.0 && ipmc::det_exp(-0.0) == 1.0);
  CHECK(ipmc::det_exp(-708.5) == 0.0 && ipmc::det_exp(-INFINITY) == 0.0 && ipmc::det_exp(-708.0) > 0.0);
  CHECK(std::isnan(ipmc::det_exp(std::nan(""))));
  const int64_t sizes[7] = {1, 2, 1023, 1024, 1025, 2049, 70001};
  for (int64_t n : sizes) {
    one_size<double>(n, 10.0, false, IPMC_F64);
    one_size<float>(n, 10.0, false, IPMC_F32);
    one_size<double>(n, 1e4, true, IPMC_F64);
    one_size<float>(n, 1e4, true, IPMC_F32);
    one_size<double>(n, 0.0, false, IPMC_F64);  // all potentials equal
  }
  {  // no valid particle at all
    const double allbad[3] = {INFINITY, std::nan(""), INFINITY};
    const double d[1] = {0.5};
    double s1 = -1, s2 = -1, cum[3];
    CHECK(ipmc_host_temper_sums(allbad, IPMC_F64, 3, 0.0, d, 1, &s1, &s2) == IPMC_OK && s1 == 0.0 && s2 == 0.0);
    CHECK(ipmc_host_temper_cumweights(allbad, IPMC_F64, 3, 0.0, 0.5, cum) == IPMC_OK && cum[2] == 0.0);
  }
  errors();
  if (g_fail) {
    std::printf("host smc selftest: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("host smc selftest ok\n");
  return 0;
}

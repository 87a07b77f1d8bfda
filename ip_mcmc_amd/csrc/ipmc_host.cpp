// libipmc_host.so: the pCN path's counter-based draws on the host CPU
// (include/ipmc_host.h).  Same source as the device draws (ipmc_rng.hpp), built
// by g++ with -ffp-contract=off, so every value equals libipmc.so's.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../include/ipmc.h"
#include "../../include/ipmc_host.h"
#include "ipmc_checks.hpp"
#include "ipmc_exp.hpp"
#include "ipmc_rng.hpp"

namespace ipmc {

static thread_local char g_err[256] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

}  // namespace ipmc

using namespace ipmc;

namespace {

// below this many elements one thread does the block (config 1's one chain)
constexpr int64_t kParallelMin = int64_t(1) << 16;

// fn(i0, i1) over [0, total) in contiguous slices, one per thread
template <typename F>
void parallel_for(int64_t total, int n_threads, F fn) {
  int nt = n_threads > 0 ? n_threads : (int)std::max(1u, std::thread::hardware_concurrency());
  if (total < kParallelMin) nt = 1;
  nt = (int)std::min<int64_t>(nt, std::max<int64_t>(1, total / 4096));
  if (nt <= 1) {
    fn((int64_t)0, total);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(nt);
  for (int t = 0; t < nt; ++t) {
    const int64_t i0 = total * t / nt, i1 = total * (t + 1) / nt;
    th.emplace_back([=] { fn(i0, i1); });
  }
  for (auto& x : th) x.join();
}

// draws_kernel's element loop (ipmc_api.hip)
template <typename T>
void draws(uint64_t seed, int64_t c_off, int64_t n, uint64_t step0, int64_t total, int k, const T* sq,
           const T* chol, T* w, double* log_r, int n_threads) {
  parallel_for(total, n_threads, [=](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) draws_element<T>(i, seed, c_off, n, step0, k, sq, chol, w, log_r);
  });
}

constexpr int64_t kSmcBlock = IPMC_SMC_BLOCK;

// w_c(delta) of particle c (ipmc_exp.hpp: smc_weight), Φ widened exactly
template <typename T>
inline double weight_of(const T* phi, int64_t c, double phi_ref, double delta) {
  return smc_weight((double)phi[c], phi_ref, delta);
}

template <typename T>
void temper_sums(const T* phi, int64_t n, double phi_ref, const double* deltas, int nd, double* s1, double* s2) {
  for (int j = 0; j < nd; ++j) {
    double t1 = 0.0, t2 = 0.0;  // the block sums from zero in block order
    for (int64_t b0 = 0; b0 < n; b0 += kSmcBlock) {
      const int64_t b1 = std::min(n, b0 + kSmcBlock);
      double a1 = 0.0, a2 = 0.0;  // one block from zero in particle order
      for (int64_t c = b0; c < b1; ++c) {
        const double w = weight_of(phi, c, phi_ref, deltas[j]);
        a1 = a1 + w;
        a2 = a2 + w * w;
      }
      t1 = t1 + a1;
      t2 = t2 + a2;
    }
    s1[j] = t1;
    s2[j] = t2;
  }
}

template <typename T>
void temper_cumweights(const T* phi, int64_t n, double phi_ref, double delta, double* cum) {
  double offset = 0.0;
  for (int64_t b0 = 0; b0 < n; b0 += kSmcBlock) {
    const int64_t b1 = std::min(n, b0 + kSmcBlock);
    double within = 0.0;
    for (int64_t c = b0; c < b1; ++c) {
      within = within + weight_of(phi, c, phi_ref, delta);
      cum[c] = offset + within;
    }
    offset = offset + within;
  }
}

}  // namespace

extern "C" {

int ipmc_host_abi_version(void) { return IPMC_HOST_ABI_VERSION; }

const char* ipmc_host_last_error(void) { return g_err; }

int ipmc_host_pcn_draws(uint64_t seed, int64_t chain_offset, int64_t n_chains, uint64_t step0, int64_t n_steps,
                        int32_t k, int32_t dtype, const void* prior_sqrt, const void* prior_chol, void* w,
                        double* log_r, int32_t n_threads) {
  int64_t total;
  const int rc = check_pcn_draws(chain_offset, n_chains, step0, n_steps, k, dtype, prior_sqrt, prior_chol, w, total);
  if (rc) return rc < 0 ? IPMC_OK : rc;
  if (dtype == IPMC_F64)
    draws<double>(seed, chain_offset, n_chains, step0, total, k, (const double*)prior_sqrt,
                  (const double*)prior_chol, (double*)w, log_r, n_threads);
  else
    draws<float>(seed, chain_offset, n_chains, step0, total, k, (const float*)prior_sqrt, (const float*)prior_chol,
                 (float*)w, log_r, n_threads);
  return IPMC_OK;
}

int ipmc_host_normal(uint64_t seed, int64_t chain_offset, int64_t n_chains, uint64_t step, int32_t k,
                     int32_t dtype, void* out) {
  const int rc = check_normal(chain_offset, n_chains, k, dtype, out);
  if (rc) return rc < 0 ? IPMC_OK : rc;
  const int64_t total = n_chains * k;
  for (int64_t i = 0; i < total; ++i) {
    if (dtype == IPMC_F64)
      ((double*)out)[i] = normal_element<double>(i, seed, chain_offset, step, k);
    else
      ((float*)out)[i] = normal_element<float>(i, seed, chain_offset, step, k);
  }
  return IPMC_OK;
}

int ipmc_host_uniform(uint64_t seed, int64_t chain_offset, int64_t n_chains, uint64_t step, double* out) {
  const int rc = check_uniform(chain_offset, n_chains, out);
  if (rc) return rc < 0 ? IPMC_OK : rc;
  for (int64_t c = 0; c < n_chains; ++c) out[c] = accept_uniform(seed, (uint64_t)(chain_offset + c), step);
  return IPMC_OK;
}

int ipmc_host_step_uniforms(uint64_t seed, int64_t chain, uint64_t step, int32_t n, double* out) {
  if (n < 0 || chain < 0 || chain >= kChainIdLimit) return fail(IPMC_ERR_INVALID, "bad chain id or count");
  if (n > 0x10000) return fail(IPMC_ERR_INVALID, "at most 65536 uniforms per step");
  if (n == 0) return IPMC_OK;
  if (!out) return fail(IPMC_ERR_INVALID, "out is NULL");
  for (int32_t i = 0; i < n; ++i) out[i] = slot_uniform(seed, (uint64_t)chain, step, 0xFFFFFFFFu - (uint32_t)i);
  return IPMC_OK;
}

int ipmc_host_ordered_sum(const double* rows, int64_t n_rows, int64_t k, int64_t row_stride, double div,
                          double* acc) {
  if (n_rows < 0 || k < 0 || row_stride < k) return fail(IPMC_ERR_INVALID, "bad shape");
  if (n_rows == 0 || k == 0) return IPMC_OK;
  if (!rows || !acc) return fail(IPMC_ERR_INVALID, "NULL pointer");
  // one pass over the rows, every column in its own sequential chain (the
  // columns vectorise: each one's additions keep their order), the running
  // sums in a local buffer; div == 1 adds the rows as they are.  Memory-bound:
  // one streaming pass beats round 4's column tiles (a pass over the rows per
  // tile) 2.4x -- 2^18 x 256 values in 0.095 vs 0.228 s on the 8-core build
  // container -- and threads over columns were slower still (each re-reads
  // every row's cache lines).
  std::vector<double> a(acc, acc + k);
  double* __restrict__ ap = a.data();
  const double* __restrict__ x = rows;
  if (div == 1.0) {
    for (int64_t r = 0; r < n_rows; ++r, x += row_stride)
      for (int64_t j = 0; j < k; ++j) ap[j] = ap[j] + x[j];
  } else {
    for (int64_t r = 0; r < n_rows; ++r, x += row_stride)
      for (int64_t j = 0; j < k; ++j) ap[j] = ap[j] + x[j] / div;
  }
  for (int64_t j = 0; j < k; ++j) acc[j] = ap[j];
  return IPMC_OK;
}

int ipmc_host_temper_sums(const void* phi, int32_t dtype, int64_t n, double phi_ref, const double* deltas,
                          int32_t n_deltas, double* s1_out, double* s2_out) {
  const char* fn = "ipmc_host_temper_sums";
  if (n < 0 || n_deltas < 0) return fail(IPMC_ERR_INVALID, "%s: negative size", fn);
  if (n == 0) return IPMC_OK;
  int rc;
  if ((rc = check_n_deltas(fn, n_deltas))) return rc;
  if ((rc = check_dtype(fn, dtype))) return rc;
  if (!phi || !deltas || !s1_out || !s2_out) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  for (int j = 0; j < n_deltas; ++j)
    if ((rc = check_delta(fn, "deltas", j, deltas[j]))) return rc;
  if (dtype == IPMC_F64)
    temper_sums((const double*)phi, n, phi_ref, deltas, n_deltas, s1_out, s2_out);
  else
    temper_sums((const float*)phi, n, phi_ref, deltas, n_deltas, s1_out, s2_out);
  return IPMC_OK;
}

int ipmc_host_temper_cumweights(const void* phi, int32_t dtype, int64_t n, double phi_ref, double delta,
                                double* cum_out) {
  const char* fn = "ipmc_host_temper_cumweights";
  if (n < 0) return fail(IPMC_ERR_INVALID, "%s: negative size", fn);
  if (n == 0) return IPMC_OK;
  int rc;
  if ((rc = check_dtype(fn, dtype))) return rc;
  if (!phi || !cum_out) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  if ((rc = check_delta(fn, "delta", -1, delta))) return rc;
  if (dtype == IPMC_F64)
    temper_cumweights((const double*)phi, n, phi_ref, delta, cum_out);
  else
    temper_cumweights((const float*)phi, n, phi_ref, delta, cum_out);
  return IPMC_OK;
}

int ipmc_host_systematic_ancestors(const double* cum, int64_t n, double u, int64_t n_out, int64_t* anc_out) {
  const int rc = check_ancestors("ipmc_host_systematic_ancestors", cum, n, u, n_out, anc_out);
  if (rc) return rc < 0 ? IPMC_OK : rc;
  const double total = cum[n - 1];
  if (!(total > 0.0) || !(total < __builtin_inf())) {
    for (int64_t i = 0; i < n_out; ++i) anc_out[i] = -1;
    return IPMC_OK;
  }
  const double step = total / (double)n_out;
  for (int64_t i = 0; i < n_out; ++i) anc_out[i] = smc_ancestor(((double)i + u) * step, cum, n, total);
  return IPMC_OK;
}

}  // extern "C"

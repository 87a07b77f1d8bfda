// Argument checks that libipmc.so (ipmc_api.hip, ipmc_smc.hip) and
// libipmc_host.so (ipmc_host.cpp) share: an entry point and its host twin turn
// down the same arguments with the same status and text because both run the
// function below.  Host code only; no HIP header.  Each library defines
// ipmc::fail over its own thread-local message buffer.  `fn` is the entry
// point's name where the message carries one.  What only the device library
// takes (workspace, stream) is checked in its entry points.
#pragma once

#include <stdint.h>

#include "../../include/ipmc.h"

// hidden: a process may load both libraries, and each has to bind its own fail
#pragma GCC visibility push(hidden)
namespace ipmc {

// sets the library's last-error text and returns `code`, so a failed check is one line
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

inline int check_dtype(const char* fn, int32_t dtype) {
  if (dtype == IPMC_F64 || dtype == IPMC_F32) return IPMC_OK;
  return fail(IPMC_ERR_INVALID, "%s: bad dtype", fn);
}

// The Philox counter holds the global chain id in one 32-bit word and the pCN
// step in two (ipmc_rng.hpp); host-side draws (rng.py) use steps from
// kHostStepBase on.  Ids or steps outside these ranges would alias other
// chains' draws, so they are rejected.
constexpr int64_t kChainIdLimit = int64_t(1) << 32;
constexpr uint64_t kHostStepBase = uint64_t(1) << 63;

inline int check_chain_range(int64_t chain_offset, int64_t n_chains) {
  if (n_chains < 0 || chain_offset < 0) return fail(IPMC_ERR_INVALID, "negative count");
  if (chain_offset > kChainIdLimit - n_chains)
    return fail(IPMC_ERR_INVALID, "global chain ids (chain_offset + n_chains) must be <= 2^32");
  return IPMC_OK;
}

// The checks of an entry point below return 0 = go on, -1 = nothing to do
// (the entry point returns IPMC_OK), else the status to return.

// ipmc_pcn_draws / ipmc_host_pcn_draws; total = n_steps * n_chains * k
inline int check_pcn_draws(int64_t chain_offset, int64_t n_chains, uint64_t step0, int64_t n_steps, int32_t k,
                           int32_t dtype, const void* prior_sqrt, const void* prior_chol, const void* w,
                           int64_t& total) {
  if (k <= 0 || n_steps < 0) return fail(IPMC_ERR_INVALID, "k must be positive and n_steps >= 0");
  const int rc = check_chain_range(chain_offset, n_chains);
  if (rc) return rc;
  if (dtype != IPMC_F32 && dtype != IPMC_F64) return fail(IPMC_ERR_INVALID, "bad dtype");
  if (step0 > kHostStepBase || (uint64_t)n_steps > kHostStepBase - step0)
    return fail(IPMC_ERR_INVALID, "pCN steps must stay below 2^63 (the host-draw range)");
  if (n_chains == 0 || n_steps == 0) return -1;
  if (!w) return fail(IPMC_ERR_INVALID, "w is NULL");
  if (!prior_sqrt && !prior_chol) return fail(IPMC_ERR_INVALID, "prior_sqrt and prior_chol are both NULL");
  if (n_chains > INT64_MAX / k / n_steps) return fail(IPMC_ERR_INVALID, "n_steps * n_chains * k overflows");
  total = n_steps * n_chains * k;
  return 0;
}

// ipmc_normal / ipmc_host_normal
inline int check_normal(int64_t chain_offset, int64_t n_chains, int32_t k, int32_t dtype, const void* out) {
  if (k < 0) return fail(IPMC_ERR_INVALID, "negative count");
  const int rc = check_chain_range(chain_offset, n_chains);
  if (rc) return rc;
  if (dtype != IPMC_F32 && dtype != IPMC_F64) return fail(IPMC_ERR_INVALID, "bad dtype");
  if (n_chains * k == 0) return -1;
  if (!out) return fail(IPMC_ERR_INVALID, "out is NULL");
  return 0;
}

// ipmc_uniform / ipmc_host_uniform
inline int check_uniform(int64_t chain_offset, int64_t n_chains, const void* out) {
  const int rc = check_chain_range(chain_offset, n_chains);
  if (rc) return rc;
  if (n_chains == 0) return -1;
  if (!out) return fail(IPMC_ERR_INVALID, "out is NULL");
  return 0;
}

// the number of candidates of ipmc_smc_workspace and ipmc_temper_sums / ipmc_host_temper_sums
inline int check_n_deltas(const char* fn, int32_t n_deltas) {
  if (n_deltas >= 1 && n_deltas <= IPMC_SMC_MAX_DELTAS) return IPMC_OK;
  return fail(IPMC_ERR_INVALID, "%s: n_deltas = %d outside [1, %d]", fn, n_deltas, IPMC_SMC_MAX_DELTAS);
}

// a temperature increment: `name`[j] of the temper_sums pair, `name` (j < 0) of the temper_cumweights pair
inline int check_delta(const char* fn, const char* name, int j, double delta) {
  if (delta >= 0.0 && delta < __builtin_inf()) return IPMC_OK;
  if (j >= 0) return fail(IPMC_ERR_INVALID, "%s: %s[%d] is not a finite number >= 0", fn, name, j);
  return fail(IPMC_ERR_INVALID, "%s: %s is not a finite number >= 0", fn, name);
}

// ipmc_systematic_ancestors / ipmc_host_systematic_ancestors
inline int check_ancestors(const char* fn, const double* cum, int64_t n, double u, int64_t n_out,
                           const int64_t* anc_out) {
  if (n < 0 || n_out < 0) return fail(IPMC_ERR_INVALID, "%s: negative size", fn);
  if (!(u >= 0.0 && u < 1.0)) return fail(IPMC_ERR_INVALID, "%s: u outside [0, 1)", fn);
  if (n == 0 || n_out == 0) return -1;
  if (!cum || !anc_out) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  return 0;
}

}  // namespace ipmc
#pragma GCC visibility pop

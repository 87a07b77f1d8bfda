// Tempered SMC over the ensemble (smc.py): ipmc_smc_workspace,
// ipmc_temper_sums, ipmc_temper_cumweights, ipmc_systematic_ancestors,
// ipmc_gather_rows.
//
// Every floating-point result is defined by a sequential order (ipmc.h), and
// ipmc_host.cpp runs that order in plain loops; the kernels run the same
// additions in the same order and put the parallelism elsewhere:
//
//   temper_sums     a workgroup takes a block of IPMC_SMC_BLOCK particles in
//                   tiles of 64: all lanes evaluate the tile's weights for every
//                   candidate into LDS (det_exp is the cost), then lane j adds
//                   candidate j's 64 weights in particle order to its running
//                   pair of sums.  A second launch adds the blocks' sums in
//                   block order, one lane per candidate.
//   cumweights      all lanes evaluate a block's weights into LDS, lane 0 runs
//                   the block's running sum; a second launch runs the blocks'
//                   totals (staged through LDS), a third adds the offsets.
//   ancestors       one binary search per offspring.
//   gather          a workgroup takes a tile of about 2 048 elements (whole
//                   rows), stages the tile's indices in LDS, and consecutive
//                   lanes copy consecutive elements: rows shorter than a wave
//                   share it, stores are dense, loads are dense inside a row.
//
// No workgroup waits on another; no atomics; nothing depends on the grid.
#include "ipmc_checks.hpp"
#include "ipmc_internal.hpp"
#include "ipmc_exp.hpp"

namespace ipmc {
namespace {

constexpr int kSmcThreads = 256;
constexpr int kSmcBlock = IPMC_SMC_BLOCK;
constexpr int kMaxDeltas = IPMC_SMC_MAX_DELTAS;
constexpr int kSumTile = 64;          // particles whose weights are in LDS at once (temper_sums)
constexpr int kSmcGroups = 1024;      // workgroups of a launch over the blocks, at most
constexpr int kGatherElems = 2048;    // elements of one gather tile, about
constexpr int kGatherGroups = 8192;   // workgroups of the gather, at most

struct Deltas {
  double d[kMaxDeltas];
};

// ------------------------------------------------------------ temper_sums
template <typename T>
__global__ __launch_bounds__(kSmcThreads) void temper_block_sums_kernel(const T* __restrict__ phi, int64_t n,
                                                                       double phi_ref, Deltas dl, int nd,
                                                                       int64_t n_blocks, double* __restrict__ part1,
                                                                       double* __restrict__ part2) {
  __shared__ double sdelta[kMaxDeltas];
  __shared__ double sphi[kSumTile];
  __shared__ double sw[kSumTile * kMaxDeltas];
  const int tid = threadIdx.x;
  if (tid < nd) sdelta[tid] = dl.d[tid];
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int64_t b0 = b * kSmcBlock;
    const int cnt = (n - b0) < kSmcBlock ? (int)(n - b0) : kSmcBlock;
    double a1 = 0.0, a2 = 0.0;  // lane j < nd: candidate j's sums over this block
    for (int t0 = 0; t0 < cnt; t0 += kSumTile) {
      const int tp = (cnt - t0) < kSumTile ? (cnt - t0) : kSumTile;
      __syncthreads();  // the previous tile's weights have been added (and sdelta is written)
      if (tid < tp) sphi[tid] = (double)phi[b0 + t0 + tid];
      __syncthreads();
      for (int e = tid; e < tp * nd; e += kSmcThreads) {
        const int p = e / nd, j = e - p * nd;
        sw[e] = smc_weight(sphi[p], phi_ref, sdelta[j]);
      }
      __syncthreads();
      if (tid < nd) {
        for (int p = 0; p < tp; ++p) {
          const double w = sw[p * nd + tid];
          a1 = a1 + w;
          a2 = a2 + w * w;
        }
      }
    }
    if (tid < nd) {
      part1[b * nd + tid] = a1;
      part2[b * nd + tid] = a2;
    }
  }
}

__global__ __launch_bounds__(kMaxDeltas) void temper_total_kernel(const double* __restrict__ part1,
                                                                 const double* __restrict__ part2, int nd,
                                                                 int64_t n_blocks, double* __restrict__ s1,
                                                                 double* __restrict__ s2) {
  const int j = threadIdx.x;
  if (j >= nd) return;
  double t1 = 0.0, t2 = 0.0;
#pragma unroll 4
  for (int64_t b = 0; b < n_blocks; ++b) {
    t1 = t1 + part1[b * nd + j];
    t2 = t2 + part2[b * nd + j];
  }
  s1[j] = t1;
  s2[j] = t2;
}

// ------------------------------------------------------------- cumweights
template <typename T>
__global__ __launch_bounds__(kSmcThreads) void cum_block_kernel(const T* __restrict__ phi, int64_t n, double phi_ref,
                                                               double delta, int64_t n_blocks,
                                                               double* __restrict__ cum, double* __restrict__ totals) {
  __shared__ double sw[kSmcBlock];
  const int tid = threadIdx.x;
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int64_t b0 = b * kSmcBlock;
    const int cnt = (n - b0) < kSmcBlock ? (int)(n - b0) : kSmcBlock;
    __syncthreads();  // the previous block's running sums have been stored
    for (int j = tid; j < cnt; j += kSmcThreads) sw[j] = smc_weight((double)phi[b0 + j], phi_ref, delta);
    __syncthreads();
    if (tid == 0) {
      double within = 0.0;
      for (int j = 0; j < cnt; ++j) {
        within = within + sw[j];
        sw[j] = within;
      }
      totals[b] = within;
    }
    __syncthreads();
    for (int j = tid; j < cnt; j += kSmcThreads) cum[b0 + j] = sw[j];
  }
}

// offsets[b] = the blocks' totals before b, from zero in block order (one workgroup)
__global__ __launch_bounds__(kSmcThreads) void cum_offsets_kernel(const double* __restrict__ totals, int64_t n_blocks,
                                                                 double* __restrict__ offsets) {
  __shared__ double st[kSmcBlock];
  __shared__ double carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0.0;
  for (int64_t c0 = 0; c0 < n_blocks; c0 += kSmcBlock) {
    const int cnt = (n_blocks - c0) < kSmcBlock ? (int)(n_blocks - c0) : kSmcBlock;
    __syncthreads();
    for (int j = tid; j < cnt; j += kSmcThreads) st[j] = totals[c0 + j];
    __syncthreads();
    if (tid == 0) {
      double off = carry;
      for (int j = 0; j < cnt; ++j) {
        const double t = st[j];
        st[j] = off;
        off = off + t;
      }
      carry = off;
    }
    __syncthreads();
    for (int j = tid; j < cnt; j += kSmcThreads) offsets[c0 + j] = st[j];
  }
}

__global__ __launch_bounds__(kSmcThreads) void cum_add_kernel(double* __restrict__ cum, int64_t n,
                                                             const double* __restrict__ offsets) {
  for (int64_t c = (int64_t)blockIdx.x * kSmcThreads + threadIdx.x; c < n; c += (int64_t)gridDim.x * kSmcThreads)
    cum[c] = offsets[c / kSmcBlock] + cum[c];
}

// -------------------------------------------------------------- ancestors
__global__ __launch_bounds__(kSmcThreads) void ancestors_kernel(const double* __restrict__ cum, int64_t n, double u,
                                                               int64_t n_out, int64_t* __restrict__ anc) {
  const double total = cum[n - 1];
  const bool ok = total > 0.0 && total < __builtin_inf();
  const double step = total / (double)n_out;
  for (int64_t i = (int64_t)blockIdx.x * kSmcThreads + threadIdx.x; i < n_out;
       i += (int64_t)gridDim.x * kSmcThreads) {
    if (!ok) {
      anc[i] = -1;
      continue;
    }
    // Mirrors smc_ancestor (ipmc_exp.hpp), which only the host library calls: the search stays written out
    // here, as at the parent commit, because the kernel that called smc_ancestor missed the timing criterion
    // against the parent (profiles/r16/README.md, "Timing").  Keep the two in step.
    const double p = ((double)i + u) * step;
    int64_t lo = 0, hi = n;  // the smallest c with cum[c] > p; n if there is none.  mid < n always
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (cum[mid] > p) hi = mid; else lo = mid + 1;
    }
    if (lo == n) {  // p >= total by rounding: the first c that holds the total
      lo = 0, hi = n - 1;
      while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (cum[mid] >= total) hi = mid; else lo = mid + 1;
      }
    }
    anc[i] = lo;
  }
}

// ----------------------------------------------------------------- gather
constexpr int kGatherMaxRows = kGatherElems;  // k = 1

template <typename T>
__global__ __launch_bounds__(kSmcThreads) void gather_rows_kernel(const T* __restrict__ src, int64_t n_src, int k,
                                                                 int64_t src_stride, const int64_t* __restrict__ idx,
                                                                 int64_t n_out, T* __restrict__ dst,
                                                                 int64_t dst_stride, int rows_per_tile,
                                                                 int64_t n_tiles) {
  __shared__ int64_t sidx[kGatherMaxRows];
  const int tid = threadIdx.x;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t r0 = tile * rows_per_tile;
    const int tr = (n_out - r0) < rows_per_tile ? (int)(n_out - r0) : rows_per_tile;
    __syncthreads();  // the previous tile's indices are no longer read
    for (int r = tid; r < tr; r += kSmcThreads) {
      const int64_t s = idx[r0 + r];
      sidx[r] = (s >= 0 && s < n_src) ? s : -1;  // an index outside the source: the row is skipped
    }
    __syncthreads();
    const unsigned total = (unsigned)tr * (unsigned)k;
    for (unsigned e = tid; e < total; e += kSmcThreads) {
      const unsigned r = e / (unsigned)k, j = e - r * (unsigned)k;
      const int64_t s = sidx[r];
      if (s >= 0) dst[(r0 + r) * dst_stride + j] = src[s * src_stride + j];
    }
  }
}

int64_t smc_blocks(int64_t n) { return (n + kSmcBlock - 1) / kSmcBlock; }

int64_t smc_workspace_bytes(int64_t n, int32_t n_deltas) { return 2 * smc_blocks(n) * (int64_t)n_deltas * 8; }

int smc_workspace_check(const char* fn, const void* workspace, int64_t have, int64_t need) {
  if (!workspace) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  if (have < need)
    return fail(IPMC_ERR_INVALID, "%s: workspace of %lld bytes, ipmc_smc_workspace asks for %lld", fn, (long long)have,
                (long long)need);
  return 0;
}

unsigned smc_groups(int64_t n_blocks) { return (unsigned)(n_blocks < kSmcGroups ? n_blocks : kSmcGroups); }

}  // namespace
}  // namespace ipmc

using namespace ipmc;

extern "C" int ipmc_smc_workspace(int64_t n, int32_t n_deltas, int64_t* bytes_out) {
  const char* fn = "ipmc_smc_workspace";
  if (n < 0 || n_deltas < 0) return fail(IPMC_ERR_INVALID, "%s: negative size", fn);
  if (const int rc = check_n_deltas(fn, n_deltas)) return rc;
  if (!bytes_out) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  *bytes_out = smc_workspace_bytes(n, n_deltas);
  return IPMC_OK;
}

extern "C" int ipmc_temper_sums(const void* phi, int32_t dtype, int64_t n, double phi_ref, const double* deltas,
                                int32_t n_deltas, double* s1_out, double* s2_out, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  const char* fn = "ipmc_temper_sums";
  if (n < 0 || n_deltas < 0 || workspace_bytes < 0) return fail(IPMC_ERR_INVALID, "%s: negative size", fn);
  if (n == 0) return IPMC_OK;
  int rc;
  if ((rc = check_n_deltas(fn, n_deltas))) return rc;
  if ((rc = check_dtype(fn, dtype))) return rc;
  if (!phi || !deltas || !s1_out || !s2_out) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  if ((rc = smc_workspace_check(fn, workspace, workspace_bytes, smc_workspace_bytes(n, n_deltas)))) return rc;
  Deltas dl = {};
  for (int j = 0; j < n_deltas; ++j) {
    if ((rc = check_delta(fn, "deltas", j, deltas[j]))) return rc;
    dl.d[j] = deltas[j];
  }
  const int64_t nb = smc_blocks(n);
  double* part1 = (double*)workspace;
  double* part2 = part1 + nb * n_deltas;
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(temper_block_sums_kernel<T>, dim3(smc_groups(nb)), dim3(kSmcThreads), 0, st, (const T*)phi, n,
                       phi_ref, dl, (int)n_deltas, nb, part1, part2);
  });
  if ((rc = check_launch("temper_block_sums_kernel"))) return rc;
  hipLaunchKernelGGL(temper_total_kernel, dim3(1), dim3(kMaxDeltas), 0, st, part1, part2, (int)n_deltas, nb, s1_out,
                     s2_out);
  return check_launch("temper_total_kernel");
}

extern "C" int ipmc_temper_cumweights(const void* phi, int32_t dtype, int64_t n, double phi_ref, double delta,
                                      double* cum_out, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "ipmc_temper_cumweights";
  if (n < 0 || workspace_bytes < 0) return fail(IPMC_ERR_INVALID, "%s: negative size", fn);
  if (n == 0) return IPMC_OK;
  int rc;
  if ((rc = check_dtype(fn, dtype))) return rc;
  if (!phi || !cum_out) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  if ((rc = smc_workspace_check(fn, workspace, workspace_bytes, smc_workspace_bytes(n, 1)))) return rc;
  if ((rc = check_delta(fn, "delta", -1, delta))) return rc;
  const int64_t nb = smc_blocks(n);
  double* totals = (double*)workspace;
  double* offsets = totals + nb;
  hipStream_t st = (hipStream_t)stream;
  with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(cum_block_kernel<T>, dim3(smc_groups(nb)), dim3(kSmcThreads), 0, st, (const T*)phi, n, phi_ref,
                       delta, nb, cum_out, totals);
  });
  if ((rc = check_launch("cum_block_kernel"))) return rc;
  hipLaunchKernelGGL(cum_offsets_kernel, dim3(1), dim3(kSmcThreads), 0, st, totals, nb, offsets);
  if ((rc = check_launch("cum_offsets_kernel"))) return rc;
  int64_t groups = (n + kSmcThreads * 4 - 1) / (kSmcThreads * 4);
  if (groups > 4096) groups = 4096;
  hipLaunchKernelGGL(cum_add_kernel, dim3((unsigned)groups), dim3(kSmcThreads), 0, st, cum_out, n, offsets);
  return check_launch("cum_add_kernel");
}

extern "C" int ipmc_systematic_ancestors(const double* cum, int64_t n, double u, int64_t n_out, int64_t* anc_out,
                                         void* stream) {
  const int rc = check_ancestors("ipmc_systematic_ancestors", cum, n, u, n_out, anc_out);
  if (rc) return rc < 0 ? IPMC_OK : rc;
  int64_t groups = (n_out + kSmcThreads - 1) / kSmcThreads;
  if (groups > 4096) groups = 4096;
  hipLaunchKernelGGL(ancestors_kernel, dim3((unsigned)groups), dim3(kSmcThreads), 0, (hipStream_t)stream, cum, n, u,
                     n_out, anc_out);
  return check_launch("ancestors_kernel");
}

extern "C" int ipmc_gather_rows(const void* src, int32_t dtype, int64_t n_src, int32_t k, int64_t src_stride,
                                const int64_t* idx, int64_t n_out, void* dst, int64_t dst_stride, void* stream) {
  const char* fn = "ipmc_gather_rows";
  if (n_src < 0 || n_out < 0 || k < 0 || src_stride < 0 || dst_stride < 0)
    return fail(IPMC_ERR_INVALID, "%s: negative size", fn);
  if (n_out == 0) return IPMC_OK;
  if (k < 1 || k > 256) return fail(IPMC_ERR_INVALID, "%s: k = %d outside [1, 256]", fn, k);
  if (src_stride < k || dst_stride < k) return fail(IPMC_ERR_INVALID, "%s: a row stride is below k = %d", fn, k);
  if (const int rc = check_dtype(fn, dtype)) return rc;
  if (!idx || !dst || (n_src > 0 && !src)) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  const int64_t esize = dtype == IPMC_F64 ? 8 : 4;
  const int64_t max_rows = (INT64_MAX / esize - k) / (src_stride > dst_stride ? src_stride : dst_stride);
  if (n_src > max_rows || n_out > max_rows) return fail(IPMC_ERR_INVALID, "%s: rows * stride overflows", fn);
  if (n_src > 0) {
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)(((n_src - 1) * src_stride + k) * esize);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)(((n_out - 1) * dst_stride + k) * esize);
    if (s0 < d1 && d0 < s1) return fail(IPMC_ERR_INVALID, "%s: dst overlaps src (the gather is out of place)", fn);
  }
  const int rows_per_tile = kGatherElems / k > 0 ? kGatherElems / k : 1;
  const int64_t n_tiles = (n_out + rows_per_tile - 1) / rows_per_tile;
  const unsigned groups = (unsigned)(n_tiles < kGatherGroups ? n_tiles : kGatherGroups);
  with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(gather_rows_kernel<T>, dim3(groups), dim3(kSmcThreads), 0, (hipStream_t)stream, (const T*)src,
                       n_src, (int)k, src_stride, idx, n_out, (T*)dst, dst_stride, rows_per_tile, n_tiles);
  });
  return check_launch("gather_rows_kernel");
}

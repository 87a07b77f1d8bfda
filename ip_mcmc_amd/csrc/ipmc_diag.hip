// Chain diagnostics on the device, everything in fp64 on load:
//   autocorrelation   ipmc_autocorr: batched normalised autocorrelation of series;
//   burn-in           ipmc_burn_in: len_burn_in for a batch of chains;
//   ordered sums      ipmc_ordered_sum, ipmc_block_sums, ipmc_centered_sq_block_sums:
//                     column sums in a fixed row order (the posterior mean and the
//                     variance across chains);
//   convergence       ipmc_split_stats, ipmc_mean_acov, ipmc_moments_stats: the
//                     per-chain parts of split-R-hat / ESS / MCSE.
// The kernels come first, grouped in that order, then the entry points.  The lag
// sum r(tau) = sum_i xs[i] xs[i + tau] of the autocorrelation and of the
// convergence kernels is one body per access pattern (lag_sum_staged,
// lag_sum_streamed), so the paths chosen by the series length add the same
// products in the same order.
#include "ipmc_internal.hpp"

namespace ipmc {

// ---------------------------------------------------------- autocorrelation
// For every series x (one chain's samples of one component, or one window of
// it) this computes what MCMCSampler.autocorr does for one series
// (sampler.py:43-54): x_ = x - mean(x), r[tau] = sum_t x_[t] x_[t+tau]
// (np.correlate(x_, x_, 'full')[-n:]), out = r / r[0], or all ones when
// r[0] == 0 (a constant series).  helpers.autocorrelation (helpers.py:41-54)
// is this over windows of tau_max samples, averaged on the host.
//
// One workgroup per series: the series is staged once in LDS (coalesced
// strided load), the mean is a block reduction, and each thread owns lags
// tau = tid, tid + 256, ... with the inner sum over t read from LDS.  Longer
// series (> kAcMaxLen samples) stream through LDS tiles instead
// (autocorr_long_kernel), with the same summation order.
constexpr int kDiagBlock = 256;  // lanes of every workgroup of the lag sums and of the convergence kernels
constexpr int kAcMaxLen = 8192;  // doubles staged per series (64 KiB LDS)
constexpr int kAcTile = 2048;    // samples per streamed tile
// products formed per batch before they are added in order: a lone wave's
// dependent add would otherwise wait out an LDS latency per term (measured:
// ~120 cycles per term without it)
constexpr int kCvBatch = 16;

// The block's partials, one per thread, added by a tree (128, 64, ..., 1);
// every thread gets the sum, and red is free again on return.
__device__ inline double block_tree_sum(double part, double* red) {
  red[threadIdx.x] = part;
  __syncthreads();
  for (int off = kDiagBlock / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// r(tau) = sum of xs[i] * xs[i + tau] over i + tau < n, ascending in i, of a
// centred series staged in LDS.
__device__ inline double lag_sum_staged(const double* xs, int n, int tau) {
  double r = 0.0;
  int i = 0;
  for (; i + kCvBatch + tau <= n; i += kCvBatch) {  // the reads of a batch in flight together
    double p[kCvBatch];
#pragma unroll
    for (int u = 0; u < kCvBatch; ++u) p[u] = xs[i + u] * xs[i + u + tau];
#pragma unroll
    for (int u = 0; u < kCvBatch; ++u) r = r + p[u];  // added in ascending i all the same
  }
  for (; i + tau < n; ++i) r = r + xs[i] * xs[i + tau];
  return r;
}

// The same sum for the lag tau0 + threadIdx.x of a series of len > kAcMaxLen
// samples in global memory, xs = src - sub.  The block owns the kDiagBlock
// consecutive lags from tau0 and streams the series through LDS in tiles of
// kAcTile samples: a = xs[t0 .. t0+kAcTile), b = xs[t0+tau0 .. t0+tau0+kAcTile+kDiagBlock).
// Each thread's r(tau) is still the ascending sum over i, so the bits equal
// lag_sum_staged's.  Every thread of the block calls this (barriers); one with
// no lag to compute passes active = false.
template <typename T>
__device__ inline double lag_sum_streamed(const T* src, int64_t stride_t, int64_t len, double sub, int tau0,
                                          bool active, double* a, double* b) {
  const int sh = (int)threadIdx.x;
  const int tau = tau0 + sh;
  double r = 0.0;
  for (int64_t t0 = 0; t0 + tau0 < len; t0 += kAcTile) {
    for (int i = sh; i < kAcTile; i += kDiagBlock) {
      const int64_t t = t0 + i;
      a[i] = t < len ? (double)src[t * stride_t] - sub : 0.0;
    }
    for (int i = sh; i < kAcTile + kDiagBlock; i += kDiagBlock) {
      const int64_t t = t0 + tau0 + i;
      b[i] = t < len ? (double)src[t * stride_t] - sub : 0.0;
    }
    __syncthreads();
    if (active) {
      const int64_t rem = len - tau - t0;  // terms t0 + i with t0 + i + tau < len
      const int n = rem < kAcTile ? (int)(rem > 0 ? rem : 0) : kAcTile;
      int i = 0;
      for (; i + kCvBatch <= n; i += kCvBatch) {
        double p[kCvBatch];
#pragma unroll
        for (int u = 0; u < kCvBatch; ++u) p[u] = a[i + u] * b[i + u + sh];
#pragma unroll
        for (int u = 0; u < kCvBatch; ++u) r = r + p[u];
      }
      for (; i < n; ++i) r = r + a[i] * b[i + sh];
    }
    __syncthreads();
  }
  return r;
}

template <typename T>
__global__ __launch_bounds__(kDiagBlock) void autocorr_kernel(const T* __restrict__ x, int64_t n_series, int64_t len,
                                                               int64_t stride_series, int64_t stride_t, int max_lag,
                                                               double* __restrict__ out) {
  __shared__ double xs[kAcMaxLen];
  __shared__ double red[kDiagBlock];
  const int64_t s = blockIdx.x;
  if (s >= n_series) return;
  const T* src = x + s * stride_series;
  double part = 0.0;
  for (int64_t t = threadIdx.x; t < len; t += kDiagBlock) {
    const double v = (double)src[t * stride_t];
    xs[t] = v;
    part += v;
  }
  const double mean = block_tree_sum(part, red) / (double)len;
  for (int64_t t = threadIdx.x; t < len; t += kDiagBlock) xs[t] = xs[t] - mean;
  __syncthreads();
  // r[0] first (every thread needs it for the normalisation)
  double r0p = 0.0;
  for (int64_t t = threadIdx.x; t < len; t += kDiagBlock) r0p += xs[t] * xs[t];
  const double r0 = block_tree_sum(r0p, red);
  double* o = out + s * max_lag;
  for (int tau = threadIdx.x; tau < max_lag; tau += kDiagBlock)
    o[tau] = r0 == 0.0 ? 1.0 : lag_sum_staged(xs, (int)len, tau) / r0;
}

// Series longer than kAcMaxLen: the same sums from global memory.  A block
// owns kDiagBlock consecutive lags of one series (grid: series x lag tiles) and
// recomputes the mean and r[0] with the short kernel's strided-partials + tree
// order, so the results equal the short kernel's bit for bit.
template <typename T>
__global__ __launch_bounds__(kDiagBlock) void autocorr_long_kernel(const T* __restrict__ x, int64_t n_series,
                                                                    int64_t len, int64_t stride_series,
                                                                    int64_t stride_t, int max_lag,
                                                                    double* __restrict__ out) {
  __shared__ double a[kAcTile];
  __shared__ double b[kAcTile + kDiagBlock];
  __shared__ double red[kDiagBlock];
  const int64_t s = blockIdx.x;
  const int tau0 = blockIdx.y * kDiagBlock;
  if (s >= n_series || tau0 >= max_lag) return;
  const T* src = x + s * stride_series;
  double part = 0.0;
  for (int64_t t = threadIdx.x; t < len; t += kDiagBlock) part += (double)src[t * stride_t];
  const double mean = block_tree_sum(part, red) / (double)len;
  part = 0.0;
  for (int64_t t = threadIdx.x; t < len; t += kDiagBlock) {
    const double c = (double)src[t * stride_t] - mean;
    part += c * c;
  }
  const double r0 = block_tree_sum(part, red);
  const int tau = tau0 + (int)threadIdx.x;
  double* o = out + s * max_lag;
  if (r0 == 0.0) {
    if (tau < max_lag) o[tau] = 1.0;
    return;
  }
  const double r = lag_sum_streamed(src, stride_t, len, mean, tau0, tau < max_lag, a, b);
  if (tau < max_lag) o[tau] = r / r0;
}

// ---------------------------------------------------------------- burn-in
// len_burn_in (burgers/utilities.py:134-167) for a batch of chains.  Per
// chain c with n_vars series of len samples and window w:
//   avg_v[j] = (cs[j+w-1] - cs[j-1]) / w   (cs = np.cumsum, cs[-1] := 0 term absent)
//   changed[i] = any_v |(avg_v[i] - avg_v[i+1]) / mean_v| > thr,  i < L = len - w
//   burn_in = largest i in [1, L-w-2] with changed[i..i+w] all set, else len-1.
// Kernel 1: one thread per series (c, v) streams the series twice (the
// leading and trailing cumulative sums are both sequential sums in np.cumsum's
// order, so their difference is bit-identical to res[l:] - res[:-l]) and ORs
// its flags into a per-chain bitmask.  Kernel 2: one thread per chain scans
// the bitmask from the end.  All arithmetic is fp64.

// numpy pairwise_sum (loops_utils.h.src) of a strided series, iteratively.
template <typename T>
__device__ double np_pairwise_strided(const T* a, int64_t n, int64_t s) {
  int64_t off[48], len[48];
  double left[48];
  int stage[48];
  int sp = 0;
  off[0] = 0;
  len[0] = n;
  stage[0] = 0;
  double ret = 0.0;
  while (sp >= 0) {
    const int64_t o = off[sp], m = len[sp];
    if (m <= 128) {
      const T* b = a + o * s;
      if (m < 8) {
        double r = 0.0;
        for (int64_t i = 0; i < m; ++i) r = r + (double)b[i * s];
        ret = r;
      } else {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = (double)b[j * s];
        int64_t i;
        for (i = 8; i < m - (m % 8); i += 8)
          for (int j = 0; j < 8; ++j) r[j] = r[j] + (double)b[(i + j) * s];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < m; ++i) res = res + (double)b[i * s];
        ret = res;
      }
      --sp;
      continue;
    }
    int64_t n2 = m / 2;
    n2 -= n2 % 8;
    if (stage[sp] == 0) {
      stage[sp] = 1;
      ++sp;
      off[sp] = o;
      len[sp] = n2;
      stage[sp] = 0;
    } else if (stage[sp] == 1) {
      left[sp] = ret;
      stage[sp] = 2;
      ++sp;
      off[sp] = o + n2;
      len[sp] = m - n2;
      stage[sp] = 0;
    } else {
      ret = left[sp] + ret;
      --sp;
    }
  }
  return ret;
}

template <typename T>
__global__ __launch_bounds__(256) void burn_in_flags_kernel(const T* __restrict__ x, int64_t n_chains, int n_vars,
                                                             int64_t len, int64_t s_chain, int64_t s_var,
                                                             int64_t s_t, int w, double thr,
                                                             unsigned* __restrict__ flags, int64_t words) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_chains * n_vars) return;
  const int64_t c = g / n_vars;
  const int v = (int)(g % n_vars);
  const T* a = x + c * s_chain + v * s_var;
  const double mean = np_pairwise_strided<T>(a, len, s_t) / (double)len;
  const double dw = (double)w;
  double lead = (double)a[0];
  for (int64_t t = 1; t < w; ++t) lead = lead + (double)a[t * s_t];
  double trail = 0.0;
  double prev = lead / dw;
  unsigned* fl = flags + c * words;
  unsigned word = 0;
  const int64_t L = len - w;
  for (int64_t j = 1; j <= L; ++j) {
    lead = lead + (double)a[(j + w - 1) * s_t];
    trail = (j == 1) ? (double)a[0] : trail + (double)a[(j - 1) * s_t];
    const double cur = (lead - trail) / dw;
    const double ch = fabs((prev - cur) / mean);
    const int64_t i = j - 1;
    if (ch > thr) word |= 1u << (i & 31);
    if ((i & 31) == 31 || j == L) {
      if (word) atomicOr(fl + (i >> 5), word);
      word = 0;
    }
    prev = cur;
  }
}

__global__ void burn_in_search_kernel(int64_t n_chains, int64_t len, int w, const unsigned* __restrict__ flags,
                                      int64_t words, int64_t* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_chains) return;
  const unsigned* fl = flags + c * words;
  const int64_t L = len - w;
  const int64_t top = L - w - 2;
  int64_t run = 0, res = len - 1;
  for (int64_t j = L - 1; j >= 1; --j) {
    run = ((fl[j >> 5] >> (j & 31)) & 1u) ? run + 1 : 0;
    if (j <= top && run >= w + 1) {
      res = j;
      break;
    }
  }
  out[c] = res;
}

// ------------------------------------------------------------ ordered sums
// The chain-ordered column sums behind the many-chain posterior mean
// (shard.ordered_sum_sharded): acc[j] = (((acc[j] + x_0j/div) + x_1j/div) + ...)
// strictly in row order, the additions of ipmc_host_ordered_sum (same IEEE
// operations, -ffp-contract=off: the same bits).  The sum of a column is one
// dependent chain of adds, so the kernel keeps that chain fed: a block owns 64
// columns; wave 0 holds one column per lane and adds chunk c (<= 8 192 values)
// from LDS while waves 1-15 stream chunk c + 1 from global memory into the other
// LDS buffer (coalesced, many loads in flight) -- one barrier per chunk.  A
// lane walking the rows straight from global memory waits out a load latency
// per row or per unrolled group (2.5 ms for 65 536 x 40 values on the MI355X,
// more than the host library's one pass).
constexpr int kOsCols = 64;     // columns per block (wave 0: one per lane)
constexpr int kOsBuf = 8192;    // doubles per LDS buffer: 8192 / kc rows per chunk
constexpr int kOsBlock = 1024;  // wave 0 adds, waves 1-15 load
constexpr int kOsLoaders = kOsBlock / 64 - 1;
constexpr int kOsPerLane = 16;  // rows per loader lane and chunk (>= ceil(8192 / kOsLoaders / 1))

__global__ __launch_bounds__(kOsBlock) void ordered_sum_kernel(const double* __restrict__ x, int64_t n_rows, int64_t k,
                                                              int64_t stride, double div, double* __restrict__ acc) {
  __shared__ double buf[2][kOsBuf];
  const int t = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * kOsCols;
  const int kc = (int)((k - c0) < kOsCols ? (k - c0) : kOsCols);
  // rows per chunk: the buffer's rows, and at most what the loaders cover in one pass
  const int R = (kOsBuf / kc) < kOsLoaders * kOsPerLane ? (kOsBuf / kc) : kOsLoaders * kOsPerLane;
  const int64_t n_chunks = (n_rows + R - 1) / R;
  auto rows_of = [&](int64_t chunk) {
    const int64_t left = n_rows - chunk * R;
    return (int)(left < R ? left : R);
  };
  // loader lane l of waves 1-15: column l % 64, rows l / 64, + 15, + 30, ...
  // of the chunk -- all of its loads issued before any LDS write, so each lane
  // has up to kOsPerLane in flight and the block ~15 x 64 x 16 (no division
  // per element)
  const int lj = (t - 64) & 63, lr = (t - 64) >> 6;
  auto load = [&](int64_t chunk, int b) {  // chunk -> buf[b], row-major [rows][kc]
    if (lj >= kc) return;
    const int rows = rows_of(chunk);
    const double* src = x + chunk * R * stride + c0 + lj;
    double* dst = buf[b] + lj;
    double v[kOsPerLane];
#pragma unroll
    for (int u = 0; u < kOsPerLane; ++u) {
      const int r = lr + kOsLoaders * u;
      v[u] = r < rows ? src[r * stride] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kOsPerLane; ++u) {
      const int r = lr + kOsLoaders * u;
      if (r < rows) dst[r * kc] = v[u];
    }
  };
  double a = 0.0;
  if (t < kc) a = acc[c0 + t];
  if (t >= 64) load(0, 0);
  __syncthreads();
  for (int64_t c = 0; c < n_chunks; ++c) {
    if (t < 64) {
      if (t < kc) {
        const int rows = rows_of(c);
        const double* bb = buf[c & 1] + t;
        if (div == 1.0) {
#pragma unroll 8
          for (int r = 0; r < rows; ++r) a = a + bb[r * kc];
        } else {
#pragma unroll 8
          for (int r = 0; r < rows; ++r) a = a + bb[r * kc] / div;
        }
      }
    } else if (c + 1 < n_chunks) {
      load(c + 1, (int)((c + 1) & 1));
    }
    __syncthreads();  // chunk c consumed and chunk c + 1 in place
  }
  if (t < kc) acc[c0 + t] = a;
}

// The posterior mean's first stage (shard.block_sum): out[b][j] = (((0 +
// x_{bB,j}/div) + x_{bB+1,j}/div) + ...) over the rows of block b (B
// consecutive rows, the last block possibly shorter), strictly in row order --
// the additions of ipmc_host_ordered_sum from zero on each block, so the same
// bits.  Blocks are independent: one lane per (block, column), its loads issued
// kBsUnroll rows ahead of its adds; a block's B dependent adds are the critical
// path (B = 1 024: tens of microseconds for any number of blocks that fits the
// chip), where a whole-column chain over 65 536 rows takes ~0.7 ms.
// The term added per row is x, x / div, or (x - center[j])^2: the centred
// second stage of a two-pass variance across chains, in the same fixed order.
constexpr int kBsThreads = 256;
constexpr int kBsUnroll = 16;
enum BsTerm { kBsPlain, kBsDiv, kBsCenteredSq };

template <BsTerm kTerm>
__global__ __launch_bounds__(kBsThreads) void block_sums_kernel(const double* __restrict__ x, int64_t n_rows, int64_t k,
                                                               int64_t stride, int64_t B, double div,
                                                               const double* __restrict__ center,
                                                               double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kBsThreads + threadIdx.x;
  const int64_t nb = (n_rows + B - 1) / B;
  if (t >= nb * k) return;
  const int64_t b = t / k, j = t - b * k;
  const int64_t r0 = b * B;
  const int64_t rows = (n_rows - r0) < B ? (n_rows - r0) : B;
  const double* p = x + r0 * stride + j;
  const double c = kTerm == kBsCenteredSq ? center[j] : 0.0;
  auto term = [&](double v) {
    if constexpr (kTerm == kBsCenteredSq) {
      const double d = v - c;
      return d * d;
    } else if constexpr (kTerm == kBsDiv) {
      return v / div;
    } else {
      return v;
    }
  };
  double s = 0.0;
  int64_t r = 0;
  for (; r + kBsUnroll <= rows; r += kBsUnroll) {
    double v[kBsUnroll];
#pragma unroll
    for (int u = 0; u < kBsUnroll; ++u) v[u] = p[(r + u) * stride];
#pragma unroll
    for (int u = 0; u < kBsUnroll; ++u) s = s + term(v[u]);
  }
  for (; r < rows; ++r) s = s + term(p[r * stride]);
  out[b * k + j] = s;
}

// ------------------------------------------------- convergence across chains
// Split-R-hat / ESS / MCSE over an ensemble (diagnostics.convergence; these
// replace nothing in the reference, which never has more than one chain).
// Chain c's samples x[c, t, :], t < len, are cut into split chains m < 2C of
// N = len / 2 samples: m < C is x[m, :N], m >= C is x[m - C, N:2N] (an odd
// last sample is dropped).  Everything is widened to fp64 on load.
//
// Lane mappings of the per-series sums (split_stats), chosen from the shape
// alone (cv_lanes_over_time), so the bits never depend on the grid:
//   over components  one lane per (m, v), t ascending in the lane: adjacent
//                    lanes read adjacent components (k = 40..256, short series);
//   over time        one wave per (m, v), lane l sums t = l, l + 64, ... ascending,
//                    then a fixed xor butterfly (32, 16, ..., 1): for k = 2..3
//                    with many samples the waves of one block share the lines
//                    they read, and with unit time stride the loads are dense.
// The mean is summed about the series' first sample, mean = x_0 + Σ (x_t - x_0) / N:
// the differences are spread-sized, so the rounding of the sum is far below
// an ulp of a mean that is many spreads large, and both mappings (and the
// host definition, in sample order) round the same value: Bn, the covariance
// of such means, multiplies a change of a mean by 2 |mean| / spread.
__host__ __device__ inline bool cv_lanes_over_time(int64_t N, int k, int64_t stride_t) {
  return N >= 32 && (stride_t == 1 || k < 16);
}

template <typename T>
__device__ inline const T* cv_series(const T* x, int64_t m, int64_t n_chains, int64_t N, int64_t s_chain,
                                     int64_t s_t) {
  return m < n_chains ? x + m * s_chain : x + (m - n_chains) * s_chain + N * s_t;
}

// every lane ends with the same bits (a + b == b + a)
__device__ inline double cv_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

template <typename T>
__global__ __launch_bounds__(kDiagBlock) void split_stats_vars_kernel(const T* __restrict__ x, int64_t n_chains,
                                                                   int64_t N, int k, int64_t s_chain, int64_t s_t,
                                                                   int64_t s_var, double* __restrict__ mean_out,
                                                                   double* __restrict__ var_out) {
  const int64_t g = (int64_t)blockIdx.x * kDiagBlock + threadIdx.x;
  if (g >= 2 * n_chains * k) return;
  const int64_t m = g / k;
  const int v = (int)(g - m * k);
  const T* a = cv_series(x, m, n_chains, N, s_chain, s_t) + v * s_var;
  const double x0 = (double)a[0];
  double s = 0.0;
#pragma unroll 8
  for (int64_t t = 0; t < N; ++t) s = s + ((double)a[t * s_t] - x0);
  const double mean = x0 + s / (double)N;
  double q = 0.0;
#pragma unroll 8
  for (int64_t t = 0; t < N; ++t) {
    const double d = (double)a[t * s_t] - mean;
    q = q + d * d;
  }
  mean_out[g] = mean;
  var_out[g] = q / (double)(N - 1);
}

template <typename T>
__global__ __launch_bounds__(kDiagBlock) void split_stats_time_kernel(const T* __restrict__ x, int64_t n_chains,
                                                                   int64_t N, int k, int64_t s_chain, int64_t s_t,
                                                                   int64_t s_var, double* __restrict__ mean_out,
                                                                   double* __restrict__ var_out) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * (kDiagBlock / 64) + (threadIdx.x >> 6);  // one series per wave
  if (g >= 2 * n_chains * k) return;
  const int64_t m = g / k;
  const int v = (int)(g - m * k);
  const T* a = cv_series(x, m, n_chains, N, s_chain, s_t) + v * s_var;
  const double x0 = (double)a[0];
  double s = 0.0;
  for (int64_t t = lane; t < N; t += 64) s = s + ((double)a[t * s_t] - x0);
  const double mean = x0 + cv_wave_sum(s) / (double)N;
  double q = 0.0;
  for (int64_t t = lane; t < N; t += 64) {
    const double d = (double)a[t * s_t] - mean;
    q = q + d * d;
  }
  q = cv_wave_sum(q);
  if (lane == 0) {
    mean_out[g] = mean;
    var_out[g] = q / (double)(N - 1);
  }
}
// partial[b, tau, v] = sum over the split chains m of block b (block_chains
// consecutive ones, from zero in m order) of gamma_m(tau) = r_m(tau) / N,
// r_m(tau) = sum_i xs[i] xs[i + tau] ascending in i, xs = x - mean[m, v].
// One workgroup per (b, v, tile of kDiagBlock lags); a thread owns one lag and
// keeps its running sum in a register while the block walks its split chains,
// each series staged (centred) in LDS once: the (2C, k, L) per-chain lag sums
// never exist.  The products are compute, not bandwidth (N loads feed N * L
// multiply-adds), so the staging load's stride matters little here.
template <typename T>
__global__ __launch_bounds__(kDiagBlock) void mean_acov_kernel(const T* __restrict__ x, int64_t n_chains, int64_t N,
                                                              int k, int64_t s_chain, int64_t s_t, int64_t s_var,
                                                              const double* __restrict__ mean, int max_lag,
                                                              int64_t block_chains, double* __restrict__ partial) {
  __shared__ double xs[kAcMaxLen];
  const int64_t b = blockIdx.x / k;
  const int v = (int)(blockIdx.x - b * k);
  const int tau = (int)blockIdx.y * kDiagBlock + (int)threadIdx.x;
  const int64_t m0 = b * block_chains;
  const int64_t m1 = (m0 + block_chains) < 2 * n_chains ? (m0 + block_chains) : 2 * n_chains;
  const int n = (int)N;
  double acc = 0.0;
  for (int64_t m = m0; m < m1; ++m) {
    const T* a = cv_series(x, m, n_chains, N, s_chain, s_t) + v * s_var;
    const double mu = mean[m * k + v];
    for (int t = threadIdx.x; t < n; t += kDiagBlock) xs[t] = (double)a[t * s_t] - mu;
    __syncthreads();
    if (tau <= max_lag) acc = acc + lag_sum_staged(xs, n, tau) / (double)N;
    __syncthreads();
  }
  if (tau <= max_lag) partial[(b * ((int64_t)max_lag + 1) + tau) * k + v] = acc;
}

// N <= kCvDirectLen: staging a handful of samples costs a block two barriers
// and a load latency per split chain with most of its lanes idle (N = 10 for
// the 65 536 x 20 ensemble).  Here one lane owns (b, tau, v), v fastest, and
// reads its two factors straight from global memory (adjacent lanes adjacent
// components; a chain's few samples stay in the caches across its lags).  The
// same centred factors in the same ascending order: the bits of mean_acov_kernel.
constexpr int kCvDirectLen = 64;

template <typename T>
__global__ __launch_bounds__(kDiagBlock) void mean_acov_direct_kernel(const T* __restrict__ x, int64_t n_chains,
                                                                     int64_t N, int k, int64_t s_chain, int64_t s_t,
                                                                     int64_t s_var, const double* __restrict__ mean,
                                                                     int max_lag, int64_t block_chains,
                                                                     int64_t n_blocks, double* __restrict__ partial) {
  const int64_t g = (int64_t)blockIdx.x * kDiagBlock + threadIdx.x;
  const int64_t per_block = ((int64_t)max_lag + 1) * k;
  if (g >= n_blocks * per_block) return;
  const int64_t b = g / per_block;
  const int64_t rest = g - b * per_block;
  const int tau = (int)(rest / k);
  const int v = (int)(rest - (int64_t)tau * k);
  const int64_t m0 = b * block_chains;
  const int64_t m1 = (m0 + block_chains) < 2 * n_chains ? (m0 + block_chains) : 2 * n_chains;
  const int n = (int)N - tau;
  double acc = 0.0;
  for (int64_t m = m0; m < m1; ++m) {
    const T* a = cv_series(x, m, n_chains, N, s_chain, s_t) + v * s_var;
    const double mu = mean[m * k + v];
    double r = 0.0;
#pragma unroll 4
    for (int i = 0; i < n; ++i) r = r + ((double)a[i * s_t] - mu) * ((double)a[(i + tau) * s_t] - mu);
    acc = acc + r / (double)N;
  }
  partial[g] = acc;  // g == (b * (max_lag + 1) + tau) * k + v
}

// N > kAcMaxLen: each split chain streams through LDS (lag_sum_streamed).
template <typename T>
__global__ __launch_bounds__(kDiagBlock) void mean_acov_long_kernel(const T* __restrict__ x, int64_t n_chains,
                                                                   int64_t N, int k, int64_t s_chain, int64_t s_t,
                                                                   int64_t s_var, const double* __restrict__ mean,
                                                                   int max_lag, int64_t block_chains,
                                                                   double* __restrict__ partial) {
  __shared__ double a[kAcTile];
  __shared__ double bq[kAcTile + kDiagBlock];
  const int64_t b = blockIdx.x / k;
  const int v = (int)(blockIdx.x - b * k);
  const int tau0 = (int)blockIdx.y * kDiagBlock;
  const int tau = tau0 + (int)threadIdx.x;
  const int64_t m0 = b * block_chains;
  const int64_t m1 = (m0 + block_chains) < 2 * n_chains ? (m0 + block_chains) : 2 * n_chains;
  double acc = 0.0;
  for (int64_t m = m0; m < m1; ++m) {
    const T* src = cv_series(x, m, n_chains, N, s_chain, s_t) + v * s_var;
    const double r = lag_sum_streamed(src, s_t, N, mean[m * k + v], tau0, tau <= max_lag, a, bq);
    if (tau <= max_lag) acc = acc + r / (double)N;
  }
  if (tau <= max_lag) partial[(b * ((int64_t)max_lag + 1) + tau) * k + v] = acc;
}

// keep="moments" sums -> per-chain mean and sample variance, the operations of
// the host formula in its order: mean = s / n, var = (s2 - (s * s) / n) / (n - 1).
__global__ __launch_bounds__(kDiagBlock) void moments_stats_kernel(const double* __restrict__ sum_u,
                                                                  const double* __restrict__ sum_u2, int64_t count,
                                                                  double n, double* __restrict__ mean_out,
                                                                  double* __restrict__ var_out) {
  const int64_t g = (int64_t)blockIdx.x * kDiagBlock + threadIdx.x;
  if (g >= count) return;
  const double s = sum_u[g];
  mean_out[g] = s / n;
  var_out[g] = (sum_u2[g] - (s * s) / n) / (n - 1.0);
}

// shared argument checks of ipmc_split_stats / ipmc_mean_acov; 0 = launch,
// -1 = nothing to do, else the status to return
static int cv_check(const char* fn, const void* x, int32_t dtype, int64_t n_chains, int64_t len, int32_t k,
                    int64_t s_chain, int64_t s_t, int64_t s_var) {
  if (n_chains < 0 || len < 0 || k < 0 || s_chain < 0 || s_t < 0 || s_var < 0)
    return fail(IPMC_ERR_INVALID, "%s: negative size", fn);
  if (n_chains == 0) return -1;
  if (len < 4)
    return fail(IPMC_ERR_INVALID, "%s: %lld samples per chain; a split chain needs at least 2 (len >= 4)", fn,
                (long long)len);
  if (k < 1 || k > 256) return fail(IPMC_ERR_INVALID, "%s: k = %d outside [1, 256]", fn, k);
  if (const int rc = check_dtype(fn, dtype)) return rc;
  if (!x) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  if (2 * n_chains > 0x7fffffff / 256)
    return fail(IPMC_ERR_INVALID, "%s: at most %d chains per call", fn, 0x7fffffff / 512);
  return 0;
}

// shared checks and launch of ipmc_block_sums / ipmc_centered_sq_block_sums
static int block_sums(const char* fn, const double* rows, int64_t n_rows, int64_t k, int64_t row_stride,
                      int64_t block_rows, double div, const double* center, bool centered, double* out,
                      void* stream) {
  if (n_rows < 0 || k < 0 || row_stride < k || block_rows <= 0)
    return fail(IPMC_ERR_INVALID, "%s: bad shape (n_rows, k >= 0, row_stride >= k, block_rows > 0)", fn);
  if (n_rows == 0 || k == 0) return IPMC_OK;
  if (!rows || !out || (centered && !center)) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  const int64_t lanes = (n_rows + block_rows - 1) / block_rows * k;
  // v / 1.0 == v: the term without the division gives the same bits sooner
  auto kern = centered ? block_sums_kernel<kBsCenteredSq>
                       : (div == 1.0 ? block_sums_kernel<kBsPlain> : block_sums_kernel<kBsDiv>);
  hipLaunchKernelGGL(kern, dim3((unsigned)((lanes + kBsThreads - 1) / kBsThreads)), dim3(kBsThreads), 0,
                     (hipStream_t)stream, rows, n_rows, k, row_stride, block_rows, div, center, out);
  return check_launch(centered ? "centered_sq_block_sums_kernel" : "block_sums_kernel");
}

}  // namespace ipmc

using namespace ipmc;

extern "C" int ipmc_autocorr(const void* x, int32_t dtype, int64_t n_series, int64_t len, int64_t stride_series,
                             int64_t stride_t, int32_t max_lag, double* out, void* stream) {
  if (n_series < 0 || len < 0 || max_lag < 0) return fail(IPMC_ERR_INVALID, "ipmc_autocorr: negative size");
  if (n_series == 0 || max_lag == 0) return IPMC_OK;
  if (len == 0 || !x || !out) return fail(IPMC_ERR_INVALID, "ipmc_autocorr: empty series or NULL pointer");
  if (max_lag > len)
    return fail(IPMC_ERR_INVALID, "ipmc_autocorr: max_lag %d exceeds the series length %lld", max_lag, (long long)len);
  const bool streamed = len > kAcMaxLen;
  if (streamed && n_series > 0x7fffffff)
    return fail(IPMC_ERR_INVALID, "ipmc_autocorr: at most 2^31 - 1 long series per call");
  if (const int rc = check_dtype("ipmc_autocorr", dtype)) return rc;
  const dim3 grid((unsigned)n_series, streamed ? (unsigned)((max_lag + kDiagBlock - 1) / kDiagBlock) : 1u);
  with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    auto kern = streamed ? autocorr_long_kernel<T> : autocorr_kernel<T>;
    hipLaunchKernelGGL(kern, grid, dim3(kDiagBlock), 0, (hipStream_t)stream, (const T*)x, n_series, len, stride_series,
                       stride_t, max_lag, out);
  });
  return check_launch(streamed ? "autocorr_long_kernel" : "autocorr_kernel");
}

extern "C" int ipmc_burn_in(const void* x, int32_t dtype, int64_t n_chains, int32_t n_vars, int64_t len,
                            int64_t stride_chain, int64_t stride_var, int64_t stride_t, int32_t window,
                            double threshold, uint32_t* flags_scratch, int64_t* out, void* stream) {
  if (n_chains < 0 || n_vars <= 0 || len < 0 || window <= 0)
    return fail(IPMC_ERR_INVALID, "ipmc_burn_in: bad sizes (n_vars and window must be positive)");
  if (n_chains == 0) return IPMC_OK;
  if (len < window)
    return fail(IPMC_ERR_INVALID, "ipmc_burn_in: series of %lld samples shorter than the window %d", (long long)len,
                window);
  if (!x || !out || !flags_scratch) return fail(IPMC_ERR_INVALID, "ipmc_burn_in: NULL pointer");
  int rc = check_dtype("ipmc_burn_in", dtype);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t words = (len + 31) / 32;
  if (hipMemsetAsync(flags_scratch, 0, (size_t)(n_chains * words) * sizeof(uint32_t), st) != hipSuccess)
    return fail(IPMC_ERR_DEVICE, "ipmc_burn_in: memset failed");
  const int64_t ns = n_chains * n_vars;
  const unsigned nb = (unsigned)((ns + 255) / 256);
  with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(burn_in_flags_kernel<T>, dim3(nb), dim3(256), 0, st, (const T*)x, n_chains, n_vars, len,
                       stride_chain, stride_var, stride_t, window, threshold, (unsigned*)flags_scratch, words);
  });
  if ((rc = check_launch("burn_in_flags_kernel"))) return rc;
  hipLaunchKernelGGL(burn_in_search_kernel, dim3((unsigned)((n_chains + 255) / 256)), dim3(256), 0, st, n_chains, len,
                     window, (const unsigned*)flags_scratch, words, out);
  return check_launch("burn_in_search_kernel");
}

extern "C" int ipmc_ordered_sum(const double* rows, int64_t n_rows, int64_t k, int64_t row_stride, double div,
                                double* acc, void* stream) {
  if (n_rows < 0 || k < 0 || row_stride < k)
    return fail(IPMC_ERR_INVALID, "ipmc_ordered_sum: bad shape (n_rows, k >= 0, row_stride >= k)");
  if (n_rows == 0 || k == 0) return IPMC_OK;
  if (!rows || !acc) return fail(IPMC_ERR_INVALID, "ipmc_ordered_sum: NULL pointer");
  hipLaunchKernelGGL(ordered_sum_kernel, dim3((unsigned)((k + kOsCols - 1) / kOsCols)), dim3(kOsBlock), 0,
                     (hipStream_t)stream, rows, n_rows, k, row_stride, div, acc);
  return check_launch("ordered_sum_kernel");
}

extern "C" int ipmc_block_sums(const double* rows, int64_t n_rows, int64_t k, int64_t row_stride, int64_t block_rows,
                               double div, double* out, void* stream) {
  return block_sums("ipmc_block_sums", rows, n_rows, k, row_stride, block_rows, div, nullptr, false, out, stream);
}

extern "C" int ipmc_centered_sq_block_sums(const double* rows, int64_t n_rows, int64_t k, int64_t row_stride,
                                           const double* center, int64_t block_rows, double* out, void* stream) {
  return block_sums("ipmc_centered_sq_block_sums", rows, n_rows, k, row_stride, block_rows, 1.0, center, true, out,
                    stream);
}

extern "C" int ipmc_split_stats(const void* x, int32_t dtype, int64_t n_chains, int64_t len, int32_t k,
                                int64_t stride_chain, int64_t stride_t, int64_t stride_var, double* mean_out,
                                double* var_out, void* stream) {
  int rc = cv_check("ipmc_split_stats", x, dtype, n_chains, len, k, stride_chain, stride_t, stride_var);
  if (rc) return rc < 0 ? IPMC_OK : rc;
  if (!mean_out || !var_out) return fail(IPMC_ERR_INVALID, "ipmc_split_stats: NULL pointer");
  const int64_t N = len / 2, series = 2 * n_chains * k;
  const bool over_time = cv_lanes_over_time(N, k, stride_t);
  const int64_t per_block = over_time ? kDiagBlock / 64 : kDiagBlock;
  const dim3 grid((unsigned)((series + per_block - 1) / per_block));
  with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    auto kern = over_time ? split_stats_time_kernel<T> : split_stats_vars_kernel<T>;
    hipLaunchKernelGGL(kern, grid, dim3(kDiagBlock), 0, (hipStream_t)stream, (const T*)x, n_chains, N, (int)k,
                       stride_chain, stride_t, stride_var, mean_out, var_out);
  });
  return check_launch(over_time ? "split_stats_time_kernel" : "split_stats_vars_kernel");
}

extern "C" int ipmc_mean_acov(const void* x, int32_t dtype, int64_t n_chains, int64_t len, int32_t k,
                              int64_t stride_chain, int64_t stride_t, int64_t stride_var, const double* mean,
                              int32_t max_lag, int64_t block_chains, double* partial_out, void* stream) {
  if (max_lag < 0) return fail(IPMC_ERR_INVALID, "ipmc_mean_acov: negative size");
  int rc = cv_check("ipmc_mean_acov", x, dtype, n_chains, len, k, stride_chain, stride_t, stride_var);
  if (rc) return rc < 0 ? IPMC_OK : rc;
  const int64_t N = len / 2;
  if (max_lag > N - 1)
    return fail(IPMC_ERR_INVALID, "ipmc_mean_acov: max_lag %d exceeds len/2 - 1 = %lld", max_lag, (long long)(N - 1));
  if (block_chains <= 0) return fail(IPMC_ERR_INVALID, "ipmc_mean_acov: block_chains must be positive");
  if (!mean || !partial_out) return fail(IPMC_ERR_INVALID, "ipmc_mean_acov: NULL pointer");
  const int64_t n_blocks = (2 * n_chains + block_chains - 1) / block_chains;
  const int64_t tiles = ((int64_t)max_lag + kDiagBlock) / kDiagBlock;  // ceil((max_lag + 1) / kDiagBlock)
  if (tiles > 65535)
    return fail(IPMC_ERR_INVALID, "ipmc_mean_acov: max_lag %d needs more than 65535 lag tiles", max_lag);
  hipStream_t st = (hipStream_t)stream;
  const bool direct = N <= kCvDirectLen, streamed = N > kAcMaxLen;
  with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (direct) {
      const int64_t lanes = n_blocks * ((int64_t)max_lag + 1) * k;
      hipLaunchKernelGGL(mean_acov_direct_kernel<T>, dim3((unsigned)((lanes + kDiagBlock - 1) / kDiagBlock)),
                         dim3(kDiagBlock), 0, st, (const T*)x, n_chains, N, (int)k, stride_chain, stride_t, stride_var,
                         mean, (int)max_lag, block_chains, n_blocks, partial_out);
    } else {
      auto kern = streamed ? mean_acov_long_kernel<T> : mean_acov_kernel<T>;
      hipLaunchKernelGGL(kern, dim3((unsigned)(n_blocks * k), (unsigned)tiles), dim3(kDiagBlock), 0, st, (const T*)x,
                         n_chains, N, (int)k, stride_chain, stride_t, stride_var, mean, (int)max_lag, block_chains,
                         partial_out);
    }
  });
  return check_launch(direct ? "mean_acov_direct_kernel" : streamed ? "mean_acov_long_kernel" : "mean_acov_kernel");
}

extern "C" int ipmc_moments_stats(const double* sum_u, const double* sum_u2, int64_t n_chains, int32_t k, int64_t n,
                                  double* mean_out, double* var_out, void* stream) {
  if (n_chains < 0 || k < 0 || n < 0) return fail(IPMC_ERR_INVALID, "ipmc_moments_stats: negative size");
  if (n_chains == 0 || k == 0) return IPMC_OK;
  if (n < 2)
    return fail(IPMC_ERR_INVALID, "ipmc_moments_stats: a variance needs n >= 2 steps, got %lld", (long long)n);
  if (!sum_u || !sum_u2 || !mean_out || !var_out) return fail(IPMC_ERR_INVALID, "ipmc_moments_stats: NULL pointer");
  const int64_t count = n_chains * k;
  if ((count + kDiagBlock - 1) / kDiagBlock > 0x7fffffff)
    return fail(IPMC_ERR_INVALID, "ipmc_moments_stats: too many values for one call");
  hipLaunchKernelGGL(moments_stats_kernel, dim3((unsigned)((count + kDiagBlock - 1) / kDiagBlock)), dim3(kDiagBlock), 0,
                     (hipStream_t)stream, sum_u, sum_u2, count, (double)n, mean_out, var_out);
  return check_launch("moments_stats_kernel");
}

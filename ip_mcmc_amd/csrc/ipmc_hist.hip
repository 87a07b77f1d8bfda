// Pooled posterior histograms over all chains and samples (posterior.py):
// ipmc_minmax (the support), ipmc_hist1d (marginal counts), ipmc_histdd (joint
// counts).  One streaming pass each over the strided geometry of
// ipmc_split_stats.  Counters are integers throughout: integer adds commute,
// so no result depends on the grid or on the order in which lanes arrive
// (the project's "no floating-point atomics" rule is kept).
//
// Bin membership (the definition in posterior.py): sample x is in bin b iff
// edges[b] <= x < edges[b + 1], the last bin closed on the right; x < edges[0]
// is below, x > edges[B] above, NaN counts nowhere.  f32 samples are widened
// to double before any comparison and the edges are double, so every decision
// is the host's np.searchsorted on the same numbers.
#include <cstdlib>

#include "ipmc_internal.hpp"

namespace ipmc {
namespace {

constexpr int kHsBlock = 256;
constexpr int kHsUnroll = 4;                   // loads of one lane in flight together
constexpr int kHsGroups = IPMC_MINMAX_GROUPS;  // workgroups (partials) of a minmax pass
// A histogram workgroup counts at most kHsMaxSpan elements (the launch code
// below sizes the grid so), and every LDS counter receives at most one add of
// one per element or, from the wave leader of the joint kernel, one add of a
// lane count whose sum over the span is again at most the span: a uint32
// counter holds at most 2^31 < 2^32 by construction, for any input size.
constexpr int64_t kHsMaxSpan = (int64_t)1 << 31;
constexpr int kHsCounterBudget = 6144;  // uint32 LDS counters of a marginal workgroup (all copies)
constexpr int kHsCellBudget = 4352;     // counters of one copy: component tile * (B + 2)
constexpr int kDdLdsCells = 8192;       // joint cells kept in LDS (20^3 = 8 000 fits)
constexpr int kDdLdsEdges = 2048;       // joint edges kept in LDS beside them
constexpr int64_t kMmChunk = 16384;     // samples of one wave's piece of a row (minmax, lanes over time)

// The samples as C x outer x inner with element strides, inner the dimension
// of the smaller stride, so that consecutive flat indices are consecutive
// addresses for both layouts run() produces: (C, n, k) has inner = component
// (k = 3 is then one dense run of the flattened array, k = 40..256 puts
// adjacent lanes on adjacent components), (C, k, n) has inner = time.
struct HsGeom {
  int64_t n_chains, outer_n, inner_n;
  int64_t s_chain, s_outer, s_inner;
  int var_inner;  // 1: the component is the inner index, 0: the outer one
  int dense;      // 1: the samples are one dense array and its extents fit 31 bits: the offset is the flat index
};

HsGeom hs_geom(int64_t n_chains, int64_t len, int k, int64_t s_chain, int64_t s_t, int64_t s_var) {
  HsGeom g;
  g.n_chains = n_chains;
  g.s_chain = s_chain;
  g.var_inner = s_var <= s_t;
  if (g.var_inner) {
    g.inner_n = k, g.s_inner = s_var, g.outer_n = len, g.s_outer = s_t;
    if (s_chain == len * s_t) {  // the chains follow one another: one long chain, no wrap to look for
      g.outer_n = n_chains * len;
      g.n_chains = 1;
    }
  } else {
    g.inner_n = len, g.s_inner = s_t, g.outer_n = k, g.s_outer = s_var;
  }
  g.dense = g.s_inner == 1 && g.s_outer == g.inner_n && (g.n_chains == 1 || g.s_chain == g.outer_n * g.inner_n) &&
            g.inner_n < ((int64_t)1 << 31) && g.outer_n < ((int64_t)1 << 31);
  return g;
}

struct HsPos {
  int64_t c, o, i;
};

__device__ inline HsPos hs_pos(const HsGeom& g, int64_t flat) {
  HsPos p;
  const int64_t row = flat / g.inner_n;
  p.i = flat - row * g.inner_n;
  p.c = row / g.outer_n;
  p.o = row - p.c * g.outer_n;
  return p;
}

// flat += dq * inner_n + dr with dr < inner_n: one carry at most into the
// outer index; the divisions of hs_pos happen once per lane
__device__ inline void hs_advance(const HsGeom& g, HsPos& p, int64_t dq, int64_t dr) {
  p.i += dr;
  p.o += dq;
  if (p.i >= g.inner_n) {
    p.i -= g.inner_n;
    ++p.o;
  }
  if (p.o >= g.outer_n) {
    if (p.o - g.outer_n < g.outer_n) {
      p.o -= g.outer_n;
      ++p.c;
    } else {
      const int64_t q = p.o / g.outer_n;
      p.c += q;
      p.o -= q * g.outer_n;
    }
  }
}

__device__ inline int64_t hs_offset(const HsGeom& g, const HsPos& p) {
  return p.c * g.s_chain + p.o * g.s_outer + p.i * g.s_inner;
}

// The position of a lane that steps through the flat elements kHsBlock at a
// time.  kDense (both layouts of run() as they come: HsGeom::dense): the
// offset is the flat index itself and only the component is tracked, in 32
// bits -- the kernels are bound by their instruction count, not by HBM
// (ipmc_hist1d on the 419 MB ensemble: 0.216 -> 0.169 ms).  Otherwise the
// general strided walk above.
template <bool kDense>
struct HsWalk;

template <>
struct HsWalk<false> {
  HsPos p;
  int64_t dq, dr;
  __device__ HsWalk(const HsGeom& g, int64_t flat) : p(hs_pos(g, flat)) {
    dq = kHsBlock / g.inner_n, dr = kHsBlock - dq * g.inner_n;
  }
  __device__ int var(const HsGeom& g) const { return (int)(g.var_inner ? p.i : p.o); }
  __device__ int64_t offset(const HsGeom& g, int64_t) const { return hs_offset(g, p); }
  __device__ void advance(const HsGeom& g) { hs_advance(g, p, dq, dr); }
};

template <>
struct HsWalk<true> {
  uint32_t i, o, dq, dr;
  __device__ HsWalk(const HsGeom& g, int64_t flat) {
    const int64_t row = flat / g.inner_n;
    i = (uint32_t)(flat - row * g.inner_n);
    o = (uint32_t)(row % g.outer_n);
    dq = (uint32_t)(kHsBlock / g.inner_n), dr = (uint32_t)(kHsBlock - dq * g.inner_n);
  }
  __device__ int var(const HsGeom& g) const { return (int)(g.var_inner ? i : o); }
  __device__ int64_t offset(const HsGeom&, int64_t flat) const { return flat; }
  __device__ void advance(const HsGeom& g) {
    const uint32_t in = (uint32_t)g.inner_n, on = (uint32_t)g.outer_n;
    i += dr;
    const uint32_t carry = i >= in;
    if (carry) i -= in;
    if (!g.var_inner) {  // the outer index is needed only where it is the component
      o += dq + carry;   // < 2^31 + 257
      if (o >= on) o = (o - on < on) ? o - on : o % on;
    }
  }
};

// Bin of x among the ascending edges e[0..B]: B = below, B + 1 = above,
// -1 = NaN.  The guess from the uniform spacing is corrected by walking
// against the edges, so any ascending edge array gives the definition's
// answer and uniform edges cost one or two comparisons.
__device__ inline int hs_bin(const double* e, int B, double scale, double x) {
  const double lo = e[0], hi = e[B];
  if (!(x >= lo)) return x < lo ? B : -1;
  if (x > hi) return B + 1;
  const double t = fmin(fmax((x - lo) * scale, 0.0), (double)(B - 1));  // fmax(NaN, 0) = 0
  int b = (int)t;
  while (b > 0 && x < e[b]) --b;
  while (b < B - 1 && x >= e[b + 1]) ++b;
  return b;
}

// ---------------------------------------------------------------- support
// Component = inner index.  Lanes step by `step`, the largest multiple of k
// within the block, so a lane keeps its component and its running min and max
// stay in registers; a wave still reads one dense run.  NaN fails both
// comparisons and is skipped.  pmin / pmax [gridDim.x, k]: every block
// writes all k of its partials (+inf / -inf where it saw nothing).
template <typename T>
__global__ __launch_bounds__(kHsBlock) void minmax_inner_kernel(const T* __restrict__ x, HsGeom g, int64_t total,
                                                               int64_t span, int k, int step,
                                                               double* __restrict__ pmin, double* __restrict__ pmax) {
  __shared__ double smn[kHsBlock], smx[kHsBlock];
  const int tid = threadIdx.x;
  double mn = INFINITY, mx = -INFINITY;
  int64_t f = (int64_t)blockIdx.x * span + tid;
  const int64_t stop = (int64_t)(blockIdx.x + 1) * span;
  const int64_t end = stop < total ? stop : total;
  if (tid < step && f < end) {
    HsPos p = hs_pos(g, f);
    const int64_t dq = step / k;  // step % inner_n == 0
    while (f < end) {
      double v[kHsUnroll];
#pragma unroll
      for (int u = 0; u < kHsUnroll; ++u) {  // the loads of a batch in flight together
        v[u] = NAN;
        if (f < end) {
          v[u] = (double)x[g.dense ? f : hs_offset(g, p)];
          if (!g.dense) hs_advance(g, p, dq, 0);
          f += step;
        }
      }
#pragma unroll
      for (int u = 0; u < kHsUnroll; ++u) {
        if (v[u] < mn) mn = v[u];
        if (v[u] > mx) mx = v[u];
      }
    }
  }
  smn[tid] = mn;
  smx[tid] = mx;
  __syncthreads();
  if (tid < k) {
    for (int j = tid + k; j < step; j += k) {
      if (smn[j] < mn) mn = smn[j];
      if (smx[j] > mx) mx = smx[j];
    }
    pmin[(int64_t)blockIdx.x * k + tid] = mn;
    pmax[(int64_t)blockIdx.x * k + tid] = mx;
  }
}

// Component = outer index (lanes over time).  A unit is one piece of at most
// kMmChunk samples of one (chain, component) row; a wave reduces a unit with
// shuffles and its lane 0 folds the result into the wave's own LDS row, so
// nothing is shared between waves before the last barrier.
template <typename T>
__global__ __launch_bounds__(kHsBlock) void minmax_outer_kernel(const T* __restrict__ x, HsGeom g, int64_t units,
                                                               int64_t uspan, int64_t nchunk, int k,
                                                               double* __restrict__ pmin, double* __restrict__ pmax) {
  __shared__ double smn[kHsBlock / 64][256], smx[kHsBlock / 64][256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int j = tid; j < (kHsBlock / 64) * 256; j += kHsBlock) {
    (&smn[0][0])[j] = INFINITY;
    (&smx[0][0])[j] = -INFINITY;
  }
  __syncthreads();
  const int64_t stop = (int64_t)(blockIdx.x + 1) * uspan;
  const int64_t end = stop < units ? stop : units;
  for (int64_t u = (int64_t)blockIdx.x * uspan + wave; u < end; u += kHsBlock / 64) {
    const int64_t row = u / nchunk, ch = u - row * nchunk;
    const int64_t c = row / k;
    const int v = (int)(row - c * k);
    const int64_t t0 = ch * kMmChunk;
    const int64_t t1 = (t0 + kMmChunk) < g.inner_n ? (t0 + kMmChunk) : g.inner_n;
    const T* a = x + c * g.s_chain + v * g.s_outer;
    double mn = INFINITY, mx = -INFINITY;
#pragma unroll 4
    for (int64_t t = t0 + lane; t < t1; t += 64) {
      const double s = (double)a[t * g.s_inner];
      if (s < mn) mn = s;
      if (s > mx) mx = s;
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double on = __shfl_xor(mn, off), ox = __shfl_xor(mx, off);
      if (on < mn) mn = on;
      if (ox > mx) mx = ox;
    }
    if (lane == 0) {
      if (mn < smn[wave][v]) smn[wave][v] = mn;
      if (mx > smx[wave][v]) smx[wave][v] = mx;
    }
  }
  __syncthreads();
  if (tid < k) {
    double mn = smn[0][tid], mx = smx[0][tid];
    for (int w = 1; w < kHsBlock / 64; ++w) {
      if (smn[w][tid] < mn) mn = smn[w][tid];
      if (smx[w][tid] > mx) mx = smx[w][tid];
    }
    pmin[(int64_t)blockIdx.x * k + tid] = mn;
    pmax[(int64_t)blockIdx.x * k + tid] = mx;
  }
}

// second stage: one workgroup per component over the n_groups partials (a lane
// that walked all 1 024 of them alone took longer than the first stage)
__global__ __launch_bounds__(kHsBlock) void minmax_combine_kernel(const double* __restrict__ pmin,
                                                                 const double* __restrict__ pmax, int n_groups, int k,
                                                                 double* __restrict__ min_out,
                                                                 double* __restrict__ max_out) {
  __shared__ double smn[kHsBlock], smx[kHsBlock];
  const int v = blockIdx.x, tid = threadIdx.x;
  double mn = INFINITY, mx = -INFINITY;
  for (int b = tid; b < n_groups; b += kHsBlock) {
    const double a = pmin[(int64_t)b * k + v], c = pmax[(int64_t)b * k + v];
    if (a < mn) mn = a;
    if (c > mx) mx = c;
  }
  smn[tid] = mn;
  smx[tid] = mx;
  __syncthreads();
  for (int s = kHsBlock / 2; s > 0; s >>= 1) {
    if (tid < s) {
      if (smn[tid + s] < smn[tid]) smn[tid] = smn[tid + s];
      if (smx[tid + s] > smx[tid]) smx[tid] = smx[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    min_out[v] = smn[0];
    max_out[v] = smx[0];
  }
}

// the three results of ipmc_hist1d zeroed in one launch
__global__ __launch_bounds__(kHsBlock) void hist1d_zero_kernel(unsigned long long* __restrict__ counts, int64_t n,
                                                              unsigned long long* __restrict__ below,
                                                              unsigned long long* __restrict__ above, int k) {
  const int64_t j = (int64_t)blockIdx.x * kHsBlock + threadIdx.x;
  if (j < n) counts[j] = 0;
  if (j < k) below[j] = 0, above[j] = 0;
}

// ------------------------------------------------------------- marginals
// Workgroup (bx, by) counts the flat elements [bx * span, (bx + 1) * span) of
// the components [by * kt, by * kt + kt) (a tile: kt * (B + 2) counters fit
// the budget; elements of other components are skipped before their load).
// LDS: the tile's edges and B / (hi - lo), then uint32 counters, per
// component B bins + below + above, each replicated 2^copies_log2 times with
// the copies of a counter in adjacent banks and lane l adding to copy
// l mod 2^copies_log2: when every sample of a component falls into one bin,
// the 64 / k lanes of a wave on that component meet on the same address only
// once per copy.  The flush adds each counter's copies and issues one 64-bit
// integer add per non-zero counter.
template <typename T, bool kDense>
__global__ __launch_bounds__(kHsBlock) void hist1d_kernel(const T* __restrict__ x, HsGeom g, int64_t total,
                                                         int64_t span, int k, int B, int kt, int copies_log2,
                                                         const double* __restrict__ edges,
                                                         unsigned long long* __restrict__ counts,
                                                         unsigned long long* __restrict__ below,
                                                         unsigned long long* __restrict__ above) {
  extern __shared__ double hs_lds[];
  const int tid = threadIdx.x;
  const int v0 = (int)blockIdx.y * kt;
  const int nv = (k - v0) < kt ? (k - v0) : kt;
  double* edg = hs_lds;                          // [kt][B + 1]
  double* scl = edg + (int64_t)kt * (B + 1);     // [kt]
  uint32_t* cnt = (uint32_t*)(scl + kt);         // [kt * (B + 2)] << copies_log2
  const int cells = nv * (B + 2);
  for (int j = tid; j < nv * (B + 1); j += kHsBlock) edg[j] = edges[(int64_t)v0 * (B + 1) + j];
  for (int j = tid; j < (cells << copies_log2); j += kHsBlock) cnt[j] = 0u;
  __syncthreads();
  for (int j = tid; j < nv; j += kHsBlock) scl[j] = (double)B / (edg[j * (B + 1) + B] - edg[j * (B + 1)]);
  __syncthreads();
  const int copy = tid & ((1 << copies_log2) - 1);
  int64_t f = (int64_t)blockIdx.x * span + tid;
  const int64_t stop = (int64_t)(blockIdx.x + 1) * span;
  const int64_t end = stop < total ? stop : total;
  if (f < end) {
    HsWalk<kDense> w(g, f);
    while (f < end) {
      double xv[kHsUnroll];
      int vv[kHsUnroll];
#pragma unroll
      for (int u = 0; u < kHsUnroll; ++u) {
        vv[u] = -1;
        if (f < end) {
          const int v = w.var(g) - v0;
          if ((unsigned)v < (unsigned)nv) {
            vv[u] = v;
            xv[u] = (double)x[w.offset(g, f)];
          }
          w.advance(g);
          f += kHsBlock;
        }
      }
#pragma unroll
      for (int u = 0; u < kHsUnroll; ++u) {
        if (vv[u] >= 0) {
          const int b = hs_bin(edg + vv[u] * (B + 1), B, scl[vv[u]], xv[u]);
          if (b >= 0) atomicAdd(&cnt[((vv[u] * (B + 2) + b) << copies_log2) + copy], 1u);
        }
      }
    }
  }
  __syncthreads();
  for (int j = tid; j < cells; j += kHsBlock) {
    unsigned long long s = 0;
    for (int r = 0; r < (1 << copies_log2); ++r) s += cnt[(j << copies_log2) + r];
    if (s == 0) continue;
    const int v = j / (B + 2), b = j - v * (B + 2);
    unsigned long long* dst = b < B ? counts + (int64_t)(v0 + v) * B + b : (b == B ? below : above) + (v0 + v);
    atomicAdd(dst, s);
  }
}

// ------------------------------------------------------------------ joint
struct HdAxes {
  int nd;
  int bins[4];
  int eoff[4];     // first edge of the axis in the concatenated edges
  int64_t off[4];  // comp[d] * stride_var
};

// One add per lane, after one round of match-and-aggregate: the lanes that
// share the first lane's cell are counted by a ballot and added once by their
// leader (a converged posterior puts most of a wave into one cell; a spread-out
// one loses a ballot and a compare).  cell == ~0u: nothing to add.  Every lane
// of the wave must call this.
template <typename C>
__device__ inline void hd_add(C* cells, uint32_t cell, int lane) {
  const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)cell);
  const bool same = cell == first;
  const unsigned long long m = __ballot(same);
  if (same) {
    if (first != ~0u && lane == __ffsll((long long)m) - 1) atomicAdd(&cells[first], (C)__popcll(m));
  } else if (cell != ~0u) {
    atomicAdd(&cells[cell], (C)1);
  }
}

// A lane owns one sample (c, t) and loads its nd selected components; the
// sample is dropped if any of them is outside its range or NaN (np.histogramdd).
// kLds: cells (uint32) and edges in LDS, flushed with 64-bit integer adds;
// otherwise 64-bit integer adds straight to the result, edges read through the
// caches.  The loop's trip count is uniform over the block (hd_add needs whole waves).
template <typename T, bool kLds>
__global__ __launch_bounds__(kHsBlock) void histdd_kernel(const T* __restrict__ x, HsGeom g, int64_t total,
                                                         int64_t span, HdAxes ax, int n_cells, int n_edges,
                                                         const double* __restrict__ edges,
                                                         unsigned long long* __restrict__ counts) {
  extern __shared__ double hs_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  double* edg = hs_lds;                        // [n_edges]
  uint32_t* cnt = (uint32_t*)(edg + n_edges);  // [n_cells]
  if (kLds) {
    for (int j = tid; j < n_edges; j += kHsBlock) edg[j] = edges[j];
    for (int j = tid; j < n_cells; j += kHsBlock) cnt[j] = 0u;
    __syncthreads();
  }
  const double* e = kLds ? edg : edges;
  double scale[4];
  for (int d = 0; d < 4; ++d)
    scale[d] = d < ax.nd ? (double)ax.bins[d] / (e[ax.eoff[d] + ax.bins[d]] - e[ax.eoff[d]]) : 0.0;
  const int64_t f0 = (int64_t)blockIdx.x * span;
  const int64_t stop = f0 + span;
  const int64_t end = stop < total ? stop : total;
  HsPos p = hs_pos(g, f0 + tid);
  const int64_t dq = kHsBlock / g.inner_n, dr = kHsBlock - dq * g.inner_n;
  for (int64_t base = f0; base < end; base += kHsBlock) {
    uint32_t cell = ~0u;
    if (base + tid < end) {
      const T* a = x + hs_offset(g, p);
      double xv[4];
#pragma unroll
      for (int d = 0; d < 4; ++d)
        if (d < ax.nd) xv[d] = (double)a[ax.off[d]];
      uint32_t acc = 0;
      bool in = true;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        if (d < ax.nd) {
          const int b = hs_bin(e + ax.eoff[d], ax.bins[d], scale[d], xv[d]);
          in = in && b >= 0 && b < ax.bins[d];
          acc = acc * (uint32_t)ax.bins[d] + (uint32_t)(in ? b : 0);
        }
      }
      if (in) cell = acc;
    }
    hs_advance(g, p, dq, dr);
    if (kLds)
      hd_add(cnt, cell, lane);
    else
      hd_add(counts, cell, lane);
  }
  if (kLds) {
    __syncthreads();
    for (int j = tid; j < n_cells; j += kHsBlock)
      if (cnt[j]) atomicAdd(&counts[j], (unsigned long long)cnt[j]);
  }
}

// shared argument checks; 0 = go on, -1 = nothing to do, else the status to return
int hs_check(const char* fn, const void* x, int32_t dtype, int64_t n_chains, int64_t len, int32_t k, int64_t s_chain,
             int64_t s_t, int64_t s_var) {
  if (n_chains < 0 || len < 0 || k < 0 || s_chain < 0 || s_t < 0 || s_var < 0)
    return fail(IPMC_ERR_INVALID, "%s: negative size", fn);
  if (n_chains == 0) return -1;
  if (k < 1 || k > 256) return fail(IPMC_ERR_INVALID, "%s: k = %d outside [1, 256]", fn, k);
  if (const int rc = check_dtype(fn, dtype)) return rc;
  if (!x) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  if ((double)n_chains * (double)(len > 0 ? len : 1) * (double)k > 1e18)
    return fail(IPMC_ERR_INVALID, "%s: more than 1e18 values in one call", fn);
  return 0;
}

// workgroups and elements per workgroup of a histogram pass over `total`
// elements: at most kHsMaxSpan per workgroup (the uint32 bound above)
void hs_grid(int64_t total, int64_t* n_groups, int64_t* span) {
  int64_t n = (total + kHsBlock * 16 - 1) / (kHsBlock * 16);
  n = n < 1 ? 1 : (n > 1024 ? 1024 : n);
  const int64_t need = (total + kHsMaxSpan - 1) / kHsMaxSpan;
  if (n < need) n = need;
  int64_t s = (total + n - 1) / n;
  s = (s + kHsBlock - 1) / kHsBlock * kHsBlock;
  *n_groups = (total + s - 1) / s > 0 ? (total + s - 1) / s : 1;
  *span = s;
}

int hs_zero(const char* fn, void* p, size_t bytes, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(p, 0, bytes, st);
  if (e != hipSuccess) return fail(IPMC_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
  return IPMC_OK;
}

}  // namespace
}  // namespace ipmc

using namespace ipmc;

extern "C" int ipmc_minmax(const void* x, int32_t dtype, int64_t n_chains, int64_t len, int32_t k,
                           int64_t stride_chain, int64_t stride_t, int64_t stride_var, double* min_out,
                           double* max_out, double* scratch, void* stream) {
  int rc = hs_check("ipmc_minmax", x, dtype, n_chains, len, k, stride_chain, stride_t, stride_var);
  if (rc) return rc < 0 ? IPMC_OK : rc;
  if (!min_out || !max_out || !scratch) return fail(IPMC_ERR_INVALID, "ipmc_minmax: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const HsGeom g = hs_geom(n_chains, len, k, stride_chain, stride_t, stride_var);
  double* pmin = scratch;
  double* pmax = scratch + (int64_t)kHsGroups * k;
  int64_t n_groups = 0;
  if (len > 0 && g.var_inner) {
    const int step = kHsBlock / k * k;
    const int64_t total = n_chains * len * k;
    n_groups = (total + (int64_t)step * 16 - 1) / ((int64_t)step * 16);
    n_groups = n_groups > kHsGroups ? kHsGroups : n_groups;
    int64_t span = (total + n_groups - 1) / n_groups;
    span = (span + step - 1) / step * step;  // a multiple of k: a lane keeps its component in every workgroup
    n_groups = (total + span - 1) / span;
    const dim3 grid((unsigned)n_groups), block(kHsBlock);
    with_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      hipLaunchKernelGGL(minmax_inner_kernel<T>, grid, block, 0, st, (const T*)x, g, total, span, (int)k, step, pmin,
                         pmax);
    });
    rc = check_launch("minmax_inner_kernel");
    if (rc) return rc;
  } else if (len > 0) {
    const int64_t nchunk = (len + kMmChunk - 1) / kMmChunk;
    const int64_t units = n_chains * k * nchunk;
    n_groups = (units + 15) / 16;
    n_groups = n_groups > kHsGroups ? kHsGroups : n_groups;
    const int64_t uspan = (units + n_groups - 1) / n_groups;
    n_groups = (units + uspan - 1) / uspan;
    const dim3 grid((unsigned)n_groups), block(kHsBlock);
    with_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      hipLaunchKernelGGL(minmax_outer_kernel<T>, grid, block, 0, st, (const T*)x, g, units, uspan, nchunk, (int)k, pmin,
                         pmax);
    });
    rc = check_launch("minmax_outer_kernel");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(minmax_combine_kernel, dim3((unsigned)k), dim3(kHsBlock), 0, st, pmin, pmax, (int)n_groups, (int)k,
                     min_out, max_out);
  return check_launch("minmax_combine_kernel");
}

extern "C" int ipmc_hist1d(const void* x, int32_t dtype, int64_t n_chains, int64_t len, int32_t k,
                           int64_t stride_chain, int64_t stride_t, int64_t stride_var, int32_t bins,
                           const double* edges, int64_t* counts, int64_t* below, int64_t* above, void* stream) {
  int rc = hs_check("ipmc_hist1d", x, dtype, n_chains, len, k, stride_chain, stride_t, stride_var);
  if (rc) return rc < 0 ? IPMC_OK : rc;
  if (bins < 1 || bins > 4096) return fail(IPMC_ERR_INVALID, "ipmc_hist1d: bins = %d outside [1, 4096]", bins);
  if (!edges || !counts || !below || !above) return fail(IPMC_ERR_INVALID, "ipmc_hist1d: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  {
    const int64_t n = (int64_t)k * bins;  // >= k
    hipLaunchKernelGGL(hist1d_zero_kernel, dim3((unsigned)((n + kHsBlock - 1) / kHsBlock)), dim3(kHsBlock), 0, st,
                       (unsigned long long*)counts, n, (unsigned long long*)below, (unsigned long long*)above, (int)k);
    if ((rc = check_launch("hist1d_zero_kernel"))) return rc;
  }
  const int64_t total = n_chains * len * k;
  if (total == 0) return IPMC_OK;
  const HsGeom g = hs_geom(n_chains, len, k, stride_chain, stride_t, stride_var);
  int kt = kHsCellBudget / (bins + 2);
  kt = kt < 1 ? 1 : (kt > k ? k : kt);
  const int tiles = (k + kt - 1) / kt;
  int copies_log2 = 0;
  while (copies_log2 < 5 && (kt * (bins + 2) << (copies_log2 + 1)) <= kHsCounterBudget) ++copies_log2;
  if (const char* env = getenv("IPMC_HIST_COPIES")) {  // measurement only (tools/posterior_bench.py): fewer copies
    int want = 0;
    while ((1 << (want + 1)) <= atoi(env)) ++want;
    if (want < copies_log2) copies_log2 = want;
  }
  const size_t lds = sizeof(double) * ((size_t)kt * (bins + 1) + kt) +
                     sizeof(uint32_t) * ((size_t)kt * (bins + 2) << copies_log2);
  int64_t n_groups, span;
  hs_grid(total, &n_groups, &span);
  if (n_groups > 0x7fffffff) return fail(IPMC_ERR_INVALID, "ipmc_hist1d: too many values for one call");
  const dim3 grid((unsigned)n_groups, (unsigned)tiles), block(kHsBlock);
  with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    with_bool(g.dense, [&](auto dense) {
      hipLaunchKernelGGL((hist1d_kernel<T, decltype(dense)::value>), grid, block, lds, st, (const T*)x, g, total, span,
                         (int)k, (int)bins, kt, copies_log2, edges, (unsigned long long*)counts,
                         (unsigned long long*)below, (unsigned long long*)above);
    });
  });
  return check_launch("hist1d_kernel");
}

extern "C" int ipmc_histdd(const void* x, int32_t dtype, int64_t n_chains, int64_t len, int32_t k,
                           int64_t stride_chain, int64_t stride_t, int64_t stride_var, int32_t nd,
                           const int32_t* comp, const int32_t* bins, const double* edges, int64_t* counts,
                           void* stream) {
  int rc = hs_check("ipmc_histdd", x, dtype, n_chains, len, k, stride_chain, stride_t, stride_var);
  if (rc) return rc < 0 ? IPMC_OK : rc;
  if (nd < 1 || nd > 4) return fail(IPMC_ERR_INVALID, "ipmc_histdd: nd = %d outside [1, 4]", nd);
  if (!comp || !bins || !edges || !counts) return fail(IPMC_ERR_INVALID, "ipmc_histdd: NULL pointer");
  HdAxes ax;
  ax.nd = nd;
  int64_t n_cells = 1;
  int n_edges = 0;
  for (int d = 0; d < 4; ++d) {
    ax.bins[d] = 1, ax.eoff[d] = 0, ax.off[d] = 0;
    if (d >= nd) continue;
    if (comp[d] < 0 || comp[d] >= k)
      return fail(IPMC_ERR_INVALID, "ipmc_histdd: comp[%d] = %d outside [0, k = %d)", d, comp[d], k);
    if (bins[d] < 1 || bins[d] > 4096)
      return fail(IPMC_ERR_INVALID, "ipmc_histdd: bins = %d outside [1, 4096]", bins[d]);
    ax.bins[d] = bins[d];
    ax.eoff[d] = n_edges;
    ax.off[d] = comp[d] * stride_var;
    n_edges += bins[d] + 1;
    n_cells *= bins[d];  // at most 2^48: no overflow before the check
  }
  if (n_cells > ((int64_t)1 << 24))
    return fail(IPMC_ERR_INVALID, "ipmc_histdd: %lld cells exceed 2^24", (long long)n_cells);
  hipStream_t st = (hipStream_t)stream;
  if ((rc = hs_zero("ipmc_histdd", counts, sizeof(int64_t) * n_cells, st))) return rc;
  const int64_t total = n_chains * len;
  if (total == 0) return IPMC_OK;
  // a lane per sample: the geometry of the samples alone (component 0), time as the inner index
  HsGeom g;
  g.var_inner = 0;
  g.n_chains = n_chains, g.s_chain = stride_chain;
  g.outer_n = 1, g.s_outer = 0;
  g.inner_n = len, g.s_inner = stride_t;
  if (stride_chain == len * stride_t) g.inner_n = n_chains * len, g.n_chains = 1;
  int64_t n_groups, span;
  hs_grid(total, &n_groups, &span);
  if (n_groups > 0x7fffffff) return fail(IPMC_ERR_INVALID, "ipmc_histdd: too many values for one call");
  const bool in_lds = n_cells <= kDdLdsCells && n_edges <= kDdLdsEdges;
  const size_t lds = in_lds ? sizeof(double) * n_edges + sizeof(uint32_t) * n_cells : 0;
  const dim3 grid((unsigned)n_groups), block(kHsBlock);
  with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    with_bool(in_lds, [&](auto cells_in_lds) {
      hipLaunchKernelGGL((histdd_kernel<T, decltype(cells_in_lds)::value>), grid, block, lds, st, (const T*)x, g, total,
                         span, ax, (int)n_cells, n_edges, edges, (unsigned long long*)counts);
    });
  });
  return check_launch(in_lds ? "histdd_kernel (LDS cells)" : "histdd_kernel (global cells)");
}

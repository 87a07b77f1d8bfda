// Pooled second moments between components (covariance.py): ipmc_scatter,
// scatter[b] = Σ (x - c)(x - c)ᵀ and dsum[b] = Σ (x - c) over the rows of
// block b of whole chains, about a centre shared by all rows or about the
// split-chain means of ipmc_split_stats.  A unit of its own, so that every
// other code object of the library stays as it was measured.
//
// Per row the kernel reads 8k bytes and does k(k+1) FLOP: bandwidth at k = 3,
// compute at k = 256.  One design covers both:
//
//   * the k x k result is cut into nt x nt column tiles of width tw <= 64
//     (nt = ceil(k / 64), tw = k / nt rounded up to a multiple of 4: k = 3 is
//     one tile of 4, k = 40 one of 40, k = 256 four of 64); one workgroup per
//     (block, tile pair I >= J) -- only the lower tile pairs are computed;
//   * the centred rows of the one or two tiles go through LDS a slab at a
//     time; the loads of the next slab are in flight (in registers) while the
//     current one is multiplied.  The walk over a slab puts adjacent lanes on
//     adjacent components when the component has the smaller stride (run()'s
//     (C, n, k)) and on adjacent samples otherwise ((C, k, n)), so both
//     layouts are read in dense runs;
//   * a thread keeps a 4 x 4 tile of accumulators (every f64 read from LDS
//     feeds four fused multiply-adds); a tile pair needs P = (tw/4)² of them
//     (a diagonal pair only its lower (tw/4)(tw/4 + 1)/2), and the G = 1024 / P
//     (at most 64) groups of P threads each take every G-th row of the slab;
//   * at the end the groups' accumulators are added in group order through
//     LDS, and each value of the lower triangle is written to [i, j] and
//     [j, i]: the two hold the same bits.
//
// The order of the adds is a function of the arguments alone (tile, slab and
// group sizes follow from k and the strides' order; no atomics), so two calls
// give the same bits.  FP64 vector FMA: on gfx950 the f64 matrix pipe has the
// vector pipe's peak, so v_mfma_f64_16x16x4_f64 would buy no rate here.
#include <cstdlib>

#include "ipmc_internal.hpp"

namespace ipmc {
namespace {

constexpr int kCovThreads = 1024;   // lanes of a workgroup: one workgroup per CU has to keep HBM busy alone
constexpr int kCovMaxGroups = 64;   // groups of threads that split the rows of a slab
constexpr int kCovRedSlots = 256;   // threads whose accumulators go through LDS in one pass of the final sum
constexpr int kCovMaxTile = 64;    // columns of a tile (16 x 16 threads of 4 x 4)
constexpr int kCovMaxRows = 2048;   // rows of a slab at most (their offsets live in LDS)
constexpr int kCovMaxRows256 = 768;  // the same for the 256-lane workgroup, which stays below 64 KiB of LDS
constexpr int kCovRed = 20 * kCovRedSlots;  // doubles of a pass of the final sum: 16 + 4 per thread

struct CovArgs {
  int64_t n_chains, rows_per_chain, half;  // rows used of a chain; first row of the second split chain
  int64_t s_chain, s_t, s_var, block_chains;
  int k, nt, tw, tg;                       // tiles per side, tile width, thread tiles per side (tw / 4)
  int slab_rows, stride;                   // rows of a slab, doubles between its rows in LDS
  int var_inner, collapsed, split;
  int off_b, off_meta;                     // LDS offsets in doubles: second tile, row offsets
};

// thread tile (ti, tj) of index p: row-major over tg x tg, or over the lower triangle (tj <= ti)
__device__ inline void cov_tile_of(int p, bool diag, int tg, int& ti, int& tj) {
  if (diag) {
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= p) ++ti;
    tj = p - ti * (ti + 1) / 2;
  } else {
    ti = p / tg;
    tj = p - ti * tg;
  }
}

// The lane's walk over the rows x w elements of a slab tile, `step` (the
// workgroup's lanes) at a time: `minor` runs fastest (the component when var_inner, else the row).
struct CovWalk {
  int major, minor, dq, dr, ext;
  __device__ CovWalk(int tid, int ext_, int step) : ext(ext_) {
    major = tid / ext, minor = tid - major * ext;
    dq = step / ext, dr = step - dq * ext;
  }
  __device__ void advance() {
    minor += dr, major += dq;
    if (minor >= ext) minor -= ext, ++major;
  }
};

template <typename T, int kT, int kE, bool kPair, bool kDsum>
__global__ __launch_bounds__(kT) void scatter_kernel(const T* __restrict__ x,
                                                             const double* __restrict__ center, CovArgs a,
                                                             double* __restrict__ scatter,
                                                             double* __restrict__ dsum) {
  extern __shared__ __align__(16) double cov_lds[];
  const int tid = threadIdx.x;
  const int npairs = a.nt * (a.nt + 1) / 2;
  const int64_t blk = blockIdx.x / npairs;
  int pair = (int)(blockIdx.x - blk * npairs);
  int I = 0;
  while (pair > I) pair -= I + 1, ++I;
  const int J = pair;
  const bool diag = !kPair || I == J;
  const int vI = I * a.tw, vJ = J * a.tw;
  const int wI = a.k - vI < a.tw ? a.k - vI : a.tw, wJ = a.k - vJ < a.tw ? a.k - vJ : a.tw;
  const int64_t c0 = blk * a.block_chains;
  const int64_t nch = a.n_chains - c0 < a.block_chains ? a.n_chains - c0 : a.block_chains;
  const int64_t rows_total = nch * a.rows_per_chain;
  const int SR = a.slab_rows, stride = a.stride;
  const int64_t n_slabs = (rows_total + SR - 1) / SR;

  double* bufA = cov_lds;
  double* bufB = kPair ? cov_lds + a.off_b : cov_lds;
  int64_t* m_off = (int64_t*)(cov_lds + a.off_meta);  // [2][SR] element offset of a row's component 0
  int32_t* m_ctr = (int32_t*)(m_off + 2 * SR);        // [2][SR] the row's row of `center`

  // the columns past a partial tile's width stay zero: they feed only accumulators that are never written
  for (int j = tid; j < SR * stride; j += kT) {
    bufA[j] = 0.0;
    if (kPair) bufB[j] = 0.0;
  }

  const int P = diag ? a.tg * (a.tg + 1) / 2 : a.tg * a.tg;
  // At most kCovMaxGroups groups: their accumulators are added one after the other at the end, and a
  // tile of one or two threads (k <= 8) has nothing to gain from a thousand of them.
  const int G = kT / P < kCovMaxGroups ? kT / P : kCovMaxGroups;
  const bool active = tid < G * P;
  const int g = tid / P, p = tid - g * P;
  int ti, tj;
  cov_tile_of(p, diag, a.tg, ti, tj);
  const bool dthread = kDsum && diag && active && ti == tj;

  double acc[16], ds[4];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) ds[e] = 0.0;

  auto slab_rows = [&](int64_t s) -> int {
    const int64_t left = rows_total - s * SR;
    return (int)(left < SR ? left : SR);
  };
  // offsets and centre rows of slab s -> meta buffer s & 1
  auto meta = [&](int64_t s) {
    if (s >= n_slabs) return;
    const int rows = slab_rows(s), buf = (int)(s & 1) * SR;
    for (int rl = tid; rl < rows; rl += kT) {
      const int64_t q = s * SR + rl;
      int64_t cc = 0, t = q;
      if (!a.collapsed) {
        if (rows_total <= 0x7fffffff) {
          const uint32_t c32 = (uint32_t)q / (uint32_t)a.rows_per_chain;
          cc = c32, t = (uint32_t)q - c32 * (uint32_t)a.rows_per_chain;
        } else {
          cc = q / a.rows_per_chain, t = q - cc * a.rows_per_chain;
        }
      }
      m_off[buf + rl] = (c0 + cc) * a.s_chain + t * a.s_t;
      m_ctr[buf + rl] = a.split ? (int32_t)((t >= a.half ? a.n_chains : 0) + c0 + cc) : 0;
    }
  };
  double xa[kE], ca[kE], xb[kPair ? kE : 1], cb[kPair ? kE : 1];
  // the walks of a full slab start from the same place every time: their divisions happen once
  const CovWalk walkA(tid, a.var_inner ? wI : SR, kT), walkB(tid, a.var_inner ? wJ : SR, kT);
  auto fetch = [&](int64_t s, int v0, int w, const CovWalk& full, double* xr, double* cr) {
    const int rows = slab_rows(s), buf = (int)(s & 1) * SR, n_el = rows * w;
    CovWalk wk = a.var_inner || rows == SR ? full : CovWalk(tid, rows, kT);
#pragma unroll
    for (int e = 0; e < kE; ++e) {
      xr[e] = 0.0, cr[e] = 0.0;
      if (tid + e * kT < n_el) {
        const int rl = a.var_inner ? wk.major : wk.minor, v = v0 + (a.var_inner ? wk.minor : wk.major);
        xr[e] = (double)x[m_off[buf + rl] + v * a.s_var];
        cr[e] = center[(int64_t)m_ctr[buf + rl] * a.k + v];
      }
      wk.advance();
    }
  };
  auto commit = [&](int64_t s, int w, const CovWalk& full, const double* xr, const double* cr, double* dst) {
    const int rows = slab_rows(s), n_el = rows * w;
    CovWalk wk = a.var_inner || rows == SR ? full : CovWalk(tid, rows, kT);
#pragma unroll
    for (int e = 0; e < kE; ++e) {
      if (tid + e * kT < n_el) {
        const int rl = a.var_inner ? wk.major : wk.minor, v = a.var_inner ? wk.minor : wk.major;
        dst[rl * stride + v] = xr[e] - cr[e];
      }
      wk.advance();
    }
  };

  meta(0);
  __syncthreads();  // also the zeroed tiles
  if (n_slabs > 0) {
    fetch(0, vI, wI, walkA, xa, ca);
    if (kPair && !diag) fetch(0, vJ, wJ, walkB, xb, cb);
  }
  meta(1);
  for (int64_t s = 0; s < n_slabs; ++s) {
    commit(s, wI, walkA, xa, ca, bufA);
    if (kPair && !diag) commit(s, wJ, walkB, xb, cb, bufB);
    __syncthreads();  // slab s is in LDS, and so are the offsets of slab s + 1
    if (s + 1 < n_slabs) {
      fetch(s + 1, vI, wI, walkA, xa, ca);
      if (kPair && !diag) fetch(s + 1, vJ, wJ, walkB, xb, cb);
    }
    if (active) {
      const int rows = slab_rows(s);
      const double* pa = bufA + 4 * ti;
      const double* pb = (diag ? bufA : bufB) + 4 * tj;
#pragma unroll 1
      for (int r = g; r < rows; r += G) {
        const double2 a01 = *(const double2*)(pa + r * stride), a23 = *(const double2*)(pa + r * stride + 2);
        const double2 b01 = *(const double2*)(pb + r * stride), b23 = *(const double2*)(pb + r * stride + 2);
        const double av[4] = {a01.x, a01.y, a23.x, a23.y}, bv[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[4 * i + j] = fma(av[i], bv[j], acc[4 * i + j]);
        if (dthread) {
#pragma unroll
          for (int i = 0; i < 4; ++i) ds[i] += av[i];
        }
      }
    }
    meta(s + 2);      // into the buffer fetch(s) read before the barrier above
    __syncthreads();  // the slab may be overwritten
  }

  // The groups' accumulators in group order, from zero: kCovRedSlots threads at a time put theirs
  // into LDS, and the owner of each result adds the groups of that pass in order to its running sum
  // (the end of the slab loop left a barrier behind: the tiles are free).
  double* red = cov_lds;  // [20][kCovRedSlots]
  constexpr int kItems = 16 * kCovRedSlots / kT > 0 ? 16 * kCovRedSlots / kT : 1;  // results per thread: 16 P <= 4096
  double tot[kItems], totd = 0.0;
#pragma unroll
  for (int j = 0; j < kItems; ++j) tot[j] = 0.0;
  const int used = G * P;
  for (int lo = 0; lo < used; lo += kCovRedSlots) {
    const int hi = lo + kCovRedSlots < used ? lo + kCovRedSlots : used;
    if (lo > 0) __syncthreads();  // the previous pass has been read
    if (tid >= lo && tid < hi) {
#pragma unroll
      for (int e = 0; e < 16; ++e) red[e * kCovRedSlots + tid - lo] = acc[e];
      if (kDsum) {
#pragma unroll
        for (int e = 0; e < 4; ++e) red[(16 + e) * kCovRedSlots + tid - lo] = ds[e];
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      const int w = tid + j * kT;
      if (w < 16 * P) {
        const int e = w / P, p2 = w - e * P;
#pragma unroll 8
        for (int slot = (lo > p2 ? (lo - p2 + P - 1) / P : 0) * P + p2; slot < hi; slot += P)
          tot[j] += red[e * kCovRedSlots + slot - lo];  // in slot order; unrolled so that the reads overlap
      }
    }
    if (kDsum && diag && tid < 4 * a.tg) {
      const int t2 = tid >> 2, pd = t2 * (t2 + 1) / 2 + t2;
#pragma unroll 8
      for (int slot = (lo > pd ? (lo - pd + P - 1) / P : 0) * P + pd; slot < hi; slot += P)
        totd += red[(16 + (tid & 3)) * kCovRedSlots + slot - lo];
    }
  }
  double* out = scatter + blk * (int64_t)a.k * a.k;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int w = tid + j * kT;
    if (w < 16 * P) {
      const int e = w / P, p2 = w - e * P;
      int ti2, tj2;
      cov_tile_of(p2, diag, a.tg, ti2, tj2);
      const int li = 4 * ti2 + (e >> 2), lj = 4 * tj2 + (e & 3);
      const int gi = vI + li, gj = vJ + lj;
      if (li < wI && lj < wJ && gi >= gj) {  // once, then mirrored
        out[(int64_t)gi * a.k + gj] = tot[j];
        out[(int64_t)gj * a.k + gi] = tot[j];
      }
    }
  }
  if (kDsum && diag && tid < 4 * a.tg) {
    const int col = 4 * (tid >> 2) + (tid & 3);
    if (col < wI) dsum[blk * (int64_t)a.k + vI + col] = totd;
  }
}

}  // namespace
}  // namespace ipmc

using namespace ipmc;

extern "C" int ipmc_scatter(const void* x, int32_t dtype, int64_t n_chains, int64_t len, int32_t k,
                            int64_t stride_chain, int64_t stride_t, int64_t stride_var, const double* center,
                            int32_t center_mode, int64_t block_chains, double* scatter_out, double* dsum_out,
                            void* stream) {
  const char* fn = "ipmc_scatter";
  if (n_chains < 0 || len < 0 || k < 0 || stride_chain < 0 || stride_t < 0 || stride_var < 0)
    return fail(IPMC_ERR_INVALID, "%s: negative size", fn);
  if (n_chains == 0) return IPMC_OK;
  if (k < 1 || k > 256) return fail(IPMC_ERR_INVALID, "%s: k = %d outside [1, 256]", fn, k);
  if (const int rc = check_dtype(fn, dtype)) return rc;
  if (center_mode != IPMC_CENTER_SHARED && center_mode != IPMC_CENTER_SPLIT)
    return fail(IPMC_ERR_INVALID, "%s: bad center_mode %d", fn, center_mode);
  if (block_chains < 1) return fail(IPMC_ERR_INVALID, "%s: block_chains = %lld < 1", fn, (long long)block_chains);
  if (!x || !center || !scatter_out) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  const bool split = center_mode == IPMC_CENTER_SPLIT;
  if (len < (split ? 4 : 1))
    return fail(IPMC_ERR_INVALID, "%s: %lld samples per chain; %s", fn, (long long)len,
                split ? "a split chain needs at least 2 (len >= 4)" : "the shared centre needs len >= 1");
  if ((double)n_chains * (double)len * (double)k > 1e18)
    return fail(IPMC_ERR_INVALID, "%s: more than 1e18 values in one call", fn);
  if (2 * n_chains > 0x7fffffff)
    return fail(IPMC_ERR_INVALID, "%s: at most %d chains per call", fn, 0x7fffffff / 2);
  if (block_chains > n_chains) block_chains = n_chains;  // one block: the same sums
  CovArgs a;
  a.n_chains = n_chains;
  a.rows_per_chain = split ? 2 * (len / 2) : len;
  a.half = split ? len / 2 : len;
  a.s_chain = stride_chain, a.s_t = stride_t, a.s_var = stride_var, a.block_chains = block_chains;
  a.k = k;
  a.nt = (k + kCovMaxTile - 1) / kCovMaxTile;
  a.tw = ((k + a.nt - 1) / a.nt + 3) / 4 * 4;
  if (const char* env = getenv("IPMC_COV_TILE")) {  // measurement only (tools/covariance_bench.py): a wider tile
    const int want = atoi(env) / 4 * 4;
    if (a.nt == 1 && want > a.tw && want <= kCovMaxTile) a.tw = want;
  }
  a.tg = a.tw / 4;
  const bool pairs = a.nt > 1;
  int threads = kCovThreads;
  if (const char* env = getenv("IPMC_COV_THREADS")) {  // measurement only: the 256-lane workgroup
    if (atoi(env) == 256) threads = 256;
  }
  // loads of one lane and tile in flight: as many as the register budget of the workgroup size holds without scratch
  const int per_lane = threads != kCovThreads ? 8 : (pairs ? 4 : 6);
  const int max_rows = threads == kCovThreads ? kCovMaxRows : kCovMaxRows256;
  a.slab_rows = threads * per_lane / a.tw < max_rows ? threads * per_lane / a.tw : max_rows;
  a.stride = a.tw + 2;  // 16-byte aligned rows; lanes over time then write 2-way, not 32-way, bank conflicts
  a.var_inner = stride_var <= stride_t;
  a.split = split;
  // chains that follow one another are one long chain (k = 1 series, the M x k array of chain means)
  a.collapsed = !split && stride_chain == len * stride_t;
  const int64_t tile_doubles = (int64_t)a.slab_rows * a.stride;
  a.off_b = (int)tile_doubles;
  int64_t doubles = tile_doubles * (pairs ? 2 : 1);
  if (doubles < kCovRed) doubles = kCovRed;
  a.off_meta = (int)doubles;
  const size_t lds = sizeof(double) * (size_t)doubles + (size_t)a.slab_rows * 2 * (sizeof(int64_t) + sizeof(int32_t));
  const int64_t nb = (n_chains + block_chains - 1) / block_chains;
  const int64_t groups = nb * (a.nt * (a.nt + 1) / 2);
  if (groups > 0x7fffffff) return fail(IPMC_ERR_INVALID, "%s: too many blocks for one call", fn);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)groups), block((unsigned)threads);
  hipError_t attr = hipSuccess;
  // more than 64 KiB of dynamic LDS has to be allowed per kernel
  with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    with_bool(threads == kCovThreads, [&](auto wide) {
      with_bool(pairs, [&](auto pair) {
        with_bool(dsum_out != nullptr, [&](auto ds) {
          constexpr bool kWide = decltype(wide)::value, kPair = decltype(pair)::value;
          // threads and loads per lane and tile: per_lane above
          auto kern = scatter_kernel<T, kWide ? kCovThreads : 256, !kWide ? 8 : (kPair ? 4 : 6), kPair,
                                     decltype(ds)::value>;
          if (lds > 65536)
            attr = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
          if (attr == hipSuccess)
            hipLaunchKernelGGL(kern, grid, block, lds, st, (const T*)x, center, a, scatter_out, dsum_out);
        });
      });
    });
  });
  if (attr != hipSuccess) return fail(IPMC_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(attr));
  return check_launch("scatter_kernel");
}

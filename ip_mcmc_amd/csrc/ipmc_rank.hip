// Pooled sort and rank scores of many chains (ranks.py):
// ipmc_sort_workspace, ipmc_pooled_sort, ipmc_rank_scores.
//
// The sort is a segmented LSD radix sort with 8-bit digits, one segment per
// component, over the order-preserving 64-bit image of the double (-0 and NaN
// canonicalised first) with a 32-bit permutation beside it:
//
//   keys     one pass over the strided samples through a 64 x 64 LDS tile:
//            widen, fold |x - c|, form the key, write keys [k, S] and the
//            identity permutation, and OR key ^ (first key of the segment)
//            into one word per segment (integer OR: any order, same bits)
//   plan     per segment: the passes whose digit is the same for every key
//            (byte of the OR word == 0) are skipped, which fixes the buffer
//            each remaining pass reads (ping-pong between the outputs and the
//            workspace), so the host enqueues all eight passes blindly
//   per pass hist     digit counts of each tile of IPMC_SORT_TILE keys
//            scan     exclusive scan over (digit, tile) inside the segment
//            scatter  stable: a wave owns a quarter of the tile, ranks inside
//                     a round of 64 keys come from wave64 ballots, the counts
//                     of earlier rounds from the wave's own LDS integer counters
//   finish   key -> double into sorted_out, the permutation into perm_out
//
// Every launch depends on the launches before it alone: no workgroup waits or
// spins on another.  Counters are integers; a key's destination is a function
// of the keys alone, so neither the grid nor arrival order reaches a result.
//
// ipmc_rank_scores: one launch.  A workgroup stages 1 024 sorted values in
// LDS; each lane finds its run of equal values by two binary searches in the
// tile, and where the run reaches the tile's edge it continues at the one
// lower / upper bound that lane 0 / lane 64 searched for in the whole segment.
// No lane walks a run.
#include "ipmc_internal.hpp"
#include "ipmc_rng.hpp"

namespace ipmc {
namespace {

constexpr int kSortBlock = 256;
constexpr int kSortTile = IPMC_SORT_TILE;              // keys of one workgroup
constexpr int kSortWaves = kSortBlock / 64;
constexpr int kSortWaveKeys = kSortTile / kSortWaves;  // consecutive keys one wave owns
constexpr int kSortRounds = kSortWaveKeys / 64;        // keys per lane
constexpr int kSortPasses = 8;
constexpr int kKeyTile = 64;      // pooled samples x components of one transposing tile
constexpr int kKeyGroups = 2048;  // workgroups of the key pass along the samples, at most
constexpr int kScanGroups = 4;    // tile ranges scanned side by side (kScanGroups * 256 lanes)
constexpr int kRankTile = 1024;   // sorted values staged by one workgroup of ipmc_rank_scores
constexpr int64_t kMaxPooled = (int64_t)1 << 32;

// plan[pass * k + v]: bit 0 = the pass is skipped for segment v, bit 1 = the
// pass reads the workspace buffers (else the output buffers);
// plan[kSortPasses * k + v] bit 1: where the sorted keys of v ended.
constexpr uint8_t kPlanSkip = 1, kPlanInB = 2;

__device__ inline uint64_t sort_key(double x) {
  if (x != x) return 0xFFF8000000000000ull;  // every NaN: one key above +inf's 0xFFF0...
  const uint64_t b = x == 0.0 ? 0ull : __builtin_bit_cast(uint64_t, x);  // -0 -> +0
  return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}

__device__ inline double sort_value(uint64_t key) {
  const uint64_t b = (key >> 63) ? key ^ 0x8000000000000000ull : ~key;
  return __builtin_bit_cast(double, b);
}

// The lanes of the wave that hold the same digit as this one (valid lanes
// only; unspecified for an invalid lane).  Every lane of the wave calls it.
__device__ inline unsigned long long digit_peers(uint32_t d, bool valid) {
  unsigned long long peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long m = __ballot(valid && bit);
    peers &= bit ? m : ~m;
  }
  return peers;
}

// ------------------------------------------------------------------- keys
// Workgroup (bx, by): components [by * 64, +64) of the pooled samples of the
// tiles bx, bx + gridDim.x, ...  The load runs along the dimension of the
// smaller stride, the store along the pooled index.
template <typename T>
__global__ __launch_bounds__(kSortBlock) void sort_keys_kernel(const T* __restrict__ x, int64_t len, int64_t S, int k,
                                                              int64_t s_chain, int64_t s_t, int64_t s_var,
                                                              int var_inner, const double* __restrict__ center,
                                                              uint64_t* __restrict__ keys, uint32_t* __restrict__ perm,
                                                              unsigned long long* __restrict__ kdiff) {
  __shared__ uint64_t tile[kKeyTile][kKeyTile + 1];  // [component][sample]
  __shared__ uint64_t sref[kKeyTile], sdiff[kKeyTile];
  __shared__ double scen[kKeyTile];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int v0 = (int)blockIdx.y * kKeyTile;
  const int tv = (k - v0) < kKeyTile ? (k - v0) : kKeyTile;
  if (tid < tv) {
    const double c = center ? center[v0 + tid] : 0.0;
    double x0 = (double)x[(int64_t)(v0 + tid) * s_var];  // pooled sample 0
    if (center) x0 = fabs(x0 - c);
    scen[tid] = c;
    sref[tid] = sort_key(x0);
    sdiff[tid] = 0;
  }
  __syncthreads();
  const int64_t n_tiles = (S + kKeyTile - 1) / kKeyTile;
  for (int64_t pt = blockIdx.x; pt < n_tiles; pt += gridDim.x) {
    const int64_t p0 = pt * kKeyTile;
    const int tp = (S - p0) < kKeyTile ? (int)(S - p0) : kKeyTile;
    for (int e = tid; e < tv * tp; e += kSortBlock) {
      int vl, pl;
      if (var_inner) {
        pl = e / tv, vl = e - pl * tv;
      } else {
        vl = e / tp, pl = e - vl * tp;
      }
      const int64_t p = p0 + pl;
      const int64_t c = p / len, t = p - c * len;
      double xv = (double)x[c * s_chain + t * s_t + (int64_t)(v0 + vl) * s_var];
      if (center) xv = fabs(xv - scen[vl]);
      tile[vl][pl] = sort_key(xv);
    }
    __syncthreads();
    for (int vl = wave; vl < tv; vl += kSortBlock / 64) {  // component vl belongs to wave vl % 4 throughout
      uint64_t d = 0;
      if (lane < tp) {
        const uint64_t key = tile[vl][lane];
        const int64_t at = (int64_t)(v0 + vl) * S + p0 + lane;
        keys[at] = key;
        perm[at] = (uint32_t)(p0 + lane);
        d = key ^ sref[vl];
      }
      for (int off = 32; off > 0; off >>= 1) d |= __shfl_xor(d, off);
      if (lane == 0) sdiff[vl] |= d;
    }
    __syncthreads();
  }
  if (tid < tv && sdiff[tid]) atomicOr(&kdiff[v0 + tid], (unsigned long long)sdiff[tid]);
}

__global__ __launch_bounds__(kSortBlock) void sort_plan_kernel(const unsigned long long* __restrict__ kdiff, int k,
                                                              uint8_t* __restrict__ plan) {
  const int v = (int)blockIdx.x * kSortBlock + threadIdx.x;
  if (v >= k) return;
  const unsigned long long d = kdiff[v];
  uint8_t in_b = 0;
  for (int p = 0; p < kSortPasses; ++p) {
    const bool skip = ((d >> (8 * p)) & 0xffull) == 0;
    plan[p * k + v] = (uint8_t)((skip ? kPlanSkip : 0) | in_b);
    if (!skip) in_b ^= kPlanInB;
  }
  plan[kSortPasses * k + v] = in_b;
}

// --------------------------------------------------------------- one pass
// tilehist [k, n_tiles, 256]: the digit counts of a tile, then (scan) the
// first destination of each digit of the tile inside the segment.
__global__ __launch_bounds__(kSortBlock) void sort_hist_kernel(const uint64_t* __restrict__ keys_a,
                                                              const uint64_t* __restrict__ keys_b, int64_t S, int k,
                                                              int pass, const uint8_t* __restrict__ plan,
                                                              uint32_t* __restrict__ tilehist, int64_t n_tiles) {
  __shared__ uint32_t cnt[256];
  const int v = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint8_t flags = plan[pass * k + v];
  if (flags & kPlanSkip) return;
  const uint64_t* src = ((flags & kPlanInB) ? keys_b : keys_a) + (int64_t)v * S;
  cnt[tid] = 0;
  __syncthreads();
  const int64_t first = (int64_t)blockIdx.x * kSortTile + wave * kSortWaveKeys + lane;
#pragma unroll 4
  for (int r = 0; r < kSortRounds; ++r) {
    const int64_t at = first + r * 64;
    const bool valid = at < S;
    const uint64_t key = valid ? src[at] : 0;
    const uint32_t d = (uint32_t)(key >> (8 * pass)) & 255u;
    const unsigned long long peers = digit_peers(d, valid);
    if (valid && lane == 63 - __clzll((long long)peers)) atomicAdd(&cnt[d], (uint32_t)__popcll(peers));
  }
  __syncthreads();
  tilehist[((int64_t)v * n_tiles + blockIdx.x) * 256 + tid] = cnt[tid];
}

// One workgroup per segment.  Lane (g, d) owns digit d over the g-th quarter
// of the tiles; the destinations ascend by digit, then by tile.
__global__ __launch_bounds__(kScanGroups * 256) void sort_scan_kernel(uint32_t* __restrict__ tilehist,
                                                                     int64_t n_tiles, int k, int pass,
                                                                     const uint8_t* __restrict__ plan) {
  __shared__ uint32_t part[kScanGroups][256];
  __shared__ uint32_t first[256];
  __shared__ uint32_t wtot[4];
  const int v = blockIdx.x, tid = threadIdx.x, d = tid & 255, g = tid >> 8;
  if (plan[pass * k + v] & kPlanSkip) return;
  uint32_t* h = tilehist + (int64_t)v * n_tiles * 256;
  const int64_t per = (n_tiles + kScanGroups - 1) / kScanGroups;
  const int64_t i0 = g * per < n_tiles ? g * per : n_tiles;
  const int64_t i1 = i0 + per < n_tiles ? i0 + per : n_tiles;
  uint32_t s = 0;
#pragma unroll 8
  for (int64_t i = i0; i < i1; ++i) s += h[i * 256 + d];
  part[g][d] = s;
  __syncthreads();
  // exclusive sums of the digits' totals: lanes 0..255 (four whole waves), shuffles inside a wave,
  // then the waves' totals, as sort_scatter_kernel does for the digits of a tile
  uint32_t tot = 0, incl = 0;
  if (tid < 256) {
    for (int q = 0; q < kScanGroups; ++q) tot += part[q][tid];
    incl = tot;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = __shfl_up(incl, off);
      if ((tid & 63) >= off) incl += up;
    }
    if ((tid & 63) == 63) wtot[tid >> 6] = incl;
  }
  __syncthreads();
  if (tid < 256) {
    uint32_t base = 0;
    for (int w = 0; w < (tid >> 6); ++w) base += wtot[w];
    first[tid] = base + incl - tot;
  }
  __syncthreads();
  uint32_t run = first[d];
  for (int q = 0; q < g; ++q) run += part[q][d];
  for (int64_t i = i0; i < i1; ++i) {
    const uint32_t c = h[i * 256 + d];
    h[i * 256 + d] = run;
    run += c;
  }
}

// Stable scatter of one tile.  Order inside the tile = (wave, round, lane) =
// ascending index.  A key's destination is
//   tilehist[tile][d]                       first destination of digit d of this tile
//   + keys of digit d in the earlier waves  (wcnt, after the barrier)
//   + those in this wave's earlier rounds   (the value the wave's counter held)
//   + those in lower lanes of this round    (ballots)
// The counter of (wave, d) is touched by that wave alone, one lane per round.
// The last three terms are the key's rank among the tile's keys of digit d;
// with the digits' first positions in the tile (an exclusive sum over the 256
// counts) that is its place in the tile sorted by digit, and the tile is
// stored from LDS in that order: first the keys, then the indices.
__global__ __launch_bounds__(kSortBlock) void sort_scatter_kernel(uint64_t* __restrict__ keys_a,
                                                                 uint64_t* __restrict__ keys_b,
                                                                 uint32_t* __restrict__ perm_a,
                                                                 uint32_t* __restrict__ perm_b, int64_t S, int k,
                                                                 int pass, const uint8_t* __restrict__ plan,
                                                                 const uint32_t* __restrict__ tilehist,
                                                                 int64_t n_tiles) {
  __shared__ uint64_t lkeys[kSortTile];  // the tile in destination order; afterwards its indices, as uint32
  __shared__ uint32_t wcnt[kSortWaves][256];
  __shared__ uint32_t dstart[256];  // first position of digit d in the reordered tile
  __shared__ uint32_t gfirst[256];  // first destination of digit d of this tile in the segment
  __shared__ uint32_t wtot[kSortWaves];
  const int v = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint8_t flags = plan[pass * k + v];
  if (flags & kPlanSkip) return;
  const bool in_b = flags & kPlanInB;
  const int64_t seg = (int64_t)v * S;
  const uint64_t* ksrc = (in_b ? keys_b : keys_a) + seg;
  const uint32_t* psrc = (in_b ? perm_b : perm_a) + seg;
  uint64_t* kdst = (in_b ? keys_a : keys_b) + seg;
  uint32_t* pdst = (in_b ? perm_a : perm_b) + seg;
  for (int w = 0; w < kSortWaves; ++w) wcnt[w][tid] = 0;
  gfirst[tid] = tilehist[((int64_t)v * n_tiles + blockIdx.x) * 256 + tid];  // digit tid
  const int64_t tile0 = (int64_t)blockIdx.x * kSortTile;
  const int count = (S - tile0) < kSortTile ? (int)(S - tile0) : kSortTile;
  const int64_t first = tile0 + wave * kSortWaveKeys + lane;
  uint64_t key[kSortRounds];
  uint32_t prm[kSortRounds], pre[kSortRounds];
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const int64_t at = first + r * 64;
    const bool valid = at < S;
    key[r] = valid ? ksrc[at] : 0;
    prm[r] = valid ? psrc[at] : 0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const bool valid = first + r * 64 < S;
    const uint32_t d = (uint32_t)(key[r] >> (8 * pass)) & 255u;
    const unsigned long long peers = digit_peers(d, valid);
    const int lead = valid ? 63 - __clzll((long long)peers) : lane;
    uint32_t before = 0;
    if (valid && lane == lead) before = atomicAdd(&wcnt[wave][d], (uint32_t)__popcll(peers));
    before = __shfl(before, lead);
    pre[r] = before + (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
  }
  __syncthreads();
  {
    // lane d: the counts of digit d per wave -> their exclusive sums over the waves, and the tile's
    // count of d -> dstart[d], its exclusive sum over the digits (shuffles in the wave, then the waves)
    uint32_t run = 0;
    for (int w = 0; w < kSortWaves; ++w) {
      const uint32_t c = wcnt[w][tid];
      wcnt[w][tid] = run;
      run += c;
    }
    uint32_t incl = run;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = __shfl_up(incl, off);
      if (lane >= off) incl += up;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; ++w) base += wtot[w];
    dstart[tid] = base + incl - run;
  }
  __syncthreads();
  // The tile goes through LDS in destination order, so that a wave's stores are a few dense runs (one
  // per digit) and not 64 single keys.  pre[r] becomes the key's position in the reordered tile.
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    if (first + r * 64 < S) {
      const uint32_t d = (uint32_t)(key[r] >> (8 * pass)) & 255u;
      const uint32_t at = dstart[d] + wcnt[wave][d] + pre[r];
      pre[r] = at;
      if (at < (uint32_t)count) lkeys[at] = key[r];  // always, when the counts are those of these keys
    }
  }
  __syncthreads();
  uint32_t to[kSortRounds];  // destination in the segment of the key at position tid + 256 j of the reordered tile
#pragma unroll
  for (int j = 0; j < kSortRounds; ++j) {
    const int i = tid + j * kSortBlock;
    to[j] = 0xffffffffu;
    if (i < count) {
      const uint64_t key_i = lkeys[i];
      const uint32_t d = (uint32_t)(key_i >> (8 * pass)) & 255u;
      to[j] = gfirst[d] + ((uint32_t)i - dstart[d]);
      if ((int64_t)to[j] < S) kdst[to[j]] = key_i;
    }
  }
  __syncthreads();
  uint32_t* lperm = (uint32_t*)lkeys;
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r)
    if (first + r * 64 < S && pre[r] < (uint32_t)count) lperm[pre[r]] = prm[r];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kSortRounds; ++j) {
    const int i = tid + j * kSortBlock;
    if (i < count && (int64_t)to[j] < S) pdst[to[j]] = lperm[i];
  }
}

__global__ __launch_bounds__(kSortBlock) void sort_finish_kernel(const uint64_t* keys_a, const uint64_t* __restrict__ keys_b,
                                                                const uint32_t* __restrict__ perm_b, int64_t S, int k,
                                                                const uint8_t* __restrict__ plan, double* sorted_out,
                                                                uint32_t* __restrict__ perm_out) {
  const int v = blockIdx.y;
  const bool in_b = plan[kSortPasses * k + v] & kPlanInB;
  const int64_t seg = (int64_t)v * S;
  for (int64_t j = (int64_t)blockIdx.x * kSortBlock + threadIdx.x; j < S; j += (int64_t)gridDim.x * kSortBlock) {
    const uint64_t key = in_b ? keys_b[seg + j] : keys_a[seg + j];  // keys_a is sorted_out: read, then written, by this lane
    sorted_out[seg + j] = sort_value(key);
    if (in_b) perm_out[seg + j] = perm_b[seg + j];
  }
}

// ------------------------------------------------------------ rank scores
__global__ __launch_bounds__(kSortBlock) void rank_scores_kernel(const double* __restrict__ sorted,
                                                                const uint32_t* __restrict__ perm, int64_t S,
                                                                int64_t len, int mode, double* __restrict__ out,
                                                                int64_t o_chain, int64_t o_t, int64_t o_var) {
  __shared__ double s[kRankTile];
  __shared__ int64_t edge[2];
  const int v = blockIdx.y, tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * kRankTile;
  const int cnt = (S - t0) < kRankTile ? (int)(S - t0) : kRankTile;
  const double* row = sorted + (int64_t)v * S;
  for (int j = tid; j < cnt; j += kSortBlock) s[j] = row[t0 + j];
  __syncthreads();
  if (tid == 0) {  // the first position in the segment of the value the tile begins with
    const double x = s[0];
    int64_t lo = 0, hi = t0;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (row[mid] < x) lo = mid + 1; else hi = mid;
    }
    edge[0] = lo;
  }
  if (tid == 64) {  // one past the last position of the value the tile ends with (NaN counts as larger)
    const double x = s[cnt - 1];
    int64_t lo = t0 + cnt, hi = S;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (row[mid] <= x) lo = mid + 1; else hi = mid;
    }
    edge[1] = lo;
  }
  __syncthreads();
  const double denom = (double)S + 0.25;
  for (int j = tid; j < cnt; j += kSortBlock) {
    const double x = s[j];
    const int64_t p = perm[(int64_t)v * S + t0 + j];
    if (p >= S) continue;  // not a pooled index: nothing of the caller's is addressed
    const int64_t c = p / len, t = p - c * len;
    double* o = out + c * o_chain + t * o_t + (int64_t)v * o_var;
    if (x != x) {
      *o = NAN;
      continue;
    }
    int lo = 0, hi = j;  // s[j] == x: the first equal value is at or before j
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s[mid] < x) lo = mid + 1; else hi = mid;
    }
    const int64_t a = lo == 0 ? edge[0] : t0 + lo;
    int lo2 = j + 1, hi2 = cnt;
    while (lo2 < hi2) {
      const int mid = (lo2 + hi2) >> 1;
      if (s[mid] <= x) lo2 = mid + 1; else hi2 = mid;
    }
    const int64_t b = (lo2 == cnt ? edge[1] : t0 + lo2) - 1;
    const double r = (double)(a + b) * 0.5 + 1.0;  // a + b < 2^33: exact
    *o = mode == 0 ? r : det_ppnd16((r - 0.375) / denom);
  }
}

int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

struct SortLayout {
  int64_t n_tiles;
  int64_t keys, perm, hist, diff, plan;  // byte offsets into the workspace
  int64_t bytes;
};

SortLayout sort_layout(int64_t S, int k) {
  SortLayout w;
  w.n_tiles = (S + kSortTile - 1) / kSortTile;
  if (w.n_tiles < 1) w.n_tiles = 1;
  int64_t at = 0;
  w.keys = at, at += align256((int64_t)k * S * 8);
  w.perm = at, at += align256((int64_t)k * S * 4);
  w.hist = at, at += align256((int64_t)k * w.n_tiles * 256 * 4);
  w.diff = at, at += align256((int64_t)k * 8);
  w.plan = at, at += align256((int64_t)k * (kSortPasses + 1));
  w.bytes = at;
  return w;
}

// shared argument checks; 0 = go on, -1 = nothing to do, else the status to return
int rank_check(const char* fn, int64_t n_chains, int64_t len, int32_t k, bool negative_other) {
  if (n_chains < 0 || len < 0 || k < 0 || negative_other) return fail(IPMC_ERR_INVALID, "%s: negative size", fn);
  if (n_chains == 0) return -1;
  if (k < 1 || k > 256) return fail(IPMC_ERR_INVALID, "%s: k = %d outside [1, 256]", fn, k);
  return 0;
}

int pooled_check(const char* fn, int64_t n_chains, int64_t len) {
  if (len > 0 && n_chains > (kMaxPooled - 1) / len)
    return fail(IPMC_ERR_INVALID,
                "%s: n_chains * len = %.0f pooled samples per component, the 32-bit permutation holds fewer than 2^32",
                fn, (double)n_chains * (double)len);
  return 0;
}

}  // namespace
}  // namespace ipmc

using namespace ipmc;

extern "C" int ipmc_sort_workspace(int64_t n_chains, int64_t len, int32_t k, int32_t dtype, int64_t* bytes_out) {
  int rc = rank_check("ipmc_sort_workspace", n_chains, len, k, false);
  if (rc > 0) return rc;
  if (rc == 0 && (rc = check_dtype("ipmc_sort_workspace", dtype))) return rc;
  if (!bytes_out) return fail(IPMC_ERR_INVALID, "ipmc_sort_workspace: NULL pointer");
  if (n_chains == 0) {
    *bytes_out = 0;
    return IPMC_OK;
  }
  if ((rc = pooled_check("ipmc_sort_workspace", n_chains, len))) return rc;
  *bytes_out = sort_layout(n_chains * len, k).bytes;
  return IPMC_OK;
}

extern "C" int ipmc_pooled_sort(const void* x, int32_t dtype, int64_t n_chains, int64_t len, int32_t k,
                                int64_t stride_chain, int64_t stride_t, int64_t stride_var,
                                const double* fold_center, double* sorted_out, uint32_t* perm_out, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  const char* fn = "ipmc_pooled_sort";
  int rc = rank_check(fn, n_chains, len, k, stride_chain < 0 || stride_t < 0 || stride_var < 0 || workspace_bytes < 0);
  if (rc) return rc < 0 ? IPMC_OK : rc;
  if ((rc = check_dtype(fn, dtype))) return rc;
  if (!x || !sorted_out || !perm_out || !workspace) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  if ((rc = pooled_check(fn, n_chains, len))) return rc;
  const int64_t S = n_chains * len;
  const SortLayout w = sort_layout(S, k);
  if (workspace_bytes < w.bytes)
    return fail(IPMC_ERR_INVALID, "%s: workspace of %lld bytes, ipmc_sort_workspace asks for %lld", fn,
                (long long)workspace_bytes, (long long)w.bytes);
  if (S == 0) return IPMC_OK;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint64_t* keys_a = (uint64_t*)sorted_out;
  uint64_t* keys_b = (uint64_t*)(ws + w.keys);
  uint32_t* perm_b = (uint32_t*)(ws + w.perm);
  uint32_t* tilehist = (uint32_t*)(ws + w.hist);
  unsigned long long* kdiff = (unsigned long long*)(ws + w.diff);
  uint8_t* plan = (uint8_t*)(ws + w.plan);
  const hipError_t e = hipMemsetAsync(kdiff, 0, sizeof(unsigned long long) * k, st);
  if (e != hipSuccess) return fail(IPMC_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
  const dim3 block(kSortBlock);
  {
    int64_t groups = (S + kKeyTile - 1) / kKeyTile;
    if (groups > kKeyGroups) groups = kKeyGroups;
    const dim3 grid((unsigned)groups, (unsigned)((k + kKeyTile - 1) / kKeyTile));
    const int var_inner = stride_var <= stride_t;
    with_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      hipLaunchKernelGGL(sort_keys_kernel<T>, grid, block, 0, st, (const T*)x, len, S, (int)k, stride_chain, stride_t,
                         stride_var, var_inner, fold_center, keys_a, perm_out, kdiff);
    });
    if ((rc = check_launch("sort_keys_kernel"))) return rc;
  }
  hipLaunchKernelGGL(sort_plan_kernel, dim3((unsigned)((k + kSortBlock - 1) / kSortBlock)), block, 0, st, kdiff, (int)k,
                     plan);
  if ((rc = check_launch("sort_plan_kernel"))) return rc;
  const dim3 tiles((unsigned)w.n_tiles, (unsigned)k);
  for (int pass = 0; pass < kSortPasses; ++pass) {
    hipLaunchKernelGGL(sort_hist_kernel, tiles, block, 0, st, keys_a, keys_b, S, (int)k, pass, plan, tilehist,
                       w.n_tiles);
    if ((rc = check_launch("sort_hist_kernel"))) return rc;
    hipLaunchKernelGGL(sort_scan_kernel, dim3((unsigned)k), dim3(kScanGroups * 256), 0, st, tilehist, w.n_tiles, (int)k,
                       pass, plan);
    if ((rc = check_launch("sort_scan_kernel"))) return rc;
    hipLaunchKernelGGL(sort_scatter_kernel, tiles, block, 0, st, keys_a, keys_b, perm_out, perm_b, S, (int)k, pass, plan,
                       tilehist, w.n_tiles);
    if ((rc = check_launch("sort_scatter_kernel"))) return rc;
  }
  {
    int64_t groups = (S + kSortBlock * 8 - 1) / (kSortBlock * 8);
    if (groups > 4096) groups = 4096;
    hipLaunchKernelGGL(sort_finish_kernel, dim3((unsigned)groups, (unsigned)k), block, 0, st, keys_a, keys_b, perm_b, S,
                       (int)k, plan, sorted_out, perm_out);
  }
  return check_launch("sort_finish_kernel");
}

extern "C" int ipmc_rank_scores(const double* sorted, const uint32_t* perm, int32_t k, int64_t n_chains, int64_t len,
                                int32_t mode, double* out, int64_t out_stride_chain, int64_t out_stride_t,
                                int64_t out_stride_var, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* fn = "ipmc_rank_scores";
  (void)workspace;  // none is needed: the runs are found inside the one launch
  int rc = rank_check(fn, n_chains, len, k,
                      out_stride_chain < 0 || out_stride_t < 0 || out_stride_var < 0 || workspace_bytes < 0);
  if (rc) return rc < 0 ? IPMC_OK : rc;
  if (mode != 0 && mode != 1)
    return fail(IPMC_ERR_INVALID, "%s: mode = %d is neither 0 (average rank) nor 1 (normal score)", fn, mode);
  if (!sorted || !perm || !out) return fail(IPMC_ERR_INVALID, "%s: NULL pointer", fn);
  if ((rc = pooled_check(fn, n_chains, len))) return rc;
  const int64_t S = n_chains * len;
  if (S == 0) return IPMC_OK;
  const dim3 grid((unsigned)((S + kRankTile - 1) / kRankTile), (unsigned)k);
  hipLaunchKernelGGL(rank_scores_kernel, grid, dim3(kSortBlock), 0, (hipStream_t)stream, sorted, perm, S, len, (int)mode,
                     out, out_stride_chain, out_stride_t, out_stride_var);
  return check_launch("rank_scores_kernel");
}

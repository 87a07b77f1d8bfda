"""Geometry and fixtures for the chain analytics past one tile, chunk and grid pass
(tests/test_analytics_tiles_cpu.py, tests/test_gpu_rank_tiles.py,
tests/test_gpu_posterior_tiles.py).  Pure numpy; not collected.

The geometry functions restate how ip_mcmc_amd/csrc/ipmc_rank.hip and
ip_mcmc_amd/csrc/ipmc_hist.hip (the line numbers below are theirs) cut their
inputs into tiles, chunks and capped grids, so that a test can assert about its
own input that it reaches the loop, seam or cap it was built for.  When one of
these assertions fails, the restatement (or the shape) is stale: re-derive it from
the kernel.  That says nothing about whether the kernel is right.
"""
import numpy as np

from ip_mcmc_amd import _abi
from ip_mcmc_amd.posterior import MINMAX_GROUPS  # IPMC_MINMAX_GROUPS: workgroups of a minmax pass, at most

T = _abi.SORT_TILE   # keys of one workgroup's tile of the sort (IPMC_SORT_TILE)
SCAN_GROUPS = 4      # kScanGroups, ipmc_rank.hip:46
KEY_TILE = 64        # kKeyTile, ipmc_rank.hip:44
KEY_GROUPS = 2048    # kKeyGroups, ipmc_rank.hip:45
RANK_TILE = 1024     # kRankTile, ipmc_rank.hip:47
MM_CHUNK = 16384     # kMmChunk, ipmc_hist.hip:33
HS_BLOCK = 256       # kHsBlock, ipmc_hist.hip:20
HS_MAX_SPAN = 1 << 31  # kHsMaxSpan, ipmc_hist.hip:28
HS_GROUPS = 1024     # the cap inside hs_grid, ipmc_hist.hip:495
# HS_GROUPS and MINMAX_GROUPS are two names on purpose: the kernels keep the two caps apart too (a literal in
# hs_grid for the histograms, IPMC_MINMAX_GROUPS for the minmax partials), though both are 1 024 today.

S_BIG = KEY_GROUPS * KEY_TILE + 3 * KEY_TILE + 5  # 131 269: the key pass takes a second grid-stride step
SORT_SIZES = {  # pooled size -> sort tiles of each of the four lane groups of sort_scan_kernel
    4 * T + 1: [2, 2, 1, 0],
    6 * T: [2, 2, 2, 0],
    7 * T - 1: [2, 2, 2, 1],
    8 * T + 1: [3, 3, 3, 0],
    9 * T + 5: [3, 3, 3, 1],
    16 * T + 3: [5, 5, 5, 2],
    S_BIG: [9, 9, 9, 6],
}
SEAM_S = 5 * RANK_TILE + 304  # 5 424 pooled samples: five whole tiles of the rank scores and a short sixth
SEAM_SHAPE = (6, 904)         # (C, n) with C n = SEAM_S and n even: every sample is used
LONG_SHAPE = (2, 3, 40000)    # (C, k, n): three chunks of a row, the last of 7 232 samples
ROWS_SHAPE = (70, 16, 256)    # (C, n, k): 17 920 rows of one chunk, more than 16 to a workgroup
CAP_SHAPE = (64, 23500, 3)    # (C, n, k): 4 512 000 elements, more than 1 024 workgroups of 4 096
TIED_CONVERGENCE = ((40, 300, 3), 47)  # shape and seed of the tied rank_convergence fixture of three tiles
QUANTILES = [0.0, 0.05, 1 / 3, 0.5, 0.95, 1.0]


def _ceil(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ geometry
def scan_groups(S):
    """Sort tiles of each lane group of sort_scan_kernel (ipmc_rank.hip:192-194)."""
    n_tiles = max(_ceil(S, T), 1)
    per = _ceil(n_tiles, SCAN_GROUPS)
    out = []
    for g in range(SCAN_GROUPS):
        i0 = min(g * per, n_tiles)
        out.append(min(i0 + per, n_tiles) - i0)
    return out


def key_iterations(S):
    """Sample tiles that workgroup 0 of sort_keys_kernel takes (ipmc_rank.hip:104-105, 528-529)."""
    n_tiles = _ceil(S, KEY_TILE)
    return _ceil(n_tiles, min(n_tiles, KEY_GROUPS))


def rank_tiles(S):
    """Workgroups of rank_scores_kernel per component (ipmc_rank.hip:582)."""
    return _ceil(S, RANK_TILE)


def minmax_outer_geometry(C, k, n):
    """(nchunk, units, uspan, workgroups) of minmax_outer_kernel (ipmc_hist.hip:549-554)."""
    nchunk = _ceil(n, MM_CHUNK)
    units = C * k * nchunk
    groups = min(_ceil(units, 16), MINMAX_GROUPS)
    uspan = _ceil(units, groups)
    return nchunk, units, uspan, _ceil(units, uspan)


def hs_grid(total):
    """(workgroups, span) of a histogram pass over `total` elements (ipmc_hist.hip:493-502)."""
    n = min(max(_ceil(total, HS_BLOCK * 16), 1), HS_GROUPS)
    n = max(n, _ceil(total, HS_MAX_SPAN))
    span = _ceil(_ceil(total, n), HS_BLOCK) * HS_BLOCK
    return max(_ceil(total, span), 1), span


def minmax_inner_grid(total, k):
    """(workgroups, span) of minmax_inner_kernel (ipmc_hist.hip:533-539)."""
    step = HS_BLOCK // k * k
    n = min(_ceil(total, step * 16), MINMAX_GROUPS)
    span = _ceil(_ceil(total, n), step) * step
    return _ceil(total, span), span


# ------------------------------------------------------------------ the sort
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310,
                     -1e-310])


def sort_columns(S, seed):
    """(S, 2) float64, read-only.
    Column 0: normal · exp(6 · normal), both signs and 20 binary orders of magnitude: all 8 passes run.
    About 1 % of the entries are copies of other entries (ties); where S allows, two of each of SPECIALS.
    Column 1: (8 + 0.01 · normal) rounded to f32 and widened: passes 3 to 6 run, 0 to 2 and 7 are skipped."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=S) * np.exp(6.0 * rng.normal(size=S))
    m = S // 100
    if m:
        dst = rng.choice(S, size=m, replace=False)
        a[dst] = a[rng.integers(0, S, size=m)]
    if S >= 20 * len(SPECIALS):
        where = rng.choice(S, size=2 * len(SPECIALS), replace=False)
        a[where] = np.tile(SPECIALS, 2)
    b = (8.0 + 0.01 * rng.normal(size=S)).astype(np.float32).astype(np.float64)
    x = np.stack([a, b], axis=1)
    x.setflags(write=False)
    return x


def low_byte_column(S, seed):
    """(S,) float64 whose keys differ in the lowest byte alone: one running pass, so the sorted segment
    ends in the other buffer than one of an even number of passes (the plan of ipmc_rank.hip:139-151)."""
    rng = np.random.default_rng(seed)
    return (np.uint64(0x4020000000000000) + rng.integers(0, 256, size=S).astype(np.uint64)).view(np.float64)


def lone_bit_column(S):
    """(S,) float64, constant but for two samples: one in the first sample tile of workgroup 0 of the key
    pass differs in key byte 0, one in its second tile (KEY_GROUPS tiles on) in key byte 1.  No other
    workgroup sees either difference, so passes 0 and 1 run only if workgroup 0 keeps what both of its
    grid-stride steps found (sdiff |= d, ipmc_rank.hip:132)."""
    assert key_iterations(S) == 2 and S > KEY_GROUPS * KEY_TILE + 7
    bits = np.full(S, 8.0).view(np.uint64)
    bits[5] += np.uint64(1)
    bits[KEY_GROUPS * KEY_TILE + 7] += np.uint64(0x100)
    return bits.view(np.float64)


# ------------------------------------------------------------ the rank seams
SEAM_RUNS = {"minus_one": RANK_TILE, "half": 2 * RANK_TILE + 7, "nan": 1500, "below_nan": 200}


def seam_sorted(seed):
    """(SEAM_S, 5) float64: the five columns of seam_columns in ascending order (NaN last)."""
    rng = np.random.default_rng(seed)
    S = SEAM_S
    cols = [np.full(S, 8.25)]
    a, b = SEAM_RUNS["minus_one"], SEAM_RUNS["half"]
    above = np.sort(1.0 + rng.random(S - a - b))
    cols.append(np.concatenate([np.full(a, -1.0), np.full(b, 0.5), above]))
    cols.append(np.sort(np.round(rng.normal(size=S) / 0.25) * 0.25))
    d = np.sort(rng.normal(size=S))
    first_nan = S - SEAM_RUNS["nan"]
    d[first_nan - SEAM_RUNS["below_nan"]:first_nan] = d[first_nan - SEAM_RUNS["below_nan"]]
    d[first_nan:] = np.nan
    cols.append(d)
    cols.append(np.sort(rng.normal(size=S)))
    for c in (above, cols[3][:first_nan - SEAM_RUNS["below_nan"] + 1], cols[4]):
        assert len(np.unique(c)) == len(c)
    return np.stack(cols, axis=1)


def seam_columns(C, n, seed):
    """(C, n, 5) float64, read-only, C n = SEAM_S and n even; the columns by their sorted order:
      0  constant
      1  1 024 copies of -1.0, then 2·1 024 + 7 copies of 0.5, then distinct values above: one run ends
         on a seam of the 1 024-value tiles, the next starts on it and covers two whole tiles
      2  normal values rounded to a grid of 0.25: about 30 values, every seam inside a run
      3  distinct values, then 200 equal ones, then 1 500 NaN: the finite run ends where the NaN tail
         begins, and the tail crosses a seam and fills a whole tile
      4  distinct values
    The rows are shuffled by a seeded permutation before the reshape."""
    assert C * n == SEAM_S and n % 2 == 0
    srt = seam_sorted(seed)
    shuffle = np.random.default_rng(seed + 1).permutation(SEAM_S)
    assert not np.array_equal(shuffle, np.arange(SEAM_S))
    x = srt[shuffle].reshape(C, n, 5)
    x.setflags(write=False)
    return x


def finite_ranks(u):
    """Average ranks (C, m, k) of the pooled samples of u (C, m, k) by scipy.stats.rankdata over the
    non-NaN samples of each component (NaN sorts last and moves no finite sample's rank); NaN has rank NaN."""
    from scipy.stats import rankdata

    C, m, k = u.shape
    pooled = u.reshape(C * m, k)
    out = np.full(pooled.shape, np.nan)
    for v in range(k):
        fin = ~np.isnan(pooled[:, v])
        out[fin, v] = rankdata(pooled[fin, v], method="average")
    return out.reshape(C, m, k)


def finite_scores(u):
    from scipy.special import ndtri

    return ndtri((finite_ranks(u) - 3 / 8) / (u.shape[0] * u.shape[1] + 1 / 4))


def folded(u):
    """|u - pooled median| per component (NaN throughout where the component has a NaN sample)."""
    with np.errstate(invalid="ignore"):
        med = np.quantile(u.reshape(-1, u.shape[2]), 0.5, axis=0)
        return np.abs(u - med)


# -------------------------------------------------------- support over time
def planted(stride=1):
    """(chain, component, t, value) of the planted extremes and NaN of long_rows, t in samples of the
    view [:, :, ::stride] (n = 40 000 // stride of them; its chunk seam is between 16 383 and 16 384)."""
    n = LONG_SHAPE[2] // stride
    # positions are indices of the view, which has n = 40 000 or 20 000 samples: an index inside the second
    # chunk is 20 000 in the full rows and has to be lower in the view of 20 000; and t = 2 MM_CHUNK - 1, the
    # last sample of the second chunk of three, does not exist in the view of two chunks, whose NaN goes to
    # its last sample instead
    mid = 20000 if n > 20000 else 18000
    return [(0, 0, n - 1, 11.0),       # the maximum of component 0: the last sample of the short last chunk
            (0, 1, MM_CHUNK, 12.0),    # the maximum of component 1: the first sample of the second chunk
            (1, 1, MM_CHUNK - 1, -12.0),  # the minimum of component 1: the last sample of the first chunk
            (1, 2, mid, -13.0),        # the minimum of component 2: inside the second chunk
            (1, 0, MM_CHUNK, np.nan), (0, 2, n - 1 if stride > 1 else 2 * MM_CHUNK - 1, np.nan),
            (1, 2, 0, np.nan), (0, 0, n - 2, np.nan)]


def long_rows(seed, stride=1):
    """(2, 3, 40 000) float64 in vars_time order (C, k, n), read-only: standard normal values (all inside
    (-7, 7)) and the planted values of planted(stride) at t · stride, each extreme strictly outside the
    rest, so that losing a chunk, or a chunk's first or last sample, changes a result."""
    x = np.random.default_rng(seed).normal(size=LONG_SHAPE)
    assert np.abs(x).max() < 7.0
    for c, v, t, value in planted(stride):
        x[c, v, t * stride] = value
    x.setflags(write=False)
    return x


def short_rows(seed):
    """ROWS_SHAPE = (70, 16, 256) as (C, n, k), returned in vars_time order (70, 256, 16), read-only: the
    minimum and maximum of component 255 in chain 69 (the last row) and of component 0 in chain 0 (the first)."""
    C, n, k = ROWS_SHAPE
    x = np.random.default_rng(seed).normal(size=(C, k, n))
    x[C - 1, k - 1, n - 1], x[C - 1, k - 1, 0] = 9.0, -9.5
    x[0, 0, 0], x[0, 0, n - 1] = 10.0, -10.5
    x.setflags(write=False)
    return x


def capped_plants():
    """(flat index into CAP_SHAPE, value) of the planted extremes of capped_rows, placed by
    minmax_inner_grid: the span of workgroup g of minmax_inner_kernel is the flat elements
    [g span, (g + 1) span) of the (C, n, k) array, and span is a multiple of k, so that a flat index f
    is component f % k in every workgroup."""
    C, n, k = CAP_SHAPE
    total = C * n * k
    groups, span = minmax_inner_grid(total, k)
    g = groups // 2
    return [(g * span, 11.0),             # the first element of an interior span: the maximum of component 0
            (g * span + 1, 12.0),         # its second: the maximum of component 1
            ((g + 1) * span - 1, 13.0),   # the last element of that span: the maximum of component 2
            ((g + 1) * span - 2, -12.0),  # the one before: the minimum of component 1
            ((groups - 1) * span, -11.0),  # the first element of the short last span: the minimum of component 0
            (total - 1, -13.0)]           # the very last element: the minimum of component 2


def capped_rows(seed):
    """CAP_SHAPE = (64, 23 500, 3) float64 (C, n, k), read-only: standard normal values (all inside
    (-7, 7)), a few NaN, among them the neighbours of two plants, and the extremes of capped_plants(),
    every one strictly outside the rest and exact in f32.  The adversarial data of the histogram tests
    holds +-inf in every span, so its support is (-inf, inf) whatever a kernel drops; here a lost first
    or last element of a span, a lost short last workgroup or a lane on the wrong component changes a result."""
    x = np.random.default_rng(seed).normal(size=CAP_SHAPE)
    assert np.abs(x).max() < 7.0
    flat = x.reshape(-1)
    plants = capped_plants()
    for f, _ in plants[:3:2]:
        flat[f + 3] = np.nan  # the same component, one sample on: skipped, not taken for the extreme
    flat[[7, 1000003, flat.size - 4]] = np.nan
    for f, value in plants:
        flat[f] = value
    x.setflags(write=False)
    return x


def nan_support(cnk):
    """(k, 2) np.nanmin / np.nanmax of the float64 (C, n, k) samples."""
    a = np.asarray(cnk, dtype=np.float64).reshape(-1, cnk.shape[2])
    return np.stack([np.nanmin(a, axis=0), np.nanmax(a, axis=0)], axis=1)


def assert_numpy_marginals(h, cnk, bins):
    """marginal_histograms(range=None)'s result h against np.histogram of each component of (C, n, k)."""
    a = np.asarray(cnk, dtype=np.float64).reshape(-1, cnk.shape[2])
    for v in range(a.shape[1]):
        col = a[:, v]
        counts, edges = np.histogram(col[~np.isnan(col)], bins=bins)
        assert np.array_equal(h["counts"][v], counts) and np.array_equal(h["edges"][v], edges), v
    assert not h["below"].any() and not h["above"].any()

"""The CPU half of the rank and histogram tests past one tile, chunk and grid pass
(tests/test_gpu_rank_tiles.py, tests/test_gpu_posterior_tiles.py).  No GPU.

First the inputs: the geometry restated in tests/analytics_tiles.py says of each
fixture that it reaches the loop, seam or cap it was built for.  Then the host
definitions (backend="host"), against which the device is compared there, on
these same inputs against scipy.stats.rankdata, np.quantile, np.nanmin /
np.nanmax, np.histogram and np.histogramdd: exactly.
"""
import numpy as np
import pytest

import analytics_tiles as A
from analytics_tiles import RANK_TILE, S_BIG, SEAM_S, T
from ip_mcmc_amd import histogramdd, marginal_histograms, pooled_quantiles, rank_normalize, support
from test_gpu_posterior import HI, LO, adversarial
from test_gpu_rank import fixture, reference, varying_key_bytes

STALE = ("the geometry restated in tests/analytics_tiles.py no longer puts this input on the path it was chosen for: "
         "re-derive the shape (and the restatement) from the kernel.  This says nothing about whether the kernel "
         "is right.")


# ------------------------------------------------------------------ the inputs
def test_sort_sizes_put_several_tiles_in_a_scan_group():
    assert T == 4096
    for S, want in A.SORT_SIZES.items():
        assert A.scan_groups(S) == want and sum(want) == -(-S // T), (S, STALE)
        assert max(want) >= 2, (S, STALE)
    assert [A.scan_groups(S) for S in (T, 3 * T + 17, 12000)] == [[1, 0, 0, 0], [1, 1, 1, 1], [1, 1, 1, 0]]
    assert 0 in A.scan_groups(4 * T + 1) and 0 in A.scan_groups(8 * T + 1), STALE  # an empty group behind full ones
    assert S_BIG == 131269 and A.key_iterations(S_BIG) == 2, STALE
    assert A.key_iterations(S_BIG - 5 - 3 * 64) == 1 and A.key_iterations(16 * T + 3) == 1
    lone = A.lone_bit_column(S_BIG)  # two key bits that only workgroup 0 sees, one in each of its two steps
    assert varying_key_bytes(lone) == {0, 1} and np.flatnonzero(lone != 8.0).tolist() == [5, 2048 * 64 + 7]
    assert varying_key_bytes(lone[:2048 * 64]) == {0} and varying_key_bytes(lone[64:]) == {1}


@pytest.mark.parametrize("S", list(A.SORT_SIZES))
def test_sort_columns_run_the_passes_they_were_built_for(S):
    x = A.sort_columns(S, S)
    a, b = x[:, 0], x[:, 1]
    assert varying_key_bytes(a[~np.isnan(a)]) == set(range(8))
    assert varying_key_bytes(b) == {3, 4, 5, 6}
    assert np.isnan(a).sum() == 4 and np.isinf(a).sum() == 4 and (a == 0).sum() == 4
    assert np.signbit(a[a == 0]).sum() == 2
    fin = a[np.isfinite(a)]
    assert len(np.unique(fin)) <= len(fin) - S // 200  # the copies tie
    assert len(np.unique(b)) < S
    a32 = a.astype(np.float32).astype(np.float64)  # as f32 input: the low bytes are 0x00 or 0xFF by sign
    assert varying_key_bytes(a32[~np.isnan(a32)]) == set(range(8))
    assert varying_key_bytes(A.low_byte_column(S, S)) == {0}  # one pass: the other buffer than 4 or 8 passes


def test_seam_columns_put_runs_on_and_across_the_seams():
    C, n = A.SEAM_SHAPE
    x = A.seam_columns(C, n, 7)
    assert x.shape == (C, n, 5) and C * n == SEAM_S == 5 * RANK_TILE + 304 and n % 2 == 0
    assert A.rank_tiles(SEAM_S) == 6
    srt = np.sort(x.reshape(-1, 5), axis=0)  # NaN last
    assert np.array_equal(srt, A.seam_sorted(7), equal_nan=True)
    assert not np.array_equal(x.reshape(-1, 5), srt, equal_nan=True)  # shuffled
    seams = [s for s in range(RANK_TILE, SEAM_S, RANK_TILE)]
    assert len(seams) == 5
    assert len(np.unique(srt[:, 0])) == 1
    one = srt[:, 1]
    assert (one[:RANK_TILE] == -1.0).all() and (one[RANK_TILE:3 * RANK_TILE + 7] == 0.5).all()
    assert one[3 * RANK_TILE + 7] > 0.5 and len(np.unique(one[3 * RANK_TILE + 7:])) == SEAM_S - 3 * RANK_TILE - 7
    grid = srt[:, 2]
    assert 20 <= len(np.unique(grid)) <= 40
    for s in seams:  # the seam lies strictly inside a run: the run has members on both sides of it
        assert grid[s - 1] == grid[s], (s, STALE)
    tail = srt[:, 3]
    first_nan = SEAM_S - 1500
    assert first_nan < 4 * RANK_TILE and np.isnan(tail[first_nan:]).all() and not np.isnan(tail[:first_nan]).any()
    assert np.isnan(tail[4 * RANK_TILE:5 * RANK_TILE]).all()  # a whole tile of NaN
    assert (tail[first_nan - 200:first_nan] == tail[first_nan - 1]).all() and tail[first_nan - 201] < tail[first_nan - 1]
    assert len(np.unique(srt[:, 4])) == SEAM_S


def test_long_and_short_rows_reach_the_chunks_and_the_unit_span():
    assert A.minmax_outer_geometry(2, 3, 40000) == (3, 18, 9, 2), STALE
    assert 40000 - 2 * A.MM_CHUNK == 7232
    assert A.minmax_outer_geometry(2, 3, 20000)[0] == 2  # the view [:, :, ::2]
    assert A.minmax_outer_geometry(2, 3, A.MM_CHUNK)[0] == 1 and A.minmax_outer_geometry(2, 3, A.MM_CHUNK + 1)[0] == 2
    C, n, k = A.ROWS_SHAPE
    nchunk, units, uspan, groups = A.minmax_outer_geometry(C, k, n)
    assert (nchunk, units, uspan) == (1, 17920, 18) and uspan != 16 and groups <= A.MINMAX_GROUPS, STALE
    assert A.minmax_outer_geometry(300, 17, 5)[2] == 16 and A.minmax_outer_geometry(64, 3, 2001)[0] == 1
    for stride in (1, 2):
        x = A.long_rows(3, stride)[:, :, ::stride]
        rest = x.copy()
        for c, v, t, value in A.planted(stride):
            assert x[c, v, t] == value or np.isnan(value)
            rest[c, v, t] = 0.0
        assert not np.isnan(rest).any() and np.abs(rest).max() < 7.0  # every extreme is outside the rest
        want = A.nan_support(x.transpose(0, 2, 1))
        assert want[0, 1] == 11.0 and want[1].tolist() == [-12.0, 12.0] and want[2, 0] == -13.0
    assert np.isnan(A.long_rows(3)[1, 0, 16384]) and np.isnan(A.long_rows(3)[0, 2, 32767])
    want = A.nan_support(A.short_rows(4).transpose(0, 2, 1))
    assert want[0].tolist() == [-10.5, 10.0] and want[255].tolist() == [-9.5, 9.0]


def test_the_large_shape_is_past_the_workgroup_caps():
    C, n, k = A.CAP_SHAPE
    total = C * n * k
    assert total == 4512000
    groups, span = A.hs_grid(total)
    assert groups < total / 4096 and groups <= A.HS_GROUPS and span > 4096 and groups * span >= total, STALE
    assert A.hs_grid(64 * 2001 * 3) == (94, 4096)  # the largest input of tests/test_gpu_posterior.py: 16 per lane
    groups, span = A.minmax_inner_grid(total, k)
    assert groups <= A.MINMAX_GROUPS and span > 16 * 255 and span % 255 == 0 and groups * span >= total, STALE
    # ipmc_histdd takes a lane per sample: the C n = 1 504 000 samples of this shape stay under its cap, and
    # the same buffer read as one component of C n k samples is past it
    assert A.hs_grid(C * n)[1] == 4096 and A.hs_grid(C * n * k)[1] > 4096


def test_the_finite_large_shape_has_its_extremes_at_the_ends_of_spans():
    C, n, k = A.CAP_SHAPE
    total = C * n * k
    groups, span = A.minmax_inner_grid(total, k)
    assert (groups, span) == (984, 4590) and span % k == 0 and total - (groups - 1) * span == 30, STALE
    plants = A.capped_plants()
    g = groups // 2
    assert [f for f, _ in plants] == [g * span, g * span + 1, (g + 1) * span - 1, (g + 1) * span - 2,
                                      (groups - 1) * span, total - 1]
    assert [f % k for f, _ in plants] == [0, 1, 2, 1, 0, 2]
    x = A.capped_rows(5)
    flat = x.reshape(-1)
    rest = flat.copy()
    for f, value in plants:
        assert flat[f] == value
        rest[f] = 0.0
    assert np.isnan(rest).sum() == 5 and np.nanmax(np.abs(rest)) < 7.0  # every extreme is outside the rest
    assert np.isnan(flat[g * span + 3]) and np.isnan(flat[(g + 1) * span + 2])
    assert A.nan_support(x).tolist() == [[-11.0, 11.0], [-12.0, 12.0], [-13.0, 13.0]]
    for dtype in (np.float64, np.float32):  # the host definition on the same input
        a = x.astype(dtype)
        assert np.array_equal(support(a, backend="host"), A.nan_support(a))
        tv = np.ascontiguousarray(a.transpose(0, 2, 1))
        assert np.array_equal(support(tv, layout="vars_time", backend="host"), A.nan_support(a))
        A.assert_numpy_marginals(marginal_histograms(a, bins=20, backend="host"), a, 20)
    # in vars_time order the rows have two chunks, and the hist1d pass is past its cap in both orders
    assert A.minmax_outer_geometry(C, k, n)[0] == 2 and A.hs_grid(total)[1] > 4096


# ------------------------------------------------- the host definitions
def seam():
    return A.seam_columns(*A.SEAM_SHAPE, 7)


def test_host_ranks_on_the_seam_columns_equal_rankdata():
    x = seam()
    got = rank_normalize(x, scores=False, backend="host")
    want = A.finite_ranks(x)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[:, :, 3]).sum() == 1500 and np.array_equal(np.isnan(got), np.isnan(x))
    assert np.array_equal(got[:, :, 0], np.full(x.shape[:2], (SEAM_S + 1) / 2))
    f = rank_normalize(x, fold=True, scores=False, backend="host")
    assert np.array_equal(f, A.finite_ranks(A.folded(x)), equal_nan=True)
    assert np.isnan(f[:, :, 3]).all() and not np.isnan(f[:, :, [0, 1, 2, 4]]).any()
    again = rank_normalize(np.ascontiguousarray(x.transpose(0, 2, 1)), scores=False, layout="vars_time", backend="host")
    assert np.array_equal(again, got, equal_nan=True)


def test_host_quantiles_on_the_seam_and_sort_columns_equal_numpy():
    for x in (seam(), A.sort_columns(S_BIG, S_BIG)[None]):
        pooled = x.reshape(-1, x.shape[2])
        with np.errstate(invalid="ignore"):
            want = np.quantile(pooled, A.QUANTILES, axis=0).T
            got = pooled_quantiles(x, A.QUANTILES, backend="host")
        assert np.array_equal(got, want, equal_nan=True)
        assert np.array_equal(np.isnan(got).all(axis=1), np.isnan(pooled).any(axis=0))
        assert not np.isnan(got[~np.isnan(pooled).any(axis=0)]).any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_support_and_marginals_of_the_rows_equal_numpy(dtype):
    for stride in (1, 2):
        x = A.long_rows(3, stride).astype(dtype)
        for view in (x[:, :, ::stride], x[:, :, :A.MM_CHUNK], x[:, :, :A.MM_CHUNK + 1]):
            assert np.array_equal(support(view, layout="vars_time", backend="host"),
                                  A.nan_support(view.transpose(0, 2, 1)))
    for x in (A.long_rows(3).astype(dtype), A.short_rows(4).astype(dtype)):
        h = marginal_histograms(x, bins=20, layout="vars_time", backend="host")
        A.assert_numpy_marginals(h, x.transpose(0, 2, 1), 20)
        assert np.array_equal(support(x, layout="vars_time", backend="host"), A.nan_support(x.transpose(0, 2, 1)))


def test_host_histograms_of_the_large_shape_equal_numpy():
    x = adversarial(A.CAP_SHAPE, np.float64)
    flat = x.reshape(-1, 3)
    h = marginal_histograms(x, bins=20, range=(LO, HI), backend="host")
    for v in range(3):
        col = flat[:, v]
        counts, edges = np.histogram(col[~np.isnan(col)], bins=20, range=(LO, HI))
        assert np.array_equal(h["counts"][v], counts) and np.array_equal(h["edges"][v], edges)
        assert h["below"][v] == np.count_nonzero(col < LO) and h["above"][v] == np.count_nonzero(col > HI)
    assert h["below"].min() > 0 and h["above"].min() > 0 and h["n"] == flat.shape[0]
    rows = flat[~np.isnan(flat).any(axis=1)]
    for bins in (20, 128):
        H, edges = histogramdd(x, bins=bins, range=[(LO, HI)] * 3, backend="host")
        Hnp, enp = np.histogramdd(rows, bins=bins, range=[(LO, HI)] * 3)
        assert np.array_equal(H, Hnp) and all(np.array_equal(a, b) for a, b in zip(edges, enp))
    assert np.isinf(support(x, backend="host")).all()  # +-inf in every span: says nothing, see capped_rows
    col = flat.reshape(-1)  # the same values as one component: ipmc_histdd's lane per sample past its cap
    for bins in (20, 4096):
        H, edges = histogramdd(col.reshape(64, -1, 1), bins=bins, range=[(LO, HI)], backend="host")
        Hnp, enp = np.histogram(col[~np.isnan(col)], bins=bins, range=(LO, HI))
        assert np.array_equal(H, Hnp) and np.array_equal(edges[0], enp)


def test_the_tied_convergence_fixture_is_clear_of_the_stop():
    """ESS contains a discrete stop: reference() asserts that every evaluated |P_j| of the four transformed
    series is above P_CLEAR on the host, which is what lets the device be compared with it."""
    shape, seed = A.TIED_CONVERGENCE
    x = fixture(shape, seed, True)
    assert len(np.unique(x[:, :, 0])) < x.shape[0] * x.shape[1] // 4  # it ties
    assert A.scan_groups(x.shape[0] * x.shape[1]) == [1, 1, 1, 0] and A.rank_tiles(x.shape[0] * x.shape[1]) == 12
    reference(x)

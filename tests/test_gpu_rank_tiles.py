"""ipmc_pooled_sort and ipmc_rank_scores past one tile per lane group, one
grid-stride step and one tile of a run.

The shapes of tests/test_gpu_rank.py hold values, edge cases and layouts; set
against the kernels' geometry (ip_mcmc_amd/csrc/ipmc_rank.hip, restated in
tests/analytics_tiles.py) they sort four tiles at most, so that each lane group
of sort_scan_kernel has one tile, they give the key pass one step of its
grid-stride loop, and every tied input that is compared with a reference fits
one 1 024-value tile of rank_scores_kernel.  The shapes here are the smallest
that give

  sort_scan_kernel    two to nine tiles per lane group, a short and an empty last group
  sort_keys_kernel    a second grid-stride step (S_BIG = 2 048 · 64 + 3 · 64 + 5), and k > 64
                      with several sample tiles per component tile
  rank_scores_kernel  runs of equal values that end on a tile seam, start on one, cover whole
                      tiles and cross every seam, and a NaN tail over a seam and a whole tile

tests/test_analytics_tiles_cpu.py asserts of every input here that it reaches
its path, and holds the host definition to scipy and numpy on the same inputs.
Sorted values, permutations, average ranks and quantiles are compared exactly;
normal scores and rank_convergence's floats with RTOL / ATOL of
tests/test_gpu_rank.py.

Pooled sizes near 2^32 (kMaxPooled, the 32-bit permutation) are not reachable by
a test of a few seconds and stay untested.
"""
import functools

import numpy as np
import pytest

import analytics_tiles as A
from analytics_tiles import S_BIG, SEAM_S, T
from ip_mcmc_amd import pooled_quantiles, rank_convergence, rank_normalize
from test_gpu_rank import (ATOL, RTOL, assert_same, check_sort, device_sort, fixture, on_gpu, quiet, ref_ranks,
                           ref_scores, reference, varying_key_bytes)

pytestmark = pytest.mark.gpu

LAYOUTS = ["time_vars", "vars_time"]
NO_NAN = [0, 1, 2, 4]  # the seam columns that ref_ranks / ref_scores take whole


@functools.lru_cache(maxsize=None)
def sort_case(S):
    return A.sort_columns(S, S)[None]  # (1, S, 2), read-only


def gpu(x, dtype=None):
    return on_gpu(np.array(x), dtype)  # a copy: the cached inputs are read-only


def sort_in(x, layout, dtype=None, center=None):
    """device_sort of x (C, n, k) handed over in `layout`."""
    C, n, k = x.shape
    if layout == "time_vars":
        return device_sort(gpu(x, dtype), C, n, k, (n * k, k, 1), center)
    return device_sort(gpu(x.transpose(0, 2, 1), dtype), C, n, k, (k * n, 1, n), center)


def same_bits(a, b):
    return np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])


# ----------------------------------------------------------------- the sort
@pytest.mark.parametrize("S", list(A.SORT_SIZES), ids=[f"{-(-S // T)}tiles" for S in A.SORT_SIZES])
def test_sort_with_several_tiles_per_scan_group(S):
    assert A.scan_groups(S) == A.SORT_SIZES[S]
    x = sort_case(S)
    check_sort(x, sort_in(x, "time_vars"))


def test_sort_of_a_second_grid_stride_step_in_every_form():
    import torch

    assert A.key_iterations(S_BIG) == 2
    x = sort_case(S_BIG)
    a, b = x[0, :, 0], x[0, :, 1]
    assert varying_key_bytes(a[~np.isnan(a)]) == set(range(8)) and varying_key_bytes(b) == {3, 4, 5, 6}
    first = sort_in(x, "vars_time")
    check_sort(x, first)
    assert same_bits(first, sort_in(x, "vars_time"))  # a second call: the same bits
    assert same_bits(first, sort_in(x, "time_vars"))
    x32 = x.astype(np.float32).astype(np.float64)
    a32 = x32[0, :, 0]
    assert varying_key_bytes(a32[~np.isnan(a32)]) == set(range(8)) and varying_key_bytes(x32[0, :, 1]) == {3, 4, 5, 6}
    for layout in LAYOUTS:
        check_sort(x32, sort_in(x, layout, dtype=torch.float32))
    # |x - c| about the column medians (the first is taken over the values that have one)
    c = np.array([np.nanmedian(a), np.median(b)])
    with np.errstate(invalid="ignore"):
        for layout in LAYOUTS:
            check_sort(x, sort_in(x, layout, center=c), center=c)


def test_sort_of_key_bits_that_one_grid_stride_step_alone_sees():
    """The passes to run are the OR of key ^ first key over all samples, and 2 047 of the 2 048 workgroups
    of the key pass see the same bits in the columns above.  Here a difference in byte 0 is in workgroup
    0's first step alone and one in byte 1 in its second alone: the two samples sort last only if both
    steps reach the OR."""
    x = np.concatenate([sort_case(S_BIG), A.lone_bit_column(S_BIG)[None, :, None]], axis=2)
    assert varying_key_bytes(x[0, :, 2]) == {0, 1}
    for layout in LAYOUTS:
        srt, perm = got = sort_in(x, layout)
        check_sort(x, got)
        assert perm[2, -2:].tolist() == [5, A.KEY_GROUPS * A.KEY_TILE + 7] and srt[2, -3] == 8.0 < srt[2, -2] < srt[2, -1]


def test_sort_segments_that_end_in_different_buffers():
    """Four and eight running passes leave a segment's keys in the output buffers, one pass in the
    workspace: the three segments of one call, ten tiles each, end in both."""
    S = 9 * T + 5
    x = np.concatenate([sort_case(S), A.low_byte_column(S, S)[None, :, None]], axis=2)
    assert varying_key_bytes(x[0, :, 2]) == {0}
    for layout in LAYOUTS:
        check_sort(x, sort_in(x, layout))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_sort_of_70_components_over_several_sample_tiles(layout):
    """k = 70: a second component tile of 6 components, each over four sample tiles of 64 (the last of 8)."""
    rng = np.random.default_rng(170)
    x = rng.normal(size=(1, 200, 70))
    x[:, :, 64] = 0.75
    x[:, :, 69] = np.round(x[:, :, 69], 1)
    assert len(np.unique(x[:, :, 69])) < 100
    check_sort(x, sort_in(x, layout))


# ------------------------------------------------- rank scores at the seams
@functools.lru_cache(maxsize=None)
def seam():
    """The seam columns (C, n, 5) with their reference ranks and scores, plain and folded; read-only."""
    x = A.seam_columns(*A.SEAM_SHAPE, 7)
    f = A.folded(x)
    out = {"x": x, "ranks": A.finite_ranks(x), "scores": A.finite_scores(x), "folded_ranks": A.finite_ranks(f),
           "folded_scores": A.finite_scores(f)}
    # the file's own references on the columns they can take (rankdata over the whole column)
    assert np.array_equal(out["ranks"][:, :, NO_NAN], ref_ranks(x[:, :, NO_NAN]))
    assert np.array_equal(out["scores"][:, :, NO_NAN], ref_scores(x[:, :, NO_NAN]))
    assert np.array_equal(out["folded_ranks"][:, :, NO_NAN], ref_ranks(f[:, :, NO_NAN]))
    assert np.array_equal(out["folded_scores"][:, :, NO_NAN], ref_scores(f[:, :, NO_NAN]))
    for a in out.values():
        a.setflags(write=False)
    return out


def assert_ranks(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert len(bad) == 0, (f"{len(bad)} average ranks differ, the first at (chain, t, component) = {bad[0].tolist()}: "
                           f"got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


def assert_scores(got, want):
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=RTOL, atol=ATOL, equal_nan=True)


@pytest.mark.parametrize("slab", [None, 2], ids=["whole", "slab2"])
def test_ranks_and_scores_of_runs_across_the_tile_seams(slab):
    s = seam()
    x = s["x"]
    assert A.rank_tiles(SEAM_S) == 6
    t = gpu(x)
    kw = dict(backend="device", component_slab=slab)
    ranks = rank_normalize(t, scores=False, **kw)
    assert_ranks(ranks, s["ranks"])
    r = ranks.cpu().numpy()
    assert np.array_equal(r[:, :, 0], np.full(x.shape[:2], (SEAM_S + 1) / 2))
    assert np.array_equal(np.isnan(r), np.isnan(x)) and np.isnan(r).sum() == 1500
    assert_scores(rank_normalize(t, **kw), s["scores"])
    assert_ranks(rank_normalize(t, fold=True, scores=False, **kw), s["folded_ranks"])
    assert_scores(rank_normalize(t, fold=True, **kw), s["folded_scores"])
    # numpy in, vars_time layout
    tv = np.ascontiguousarray(x.transpose(0, 2, 1))
    assert_ranks(rank_normalize(tv, scores=False, layout="vars_time", **kw), s["ranks"])
    assert_scores(rank_normalize(tv, layout="vars_time", **kw), s["scores"])
    assert_ranks(rank_normalize(tv, fold=True, scores=False, layout="vars_time", **kw), s["folded_ranks"])
    assert_scores(rank_normalize(tv, fold=True, layout="vars_time", **kw), s["folded_scores"])


@pytest.mark.parametrize("mode", [0, 1], ids=["ranks", "scores"])
def test_rank_scores_alone_on_a_numpy_sort(mode):
    """ipmc_rank_scores on sorted values and a permutation made by numpy, so that a failure at a seam is
    not one of the sort; the output is filled first, and every entry has to be written."""
    import torch

    from ip_mcmc_amd import device as dev
    from ip_mcmc_amd._lib import call

    s = seam()
    x = s["x"]
    C, n, k = x.shape
    col = x.reshape(-1, k).T
    perm = np.argsort(col, axis=1, kind="stable")  # NaN last
    srt, pm = on_gpu(np.take_along_axis(col, perm, axis=1)), on_gpu(perm.astype(np.int32))
    out = torch.full((C, n, k), -7.0, dtype=torch.float64, device="cuda")
    call("ipmc_rank_scores", srt.data_ptr(), pm.data_ptr(), k, C, n, mode, out.data_ptr(), n * k, k, 1, None, 0,
         dev.stream_handle(out.device))
    got = out.cpu().numpy()
    assert not (got == -7.0).any(), f"{(got == -7.0).sum()} entries were not written"
    if mode == 0:
        assert_ranks(out, s["ranks"])
    else:
        assert_scores(out, s["scores"])


# ---------------------------------------------------------------- quantiles
def test_pooled_quantiles_of_many_tiles():
    for x in (seam()["x"], sort_case(S_BIG), np.nan_to_num(sort_case(S_BIG), nan=0.0, posinf=1e300, neginf=-1e300)):
        pooled = x.reshape(-1, x.shape[2])
        with np.errstate(invalid="ignore"):
            want = np.quantile(pooled, A.QUANTILES, axis=0).T
        has_nan = np.isnan(pooled).any(axis=0)
        assert np.array_equal(np.isnan(want).all(axis=1), has_nan) and not np.isnan(want[~has_nan]).any()
        with np.errstate(invalid="ignore"):  # inf - inf between two order statistics of a column with NaN
            got = pooled_quantiles(gpu(x), A.QUANTILES, backend="device")
            one = pooled_quantiles(gpu(x), A.QUANTILES, backend="device", component_slab=1)
        assert np.array_equal(got, want, equal_nan=True), (got, want)
        assert np.array_equal(one, want, equal_nan=True)


# ------------------------------------------------------- rank_convergence
def test_rank_convergence_of_a_tied_input_of_three_sort_tiles():
    """S = 12 000 with runs of equal values: twelve tiles of the rank scores.  reference() holds the
    |P_j| > P_CLEAR guard on the host first (tests/test_analytics_tiles_cpu.py runs it without a GPU)."""
    shape, seed = A.TIED_CONVERGENCE
    x = fixture(shape, seed, True)
    ref = reference(x)
    assert_same(quiet(rank_convergence, on_gpu(x), backend="device"), ref)
    assert_same(quiet(rank_convergence, on_gpu(x), backend="device", component_slab=2), ref)

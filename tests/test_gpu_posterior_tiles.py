"""ipmc_minmax, ipmc_hist1d and ipmc_histdd past one chunk of a row, past 16
rows per workgroup and past the 1 024-workgroup caps.

The shapes of tests/test_gpu_posterior.py hold every edge, layout and bin
count; set against the kernels' geometry (ip_mcmc_amd/csrc/ipmc_hist.hip,
restated in tests/analytics_tiles.py) their rows have one chunk, their
workgroups 16 rows and 4 096 elements.  The shapes here are the smallest that
give

  minmax_outer_kernel  rows of three and of two chunks of 16 384 samples with a short last one,
                       the two sides of a chunk's end, a strided row, and 18 rows per workgroup
  hs_grid, minmax_inner_kernel   more elements than 1 024 workgroups take at 16 per lane, so that
                       the span of a workgroup grows instead of the grid

tests/test_analytics_tiles_cpu.py asserts of every input here that it reaches
its path, and holds the host definition to numpy on the same inputs.
Everything compared is a count or a min / max of the inputs: np.array_equal.

Spans of 2^31 elements (kHsMaxSpan, and the 31-bit extents of the dense walk)
are not reachable by a test of a few seconds and stay untested.
"""
import numpy as np
import pytest

import analytics_tiles as A
from ip_mcmc_amd import histogramdd, marginal_histograms, support
from test_gpu_posterior import HI, LO, adversarial, assert_same_hist, laid_out, on_gpu

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
VT = dict(layout="vars_time")


def check_support(t, x):
    """support of the device tensor t (C, k, n) against nanmin / nanmax of its host twin x and the host backend."""
    want = A.nan_support(x.transpose(0, 2, 1))
    got = support(t, backend="device", **VT)
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(got, support(x, backend="host", **VT))


def check_marginals(t, x):
    got = marginal_histograms(t, bins=20, backend="device", **VT)
    assert_same_hist(got, marginal_histograms(x, bins=20, backend="host", **VT))
    A.assert_numpy_marginals(got, x.transpose(0, 2, 1), 20)


# ------------------------------------------------------- support over time
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_rows_of_three_chunks(dtype):
    C, k, n = A.LONG_SHAPE
    assert A.minmax_outer_geometry(C, k, n) == (3, 18, 9, 2)
    x = A.long_rows(3).astype(dtype)
    t = on_gpu(x)
    check_support(t, x)
    want = support(t, backend="device", **VT)
    assert want[0, 1] == 11.0 and want[1].tolist() == [-12.0, 12.0] and want[2, 0] == -13.0  # the planted values
    check_marginals(t, x)
    # the two sides of the first chunk's end: one chunk, and two of which the second has one sample
    for stop in (A.MM_CHUNK, A.MM_CHUNK + 1):
        assert A.minmax_outer_geometry(C, k, stop)[0] == stop - A.MM_CHUNK + 1
        view = t[:, :, :stop]
        assert not view.is_contiguous()
        check_support(view, x[:, :, :stop])
    assert support(t[:, :, :A.MM_CHUNK], backend="device", **VT)[1, 1] < 7.0
    assert support(t[:, :, :A.MM_CHUNK + 1], backend="device", **VT)[1, 1] == 12.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_every_other_sample_of_rows_of_two_chunks(dtype):
    """[:, :, ::2] in place: 20 000 samples of stride 2, the planted values on even t."""
    C, k, n = A.LONG_SHAPE
    assert A.minmax_outer_geometry(C, k, n // 2)[0] == 2
    x = A.long_rows(3, stride=2).astype(dtype)
    t = on_gpu(x)
    view = t[:, :, ::2]
    assert view.stride() == (k * n, n, 2) and view.data_ptr() == t.data_ptr()
    check_support(view, x[:, :, ::2])
    got = support(view, backend="device", **VT)
    assert got[0, 1] == 11.0 and got[1].tolist() == [-12.0, 12.0] and got[2, 0] == -13.0
    check_marginals(view, x[:, :, ::2])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_many_short_rows(dtype):
    """17 920 rows of 16 samples: 18 rows to a workgroup; the extremes sit in the first and the last row."""
    C, n, k = A.ROWS_SHAPE
    assert A.minmax_outer_geometry(C, k, n)[1:3] == (17920, 18)
    x = A.short_rows(4).astype(dtype)
    assert x.shape == (C, k, n)
    t = on_gpu(x)
    check_support(t, x)
    got = support(t, backend="device", **VT)
    assert got[0].tolist() == [-10.5, 10.0] and got[255].tolist() == [-9.5, 9.0]
    check_marginals(t, x)


# ------------------------------------------------------------ past the caps
@pytest.mark.parametrize("dtype,layout", [(np.float64, "time_vars"), (np.float32, "vars_time")],
                         ids=["f64-time_vars", "f32-vars_time"])
def test_support_and_data_edges_past_the_caps(dtype, layout):
    """Finite data with each extreme at the first, second, last-but-one or last element of an interior
    span of minmax_inner_kernel, at the first element of its short last workgroup and at the very last
    element, one component and side each: a lost end of a span, a lost workgroup or a lane on another
    component changes a result.  (The data of the test below holds +-inf in every span: its support is
    (-inf, inf) whatever is lost.)  In vars_time order the same values are rows of two chunks.  The
    marginals then take their edges from that support, past the cap of the histogram pass."""
    C, n, k = A.CAP_SHAPE
    groups, span = A.minmax_inner_grid(C * n * k, k)
    assert span > 16 * (256 // k * k) and span % k == 0 and A.minmax_outer_geometry(C, k, n)[0] == 2
    cnk = A.capped_rows(5).astype(dtype)
    x = laid_out(cnk, layout)
    t = on_gpu(x)
    want = A.nan_support(cnk)
    assert want.tolist() == [[-11.0, 11.0], [-12.0, 12.0], [-13.0, 13.0]]
    got = support(t, layout=layout, backend="device")
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(got, support(x, layout=layout, backend="host"))
    h = marginal_histograms(t, bins=20, layout=layout, backend="device")
    assert_same_hist(h, marginal_histograms(x, bins=20, layout=layout, backend="host"))
    A.assert_numpy_marginals(h, cnk, 20)


@pytest.mark.parametrize("dtype,layout", [(np.float64, "time_vars"), (np.float32, "vars_time")],
                         ids=["f64-time_vars", "f32-vars_time"])
def test_more_elements_than_the_capped_grids_take_at_16_per_lane(dtype, layout):
    C, n, k = A.CAP_SHAPE
    groups, span = A.hs_grid(C * n * k)
    assert groups < C * n * k / 4096 and span > 4096
    cnk = adversarial(A.CAP_SHAPE, dtype)
    x = laid_out(cnk, layout)
    t = on_gpu(x)
    kw = dict(layout=layout)
    assert np.array_equal(support(t, backend="device", **kw), support(x, backend="host", **kw))
    ref = marginal_histograms(x, bins=20, range=(LO, HI), backend="host", **kw)
    assert_same_hist(marginal_histograms(t, bins=20, range=(LO, HI), backend="device", **kw), ref)
    flat = cnk.reshape(-1, 3).astype(np.float64)
    nan = np.isnan(flat).sum(axis=0)
    assert np.array_equal(ref["counts"].sum(axis=1) + ref["below"] + ref["above"] + nan, np.full(k, C * n))
    rows = flat[~np.isnan(flat).any(axis=1)]
    rng3 = [(LO, HI)] * 3
    for bins in (20, 128):  # cells in LDS, cells in global memory
        H, edges = histogramdd(t, bins=bins, range=rng3, backend="device", **kw)
        assert np.array_equal(H, histogramdd(x, bins=bins, range=rng3, backend="host", **kw)[0])
        Hnp, enp = np.histogramdd(rows, bins=bins, range=rng3)
        assert np.array_equal(H, Hnp) and all(np.array_equal(a, b) for a, b in zip(edges, enp))
    # ipmc_histdd has a lane per sample, and C n samples stay under its cap: the same buffer as one
    # component of C n k samples is past it (4 096 bins: more edges than LDS keeps, cells in global memory)
    assert A.hs_grid(C * n)[1] == 4096 and A.hs_grid(C * n * k)[1] > 4096
    one = (C, n * k, 1) if layout == "time_vars" else (C, 1, n * k)
    t1, x1 = t.reshape(one), x.reshape(one)
    assert t1.data_ptr() == t.data_ptr()
    col = x1.reshape(-1).astype(np.float64)
    for bins in (20, 4096):
        H, edges = histogramdd(t1, bins=bins, range=[(LO, HI)], backend="device", **kw)
        assert np.array_equal(H, histogramdd(x1, bins=bins, range=[(LO, HI)], backend="host", **kw)[0])
        Hnp, enp = np.histogram(col[~np.isnan(col)], bins=bins, range=(LO, HI))
        assert np.array_equal(H, Hnp) and np.array_equal(edges[0], enp)

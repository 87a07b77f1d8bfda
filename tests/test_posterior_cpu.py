"""The host definition of ip_mcmc_amd.posterior (backend="host", no GPU): the
histograms against numpy's own, the two W1 forms against known answers and
against an optimal-transport LP / scipy, the quantiles against np.quantile."""
import numpy as np
import pytest

from ip_mcmc_amd import (hist_quantiles, histogramdd, marginal_histograms, support, wasserstein_1d,
                         wasserstein_distance, wasserstein_to_point)

LO, HI = -1.0, 1.5


def edge_cases(bins, k, seed):
    """(n, k) float64: every edge of np.linspace(LO, HI, bins + 1), one ulp to either side of
    each, values outside both ends, and random values, shuffled independently per component."""
    rng = np.random.default_rng(seed)
    e = np.linspace(LO, HI, bins + 1)
    col = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), [LO - 2.0, LO - 1e-9, HI + 1e-9, HI + 3.0],
                          rng.normal(0.2, 0.8, size=200)])
    return np.stack([rng.permutation(col) for _ in range(k)], axis=1)


@pytest.mark.parametrize("bins", [1, 7, 20])
def test_host_marginals_equal_np_histogram(bins):
    x = edge_cases(bins, 3, bins)
    h = marginal_histograms(x.reshape(3, -1, 3), bins=bins, range=(LO, HI), backend="host")
    assert h["counts"].dtype == np.int64 and h["n"] == x.shape[0]
    for v in range(3):
        counts, edges = np.histogram(x[:, v], bins=bins, range=(LO, HI))
        assert np.array_equal(h["counts"][v], counts)
        assert np.array_equal(h["edges"][v], edges)
        assert h["below"][v] == np.count_nonzero(x[:, v] < LO) and h["above"][v] == np.count_nonzero(x[:, v] > HI)


def test_host_marginals_range_none_constant_component_and_nan():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(4, 50, 3))
    x[..., 1] = 2.5  # constant: numpy widens the range to (2.0, 3.0)
    h = marginal_histograms(x, bins=20, backend="host")
    for v in range(3):
        counts, edges = np.histogram(x[..., v].ravel(), bins=20)
        assert np.array_equal(h["counts"][v], counts) and np.array_equal(h["edges"][v], edges)
    assert np.array_equal(h["edges"][1][[0, -1]], [2.0, 3.0])
    assert np.array_equal(support(x, backend="host"),
                          np.stack([x.reshape(-1, 3).min(axis=0), x.reshape(-1, 3).max(axis=0)], axis=1))
    x[1, 2, 0] = np.nan  # counts nowhere, and does not poison the support
    g = marginal_histograms(x, bins=20, backend="host")
    assert g["counts"][0].sum() + g["below"][0] + g["above"][0] == 199
    assert np.array_equal(g["counts"][2], h["counts"][2])
    # both layouts and a single (n, k) chain are the same pool
    assert np.array_equal(marginal_histograms(x.transpose(0, 2, 1), bins=20, layout="vars_time",
                                              backend="host")["counts"], g["counts"])
    assert np.array_equal(marginal_histograms(x.reshape(-1, 3), bins=20, backend="host")["counts"], g["counts"])
    f32 = marginal_histograms(x.astype(np.float32), bins=20, backend="host")
    for v in (0, 2):
        col = x[..., v].astype(np.float32).astype(np.float64).ravel()
        assert np.array_equal(f32["counts"][v], np.histogram(col[~np.isnan(col)], bins=20)[0])


@pytest.mark.parametrize("bins", [(3, 4, 5), 6])
def test_host_histogramdd_equals_np_histogramdd(bins):
    x = edge_cases(20, 3, 11)
    rng3 = [(LO, HI), (LO, 0.5), (0.0, HI)]
    H, edges = histogramdd(x[None], bins=bins, range=rng3, backend="host")
    Hnp, enp = np.histogramdd(x, bins=bins, range=rng3)
    assert H.dtype == np.int64 and np.array_equal(H, Hnp)
    assert all(np.array_equal(a, b) for a, b in zip(edges, enp))
    H, edges = histogramdd(x[None], bins=bins, backend="host")  # range=None
    Hnp, enp = np.histogramdd(x, bins=bins)
    assert np.array_equal(H, Hnp) and all(np.array_equal(a, b) for a, b in zip(edges, enp))
    H2, _ = histogramdd(x[None], bins=(4, 9), range=[rng3[0], rng3[2]], components=(0, 2), backend="host")
    assert np.array_equal(H2, np.histogramdd(x[:, [0, 2]], bins=(4, 9), range=[rng3[0], rng3[2]])[0])
    # chunks of whole chains add up to the same counts
    x4 = np.concatenate([x, x[::-1]])[:x.shape[0] // 2 * 4].reshape(4, -1, 3)
    one = histogramdd(x4, bins=bins, range=rng3, backend="host")[0]
    assert np.array_equal(histogramdd(x4, bins=bins, range=rng3, backend="host", chunk_bytes=1)[0], one)


def test_histogramdd_argument_errors():
    x = np.zeros((2, 5, 6))
    with pytest.raises(ValueError, match="components"):
        histogramdd(x, backend="host")  # k > 4 needs a selection
    with pytest.raises(ValueError, match="1 to 4"):
        histogramdd(x, components=(0, 1, 2, 3, 4), backend="host")
    with pytest.raises(ValueError, match="outside"):
        histogramdd(x, components=(0, 6), backend="host")
    with pytest.raises(ValueError, match="2\\^24"):
        histogramdd(x, bins=4096, components=(0, 1, 2), backend="host")
    with pytest.raises(ValueError, match="bins"):
        marginal_histograms(x, bins=0, backend="host")
    with pytest.raises(ValueError, match="bins"):
        marginal_histograms(x, bins=4097, backend="host")


def test_w1_known_answers():
    a, b = np.zeros(5), np.zeros(5)
    a[1], b[3] = 1.0, 1.0
    assert wasserstein_1d(a, b, (0.0, 4.0)) == 2.0  # two unit peaks 2 ticks apart on 5 unit-spaced ticks
    intervals = np.array([[-1.0, 1.0], [0.0, 3.0], [-5.0, 0.0]])  # unit-spaced ticks on a (3, 4, 6) grid
    d = np.zeros((3, 4, 6))
    d[0, 0, 0] = 1.0
    point = [0.9, 2.0, -3.0]  # the point of cell [2, 2, 2]
    target = np.histogramdd(np.array([point]), bins=d.shape, range=intervals)[0]
    assert target[2, 2, 2] == 1
    assert wasserstein_to_point(d, intervals, point) == pytest.approx(np.sqrt(12.0), abs=1e-15)
    assert wasserstein_distance(d, target, intervals) == pytest.approx(np.sqrt(12.0), abs=1e-15)
    assert wasserstein_distance(target, d, intervals) == pytest.approx(np.sqrt(12.0), abs=1e-15)
    assert wasserstein_distance(a, b, np.array([[0.0, 4.0]])) == 2.0
    with pytest.raises(ValueError, match="outside"):
        wasserstein_to_point(d, intervals, [1.5, 2.0, -3.0])


def test_general_nd_pair_is_out_of_scope():
    rng = np.random.default_rng(0)
    with pytest.raises(NotImplementedError, match="linear program"):
        wasserstein_distance(rng.random((3, 4)), rng.random((3, 4)), np.array([[0.0, 1.0], [0.0, 1.0]]))


def test_w1_to_point_equals_the_transport_lp():
    """helpers.wasserstein_distance's problem (min <T, M>, T 1 = d1, Tᵀ 1 = d2, T >= 0 with the
    Euclidean metric on the reference's ticks) solved as an LP, for a point-mass d2."""
    optimize = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(4)
    d1 = rng.random((3, 4, 2))
    d1 /= d1.sum()
    intervals = np.array([[-1.0, 2.0], [0.0, 0.7], [3.0, 5.0]])
    point = np.array([1.3, 0.2, 4.9])
    d2 = np.histogramdd(point[None], bins=d1.shape, range=intervals)[0]
    ticks = np.meshgrid(*[np.linspace(intervals[i, 0], intervals[i, 1], d1.shape[i]) for i in range(3)], indexing="ij")
    grid = np.stack([t.ravel() for t in ticks], axis=1)
    M = np.sqrt(((grid[:, None, :] - grid[None, :, :]) ** 2).sum(axis=2))
    n = grid.shape[0]
    A = np.zeros((2 * n, n * n))
    for i in range(n):
        A[i, i * n:(i + 1) * n] = 1.0  # row sums = d1
        A[n + i, i::n] = 1.0  # column sums = d2
    res = optimize.linprog(M.ravel(), A_eq=A, b_eq=np.concatenate([d1.ravel(), d2.ravel()]), bounds=(0, None),
                           method="highs")
    assert res.status == 0
    assert wasserstein_to_point(d1, intervals, point) == pytest.approx(res.fun, abs=1e-9)
    assert wasserstein_distance(d1, d2, intervals) == pytest.approx(res.fun, abs=1e-9)


def test_w1_1d_equals_scipy():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(6)
    a, b = rng.random(17), rng.random(17)
    ticks = np.linspace(-2.0, 3.5, 17)
    assert wasserstein_1d(a, b, (-2.0, 3.5)) == pytest.approx(stats.wasserstein_distance(ticks, ticks, a, b),
                                                              abs=1e-12)


def test_hist_quantiles_within_one_bin_width():
    rng = np.random.default_rng(8)
    x = np.stack([rng.normal(size=20000), rng.exponential(size=20000), rng.uniform(-3, 5, size=20000)], axis=1)
    h = marginal_histograms(x, bins=50, backend="host")
    q = np.array([0.0, 0.025, 0.25, 0.5, 0.9, 0.975, 1.0])
    got = hist_quantiles(h, q)
    want = np.quantile(x, q, axis=0).T
    width = np.diff(h["edges"], axis=1)[:, :1]
    assert got.shape == (3, len(q))
    assert np.all(np.abs(got - want) <= width)
    assert np.array_equal(hist_quantiles(h, 0.5), got[:, 3])

"""The host definition of covariance.posterior_covariance / multivariate_rhat
(backend="host", numpy float64) against np.cov, np.corrcoef and a direct
numpy / scipy evaluation of the formulas.  No GPU."""
import numpy as np
import pytest

from ip_mcmc_amd import convergence, multivariate_rhat, posterior_covariance
from ip_mcmc_amd.covariance import default_block_chains

# (C, n, k, block_chains): a single partial tile, the headline k, every tile pair, a tile remainder,
# a short last block, the minimum
SHAPES = [(5, 13, 3, None), (3, 10, 40, None), (2, 6, 256, None), (7, 9, 17, None), (70, 8, 5, 16), (1, 2, 1, None)]
IDS = ["-".join(str(v) for v in s) for s in SHAPES]
# the shapes on which tests/test_gpu_covariance_slabs.py runs the API on the device against this
# definition (several slabs per block, partial last tiles); the last one takes the default block
SLAB_SHAPES = [(7, 53, 65, 7), (5, 61, 129, 5), (9, 29, 200, 4), (3, 71, 255, 3), (11, 19, 256, 11), (8, 24, 256, 8),
               (7, 53, 65, None)]
SLAB_IDS = ["-".join(str(v) for v in s) for s in SLAB_SHAPES]


def make_samples(C, n, k, seed=0, dtype=np.float64, layout="time_vars", offset=1e5, sd_lo=0.01):
    """(C, n, k) samples (or (C, k, n)): component v has standard deviation about sd_v in
    [sd_lo, 1] and mean offset * sd_v, and neighbouring components are mixed, so every
    off-diagonal entry of the covariance is non-zero."""
    rng = np.random.default_rng(seed)
    sd = np.logspace(np.log10(sd_lo), 0.0, k) if k > 1 else np.array([0.3])
    z = rng.normal(size=(C, n, k))
    mixed = z + 0.5 * np.roll(z, 1, axis=2) + (0.3 * z[..., :1] if k > 2 else 0.0)
    x = (sd * (offset + mixed)).astype(dtype)
    return np.ascontiguousarray(x.transpose(0, 2, 1)) if layout == "vars_time" else x


def pooled(x, layout):
    a = np.asarray(x, dtype=np.float64)
    a = a.transpose(0, 2, 1) if layout == "vars_time" else a
    return a.reshape(-1, a.shape[2])


def assert_cov_close(got, want, rel):
    scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
    err = np.abs(got - want) / scale
    assert np.all(err <= rel), float(err.max())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("layout", ["time_vars", "vars_time"])
@pytest.mark.parametrize("shape", SHAPES + SLAB_SHAPES, ids=IDS + SLAB_IDS)
def test_host_definition_equals_numpy(shape, layout, dtype):
    C, n, k, block = shape
    x = make_samples(C, n, k, seed=k + n, dtype=dtype, layout=layout)
    r = posterior_covariance(x, layout=layout, backend="host", block_chains=block)
    p = pooled(x, layout)
    want = np.atleast_2d(np.cov(p, rowvar=False))
    assert r["n"] == C * n and r["cov"].shape == (k, k) and r["mean"].shape == (k,)
    assert_cov_close(r["cov"], want, 1e-12)
    m = p.mean(axis=0)
    assert np.all(np.abs(r["mean"] - m) <= 1e-14 * np.abs(m))
    assert np.all(np.abs(r["corr"] - np.atleast_2d(np.corrcoef(p, rowvar=False))) <= 1e-12)


@pytest.mark.parametrize("shape", SLAB_SHAPES, ids=SLAB_IDS)
def test_host_definition_does_not_depend_on_the_layout(shape):
    """The same samples as (C, n, k) and as (C, k, n) give the same bits: the split-chain means are
    added in sample order in both.  numpy adds a contiguous axis pairwise from 8 terms on, and Bn of
    chain means of 10⁵ standard deviations moves by 1e-10 when a mean moves in its last bits."""
    C, n, k, block = shape
    x = make_samples(C, n, k, seed=k + n)
    xt = np.ascontiguousarray(x.transpose(0, 2, 1))
    a = posterior_covariance(x, backend="host", block_chains=block)
    b = posterior_covariance(xt, layout="vars_time", backend="host", block_chains=block)
    for key in ("mean", "cov", "corr"):
        assert np.array_equal(a[key], b[key]), key
    ra = multivariate_rhat(x, backend="host", block_chains=block)
    rb = multivariate_rhat(xt, layout="vars_time", backend="host", block_chains=block)
    for key in ("W", "Bn", "rhat"):
        assert np.array_equal(ra[key], rb[key]), key


def test_split_chain_means_do_not_depend_on_the_order_of_the_adds():
    """Means summed about the first sample (diagnostics._pivot_mean, as ipmc_split_stats): the
    differences are spread-sized, so sample order and numpy's pairwise order round the same mean,
    within 1 ulp of the exact one; plain sums of numbers 1e5 spreads large are up to 6 ulp off."""
    import math

    from ip_mcmc_amd.diagnostics import _pivot_mean

    x = make_samples(3, 71, 255, seed=326)
    S = np.concatenate([x[:, :35], x[:, 35:70]], axis=0)
    mu = _pivot_mean(S)
    d = S - S[:, :1]
    pairwise = S[:, 0] + np.ascontiguousarray(d.transpose(0, 2, 1)).sum(axis=2) / 35
    assert np.array_equal(mu, pairwise)
    exact = np.array([[math.fsum(S[m, :, v]) / 35 for v in range(255)] for m in range(6)])
    assert np.all(np.abs(mu - exact) <= np.spacing(exact))
    assert np.any(np.abs(S.mean(axis=1) - exact) > 2 * np.spacing(exact))  # the plain sum is not


def test_the_tolerance_rejects_the_one_pass_form():
    x = make_samples(3, 10, 40, seed=50)
    p = pooled(x, "time_vars")
    R = p.shape[0]
    s = p.sum(axis=0)
    one_pass = (p.T @ p - np.outer(s, s) / R) / (R - 1)
    want = np.cov(p, rowvar=False)
    err = np.abs(one_pass - want) / np.sqrt(np.outer(np.diag(want), np.diag(want)))
    assert err.max() > 1e-9


def test_symmetry_and_unit_diagonal():
    x = make_samples(7, 9, 17, seed=1)
    r = posterior_covariance(x, backend="host")
    assert np.array_equal(r["cov"], r["cov"].T)
    assert np.array_equal(r["corr"], r["corr"].T)
    assert np.array_equal(np.diag(r["corr"]), np.ones(17))
    assert np.all(np.abs(r["corr"]) <= 1.0)


def test_constant_component_gives_nan_in_corr_only():
    x = make_samples(5, 13, 3, seed=2)
    x[:, :, 1] = 2.5
    r = posterior_covariance(x, backend="host")
    assert np.all(np.isfinite(r["cov"])) and np.all(np.isfinite(r["mean"]))
    assert r["mean"][1] == 2.5 and np.all(r["cov"][1] == 0) and np.all(r["cov"][:, 1] == 0)
    bad = np.zeros((3, 3), dtype=bool)
    bad[1], bad[:, 1] = True, True
    assert np.array_equal(np.isnan(r["corr"]), bad)
    assert r["corr"][0, 0] == 1.0 and r["corr"][2, 2] == 1.0


def test_nan_poisons_only_its_component():
    x = make_samples(7, 9, 17, seed=3)
    clean = posterior_covariance(x, backend="host")
    x[4, 5, 11] = np.nan
    r = posterior_covariance(x, backend="host")
    bad = np.zeros((17, 17), dtype=bool)
    bad[11], bad[:, 11] = True, True
    assert np.array_equal(np.isnan(r["cov"]), bad)
    assert np.array_equal(np.isnan(r["corr"]), bad)
    assert np.array_equal(np.isnan(r["mean"]), bad[11] & (np.arange(17) == 11))
    keep = ~bad
    assert_cov_close(np.where(keep, r["cov"], clean["cov"]), clean["cov"], 1e-12)


def test_odd_n_uses_the_last_sample():
    x = make_samples(5, 13, 3, seed=4)
    x[:, -1, :] += 3.0  # the sample the split chains drop
    r = posterior_covariance(x, backend="host")
    assert_cov_close(r["cov"], np.cov(pooled(x, "time_vars"), rowvar=False), 1e-12)
    short = posterior_covariance(x[:, :-1], backend="host")
    assert np.abs(r["cov"] - short["cov"]).max() > 1e-3 * np.abs(short["cov"]).max()


def test_one_chain_as_a_matrix_and_too_few_samples():
    x = make_samples(1, 30, 4, seed=5)
    a, b = posterior_covariance(x[0], backend="host"), posterior_covariance(x, backend="host")
    assert np.array_equal(a["cov"], b["cov"]) and np.array_equal(a["mean"], b["mean"])
    with pytest.raises(ValueError, match="at least 2 samples"):
        posterior_covariance(np.zeros((1, 1, 3)), backend="host")
    with pytest.raises(ValueError, match="block_chains"):
        posterior_covariance(x, backend="host", block_chains=0)
    with pytest.raises(ValueError, match="layout"):
        posterior_covariance(x, layout="vars", backend="host")


def test_default_block_depends_on_the_chain_count_and_k_alone():
    assert default_block_chains(1024, 3) == 4  # 256 blocks however long the chains are
    assert default_block_chains(65536, 40) == 256
    assert default_block_chains(5, 3) == 1
    assert default_block_chains(1 << 20, 40) == 1024
    b = default_block_chains(16384, 256)  # 256 blocks of k² doubles are 128 MiB
    assert b == 64 and -(-16384 // b) * 256 * 256 * 8 <= 256 << 20
    assert default_block_chains(1 << 17, 256) * 2 == default_block_chains(1 << 18, 256)
    big = default_block_chains(1 << 20, 256)
    assert -(-(1 << 20) // big) * 256 * 256 * 8 <= 256 << 20


# ------------------------------------------------------------ multivariate R-hat
def direct_rhat(x):
    """The formulas of the definition, written out: (W, Bn, rhat, lambda_max, rhat_mv)."""
    from scipy.linalg import eigh

    C, n, k = x.shape
    N, M = n // 2, 2 * C
    S = np.concatenate([x[:, :N], x[:, N:2 * N]], axis=0)
    mu = S.mean(axis=1)
    W = np.zeros((k, k))
    for m in range(M):
        d = S[m] - mu[m]
        W += d.T @ d / (N - 1)
    W /= M
    Bn = np.atleast_2d(np.cov(mu, rowvar=False, ddof=1))
    rhat = np.sqrt((N - 1) / N + np.diag(Bn) / np.diag(W))
    lam = eigh(Bn, W, eigvals_only=True)[-1]
    return W, Bn, rhat, lam, np.sqrt((N - 1) / N + lam)


@pytest.mark.parametrize("layout", ["time_vars", "vars_time"])
@pytest.mark.parametrize("shape", [(5, 13, 3, None), (70, 8, 5, 16), (40, 24, 17, None), (32, 40, 40, 5), (6, 9, 1, None)],
                         ids=["5-13-3", "70-8-5", "40-24-17", "32-40-40", "6-9-1"])
def test_multivariate_rhat_equals_the_formulas(shape, layout):
    C, n, k, block = shape
    x = make_samples(C, n, k, seed=7 * k + C, layout=layout)
    r = multivariate_rhat(x, layout=layout, backend="host", block_chains=block)
    a = np.asarray(x).transpose(0, 2, 1) if layout == "vars_time" else x
    W, Bn, rhat, lam, rmv = direct_rhat(a)
    assert_cov_close(r["W"], W, 1e-12)
    assert np.all(np.abs(r["Bn"] - Bn) <= 1e-10 * np.sqrt(np.outer(np.diag(Bn), np.diag(Bn))))
    assert np.array_equal(r["W"], r["W"].T) and np.array_equal(r["Bn"], r["Bn"].T)
    np.testing.assert_allclose(r["rhat"], rhat, rtol=1e-10)
    np.testing.assert_allclose(r["lambda_max"], lam, rtol=1e-8)
    np.testing.assert_allclose(r["rhat_mv"], rmv, rtol=1e-8)
    with np.testing.suppress_warnings() as sup:
        sup.filter(UserWarning)
        ref = convergence(x, layout=layout, backend="host")["rhat"]
    assert np.all(np.abs(r["rhat"] - ref) <= 1e-10)
    assert r["rhat_mv"] >= r["rhat"].max() - 1e-12
    if k == 1:
        assert abs(r["rhat_mv"] - r["rhat"][0]) <= 1e-12


def narrow_direction_ensemble(seed, shift):
    """64 chains of 200 iid draws with within-chain correlation 0.99; the chain means are
    shifted by +-shift along (1, -1)/sqrt(2), the narrow direction of the posterior."""
    rng = np.random.default_rng(seed)
    L = np.linalg.cholesky(np.array([[1.0, 0.99], [0.99, 1.0]]))
    x = rng.normal(size=(64, 200, 2)) @ L.T
    sign = np.where(np.arange(64) % 2 == 0, 1.0, -1.0)
    return x + shift * sign[:, None, None] * np.array([1.0, -1.0]) / np.sqrt(2.0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_narrow_direction_shows_only_in_the_multivariate_statistic(seed):
    r = multivariate_rhat(narrow_direction_ensemble(seed, 0.1), backend="host")
    assert r["rhat"].max() < 1.01, r["rhat"]
    assert r["rhat_mv"] > 1.3, r["rhat_mv"]
    r0 = multivariate_rhat(narrow_direction_ensemble(seed, 0.0), backend="host")
    assert r0["rhat_mv"] < 1.01, r0["rhat_mv"]


def test_constant_component_gives_nan_rhat_mv():
    x = make_samples(5, 13, 3, seed=8)
    x[:, :, 2] = 2.5
    r = multivariate_rhat(x, backend="host")
    assert np.isnan(r["rhat_mv"]) and np.isnan(r["lambda_max"])
    assert np.isnan(r["rhat"][2]) and np.all(np.isfinite(r["rhat"][:2]))


def test_multivariate_rhat_needs_four_samples():
    with pytest.raises(ValueError, match="at least 4 samples"):
        multivariate_rhat(np.zeros((3, 3, 2)), backend="host")


def test_exported_from_the_package():
    import ip_mcmc_amd

    assert "posterior_covariance" in ip_mcmc_amd.__all__ and "multivariate_rhat" in ip_mcmc_amd.__all__

"""Split-R̂ / ESS / MCSE across chains on the device (ipmc_split_stats,
ipmc_mean_acov, ipmc_moments_stats, ipmc_centered_sq_block_sums) against the
host definition (diagnostics.convergence, backend="host") evaluated on the
same values widened to float64.

The two differ only in summation order: rtol 1e-10 / atol 1e-12, the bound
tests/test_gpu_diag.py uses for device-vs-numpy sums.  ESS contains a discrete
stop (the first negative pair), so every ESS case first asserts, on the host
reference, that each evaluated |P_j| > 1e-6: no rounding can move the stop,
and lag_used / truncated must then be equal exactly.
"""
import warnings

import numpy as np
import pytest

from ip_mcmc_amd import convergence, moments_convergence, split_rhat
from ip_mcmc_amd import diagnostics as D

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-10, 1e-12
FLOAT_KEYS = ("mean", "sd", "rhat", "ess", "mcse", "tau")
EXACT_KEYS = ("lag_used", "truncated", "n_chains", "n_samples", "n_split")
P_CLEAR = 1e-6


def ar1(C, n, k, phi, seed, offset=8.0, scale=0.01):
    """AR(1) chains around `offset` with spread ~`scale` (θ = 8 + u: the normal case), (C, n, k)."""
    rng = np.random.default_rng(seed)
    e = rng.normal(size=(C, n, k))
    x = np.empty((C, n, k))
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return offset + scale * x + 0.2 * scale * rng.normal(size=(C, 1, k))


def quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


def reference(x64, max_lag=None):
    """Host definition on float64 (C, n, k), after checking that no evaluated pair is near zero."""
    ref = quiet(convergence, x64, max_lag=max_lag, backend="host")
    N = ref["n_split"]
    L = min(N - 1, 1000) if max_lag is None else max_lag
    mean, W, Bn, acov = D._host_parts(np.ascontiguousarray(x64, dtype=np.float64), L)
    rho = D._rho(W, Bn, acov, N)
    for v in np.flatnonzero(W > 0):
        last = ref["lag_used"][v] // 2 if ref["truncated"][v] else ref["lag_used"][v] // 2 - 1
        P = np.array([rho[2 * j, v] + rho[2 * j + 1, v] for j in range(last + 1)])
        assert np.abs(P).min() > P_CLEAR, (v, P)
    return ref


def assert_same(got, ref):
    for key in FLOAT_KEYS:
        np.testing.assert_allclose(got[key], ref[key], rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=key)
    for key in EXACT_KEYS:
        assert np.array_equal(got[key], ref[key]), (key, got[key], ref[key])


def on_gpu(x, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to("cuda")


# shape (C, n, k), seed: the smallest shapes that reach each code path
SHAPES = [
    ((3, 64, 40), 21),  # k neither a power of two nor a wave multiple, odd C; lanes over components
    ((1, 200, 2), 22),  # small k, one chain (M = 2); lanes over time
    ((8, 101, 3), 23),  # small k, odd n; lanes over time
    ((2, 16, 256), 24),  # the largest k
    ((5, 32, 1), 25),  # the smallest k
]


@pytest.mark.parametrize("shape,seed", SHAPES)
def test_device_equals_host_definition(shape, seed):
    x = ar1(*shape, 0.5, seed)
    ref = reference(x)
    got = quiet(convergence, on_gpu(x), backend="device")
    assert_same(got, ref)
    np.testing.assert_allclose(split_rhat(on_gpu(x), backend="device"), ref["rhat"], rtol=RTOL, atol=ATOL)
    # numpy in, device backend: the same bits as the device tensor
    again = quiet(convergence, x, backend="device")
    for key in FLOAT_KEYS + EXACT_KEYS:
        assert np.array_equal(got[key], again[key], equal_nan=True), key


def test_short_last_block():
    """18 split chains in blocks of 4: 5 partial sums, the last over 2 chains."""
    x = ar1(9, 40, 4, 0.5, 26)
    ref = reference(x)
    t = on_gpu(x)
    small = quiet(convergence, t, backend="device", block_chains=4)
    whole = quiet(convergence, t, backend="device", block_chains=1024)
    assert_same(small, ref)
    assert_same(whole, ref)
    assert_same(small, whole)  # to the tolerance: the order of the additions differs


def test_long_series_tiles():
    x = ar1(2, 20000, 2, 0.5, 27)  # N = 10 000 > 8192: tiled, two lag tiles
    assert_same(quiet(convergence, on_gpu(x), max_lag=300, backend="device"), reference(x, 300))


def test_both_sides_of_the_lds_threshold():
    """N = 8192 (staged in LDS) and N = 8193 (tiled) on the same data prefix."""
    x = ar1(1, 16386, 1, 0.5, 28)
    for n in (16384, 16386):
        assert_same(quiet(convergence, on_gpu(x[:, :n]), max_lag=40, backend="device"), reference(x[:, :n], 40))


def test_both_sides_of_the_in_place_threshold():
    """N = 64 (factors read in place) and N = 65 (staged in LDS) on the same data prefix."""
    x = ar1(2, 130, 3, 0.5, 38)
    for n in (128, 130):
        assert_same(quiet(convergence, on_gpu(x[:, :n]), backend="device"), reference(x[:, :n]))


def test_f32_tensor():
    x32 = ar1(4, 80, 5, 0.5, 29, offset=1.0, scale=0.5).astype(np.float32)
    assert_same(quiet(convergence, on_gpu(x32), backend="device"), reference(x32.astype(np.float64)))


@pytest.mark.parametrize("shape,seed", [((3, 64, 40), 30), ((4, 300, 3), 31)])
def test_vars_time_tensor(shape, seed):
    x = ar1(*shape, 0.5, seed)
    t = on_gpu(x.transpose(0, 2, 1))  # (C, k, n), contiguous
    assert_same(quiet(convergence, t, layout="vars_time", backend="device"), reference(x))


def test_non_contiguous_view():
    x = ar1(4, 120, 3, 0.5, 32)
    t = on_gpu(x)[:, ::2]
    assert not t.is_contiguous()
    assert_same(quiet(convergence, t, backend="device"), reference(x[:, ::2]))


def test_constant_component():
    x = ar1(4, 60, 3, 0.5, 33)
    x[:, :, 1] = 8.0
    ref = reference(x)
    got = quiet(convergence, on_gpu(x), backend="device")
    assert_same(got, ref)
    assert np.isnan(got["rhat"][1]) and np.isnan(got["ess"][1]) and np.isnan(got["mcse"][1])
    assert np.isfinite(got["ess"][[0, 2]]).all()


def test_two_calls_give_the_same_bits():
    for shape, kw in (((6, 90, 40), {}), ((6, 300, 3), {}), ((2, 17000, 2), {"max_lag": 64})):
        t = on_gpu(ar1(*shape, 0.5, 34))
        a, b = quiet(convergence, t, backend="device", **kw), quiet(convergence, t, backend="device", **kw)
        for key in FLOAT_KEYS + EXACT_KEYS:
            assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_short_max_lag_warns_on_the_device_too():
    t = on_gpu(ar1(4, 200, 3, 0.9, 35))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = convergence(t, max_lag=3, backend="device")
    assert len(w) == 1 and "component(s) [0, 1, 2]" in str(w[0].message)
    assert not r["truncated"].any() and (r["lag_used"] == 4).all()
    with pytest.raises(ValueError, match="max_lag"):
        convergence(t, max_lag=100, backend="device")
    with pytest.raises(ValueError, match="at least 4 samples"):
        convergence(t[:, :3], backend="device")


def test_moments_on_device_tensors():
    x = ar1(2500, 50, 7, 0.5, 36, offset=1.0, scale=0.5)  # 3 blocks of 1 024 chains, the last short
    m = {"sum_u": x.sum(axis=1), "sum_u2": (x * x).sum(axis=1), "n": 50}
    ref = moments_convergence(m)
    got = moments_convergence({"sum_u": on_gpu(m["sum_u"]), "sum_u2": on_gpu(m["sum_u2"]), "n": 50})
    for key in ("mean", "se", "rhat"):
        np.testing.assert_allclose(got[key], ref[key], rtol=RTOL, atol=ATOL, err_msg=key)


def _linear_sampler():
    """Stuart (2010) example 2.1's shape: G(u) = <g, u>, k = 2, scalar noise, prior N(0, I), pCN."""
    from ip_mcmc_amd import (ConstSteppCNProposer, CountedAccepter, EvolutionPotential, GaussianDistribution,
                             LinearOperator, MCMCSampler, pCNAccepter)

    g, gamma = np.array([3.0, 1.0]), 0.5
    y = np.array([g @ np.array([2.0, 7.0]) + 0.3])
    pot = EvolutionPotential(LinearOperator(g), y, GaussianDistribution(0, gamma**2))
    prior = GaussianDistribution(np.zeros(2), np.eye(2))
    return MCMCSampler(ConstSteppCNProposer(0.25, prior), CountedAccepter(pCNAccepter(pot)), 20261)


def test_end_to_end_linear_problem():
    u0 = 5.0 * np.random.default_rng(37).normal(size=(256, 2))  # dispersed starts
    early = _linear_sampler().run(u0, n_samples=20, burn_in=0, sample_interval=1)
    late = _linear_sampler().run(u0, n_samples=200, burn_in=2000, sample_interval=5)
    for samples in (early, late):
        assert_same(quiet(convergence, samples, backend="device"), reference(samples))
    r_early = quiet(convergence, early, backend="device")["rhat"]
    r_late = quiet(convergence, late, backend="device")["rhat"]
    assert (r_early > r_late).all(), f"rhat without burn-in {r_early} vs after 2000 steps of burn-in {r_late}"

    sums = _linear_sampler().run(u0, n_samples=200, burn_in=2000, sample_interval=5, keep="moments",
                                 results="device")
    assert sums["sum_u"].is_cuda
    got = moments_convergence(sums)
    ref = moments_convergence({"sum_u": sums["sum_u"].cpu().numpy(), "sum_u2": sums["sum_u2"].cpu().numpy(),
                               "n": sums["n"]})
    for key in ("mean", "se", "rhat"):
        np.testing.assert_allclose(got[key], ref[key], rtol=RTOL, atol=ATOL, err_msg=key)

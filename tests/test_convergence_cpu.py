"""Split-R̂ / ESS / MCSE across chains: the host definition (diagnostics.convergence,
backend="host").  No GPU: this is the written definition the kernels are
tested against (tests/test_gpu_convergence.py)."""
import warnings

import numpy as np
import pytest

from ip_mcmc_amd import convergence, moments_convergence, split_rhat
from ip_mcmc_amd import diagnostics as D


def ar1(C, n, k, phi, seed):
    """Stationary AR(1) chains with unit-variance innovations, (C, n, k)."""
    rng = np.random.default_rng(seed)
    e = rng.normal(size=(C, n, k))
    x = np.empty((C, n, k))
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return x


def host(x, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return convergence(x, backend="host", **kw)


def moments_of(x):
    return {"sum_u": x.sum(axis=1), "sum_u2": (x * x).sum(axis=1), "n": x.shape[1]}


def test_hand_case():
    """C=2, n=4, k=1: split chains [1,2], [2,2], [4,3], [5,7] (first halves, then second halves)."""
    x = np.array([[1.0, 2.0, 4.0, 3.0], [2.0, 2.0, 5.0, 7.0]])[:, :, None]
    N, M = 2, 4
    mu = np.array([1.5, 2.0, 3.5, 6.0])
    s2 = np.array([0.5, 0.0, 0.5, 2.0])  # Σ(x-μ)²/(N-1)
    W = s2.sum() / M  # 0.75
    mean = mu.sum() / M  # 3.25
    Bn = ((mu - mean) ** 2).sum() / (M - 1)  # 12.25 / 3
    rhat = np.sqrt(((N - 1) / N * W + Bn) / W)
    r = host(x)
    assert r["mean"][0] == 3.25
    np.testing.assert_allclose(r["rhat"], [rhat], rtol=1e-15)
    np.testing.assert_allclose(rhat, np.sqrt((0.375 + 12.25 / 3) / 0.75), rtol=1e-15)
    assert (r["n_chains"], r["n_samples"], r["n_split"]) == (2, 4, 2)
    np.testing.assert_allclose(split_rhat(x, backend="host"), [rhat], rtol=1e-15)


def test_agrees_with_the_posterior_agreement_tool():
    import os
    import sys

    from conftest import REPO

    sys.path.insert(0, os.path.join(REPO, "tools"))
    from posterior_agreement import _split_rhat

    x = ar1(16, 120, 4, 0.6, seed=11)
    np.testing.assert_allclose(host(x)["rhat"], _split_rhat(x), rtol=1e-12)
    np.testing.assert_allclose(split_rhat(x, backend="host"), _split_rhat(x), rtol=1e-12)


C_CAL, N_CAL, K_CAL = 64, 400, 5


def test_calibration_independent_draws():
    r = host(ar1(C_CAL, N_CAL, K_CAL, 0.0, seed=1))
    print("phi=0: rhat", r["rhat"], "ess/(C n)", r["ess"] / (C_CAL * N_CAL))
    assert r["rhat"].max() < 1.01
    ratio = r["ess"] / (C_CAL * N_CAL)
    assert ratio.min() >= 0.9 and ratio.max() <= 1.1
    assert r["truncated"].all()


def test_calibration_unmixed_chains():
    x = ar1(C_CAL, N_CAL, K_CAL, 0.5, seed=2)
    x[: C_CAL // 2] += 3.0
    r = host(x)
    print("shifted half: rhat", r["rhat"], "ess", r["ess"])
    assert r["rhat"].min() > 1.5
    assert r["ess"].max() < 0.01 * C_CAL * N_CAL


def test_split_sees_a_drift_every_chain_shares():
    x = ar1(C_CAL, N_CAL, K_CAL, 0.0, seed=3)
    x[:, N_CAL // 2:] += 1.0
    rs = split_rhat(x, backend="host")
    rm = moments_convergence(moments_of(x))["rhat"]
    print("common drift: split", rs, "non-split", rm)
    assert rs.min() > 1.1
    assert rm.max() < 1.01


def test_odd_n_drops_the_last_sample():
    x = ar1(4, 41, 3, 0.3, seed=4)
    a, b = host(x), host(x[:, :40])
    for key in ("mean", "sd", "rhat", "ess", "mcse", "tau", "lag_used", "truncated"):
        assert np.array_equal(a[key], b[key]), key
    assert a["n_samples"] == 41 and a["n_split"] == 20


def test_one_chain_and_2d_input():
    x = ar1(1, 200, 2, 0.4, seed=5)
    a, b = host(x), host(x[0])
    assert a["n_chains"] == b["n_chains"] == 1
    assert np.isfinite(a["rhat"]).all() and np.isfinite(a["ess"]).all()
    for key in ("rhat", "ess", "mcse"):
        assert np.array_equal(a[key], b[key])


def test_constant_component_is_nan():
    x = ar1(4, 60, 3, 0.2, seed=6)
    x[:, :, 1] = 8.0
    r = host(x)
    for key in ("rhat", "ess", "mcse"):
        assert np.isnan(r[key][1]), key
        assert np.isfinite(r[key][[0, 2]]).all(), key
    assert r["mean"][1] == 8.0 and r["sd"][1] == 0.0


def test_vars_time_is_the_transpose():
    x = ar1(3, 50, 4, 0.5, seed=7)
    a, b = host(x), host(np.ascontiguousarray(x.transpose(0, 2, 1)), layout="vars_time")
    for key in a:
        assert np.array_equal(a[key], b[key]), key


def test_short_max_lag_warns_once():
    x = ar1(4, 200, 3, 0.9, seed=8)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = convergence(x, max_lag=3, backend="host")
    assert len(w) == 1 and "component(s) [0, 1, 2]" in str(w[0].message)
    assert not r["truncated"].any()
    assert (r["lag_used"] == 4).all()  # pairs (0,1) and (2,3) added, 2j = 4 at the stop
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = convergence(ar1(8, 400, 2, 0.0, seed=9), backend="host")
    assert len(w) == 0 and r["truncated"].all()


def test_bad_arguments():
    x = ar1(2, 3, 2, 0.0, seed=10)
    with pytest.raises(ValueError, match="at least 4 samples"):
        convergence(x, backend="host")
    with pytest.raises(ValueError, match="at least 4 samples"):
        split_rhat(x, backend="host")
    x = ar1(2, 20, 2, 0.0, seed=10)
    with pytest.raises(ValueError, match="max_lag"):
        convergence(x, max_lag=10, backend="host")  # N - 1 = 9
    host(x, max_lag=9)
    with pytest.raises(ValueError, match="backend"):
        convergence(x, backend="cpu")
    with pytest.raises(ValueError, match="layout"):
        convergence(x, layout="chains_first", backend="host")


def test_ess_and_mcse_follow_the_formulas():
    """tau, ess and mcse from the ρ of the definition, recomputed here pair by pair."""
    x = ar1(6, 300, 2, 0.7, seed=12)
    r = host(x)
    C, n, k = x.shape
    N, M, L = n // 2, 2 * C, min(n // 2 - 1, 1000)
    mean, W, Bn, acov = D._host_parts(x, L)
    rho = D._rho(W, Bn, acov, N)
    for v in range(k):
        total, prev, j = 0.0, np.inf, 0
        while 2 * j + 1 <= L:
            P = rho[2 * j, v] + rho[2 * j + 1, v]
            if P < 0:
                break
            prev = min(P, prev)
            total += prev
            j += 1
        assert r["lag_used"][v] == 2 * j and r["truncated"][v]
        tau = -1 + 2 * total
        np.testing.assert_allclose(r["tau"][v], tau, rtol=1e-14)
        ess = min(M * N / tau, M * N * np.log10(M * N))
        np.testing.assert_allclose(r["ess"][v], ess, rtol=1e-14)
        np.testing.assert_allclose(r["mcse"][v], r["sd"][v] / np.sqrt(ess), rtol=1e-14)
    # AR(1) with φ = 0.7: τ = (1 + φ)/(1 - φ) ≈ 5.7; a loose band, the estimate is noisy
    assert 3.0 < r["tau"].min() and r["tau"].max() < 9.0


def test_moments_equal_the_sample_formula():
    rng = np.random.default_rng(13)
    x = ar1(32, 250, 4, 0.3, seed=13) * 0.5 + rng.uniform(-5.0, 5.0, size=4)  # |mean|/sd <= 10
    C, n, k = x.shape
    mc = x.mean(axis=1)
    W = x.var(axis=1, ddof=1).mean(axis=0)
    Bn = mc.var(axis=0, ddof=1)
    r = moments_convergence(moments_of(x))
    np.testing.assert_allclose(r["mean"], mc.mean(axis=0), rtol=1e-9)
    np.testing.assert_allclose(r["rhat"], np.sqrt(((n - 1) / n * W + Bn) / W), rtol=1e-9)
    np.testing.assert_allclose(r["se"], mc.std(axis=0, ddof=1) / np.sqrt(C), rtol=1e-9)
    with pytest.raises(ValueError, match="C >= 2"):
        moments_convergence({"sum_u": x.sum(axis=1)[0], "sum_u2": (x * x).sum(axis=1)[0], "n": n})

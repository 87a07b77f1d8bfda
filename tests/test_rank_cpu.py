"""The host definition of the rank statistics (ranks.py, backend="host")
against independent formulas: scipy.stats.rankdata, scipy.special.ndtri,
np.quantile and convergence(backend="host") on transformed arrays written out
here; and the AS241 Φ⁻¹ of ipmc_rng.hpp, compiled stand-alone by g++, against
ndtri."""
import os
import subprocess
import warnings

import numpy as np
import pytest
from scipy.special import ndtri
from scipy.stats import rankdata

from conftest import REPO
from ip_mcmc_amd import convergence, pooled_quantiles, rank_convergence, rank_normalize

RTOL, ATOL = 1e-10, 1e-12


def quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


def ar1(C, n, k, phi, seed, offset=8.0, scale=0.01):
    rng = np.random.default_rng(seed)
    e = rng.normal(size=(C, n, k))
    x = np.empty((C, n, k))
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return offset + scale * x + 0.2 * scale * rng.normal(size=(C, 1, k))


def ties(x, seed, grid=0.002):
    rng = np.random.default_rng(seed); C, n, k = x.shape; out = np.empty_like(x)
    for c in range(C):
        keep = rng.random(n) < 0.3; keep[0] = True
        out[c] = x[c, np.maximum.accumulate(np.where(keep, np.arange(n), 0))]
    return np.round(out / grid) * grid


CASES = {
    "continuous": ar1(3, 64, 5, 0.5, 61),
    "odd_n_ties": ties(ar1(4, 101, 3, 0.5, 62), 63),
    "one_chain": ar1(1, 40, 2, 0.5, 64),
}


def used(x):
    return x[:, :2 * (x.shape[1] // 2)]


def ref_ranks(x):
    """Average ranks of the used samples among the pooled ones, (C, 2N, k)."""
    u = used(x)
    C, m, k = u.shape
    return rankdata(u.reshape(C * m, k), method="average", axis=0).reshape(C, m, k)


def ref_scores(x):
    u = used(x)
    return ndtri((ref_ranks(x) - 3 / 8) / (u.shape[0] * u.shape[1] + 1 / 4))


@pytest.mark.parametrize("name", sorted(CASES))
def test_average_ranks_equal_rankdata(name):
    x = CASES[name]
    got = rank_normalize(x, scores=False, backend="host")
    assert got.dtype == np.float64 and got.shape == used(x).shape
    assert np.array_equal(got, ref_ranks(x))
    if name == "odd_n_ties":
        assert len(np.unique(got[:, :, 0])) < 60  # the fixture does tie: few distinct ranks among 400 samples


@pytest.mark.parametrize("name", sorted(CASES))
def test_normal_scores_equal_ndtri(name):
    x = CASES[name]
    np.testing.assert_allclose(rank_normalize(x, backend="host"), ref_scores(x), rtol=RTOL, atol=ATOL)
    # folded: the ranks of |x - pooled median of the used samples|
    u = used(x)
    med = np.median(u.reshape(-1, u.shape[2]), axis=0)
    np.testing.assert_allclose(rank_normalize(x, fold=True, backend="host"), ref_scores(np.abs(u - med)),
                               rtol=RTOL, atol=ATOL)
    assert np.array_equal(rank_normalize(x, fold=True, scores=False, backend="host"), ref_ranks(np.abs(u - med)))


def test_layouts_and_one_chain_shape():
    x = CASES["continuous"]
    a = rank_normalize(x, backend="host")
    assert np.array_equal(a, rank_normalize(x.transpose(0, 2, 1), layout="vars_time", backend="host"))
    assert np.array_equal(rank_normalize(x[0], backend="host"), rank_normalize(x[:1], backend="host"))  # (n, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_pooled_quantiles_equal_numpy(name):
    x = CASES[name]
    pooled = x.reshape(-1, x.shape[2])  # all n samples: the odd last one counts here
    q = [0.0, 0.001, 0.05, 0.25, 1 / 3, 0.5, 0.77, 0.95, 0.999, 1.0]
    got = pooled_quantiles(x, q, backend="host")
    assert got.shape == (x.shape[2], len(q)) and got.dtype == np.float64
    assert np.array_equal(got, np.quantile(pooled, q, axis=0).T)
    assert np.array_equal(pooled_quantiles(x, 0.5, backend="host")[:, 0], np.median(pooled, axis=0))
    assert np.array_equal(pooled_quantiles(x.transpose(0, 2, 1), q, layout="vars_time", backend="host"), got)


def test_pooled_quantiles_nan_and_infinities():
    x = CASES["continuous"].copy()
    x[1, 7, 2] = np.nan
    x[0, 3, 1], x[2, 5, 1] = np.inf, -np.inf
    pooled = x.reshape(-1, x.shape[2])
    q = [0.0, 0.3, 1.0]
    with np.errstate(invalid="ignore"):
        want = np.quantile(pooled, q, axis=0).T
        got = pooled_quantiles(x, q, backend="host")
    assert np.isnan(got[2]).all() and np.isfinite(got[[0, 3, 4]]).all()
    assert np.array_equal(got, want, equal_nan=True)


def by_hand(x, max_lag, tail=(0.05, 0.95)):
    """rank_convergence from its definition: four convergence() calls on transformed arrays."""
    u = used(x)
    pooled = u.reshape(-1, u.shape[2])
    med = np.quantile(pooled, 0.5, axis=0)
    q_lo, q_hi = np.quantile(pooled, tail[0], axis=0), np.quantile(pooled, tail[1], axis=0)
    bulk = quiet(convergence, ref_scores(x), max_lag=max_lag, backend="host")
    fold = quiet(convergence, ref_scores(np.abs(u - med)), max_lag=max_lag, backend="host")
    lo = quiet(convergence, (u <= q_lo).astype(np.float64), max_lag=max_lag, backend="host")
    hi = quiet(convergence, (u <= q_hi).astype(np.float64), max_lag=max_lag, backend="host")
    return {"rhat_bulk": bulk["rhat"], "ess_bulk": bulk["ess"], "rhat_tail": fold["rhat"],
            "rhat": np.maximum(bulk["rhat"], fold["rhat"]), "ess_tail": np.minimum(lo["ess"], hi["ess"]),
            "median": med, "q_lo": q_lo, "q_hi": q_hi, "lag_used": bulk["lag_used"], "truncated": bulk["truncated"],
            "n_chains": x.shape[0], "n_samples": x.shape[1], "n_split": x.shape[1] // 2}


@pytest.mark.parametrize("name,max_lag,tail", [("continuous", None, (0.05, 0.95)), ("odd_n_ties", 20, (0.1, 0.8)),
                                               ("one_chain", None, (0.05, 0.95))])
def test_rank_convergence_is_four_convergence_calls(name, max_lag, tail):
    x = CASES[name]
    got = quiet(rank_convergence, x, max_lag=max_lag, tail=tail, backend="host")
    want = by_hand(x, max_lag, tail)
    assert set(got) == set(want)
    for key, w in want.items():
        # the scores of the definition are scipy's ndtri on both sides: the same code path, the same bits
        assert np.array_equal(got[key], w, equal_nan=True), (key, got[key], w)
    assert got["lag_used"].dtype == np.int64 and got["truncated"].dtype == bool


def test_scale_difference_is_seen_by_the_ranks_only():
    """Eight chains of 400 N(0, 1) draws, four of them three times as wide: the same location."""
    x = np.random.default_rng(7).normal(size=(8, 400, 2))
    x[:4] *= 3.0
    classic = quiet(convergence, x, backend="host")["rhat"]
    r = quiet(rank_convergence, x, backend="host")
    print("classic rhat", classic, "rank rhat", r["rhat"], "bulk", r["rhat_bulk"], "tail", r["rhat_tail"])
    assert (classic < 1.01).all()
    assert (r["rhat"] > 1.1).all()
    assert np.array_equal(r["rhat"], r["rhat_tail"])  # the folded ranks see it


def test_cauchy_draws_have_finite_results():
    x = np.random.default_rng(8).standard_cauchy(size=(8, 400, 2))
    r = quiet(rank_convergence, x, backend="host")
    print("cauchy rhat", r["rhat"], "ess", r["ess_bulk"], r["ess_tail"])
    assert (r["rhat"] < 1.01).all()
    assert np.isfinite(r["ess_bulk"]).all() and np.isfinite(r["ess_tail"]).all()


def test_constant_and_nan_components():
    x = ar1(4, 60, 4, 0.5, 65)
    x[:, :, 1] = 8.0
    x[2, 17, 3] = np.nan
    r = quiet(rank_convergence, x, backend="host")
    clean = quiet(rank_convergence, x[:, :, [0, 2]], backend="host")
    for key in ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail"):
        assert np.isnan(r[key][[1, 3]]).all(), key
        assert np.array_equal(r[key][[0, 2]], clean[key]), key  # the other components are unaffected
    assert r["median"][1] == 8.0 and np.isnan(r["median"][3]) and np.isnan(r["q_lo"][3])
    z = rank_normalize(x, backend="host")
    assert np.isnan(z[2, 17, 3]) and np.isnan(z[:, :, 3]).sum() == 1
    assert np.array_equal(rank_normalize(x, scores=False, backend="host")[:, :, 1], np.full((4, 60), 120.5))


def test_one_warning_per_call():
    x = ar1(4, 200, 3, 0.9, 66)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = rank_convergence(x, max_lag=3, backend="host")
    assert len(w) == 1 and "max_lag=3 ended the autocorrelation sum" in str(w[0].message)
    assert "component(s) [0, 1, 2]" in str(w[0].message)
    assert not r["truncated"].any() and (r["lag_used"] == 4).all()
    with pytest.raises(ValueError, match="max_lag"):
        rank_convergence(x, max_lag=100, backend="host")
    with pytest.raises(ValueError, match="at least 4 samples"):
        rank_convergence(x[:, :3], backend="host")
    with pytest.raises(ValueError, match="tail"):
        rank_convergence(x, tail=(0.9, 0.1), backend="host")


def test_as241_of_the_kernels_equals_ndtri(tmp_path):
    """det_ppnd16 (ipmc_rng.hpp) through its stand-alone program, compiled by g++ with the library's
    floating-point flags: rtol 1e-10 / atol 1e-12 against scipy (AS241 states about 1e-16)."""
    csrc = os.path.join(REPO, "ip_mcmc_amd", "csrc")
    exe = str(tmp_path / "ppnd16_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unknown-pragmas",
                    os.path.join(csrc, "ipmc_ppnd16_check.cpp"), "-o", exe], check=True, cwd=csrc)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    table = np.array([[float(v) for v in line.split()] for line in out.splitlines()])
    p, z = table[:, 0], table[:, 1]
    assert len(p) > 400 and p.min() <= 1e-10 and p.max() >= 1 - 1e-10
    assert (np.abs(p - 0.5) <= 0.425).sum() > 100 and (p < 0.075).sum() > 30 and (p > 0.925).sum() > 30
    err = np.abs(z - ndtri(p)) / np.maximum(np.abs(ndtri(p)), 1e-300)
    print("largest relative difference to ndtri:", err[ndtri(p) != 0].max())
    np.testing.assert_allclose(z, ndtri(p), rtol=RTOL, atol=ATOL)
    assert z[p == 0.5] == 0.0

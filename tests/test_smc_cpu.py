"""Tempered SMC without a GPU (smc.py): det_exp through its stand-alone program, the host twins
of the resampling kernels against plain numpy, the search for the next temperature, the whole run on the
host tier against a linear-Gaussian problem's exact evidence and posterior, the compositions out of scope,
and the twins' sanitized self-test."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from ip_mcmc_amd import (ConstrainAccepter, ConstSteppCNProposer, ConstStepStandardRWProposer, EvolutionPotential,
                         GaussianDistribution, SMCResult, StandardRWAccepter, TemperedSMC, _hostlib, next_temperature,
                         pCNAccepter, systematic_resample, tempering_sums)

CSRC = os.path.join(REPO, "ip_mcmc_amd", "csrc")
BLOCK = 1024
SIZES = [1, 2, 1023, 1024, 1025, 2049, 70001]


# ------------------------------------------------------------------ det_exp
def test_det_exp_against_long_double_exp(tmp_path):
    """det_exp (ipmc_exp.hpp) through its stand-alone program, compiled by g++ with the library's
    floating-point flags: relative error <= 2^-50 against numpy's long double exp on [-708, 0]; 1 exactly
    at 0 and -0, 0 exactly below -708."""
    exe = str(tmp_path / "exp_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unknown-pragmas",
                    os.path.join(CSRC, "ipmc_exp_check.cpp"), "-o", exe], check=True, cwd=CSRC)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    table = np.array([[float(v) for v in line.split()] for line in out.splitlines()])
    x, y = table[:, 0], table[:, 1]
    assert np.finfo(np.longdouble).eps < 2.0**-60  # the comparison needs a wider type than double
    assert len(x) > 70000 and x.min() < -1e299 and (x == -708.0).any()
    assert ((x > -2.0**-50) & (x < 0)).sum() >= 10  # the tiny arguments
    inside = (x >= -708.0) & (x != 0)
    ref = np.exp(x[inside].astype(np.longdouble))
    err = np.abs(y[inside].astype(np.longdouble) - ref) / ref
    print("largest relative error of det_exp:", float(err.max()), "=", float(err.max()) * 2.0**53, "x 2^-53 at x =",
          x[inside][np.argmax(err)])
    assert float(err.max()) <= 2.0**-50
    zero = x == 0
    assert np.signbit(x[zero]).any() and not np.signbit(x[zero]).all() and (y[zero] == 1.0).all()  # 0 and -0
    assert (x < -708.0).sum() >= 4 and (y[x < -708.0] == 0.0).all()
    assert (y[inside] > 0).all() and (y[inside] >= np.finfo(np.float64).tiny).all()  # never subnormal


# -------------------------------------------------------------- host twins
def _phi_cases(n, seed):
    """name -> Φ (float64): a moderate spread, +inf and NaN entries, all equal, a spread of 10^4."""
    r = np.random.default_rng(seed)
    base = 3.0 + 10.0 * r.random(n)
    bad = base.copy()
    bad[0] = np.inf
    if n > 2:
        bad[n // 2] = np.nan
        bad[-1] = np.inf
    if n > 1030:
        bad[1024] = np.nan
    return {"spread10": base, "nonfinite": bad, "equal": np.full(n, 2.5), "spread1e4": 1.0 + 1e4 * r.random(n)}


def _weights(phi64, ref, delta):
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp(-(delta * (phi64 - ref)))
    return np.where(np.isfinite(phi64), w, 0.0)


def _block_order_sum(w):
    """Inside each block of 1 024 from zero in order, then the blocks' sums from zero in order."""
    total = 0.0
    for b0 in range(0, len(w), BLOCK):
        a = 0.0
        for v in w[b0:b0 + BLOCK].tolist():
            a = a + v
        total = total + a
    return total


def _block_order_cum(w):
    cum = np.empty(len(w))
    off = 0.0
    for b0 in range(0, len(w), BLOCK):
        within = np.cumsum(w[b0:b0 + BLOCK])  # numpy's cumsum is the sequential running sum
        cum[b0:b0 + BLOCK] = off + within
        off = off + within[-1]
    return cum


def _finite_min(phi):
    f = phi[np.isfinite(phi)]
    return float(f.min()) if f.size else None


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", SIZES)
def test_host_twins_against_numpy(n, dtype):
    deltas = np.array([0.0, 1e-3, 0.3, 1.0])
    for name, phi64 in _phi_cases(n, 100 + n).items():
        phi = phi64.astype(dtype)
        wide = phi.astype(np.float64)
        ref = _finite_min(wide)
        if ref is None:  # n = 1 with its one potential infinite
            s1, s2 = _hostlib.temper_sums(phi, 0.0, deltas)
            assert (s1 == 0).all() and (s2 == 0).all()
            continue
        s1, s2 = _hostlib.temper_sums(phi, ref, deltas)
        for j, d in enumerate(deltas):
            w = _weights(wide, ref, d)
            np.testing.assert_allclose(s1[j], _block_order_sum(w), rtol=1e-12, atol=0, err_msg=f"{name} s1 {d}")
            np.testing.assert_allclose(s2[j], _block_order_sum(w * w), rtol=1e-12, atol=0, err_msg=f"{name} s2 {d}")
        assert s1[0] == s2[0] == np.isfinite(wide).sum()  # delta = 0: every valid particle weighs exactly 1
        cum = _hostlib.temper_cumweights(phi, ref, 0.3)
        np.testing.assert_allclose(cum, _block_order_cum(_weights(wide, ref, 0.3)), rtol=1e-12, atol=0)
        assert (np.diff(cum) >= 0).all() and cum[-1] == s1[2]
        if name == "equal":
            assert (s1 == n).all() and (s2 == n).all() and ((s1 * s1 / s2) == n).all()  # ESS == n exactly
            assert np.array_equal(cum, np.arange(1, n + 1))
        if name == "spread1e4" and n >= 1023:
            w1 = np.diff(np.concatenate([[0.0], _hostlib.temper_cumweights(phi, ref, 1.0)]))
            assert (w1 == 0).mean() > 0.8  # most weights are exactly 0: exp underflows past Φ − Φ_ref = 708


@pytest.mark.parametrize("n", SIZES)
def test_ancestors_against_searchsorted(n):
    for name, phi in _phi_cases(n, 200 + n).items():
        ref = _finite_min(phi)
        if ref is None:
            continue
        delta = 0.3 if name != "spread1e4" else 0.002
        cum = _hostlib.temper_cumweights(phi, ref, delta)
        w = np.diff(np.concatenate([[0.0], cum]))
        total = cum[-1]
        for n_out in sorted({1, n, 3 * n}):
            for u in (0.0, 0.5, 0.73):
                anc = _hostlib.systematic_ancestors(cum, u, n_out)
                p = (np.arange(n_out, dtype=np.float64) + u) * (total / float(n_out))
                assert (p < total).all()
                assert np.array_equal(anc, np.searchsorted(cum, p, side="right")), (name, n_out, u)
                assert (np.diff(anc) >= 0).all() and anc.min() >= 0 and anc.max() < n
                assert (w[anc] > 0).all()  # a parent of weight 0 never appears
                counts = np.bincount(anc, minlength=n)
                assert (np.abs(counts - n_out * w / total) <= 1.0 + 1e-6).all()  # 1e-6: w is a difference of cum


def test_systematic_resample_is_the_identity_for_equal_weights():
    for n in SIZES:
        phi = np.full(n, 7.25)
        for u in (0.0, 0.5):
            anc = systematic_resample(phi, 7.25, 0.4, u, backend="host")
            assert anc.dtype == np.int64 and np.array_equal(anc, np.arange(n))
        s1, s2 = tempering_sums(phi, None, [0.0, 0.5, 1.0], backend="host")
        assert ((s1 * s1 / s2) == n).all()


def test_ancestors_without_weight_and_fallback():
    assert (_hostlib.systematic_ancestors(np.zeros(5), 0.5, 7) == -1).all()
    assert (_hostlib.systematic_ancestors(np.array([1.0, np.nan]), 0.5, 3) == -1).all()
    assert (_hostlib.systematic_ancestors(np.array([0.0, 0.0, 2.0, 2.0]), 0.99, 5) == 2).all()
    # p_i >= total by rounding cannot be arranged portably; the fallback's definition is the first c that
    # holds the total, which the sanitized self-test checks on its own cum.  Here: a total at the last index
    anc = _hostlib.systematic_ancestors(np.array([0.0, 1.0, 1.0, 3.0]), 0.999999, 3)
    assert anc.tolist() == [1, 3, 3]
    with pytest.raises(_hostlib.IpmcError, match="u outside"):
        _hostlib.systematic_ancestors(np.ones(3), 1.0, 3)
    with pytest.raises(ValueError, match="u must be"):
        systematic_resample(np.ones(3), None, 0.5, -0.1, backend="host")


def test_tempering_sums_many_candidates_and_checks():
    phi = 3.0 + np.random.default_rng(3).random(5000) * 40
    d = np.linspace(0, 1, 150)  # more than one call's 64 candidates
    s1, s2 = tempering_sums(phi, None, d, backend="host")
    a1, a2 = _hostlib.temper_sums(phi, phi.min(), d[64:128])
    assert np.array_equal(s1[64:128], a1) and np.array_equal(s2[64:128], a2)
    assert (np.diff(s1) < 0).all()
    with pytest.raises(ValueError, match="delta"):
        tempering_sums(phi, None, [-0.1], backend="host")
    with pytest.raises(ValueError, match="finite"):
        tempering_sums(np.array([np.inf, np.nan]), None, [0.1], backend="host")
    with pytest.raises(_hostlib.IpmcError, match=r"outside \[1, 64\]"):
        _hostlib.temper_sums(phi, phi.min(), np.zeros(65))


# --------------------------------------------------------- next_temperature
def _ess_at(phi, ref, delta):
    s1, s2 = _hostlib.temper_sums(phi, ref, [delta])
    return s1[0] * s1[0] / s2[0]


@pytest.mark.parametrize("n", [50, 1025, 20000])
def test_next_temperature_keeps_the_target(n):
    phi = 5.0 + 300.0 * np.random.default_rng(n).random(n) ** 2
    phi[n // 3] = np.inf
    target = 0.5 * n
    t = 0.0
    ladder = [t]
    while t < 1.0:
        st = next_temperature(phi, t, target, backend="host")
        assert st.phi_ref == phi[np.isfinite(phi)].min()
        assert st.delta > 0 and st.ess >= target and st.ess == _ess_at(phi, st.phi_ref, st.delta)
        assert st.s1 == _hostlib.temper_sums(phi, st.phi_ref, [st.delta])[0][0]
        if st.final:
            assert st.t_next == 1.0 and st.delta == 1.0 - t and st.upper is None
        else:
            assert st.upper > st.delta and _ess_at(phi, st.phi_ref, st.upper) < target
            assert (st.upper - st.delta) <= (1.0 - t) * 16.0**-10 * 1.01
            assert st.t_next == t + st.delta < 1.0
        # the weights of later stages are those of Φ again (no resampling here): the ladder still ends
        t = st.t_next
        ladder.append(t)
        assert len(ladder) < 200
    assert ladder[-1] == 1.0 and (np.diff(ladder) > 0).all()


def test_next_temperature_final_step_shortcut_and_failure():
    phi = np.linspace(1.0, 1.5, 1000)
    st = next_temperature(phi, 0.25, 500.0, backend="host")  # flat weights: ESS(0.75) is far above the target
    assert st.final and st.delta == 0.75 and st.t_next == 1.0 and st.ess >= 500.0
    bad = np.full(1000, np.inf)
    bad[:300] = np.linspace(1.0, 900.0, 300)
    with pytest.raises(RuntimeError, match="300 of the 1000 particles"):  # ESS(0) = 300 < 500: delta = 0
        next_temperature(bad, 0.0, 500.0, backend="host")
    with pytest.raises(ValueError, match="no potential is finite"):
        next_temperature(np.full(10, np.nan), 0.0, 5.0, backend="host")
    with pytest.raises(ValueError, match="t must be"):
        next_temperature(phi, 1.0, 500.0, backend="host")


# ------------------------------------------------------------ the whole run
G_VEC = np.array([3.0, 1.0, 4.0, 1.0])
GAMMA = 0.05
Y_OBS = 2.0


def linear_exact():
    S = GAMMA**2 + G_VEC @ G_VEC
    return (0.5 * np.log(GAMMA**2 / S) - Y_OBS**2 / (2 * S), G_VEC * Y_OBS / S,
            np.eye(4) - np.outer(G_VEC, G_VEC) / S)


def linear_problem_host():
    prior = GaussianDistribution(np.zeros(4), np.eye(4))
    pot = EvolutionPotential(lambda u: np.dot(G_VEC, u), np.array([Y_OBS]),
                             GaussianDistribution(np.zeros(1), GAMMA**2 * np.eye(1)))
    return prior, pot


def check_run_invariants(res, C, ess_frac):
    assert isinstance(res, SMCResult)
    S = res.n_stages
    assert res.temperatures.shape == (S + 1,) and res.ess.shape == (S,) and res.accept_rate.shape == (S,)
    assert res.log_evidence_increments.shape == (S,)
    assert res.temperatures[0] == 0.0 and res.temperatures[-1] == 1.0 and (np.diff(res.temperatures) > 0).all()
    assert (res.ess >= ess_frac * C).all()
    assert res.log_evidence == float(np.sum(res.log_evidence_increments)) and np.isfinite(res.log_evidence)
    assert ((res.accept_rate > 0) & (res.accept_rate < 1)).all()


def check_against_exact(results):
    """The two assertions on 16 seeds: the mean log-evidence within 5 standard errors plus the Jensen bias
    sd²/2 of the log of an unbiased estimate, and every component of the mean posterior mean within 5
    between-seed standard errors."""
    log_z, mean, _ = linear_exact()
    lz = np.array([r.log_evidence for r in results])
    sd = lz.std(ddof=1)
    bound = 5 * sd / np.sqrt(len(lz)) + sd**2 / 2
    print("log Z exact", log_z, "mean", lz.mean(), "error", abs(lz.mean() - log_z), "bound", bound)
    assert abs(lz.mean() - log_z) <= bound
    means = np.array([np.asarray(r.particles, dtype=np.float64).mean(axis=0) for r in results])
    se = means.std(axis=0, ddof=1) / np.sqrt(len(means))
    z = np.abs(means.mean(axis=0) - mean) / se
    print("posterior mean z", z)
    assert (z <= 5).all()


@pytest.fixture(scope="module")
def host_runs():
    prior, pot = linear_problem_host()
    return [TemperedSMC(prior, pot, beta=0.25, rng=seed).run(n_particles=512, steps_per_stage=5, ess_frac=0.5,
                                                             results="host", backend="host")
            for seed in range(16)]


def test_linear_problem_evidence_and_posterior_on_the_host_tier(host_runs):
    for r in host_runs:
        check_run_invariants(r, 512, 0.5)
        assert r.last_path == "host" and isinstance(r.particles, np.ndarray) and r.particles.shape == (512, 4)
        assert r.phi.shape == (512,) and np.isfinite(r.phi).all()
    print("stages", [r.n_stages for r in host_runs], "ladder of seed 0", host_runs[0].temperatures)
    check_against_exact(host_runs)


def test_run_is_deterministic_per_seed(host_runs):
    prior, pot = linear_problem_host()
    again = TemperedSMC(prior, pot, beta=0.25, rng=3).run(n_particles=512, steps_per_stage=5, ess_frac=0.5,
                                                          results="host", backend="host", record=True)
    first = host_runs[3]
    for f in ("particles", "phi", "temperatures", "ess", "log_evidence_increments", "accept_rate"):
        assert np.array_equal(getattr(first, f), getattr(again, f)), f
    assert first.log_evidence == again.log_evidence and first.n_stages == again.n_stages
    assert len(again.record) == again.n_stages
    for s, rec in enumerate(again.record):  # the record replays through the public pieces
        st = next_temperature(rec["phi"], again.temperatures[s], 256.0, backend="host")
        assert st.delta == rec["delta"] and st.t_next == again.temperatures[s + 1] and st.ess == again.ess[s]
        assert np.array_equal(systematic_resample(rec["phi"], None, st.delta, rec["u"], backend="host"),
                              rec["ancestors"])
        assert 0.0 <= rec["u"] < 1.0 and rec["particles"].shape == (512, 4)


def test_beta_schedule_callable_and_seed_changes_the_run():
    prior, pot = linear_problem_host()
    seen = []

    def beta(stage, t, prev):
        seen.append((stage, t, prev))
        return 0.5 if stage == 0 else 0.2

    r = TemperedSMC(prior, pot, beta=beta, rng=1).run(n_particles=128, steps_per_stage=2, backend="host",
                                                      results="host")
    assert [s for s, _, _ in seen] == list(range(r.n_stages)) and seen[0][2] is None
    assert [t for _, t, _ in seen] == r.temperatures[1:].tolist()
    assert [p for _, _, p in seen[1:]] == r.accept_rate[:-1].tolist()
    r2 = TemperedSMC(prior, pot, beta=0.25, rng=2).run(n_particles=128, steps_per_stage=2, backend="host",
                                                       results="host")
    assert not np.array_equal(r.particles, r2.particles)


# ------------------------------------------------------------- out of scope
def test_out_of_scope_compositions_raise():
    prior, pot = linear_problem_host()
    with pytest.raises(NotImplementedError, match="ConstrainAccepter"):
        TemperedSMC(prior, ConstrainAccepter(pCNAccepter(pot), lambda v: True))
    with pytest.raises(NotImplementedError, match="[Rr]andom-walk"):
        TemperedSMC(ConstStepStandardRWProposer(0.1, prior), pot)
    with pytest.raises(NotImplementedError, match="[Rr]andom-walk"):
        TemperedSMC(prior, StandardRWAccepter(pot, prior))
    with pytest.raises(NotImplementedError, match="chain_offset"):
        TemperedSMC(prior, pot, chain_offset=512)
    with pytest.raises(NotImplementedError, match="process group"):
        TemperedSMC(prior, pot, process_group=object())
    for kind in ("multinomial", "residual"):
        with pytest.raises(NotImplementedError, match="systematic only"):
            TemperedSMC(prior, pot).run(n_particles=8, resampling=kind, backend="host")
    with pytest.raises(TypeError, match="EvolutionPotential"):
        TemperedSMC(prior, lambda u: 0.0)
    with pytest.raises(ValueError, match="ess_frac"):
        TemperedSMC(prior, pot).run(n_particles=8, ess_frac=0.0, backend="host")
    # a pCN proposer or accepter in place of its distribution / potential is unwrapped
    smc = TemperedSMC(ConstSteppCNProposer(0.3, prior), pCNAccepter(pot))
    assert smc.prior.k == 4 and smc.potential is pot


# ---------------------------------------------------------------- sanitizer
def test_host_twins_clean_under_asan_ubsan():
    """ipmc_host_smc_selftest.cpp (its own main: sizes around the block edge, potentials that are not
    finite, every error return, each result checked) built from the host library's source with
    -fsanitize=address,undefined and run on its own; nothing loaded into Python is sanitized."""
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    b = subprocess.run(["make", "-C", CSRC, "-s", "host-smc-asan"], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in (b.stderr + b.stdout) and "cannot find" in (b.stderr + b.stdout):
        pytest.skip("sanitizer runtime not available")
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([os.path.join(REPO, "build", "host_san", "host_smc_selftest_asan")], capture_output=True,
                       text=True, env=env, timeout=600)
    report = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, report
    for marker in ("runtime error", "AddressSanitizer", "LeakSanitizer"):
        assert marker not in r.stderr, report
    assert "host smc selftest ok" in r.stdout

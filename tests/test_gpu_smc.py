"""Tempered SMC on the device (smc.py): the kernels against their host twins bit for bit,
ipmc_gather_rows against numpy indexing, the linear-Gaussian problem's exact evidence and posterior on the
device tier, a recorded run replayed through the host twins, and a Lorenz-96 run that stays in HBM."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from ip_mcmc_amd import (EvolutionPotential, GaussianDistribution, LinearOperator, Lorenz96Operator, TemperedSMC,
                         _abi, _hostlib, next_temperature, systematic_resample, tempering_sums)
from ip_mcmc_amd._lib import call
from test_smc_cpu import G_VEC, GAMMA, Y_OBS, check_against_exact, check_run_invariants, linear_problem_host

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 1023, 1024, 1025, 2049, 70001]
BIG = 1048577  # 1 025 blocks: one more than the workgroups of a launch


def _dev():
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


@functools.lru_cache(maxsize=None)
def _phi(n, name):
    """A read-only Φ (float64): a moderate spread, +inf / NaN entries around the block edges, a spread of
    10^4, or both of the latter (the large size's one input)."""
    r = np.random.default_rng(1000 + n)
    if name == "spread10":
        a = 3.0 + 10.0 * r.random(n)
    else:
        a = 1.0 + (1e4 if name in ("spread1e4", "mixed") else 10.0) * r.random(n) ** 2
    if name in ("nonfinite", "mixed"):
        a[0] = np.inf
        if n > 2:
            a[n // 2] = np.nan
            a[-1] = np.inf
        if n > 1030:
            a[1023], a[1024] = np.nan, np.inf
    a.setflags(write=False)
    return a


def _ref_of(phi):
    f = phi[np.isfinite(phi)]
    return float(f.min()) if f.size else 0.0


def _deltas(nd):
    return np.array([0.37]) if nd == 1 else np.concatenate([[0.0], np.geomspace(1e-4, 1.0, nd - 1)])


@functools.lru_cache(maxsize=None)
def _host_sums(n, name, dtype, nd):
    phi = _phi(n, name).astype(dtype)
    return _hostlib.temper_sums(phi, _ref_of(phi.astype(np.float64)), _deltas(nd))


def _device_sums(phi_t, ref, deltas):
    n, nd = phi_t.shape[0], len(deltas)
    need = ctypes.c_int64(0)
    call("ipmc_smc_workspace", n, nd, ctypes.byref(need))
    ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device=_dev())
    out = torch.full((2, nd), -1.0, dtype=torch.float64, device=_dev())
    d = np.ascontiguousarray(deltas, dtype=np.float64)
    call("ipmc_temper_sums", phi_t.data_ptr(), _abi.F64 if phi_t.dtype == torch.float64 else _abi.F32, n, ref,
         d.ctypes.data, nd, out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), need.value, _stream())
    o = out.cpu().numpy()
    return o[0], o[1]


def _device_cum(phi_t, ref, delta):
    n = phi_t.shape[0]
    need = ctypes.c_int64(0)
    call("ipmc_smc_workspace", n, 1, ctypes.byref(need))
    ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device=_dev())
    cum = torch.full((n,), -1.0, dtype=torch.float64, device=_dev())
    call("ipmc_temper_cumweights", phi_t.data_ptr(), _abi.F64 if phi_t.dtype == torch.float64 else _abi.F32, n, ref,
         delta, cum.data_ptr(), ws.data_ptr(), need.value, _stream())
    return cum


def _check_sums_and_cum(n, name, dtype, nds):
    phi = _phi(n, name).astype(dtype)
    ref = _ref_of(phi.astype(np.float64))
    phi_t = torch.from_numpy(phi).to(_dev())
    for nd in nds:
        want1, want2 = _host_sums(n, name, dtype, nd)
        got1, got2 = _device_sums(phi_t, ref, _deltas(nd))
        assert np.array_equal(got1, want1) and np.array_equal(got2, want2), (n, name, dtype, nd)
        again1, again2 = _device_sums(phi_t, ref, _deltas(nd))
        assert np.array_equal(again1, got1) and np.array_equal(again2, got2)
    cum = _device_cum(phi_t, ref, 0.37)
    want = _hostlib.temper_cumweights(phi, ref, 0.37)
    assert np.array_equal(cum.cpu().numpy(), want), (n, name, dtype)
    assert np.array_equal(_device_cum(phi_t, ref, 0.37).cpu().numpy(), want)
    return cum, want


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", SIZES)
def test_temper_kernels_equal_their_host_twins(n, dtype):
    for name in ("spread10", "nonfinite", "spread1e4"):
        _check_sums_and_cum(n, name, dtype, (1, 15, 64))


@pytest.mark.parametrize("dtype,nd", [(np.float64, 15), (np.float32, 64)])
def test_temper_kernels_past_the_first_pass_over_the_grid(dtype, nd):
    _check_sums_and_cum(BIG, "mixed", dtype, (nd,))


def _device_ancestors(cum_t, u, n_out):
    anc = torch.full((n_out,), -7, dtype=torch.int64, device=_dev())
    call("ipmc_systematic_ancestors", cum_t.data_ptr(), cum_t.shape[0], u, n_out, anc.data_ptr(), _stream())
    return anc.cpu().numpy()


@pytest.mark.parametrize("n", SIZES + [BIG])
def test_ancestors_equal_the_host_twin(n):
    name = "mixed" if n == BIG else ("nonfinite" if n > 1 else "spread10")  # n = 1: its one potential finite
    phi = _phi(n, name)
    delta = 0.002 if n == BIG else 0.37
    cum = _hostlib.temper_cumweights(phi, _ref_of(phi), delta)
    cum_t = torch.from_numpy(cum).to(_dev())
    for n_out in sorted({1, n, 3 * n} if n != BIG else {n, 1000}):
        for u in (0.0, 0.5, 0.999999):
            want = _hostlib.systematic_ancestors(cum, u, n_out)
            assert np.array_equal(_device_ancestors(cum_t, u, n_out), want), (n, n_out, u)
            assert want.min() >= 0 and (np.diff(want) >= 0).all()


def test_ancestors_special_totals():
    single = np.zeros(3000)
    single[1500:] = 4.0  # one parent holds all the weight
    got = _device_ancestors(torch.from_numpy(single).to(_dev()), 0.25, 5000)
    assert (got == 1500).all() and np.array_equal(got, _hostlib.systematic_ancestors(single, 0.25, 5000))
    for cum in (np.zeros(2500), np.array([1.0, np.nan]), np.array([1.0, np.inf])):
        got = _device_ancestors(torch.from_numpy(cum).to(_dev()), 0.5, 1300)
        assert (got == -1).all() and np.array_equal(got, _hostlib.systematic_ancestors(cum, 0.5, 1300))
    # through the public pieces, device tensors in and out
    phi = _phi(2049, "nonfinite")
    phi_t = torch.from_numpy(phi.copy()).to(_dev())
    anc = systematic_resample(phi_t, None, 0.37, 0.5)
    assert anc.is_cuda and np.array_equal(anc.cpu().numpy(), systematic_resample(phi, None, 0.37, 0.5, backend="host"))
    s_dev = tempering_sums(phi_t, None, np.linspace(0, 1, 100))
    s_host = tempering_sums(phi, None, np.linspace(0, 1, 100), backend="host")
    assert np.array_equal(s_dev[0], s_host[0]) and np.array_equal(s_dev[1], s_host[1])
    assert next_temperature(phi, 0.0, 900.0, backend="device") == next_temperature(phi, 0.0, 900.0, backend="host")


# ------------------------------------------------------------------ gather
def _indices(pattern, n_out, n_src, seed):
    r = np.random.default_rng(seed)
    if pattern == "equal":
        idx = np.full(n_out, n_src // 3, dtype=np.int64)
    elif pattern == "reversed":
        idx = (n_src - 1 - (np.arange(n_out, dtype=np.int64) % n_src))
    else:  # sorted with runs of repeats: what resampling produces
        idx = np.sort(r.integers(0, n_src, n_out)).astype(np.int64)
    if n_out >= 65:  # two indices outside the source: their rows keep the sentinel
        idx[7], idx[n_out - 3] = -1, n_src
    return idx


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", [1, 3, 40, 256])
def test_gather_rows_equals_numpy_indexing(k, dtype):
    n_src, s_stride, d_stride = 3001, k + 3, k + 5
    src = np.random.default_rng(k).standard_normal((n_src, s_stride)).astype(dtype)
    src_t = torch.from_numpy(src).to(_dev())
    for n_out in (1, 65, 70001):
        for pattern in ("equal", "reversed", "sorted"):
            idx = _indices(pattern, n_out, n_src, n_out + k)
            dst_t = torch.full((n_out, d_stride), -123.0, dtype=src_t.dtype, device=_dev())
            idx_t = torch.from_numpy(idx).to(_dev())
            call("ipmc_gather_rows", src_t.data_ptr(), _abi.F64 if dtype == np.float64 else _abi.F32, n_src, k,
                 s_stride, idx_t.data_ptr(), n_out, dst_t.data_ptr(), d_stride, _stream())
            got = dst_t.cpu().numpy()
            ok = (idx >= 0) & (idx < n_src)
            want = np.full((n_out, d_stride), -123.0, dtype=dtype)
            want[ok, :k] = src[idx[ok], :k]
            assert np.array_equal(got, want), (k, dtype, n_out, pattern)  # the padding and skipped rows: the sentinel
            assert n_out < 65 or (~ok).sum() == 2


# ------------------------------------------------------ the linear problem
def _linear_device():
    prior = GaussianDistribution(np.zeros(4), np.eye(4))
    pot = EvolutionPotential(LinearOperator(G_VEC), np.array([Y_OBS]),
                             GaussianDistribution(np.zeros(1), GAMMA**2 * np.eye(1)))
    return prior, pot


def test_linear_problem_evidence_and_posterior_on_the_device_tier():
    prior, pot = _linear_device()
    runs = [TemperedSMC(prior, pot, beta=0.25, rng=seed).run(n_particles=4096, steps_per_stage=5, ess_frac=0.5,
                                                             results="host")
            for seed in range(16)]
    for r in runs:
        check_run_invariants(r, 4096, 0.5)
        assert r.last_path == "device" and r.particles.shape == (4096, 4)
    print("stages", [r.n_stages for r in runs], "ladder of seed 0", runs[0].temperatures)
    check_against_exact(runs)


def test_linear_problem_in_f32_reaches_the_posterior():
    prior, pot = _linear_device()
    r = TemperedSMC(prior, pot, beta=0.25, rng=5, dtype=np.float32).run(n_particles=4096, steps_per_stage=5)
    check_run_invariants(r, 4096, 0.5)
    assert r.particles.is_cuda and r.particles.dtype == torch.float32 and r.phi.dtype == torch.float32
    assert torch.isfinite(r.particles).all() and np.isfinite(r.log_evidence)


def test_recorded_run_replays_through_the_host_twins():
    prior, pot = _linear_device()
    C = 1500  # not a multiple of the block
    r = TemperedSMC(prior, pot, beta=0.25, rng=11).run(n_particles=C, steps_per_stage=3, record=True, results="host")
    check_run_invariants(r, C, 0.5)
    assert len(r.record) == r.n_stages >= 2
    for s, rec in enumerate(r.record):
        phi = rec["phi"]
        assert phi.shape == (C,) and phi.dtype == np.float64
        st = next_temperature(phi, r.temperatures[s], 0.5 * C, backend="host")
        assert st.delta == rec["delta"] and st.ess == r.ess[s] and st.t_next == r.temperatures[s + 1]
        assert np.log(st.s1 / C) - st.delta * st.phi_ref == r.log_evidence_increments[s]
        cum = _hostlib.temper_cumweights(phi, st.phi_ref, st.delta)
        anc = _hostlib.systematic_ancestors(cum, rec["u"], C)
        assert np.array_equal(anc, rec["ancestors"])
        assert np.array_equal(rec["resampled"], rec["particles"][anc])
        assert rec["u"] == _hostlib.uniforms(11, 0, 1, 1 + s * 4)[0]  # the stream: draw, then (U, 3 steps) per stage
    # the resampling pieces forced to the other side give the same run: the host twins under the device tier ...
    twin = TemperedSMC(prior, pot, beta=0.25, rng=11).run(n_particles=C, steps_per_stage=3, results="host",
                                                          backend="host")
    assert np.array_equal(twin.particles, r.particles) and np.array_equal(twin.log_evidence_increments,
                                                                          r.log_evidence_increments)
    # ... and the kernels under the host tier (a Python forward map)
    prior_h, pot_h = linear_problem_host()
    a, b = (TemperedSMC(prior_h, pot_h, beta=0.25, rng=4).run(n_particles=300, steps_per_stage=2, results="host",
                                                              backend=side) for side in ("device", "host"))
    assert a.last_path == b.last_path == "host" and a.n_stages == b.n_stages
    assert np.array_equal(a.particles, b.particles) and np.array_equal(a.temperatures, b.temperatures)
    assert a.log_evidence == b.log_evidence


# ---------------------------------------------------------------- Lorenz-96
def test_lorenz96_run_stays_on_the_device():
    op = Lorenz96Operator(40, 8.0, dt=0.01, n_steps=50)
    truth = 0.5 * np.random.default_rng(4).standard_normal(40)
    y = op(truth) + 0.1 * np.random.default_rng(5).standard_normal(40)
    prior = GaussianDistribution(np.zeros(40), np.eye(40))
    pot = EvolutionPotential(op, y, GaussianDistribution(np.zeros(40), 0.1**2 * np.eye(40)))

    def run():
        return TemperedSMC(prior, pot, beta=0.1, rng=7).run(n_particles=2048, steps_per_stage=3, results="device")

    a, b = run(), run()
    check_run_invariants(a, 2048, 0.5)
    print("Lorenz-96 ladder:", a.n_stages, "stages", a.temperatures, "log Z", a.log_evidence)
    assert a.last_path == "device" and a.particles.is_cuda and a.phi.is_cuda and a.particles.shape == (2048, 40)
    # the driver's own device calls copied only scalars: Φ_ref, the sums of the searches, U
    assert 0 < a.driver_d2h_bytes <= a.n_stages * (16 + 11 * 2 * 15 * 8 + 8)
    for f in ("temperatures", "ess", "log_evidence_increments", "accept_rate"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert torch.equal(a.particles, b.particles) and torch.equal(a.phi, b.phi)
    host = TemperedSMC(prior, pot, beta=0.1, rng=7).run(n_particles=2048, steps_per_stage=3, results="host")
    assert isinstance(host.particles, np.ndarray) and np.array_equal(host.particles, a.particles.cpu().numpy())

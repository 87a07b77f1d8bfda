"""The Burgers HIP kernels against the CPU oracle, bit for bit, off the
reference's one geometry: every (cells per lane, lanes per group) instance the
library compiles, with a partly filled and with a full group; groups of one
live lane (N = 4, 8); observation windows of every length the pairwise sum
treats differently, on the domain's edges, empty, reversed and duplicate; 1
and 64 windows; the CFL iteration cap; and the grid sizes the library refuses.
The oracle is held to plain numpy on the same operators in
test_burgers_geometry_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from burgers_reference import (CASE_IDS, DEFAULT_DOMAIN, NU, base_u, case_by_id, input_rows, layout,  # noqa: E402
                               make_operator)
from test_gpu_parity import _assert_same, _np, _stream, _sweep_device, _sweep_oracle, _t  # noqa: E402

DTYPES = [torch.float64, torch.float32]
N_EVAL = 75  # chains per forward / potential launch: no multiple of 256 / GS, the last block is partial


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _length(op):
    return op.N * float(op.dx)


def _eval_inputs(op, dtype):
    """The shared input rows, then random states around the base up to N_EVAL chains."""
    rows = input_rows(op, _np(dtype))
    L = _length(op)
    rng = np.random.default_rng(op.N)
    fill = base_u((0.0, L)) + np.array([0.2, 0.2, 0.1 * L]) * rng.normal(size=(N_EVAL - len(rows), 3))
    return np.concatenate([rows, fill])


# ------------------------------------------------------ forward and potential
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_forward_and_potential_bit_exact(dev, orc, cid, dtype):
    from ip_mcmc_amd import EvolutionPotential, GaussianDistribution

    op = make_operator(case_by_id(cid))
    cpl, gs = layout(op.N)
    assert 64 <= N_EVAL <= 96 and N_EVAL % (256 // gs) != 0
    U = _eval_inputs(op, dtype)
    g = op.forward_device(_t(U, dtype, dev)).cpu().numpy()
    go = orc.forward(op, U, _np(dtype))
    assert np.isfinite(go[0]).all()
    assert np.array_equal(g, go, equal_nan=True), (cid, np.nanmax(np.abs(g - go)))
    rng = np.random.default_rng(5)
    y = go[0] + 0.05 * rng.normal(size=op.q)
    ginv = 1.0 / (0.1 + rng.random(op.q))
    pot = EvolutionPotential(op, y, GaussianDistribution(np.zeros(op.q), np.diag(1 / ginv**2)))
    phi = pot.phi_device(_t(U, dtype, dev)).cpu().numpy()
    phio = orc.potential(op, U, y, pot.device_terms()[1], _np(dtype))
    assert np.array_equal(phi, phio, equal_nan=True), cid
    assert np.array_equal(np.isposinf(phio), np.isnan(go[:, 0]))


# -------------------------------------------------------------------- init Φ
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", ["N4-std-cfl-fma-nu0.002", "N8-std-fixed-reference-nu0.002",
                                 "N512-std-cfl-reference-nu0", "N512-max-cfl-fma-nu0.002"])
def test_init_phi_with_regularizer_bit_exact(dev, orc, cid, dtype):
    """ipmc_init_phi on a group of one live lane and on the (8, 64) layout."""
    from ip_mcmc_amd import _abi
    from ip_mcmc_amd._lib import call

    op = make_operator(case_by_id(cid))
    assert op.N // layout(op.N)[0] == 1 or layout(op.N) == (8, 64)
    U0 = _eval_inputs(op, dtype)
    npd = _np(dtype)
    y = orc.forward(op, U0[:1])[0] + 0.05
    ginv = np.full(op.q, 4.0)
    rs = np.array([0.5, 1.0, 2.0])
    want = orc.init_phi(op, np.ascontiguousarray(U0.astype(npd)), y, ginv, reg_scale=rs)
    U, yt, gt, rt = _t(U0, dtype, dev), _t(y, dtype, dev), _t(ginv, dtype, dev), _t(rs, dtype, dev)
    phi = torch.empty(len(U0), dtype=dtype, device=dev)
    m, _ = op.model(dtype, dev)
    s = _abi.IpmcSweep()
    s.dtype = _abi.F64 if dtype == torch.float64 else _abi.F32
    s.n_chains, s.u, s.phi = len(U0), U.data_ptr(), phi.data_ptr()
    s.y, s.gamma_inv, s.reg_scale = yt.data_ptr(), gt.data_ptr(), rt.data_ptr()
    call("ipmc_init_phi", C.byref(m), C.byref(s), _stream(dev))
    torch.cuda.synchronize(dev)
    assert np.isfinite(want).any()
    assert np.array_equal(phi.cpu().numpy(), want, equal_nan=True)


# --------------------------------------------------------------------- sweep
SWEEP_GRIDS = [(4, DEFAULT_DOMAIN), (8, DEFAULT_DOMAIN), (12, DEFAULT_DOMAIN), (16, DEFAULT_DOMAIN),
               (24, DEFAULT_DOMAIN), (64, (0.0, 3.0)), (68, DEFAULT_DOMAIN), (128, DEFAULT_DOMAIN),
               (132, DEFAULT_DOMAIN), (136, DEFAULT_DOMAIN), (200, DEFAULT_DOMAIN), (256, DEFAULT_DOMAIN),
               (264, DEFAULT_DOMAIN), (512, DEFAULT_DOMAIN)]
# the sequential kernel, the library's choice, and every forced width the group size admits
# (w * GS <= 64, or w * GS = 256: one chain per block)
SPEC_WIDTHS = {16: (1, 0, 2, 4, 16), 32: (1, 0, 2, 8), 64: (1, 0, 4)}
N_SWEEP, STEPS = 40, 4


def _sweep_case(N, domain, dt_mode="cfl", arith="fma", nu=0.0, **over):
    case = dict(id=f"sweep-N{N}", N=N, domain=domain, q_mode="std", dt_mode=dt_mode, arith=arith, nu=nu,
                meas_scale=10.0)
    return make_operator(case, **over)


def _physics(k):
    """Two operators per grid: inviscid and viscous, the arithmetic modes and
    the second one's dt mode alternating from grid to grid."""
    a, b = ("reference", "fma") if k % 2 == 0 else ("fma", "reference")
    return [dict(dt_mode="cfl", arith=a, nu=0.0), dict(dt_mode="fixed" if k % 2 else "cfl", arith=b, nu=NU)]


def _layouts(N):
    """(lanes_per_chain, cells per lane, group size) of every layout the library accepts for N."""
    return [(lanes,) + layout(N, lanes) for lanes in (0, 16, 32, 64) if layout(N, lanes)]


def _problem(orc, op, dtype, seed, n=N_SWEEP, spread=0.1):
    L = _length(op)
    rng = np.random.default_rng(seed)
    base = base_u((0.0, L))
    U0 = base + spread * np.array([1.0, 1.0, 0.5 * L]) * rng.normal(size=(n, 3))
    U0 = U0.astype(_np(dtype)).astype(np.float64)
    y = orc.forward(op, base[None, :])[0] + 0.05 * rng.normal(size=op.q)
    assert np.isfinite(y).all()
    ginv = np.full(op.q, 2.0)
    sq = 0.25 * np.array([1.0, 1.0, 0.5 * L])
    return U0, y, ginv, sq


def test_sweep_set_covers_every_compiled_layout():
    """The sweeps below launch all six (cells per lane, group size) instances,
    each with a partly filled group and with a full one, and the block-wide
    speculation of a 64-lane group with 8 cells per lane."""
    seen = set()
    for N, _ in SWEEP_GRIDS:
        for lanes, cpl, gs in _layouts(N):
            seen.add((cpl, gs, N // cpl == gs))
    for cpl in (8, 4):
        for gs in (16, 32, 64):
            assert (cpl, gs, False) in seen and (cpl, gs, True) in seen, (cpl, gs, sorted(seen))
    assert {c for c, g, _ in seen} == {4, 8} and {g for c, g, _ in seen} == {16, 32, 64}
    assert 4 in SPEC_WIDTHS[64] and (8, 64, True) in seen
    assert any(N // cpl == 1 for N, _ in SWEEP_GRIDS for _, cpl, _ in _layouts(N)), "no group of one live lane"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", range(len(SWEEP_GRIDS)), ids=[f"N{n}" for n, _ in SWEEP_GRIDS])
def test_sweep_every_layout_and_width_bit_exact(dev, orc, k, dtype):
    N, domain = SWEEP_GRIDS[k]
    accepted = 0
    for phys in _physics(k):
        op = _sweep_case(N, domain, **phys)
        U0, y, ginv, sq = _problem(orc, op, dtype, seed=N)
        phi0 = orc.potential(op, U0, y, ginv, _np(dtype)).astype(np.float64)
        o = _sweep_oracle(orc, op, U0, phi0, y, ginv, sq, 0.15, 3, 0, STEPS, dtype)
        accepted += int(o["acc"].sum())
        for lanes, cpl, gs in _layouts(N):
            for spec in SPEC_WIDTHS[gs]:
                d = _sweep_device(op, U0, phi0, y, ginv, sq, 0.15, 3, 0, STEPS, dtype, dev, lanes=lanes, spec=spec)
                _assert_same(d, o, (N, phys, lanes, cpl, gs, spec))
                assert np.array_equal(d["samp"], o["u"])
    assert accepted > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_rw_regularizer_on_512_cells(dev, orc, dtype):
    op = _sweep_case(512, DEFAULT_DOMAIN, arith="fma", nu=NU)
    U0, y, ginv, sq = _problem(orc, op, dtype, seed=1)
    rs = np.array([0.5, 1.0, 2.0])
    phi0 = orc.init_phi(op, np.ascontiguousarray(U0.astype(_np(dtype))), y, ginv, reg_scale=rs).astype(np.float64)
    o = _sweep_oracle(orc, op, U0, phi0, y, ginv, sq, 0.1, 4, 3, STEPS, dtype, proposal="rw", reg_scale=rs)
    assert o["acc"].sum() > 0
    for spec in SPEC_WIDTHS[64]:
        d = _sweep_device(op, U0, phi0, y, ginv, sq, 0.1, 4, 3, STEPS, dtype, dev, proposal="rw", reg_scale=rs,
                          spec=spec)
        _assert_same(d, o, ("rw", spec))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_box_constraint_on_a_ragged_group(dev, orc, dtype):
    op = _sweep_case(136, DEFAULT_DOMAIN, arith="reference")
    assert layout(136) == (8, 32)
    U0, y, ginv, sq = _problem(orc, op, dtype, seed=2)
    phi0 = orc.potential(op, U0, y, ginv, _np(dtype)).astype(np.float64)
    box = (np.array([-np.inf, -np.inf, 0.0]), np.array([np.inf, np.inf, 0.5]), op.theta0)
    o = _sweep_oracle(orc, op, U0, phi0, y, ginv, sq, 0.15, 7, 0, STEPS, dtype, box=box)
    assert (o["calls"] < STEPS).any() and o["calls"].sum() > 0, "the box rejected nothing, or everything"
    assert o["acc"].sum() > 0
    for spec in SPEC_WIDTHS[32]:
        d = _sweep_device(op, U0, phi0, y, ginv, sq, 0.15, 7, 0, STEPS, dtype, dev, box=box, spec=spec)
        _assert_same(d, o, ("box", spec))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_running_sums_on_a_ragged_group(dev, orc, dtype):
    op = _sweep_case(24, DEFAULT_DOMAIN, arith="fma", nu=NU)
    assert layout(24) == (8, 16)
    U0, y, ginv, sq = _problem(orc, op, dtype, seed=3)
    phi0 = orc.potential(op, U0, y, ginv, _np(dtype)).astype(np.float64)
    o = _sweep_oracle(orc, op, U0, phi0, y, ginv, sq, 0.15, 9, 0, STEPS, dtype, want_sums=True)
    assert o["acc"].sum() > 0
    for spec in SPEC_WIDTHS[16]:
        d = _sweep_device(op, U0, phi0, y, ginv, sq, 0.15, 9, 0, STEPS, dtype, dev, want_sums=True, spec=spec)
        _assert_same(d, o, ("sums", spec))
        assert np.array_equal(d["sum_u"], o["sum_u"]) and np.array_equal(d["sum_u2"], o["sum_u2"]), spec


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_across_the_iteration_cap(dev, orc, dtype):
    """max_iter = the median of the chains' CFL iteration counts at u0: about
    half the chains start at Phi = +inf, and proposals land on either side.  A
    chain at +inf accepts every valid proposal (inf - finite > log r) and
    rejects every invalid one (inf - inf is NaN)."""
    kw = dict(arith="reference")
    free = _sweep_case(68, DEFAULT_DOMAIN, **kw)
    assert layout(68) == (4, 32)
    U0, y, ginv, sq = _problem(orc, free, dtype, seed=4)
    npd = _np(dtype)
    iters = np.full(N_SWEEP, -1)
    for m in range(1, 120):  # a chain's count: the smallest cap its G survives
        ok = np.isfinite(orc.forward(_sweep_case(68, DEFAULT_DOMAIN, max_iter=m, **kw), U0, npd)).all(axis=1)
        iters[(iters < 0) & ok] = m
        if (iters > 0).all():
            break
    assert (iters > 0).all() and iters.min() < iters.max(), iters
    op = _sweep_case(68, DEFAULT_DOMAIN, max_iter=int(np.median(iters)), **kw)
    phi0 = orc.potential(op, U0, y, ginv, npd).astype(np.float64)
    inf0 = np.isposinf(phi0)
    assert inf0.any() and np.isfinite(phi0).any(), "every chain starts on one side of the cap"
    o = _sweep_oracle(orc, op, U0, phi0, y, ginv, sq, 0.15, 11, 0, STEPS, dtype)
    assert (inf0 & np.isfinite(o["phi"])).any(), "no valid proposal from a chain at +inf: vacuous"
    assert (inf0 & (o["acc"] < STEPS)).any(), "no invalid proposal from a chain at +inf: vacuous"
    assert o["acc"].sum() > 0
    for spec in SPEC_WIDTHS[32]:
        d = _sweep_device(op, U0, phi0, y, ginv, sq, 0.15, 11, 0, STEPS, dtype, dev, spec=spec)
        for key in ("u", "phi", "acc", "calls"):
            assert np.array_equal(d[key], o[key], equal_nan=True), ("cap", spec, key)


# ------------------------------------------------------------- unsupported N
def _raw_sweep(op, dtype, dev, lanes):
    """An ipmc_pcn_sweep call whose outputs stay in reach: (model, sweep, outputs, keep-alive)."""
    from ip_mcmc_amd import _abi

    U = torch.full((8, 3), 0.125, dtype=dtype, device=dev)
    phi = torch.full((8,), 7.0, dtype=dtype, device=dev)
    acc = torch.full((8,), 5, dtype=torch.int64, device=dev)
    samp = torch.full((8, 3), -3.0, dtype=dtype, device=dev)
    keep = [_t(np.zeros(op.q), dtype, dev), _t(np.ones(op.q), dtype, dev), _t(np.ones(3), dtype, dev)]
    m, _ = op.model(dtype, dev)
    s = _abi.IpmcSweep()
    s.dtype = _abi.F64 if dtype == torch.float64 else _abi.F32
    s.lanes_per_chain, s.spec_width, s.n_chains = lanes, 1, 8
    s.u, s.phi, s.accepts = U.data_ptr(), phi.data_ptr(), acc.data_ptr()
    s.y, s.gamma_inv, s.prior_sqrt = (t.data_ptr() for t in keep)
    s.beta, s.contraction = 0.6, 0.8
    s.seed, s.step0, s.n_steps = 1, 0, 2
    s.sample_out, s.sample_stride = samp.data_ptr(), 3
    return m, s, (U, phi, acc, samp), keep


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,lanes", [(6, 0), (260, 0), (516, 0), (520, 0), (256, 16)])
def test_unsupported_grid_sizes_are_refused(dev, N, lanes, dtype):
    """N must be a multiple of 8 up to 512 or a multiple of 4 up to 256;
    lanes_per_chain must leave 4 or 8 cells per lane.  The library says so
    (IPMC_ERR_UNSUPPORTED) and writes nothing."""
    from ip_mcmc_amd import BurgersOperator
    from ip_mcmc_amd._lib import UnsupportedOnDevice, call
    from ip_mcmc_amd.device import abi_dtype

    assert layout(N, lanes) is None
    op = BurgersOperator(N=N, T=0.1)
    m, s, outs, keep = _raw_sweep(op, dtype, dev, lanes)
    before = [t.clone() for t in outs]
    with pytest.raises(UnsupportedOnDevice, match=f"N={N} "):
        call("ipmc_pcn_sweep", C.byref(m), C.byref(s), _stream(dev))
    torch.cuda.synchronize(dev)
    assert all(torch.equal(a, b) for a, b in zip(outs, before))
    if lanes == 0:  # ipmc_forward and ipmc_potential take no layout
        u = torch.zeros((8, 3), dtype=dtype, device=dev)
        out = torch.full((8, op.q), -3.0, dtype=dtype, device=dev)
        with pytest.raises(UnsupportedOnDevice, match=f"N={N} "):
            call("ipmc_forward", C.byref(m), abi_dtype(dtype), 8, u.data_ptr(), out.data_ptr(), _stream(dev))
        ph = torch.full((8,), -3.0, dtype=dtype, device=dev)
        rule = "multiple of 8 and at most 512, or a multiple of 4 and at most 256"
        with pytest.raises(UnsupportedOnDevice, match=rule):
            call("ipmc_potential", C.byref(m), abi_dtype(dtype), 8, u.data_ptr(), keep[0].data_ptr(),
                 keep[1].data_ptr(), ph.data_ptr(), _stream(dev))
        torch.cuda.synchronize(dev)
        assert bool((out == -3.0).all()) and bool((ph == -3.0).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [4, 512])
def test_smallest_and_largest_grid_are_accepted(dev, orc, N, dtype):
    from ip_mcmc_amd import BurgersOperator

    op = BurgersOperator(N=N, T=0.1)
    U = np.zeros((3, 3))
    g = op.forward_device(_t(U, dtype, dev)).cpu().numpy()
    assert np.array_equal(g, orc.forward(op, U, _np(dtype)))
    m, s, outs, _ = _raw_sweep(op, dtype, dev, 0)
    from ip_mcmc_amd._lib import call

    call("ipmc_pcn_sweep", C.byref(m), C.byref(s), _stream(dev))
    torch.cuda.synchronize(dev)
    assert bool((outs[3] != -3.0).all())  # the final states were written

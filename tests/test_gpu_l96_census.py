"""Every compiled Lorenz-96 kernel instantiation against the oracle, bit for bit.

ipmc_l96_dispatch.hpp compiles l96_sweep_kernel, l96_spec_kernel,
l96_sweep_pk_kernel and l96_eval_kernel as a table over (D, lanes per chain,
dtype, arithmetic mode); tests/l96_census.py restates the table (pinned to the
library by test_l96_census_cpu.py) and the cases here are generated from it,
one per entry.  The per-lane code branches on the components per lane M = D /
LPC (the unrolled RK loop up to M = 10, the LDS park at fp64 M = 17-20, the
packed kernel's M = 20 Philox case), and the halos and group sums on LPC: a
fault at one (M, LPC) shows in the case of that name only.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import l96_census as LC  # noqa: E402
from test_gpu_parity import _assert_same, _np, _problem, _stream, _sweep_device, _t  # noqa: E402

OUTPUTS = ("u", "phi", "acc", "calls", "samp", "sum_u", "sum_u2")


@pytest.fixture(scope="module")
def dev_census():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("case", LC.SWEEP_CASES, ids=LC.case_id)
def test_sweep_census(dev_census, orc, case):
    """l96_sweep_kernel (cpl 1) or l96_sweep_pk_kernel (cpl 2) at the requested
    layout equals the oracle; for cpl 1 l96_spec_kernel with 2 slots (within
    one wave) and with 256 / LPC slots (one chain per block) equals it too."""
    D, lpc, dt, cpl = case
    dtype = LC.torch_dtype(dt)
    for arith in LC.ARITHS:
        op, (U0, phi0, y, ginv, sq), o = LC.oracle_sweep(orc, D, dt, arith)
        assert 0 < o["acc"].sum() < LC.N_CHAINS * LC.N_PCN, (case, arith)

        def run(spec):
            return _sweep_device(op, U0, phi0, y, ginv, sq, LC.BETA, LC.SEED, LC.STEP0, LC.N_PCN, dtype, dev_census,
                                 lanes=lpc, cpl=cpl, spec=spec, want_sums=True)

        d = run(1)
        _assert_same(d, o, (case, arith))
        assert np.array_equal(d["samp"], o["u"]), (case, arith)
        assert np.array_equal(d["sum_u"], o["sum_u"]) and np.array_equal(d["sum_u2"], o["sum_u2"]), (case, arith)
        if cpl == 1:
            for spec in (2, 256 // lpc):
                ds = run(spec)
                for key in OUTPUTS:
                    assert np.array_equal(ds[key], d[key]), (case, arith, spec, key)


def _auto_lpc(op, dtype, dev, n):
    from ip_mcmc_amd import _abi
    from ip_mcmc_amd._lib import lib

    m, _ = op.model(dtype, dev)
    return lib().ipmc_auto_layout(C.byref(m), _abi.F64, n) % 100


@pytest.mark.parametrize("case", LC.EVAL_CASES, ids=LC.case_id)
def test_eval_census(dev_census, orc, case):
    """l96_eval_kernel<T, D, LPC, FM, PHI> behind ipmc_forward and
    ipmc_potential.  The eval kernels take no layout argument: dispatch_eval
    asks the layout rule for the fp64 layout of the ensemble size, and 65 536 /
    LPC chains is the smallest ensemble at which the rule picks LPC."""
    from ip_mcmc_amd import EvolutionPotential, GaussianDistribution

    D, lpc, dt = case
    dtype = LC.torch_dtype(dt)
    n = 65536 // lpc
    rng = np.random.default_rng(1000 * D + lpc)
    U = 0.3 * rng.normal(size=(n, D))
    Ut = _t(U, dtype, dev_census)
    ginv = 1.0 / (0.1 + rng.random(D))
    noise = 0.1 * rng.normal(size=D)
    for arith in LC.ARITHS:
        op = LC.l96_op(D, arith, n_steps=3)
        assert _auto_lpc(op, dtype, dev_census, n) == lpc, "the layout rule changed: this case would run another kernel"
        go = orc.forward(op, U, _np(dtype))
        g = op.forward_device(Ut).cpu().numpy()
        assert np.array_equal(g, go), (case, arith, np.abs(g - go).max())
        y = go[0] + noise
        pot = EvolutionPotential(op, y, GaussianDistribution(np.zeros(D), np.diag(1 / ginv**2)))
        phi = pot.phi_device(Ut).cpu().numpy()
        phio = orc.potential(op, U, y, pot.device_terms()[1], _np(dtype))
        assert phi.shape == (n,) and np.array_equal(phi, phio), (case, arith)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("D,lpc", [(36, 2), (128, 8)])
def test_init_phi_census(dev_census, orc, D, lpc, dt):
    """ipmc_init_phi (the eval kernel, then the regularizer) on an interleaved
    8-lane layout and on a quad-permute one, 18 and 16 components per lane."""
    from ip_mcmc_amd import _abi
    from ip_mcmc_amd._lib import call

    dtype = LC.torch_dtype(dt)
    n = 65536 // lpc
    for arith in LC.ARITHS:
        op = LC.l96_op(D, arith, n_steps=3)
        assert _auto_lpc(op, dtype, dev_census, n) == lpc
        U0, _, y, ginv, _ = _problem(op, n, dtype, orc, seed=D + 1)
        rs = np.linspace(0.5, 2.0, D)
        want = orc.init_phi(op, U0.astype(_np(dtype)), y, ginv, reg_scale=rs)
        U, yt, gt, rt = (_t(a, dtype, dev_census) for a in (U0, y, ginv, rs))
        phi = torch.empty(n, dtype=dtype, device=dev_census)
        m, _ = op.model(dtype, dev_census)
        s = _abi.IpmcSweep()
        s.dtype = _abi.F64 if dt == "f64" else _abi.F32
        s.n_chains, s.u, s.phi = n, U.data_ptr(), phi.data_ptr()
        s.y, s.gamma_inv, s.reg_scale = yt.data_ptr(), gt.data_ptr(), rt.data_ptr()
        call("ipmc_init_phi", C.byref(m), C.byref(s), _stream(dev_census))
        torch.cuda.synchronize(dev_census)
        assert np.array_equal(phi.cpu().numpy(), want), (D, lpc, dt, arith)

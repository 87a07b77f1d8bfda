"""The Lorenz-96 instantiation table, checked without a GPU.

tests/l96_census.py restates the rule of ipmc_l96_dispatch.hpp (l96_ok over
IPMC_L96_DIMS); test_gpu_l96_census.py runs one case per entry of it.  Here the
restated table is pinned to the library through ipmc_plan_sweep (which
validates a requested layout on the host, before anything reaches a device),
its sizes are pinned so that it cannot be emptied, and the census recipe is
pinned, on the oracle alone, to accept some proposals and reject some in every
case.
"""
import ctypes as C

import pytest

import l96_census as LC
from ip_mcmc_amd import _abi, _lib

DUMMY = 0x10000  # a non-NULL "device pointer"; ipmc_plan_sweep never dereferences it


@pytest.fixture(scope="module")
def h():
    return _lib.lib()


def test_table_sizes():
    """46 (D, LPC) pairs at 8 bytes per component (fp64, packed fp32), 57 at 4:
    298 sequential, 206 speculative and 412 eval kernels over both arithmetic
    modes (and both PHI values of the eval kernel)."""
    for key, want in LC.TABLE_SIZES.items():
        assert len(LC.pairs(LC.STORAGE[key])) == want, key
    assert len(LC.SWEEP_CASES) == 46 + 57 + 46 and len(set(LC.SWEEP_CASES)) == 149
    assert len(LC.EVAL_CASES) == 2 * 46
    assert 2 * len(LC.SWEEP_CASES) == 298
    assert 2 * (46 + 57) == 206 and 2 * 2 * (46 + 57) == 412
    assert len(set(LC.DIMS)) == 18
    # every dim and every LPC has a kernel; more than 20 components per lane only in fp32
    for size in (4, 8):
        assert {D for D, _ in LC.pairs(size)} == set(LC.DIMS)
        assert {lpc for _, lpc in LC.pairs(size)} == set(LC.LPCS)
    assert max(D // lpc for D, lpc in LC.pairs(8)) == 20 and max(D // lpc for D, lpc in LC.pairs(4)) == 40
    assert len(set(LC.pairs(4)) - set(LC.pairs(8))) == 11 and set(LC.pairs(8)) <= set(LC.pairs(4))


@pytest.mark.parametrize("dt,cpl", [("f64", 1), ("f64", 2), ("f32", 1), ("f32", 2)])
def test_table_equals_what_plan_sweep_accepts(h, dt, cpl):
    """For every D in 2..260 and a requested LPC (compiled ones and 3 and 32)
    ipmc_plan_sweep succeeds exactly on the Python table and otherwise reports
    IPMC_ERR_UNSUPPORTED with the dim and the lanes in the message.  fp64 has
    no packed layout: (f64, cpl 2) is the empty table."""
    size = LC.STORAGE.get((dt, cpl))
    accepted = []
    for D in range(2, 261):
        m = _abi.IpmcModel()
        m.kind, m.arith, m.k, m.q, m.dim, m.n_steps, m.dt = _abi.MODEL_LORENZ96, _abi.ARITH_FMA, D, D, D, 7, 0.005
        m.x0 = m.theta0 = DUMMY
        for lpc in (1, 2, 3, 4, 8, 16, 32):
            s = _abi.IpmcSweep()
            s.dtype = _abi.F64 if dt == "f64" else _abi.F32
            s.n_chains, s.n_steps = 37, 4
            s.lanes_per_chain, s.chains_per_lane, s.spec_width = lpc, cpl, 1
            p = _abi.IpmcPlan()
            rc = h.ipmc_plan_sweep(C.byref(m), C.byref(s), C.byref(p))
            want = size is not None and LC.compiled(D, lpc, size)
            if want:
                assert rc == _abi.OK, (D, lpc, h.ipmc_last_error())
                assert (p.lanes_per_chain, p.chains_per_lane, p.spec_width) == (lpc, cpl, 1)
                accepted.append((D, lpc))
            else:
                assert rc == _abi.ERR_UNSUPPORTED, (D, lpc, rc)
                text = h.ipmc_last_error().decode()
                assert f"dim={D} " in text and f"lanes_per_chain={lpc} " in text, text
    assert accepted == (LC.pairs(size) if size else [])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("D", LC.DIMS)
def test_census_recipe_accepts_and_rejects(orc, D, dt):
    """The sweep census is not vacuous: in every case (the oracle's sweep
    depends on D, dtype and arithmetic only) some of the 37 x 4 proposals are
    accepted and some rejected."""
    for arith in LC.ARITHS:
        _, _, o = LC.oracle_sweep(orc, D, dt, arith)
        assert 0 < o["acc"].sum() < LC.N_CHAINS * LC.N_PCN, (D, dt, arith, int(o["acc"].sum()))
        assert (o["calls"] == LC.N_PCN).all()  # no box: every proposal is evaluated

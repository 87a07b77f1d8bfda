"""The CPU oracle's Burgers forward map against plain numpy (burgers_reference.py)
off the reference's one geometry: grids from 4 to 512 cells, a shifted domain,
observation windows of every length the pairwise sum treats differently
(nt < 8, the 8-accumulator loop run 1-16 times, every tail), windows on the
domain's edges, empty, reversed, overlapping and duplicate windows, 1 and 64
windows, both dt modes, viscous and inviscid, both arithmetic modes, and the
CFL iteration cap.  The HIP kernels are held to the oracle bit for bit on the
same operators in test_gpu_burgers_geometry.py.
"""
import numpy as np
import pytest

from burgers_reference import (CASE_IDS, CASES, burgers_numpy, case_by_id, input_rows, layout, make_operator,
                               nt_classes, numpy_results)

# Worst |oracle_f32 - numpy_f64| / max(|numpy_f64|, 1e-3) over every case and row
# below, measured: 9.53e-6 (N=68, CFL, FMA arith, inviscid; the next are 8.8e-6 at N=4 and
# 7.4e-6 at N=16).  The bound is 4x that: a float32 CFL run may take one step more or
# fewer than float64 near t = T.
F32_WORST = 9.53e-6
F32_TOL = 4 * F32_WORST
SPREAD = 0.05  # a window whose cells span at least this much sees a one-cell shift


def _rel(got, want):
    return np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-3)


def _want(res):
    return np.stack([r[0] for r in res])


def test_windows_cover_every_regime_of_the_pairwise_sum():
    """The searchsorted limits are the intended cells (make_operator asserts
    it) and their term counts nt = hi - lo - 1 cover every class the grid has
    room for, the edges of the domain, the degenerate windows and a duplicate."""
    seen = set()
    for case in CASES:
        key = (case["N"], case["q_mode"])
        if key in seen:
            continue
        seen.add(key)
        op = make_operator(case)
        N, lo, hi = op.N, op.win_lo, op.win_hi
        nt = hi - lo - 1
        if case["q_mode"] == "one":
            assert op.q == 1
            continue
        assert set(nt_classes(N)) <= set(nt.tolist()), (N, sorted(set(nt.tolist())))
        assert (hi == lo).any() and (hi == lo + 1).any() and (hi < lo).any(), N  # nt = -1, 0 and below
        assert (lo == 0).any() and (hi == N).any(), N
        assert nt.max() <= 128
        wins = list(zip(lo.tolist(), hi.tolist()))
        assert len(set(wins)) < len(wins), "no duplicate window"
        if N - 1 <= 128:
            assert (0, N) in wins
        if case["q_mode"] == "max":
            assert op.q == 64
    big = {n for n, _ in seen if n >= 132}
    assert big and all({127, 128} <= set(nt_classes(n)) for n in big)


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["N"] >= 64 and c["q_mode"] == "std"])
def test_state_varies_inside_the_windows(cid):
    """A constant window is blind to indexing: for every nt class >= 8 at
    least one window's cells span SPREAD or more in the base state."""
    op = make_operator(case_by_id(cid))
    v = numpy_results(cid, "float64")[1][0][2]
    nt = op.win_hi - op.win_lo - 1
    for cls in (c for c in nt_classes(op.N) if c >= 8):
        spans = [np.ptp(v[lo:hi]) for lo, hi, n in zip(op.win_lo, op.win_hi, nt) if n == cls]
        assert spans and max(spans) >= SPREAD, (cid, cls, spans)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_oracle_f64_is_numpy(orc, cid):
    """REFERENCE arith: the reference's operation order and numpy's pairwise
    sum, bit for bit.  FMA arith: the same scheme to rounding (the tolerance of
    test_viscous_burgers_is_the_central_difference_scheme)."""
    case = case_by_id(cid)
    op = make_operator(case)
    rows, res = numpy_results(cid, "float64")
    want = _want(res)
    got = orc.forward(op, rows)
    assert np.isfinite(want[0]).all(), "the base state must be valid"
    if case["dt_mode"] == "fixed":
        assert np.isnan(want[-1]).all() and np.isfinite(want[:-1]).all(), "the CFL guard row, and only it, trips"
    assert np.array_equal(np.isnan(got), np.isnan(want)), cid
    if case["arith"] == "reference":
        assert np.array_equal(got, want, equal_nan=True), (cid, np.nanmax(np.abs(got - want)))
    else:
        assert np.allclose(got, want, rtol=1e-10, atol=1e-12, equal_nan=True), (cid, np.nanmax(_rel(got, want)))
    phi = orc.potential(op, rows, np.zeros(op.q), np.ones(op.q))
    assert np.array_equal(np.isposinf(phi), np.isnan(want[:, 0])), cid


@pytest.mark.parametrize("cid", CASE_IDS)
def test_oracle_f32_is_close_to_numpy(orc, cid):
    """The float32 oracle against float64 numpy on the same (float32) inputs."""
    op = make_operator(case_by_id(cid))
    rows, res = numpy_results(cid, "float32")
    want = _want(res)
    got = orc.forward(op, rows, np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)), cid
    rel = np.nanmax(_rel(got, want), initial=0.0)
    print(f"f32 worst relative difference {cid}: {rel:.3e}")
    assert rel <= F32_TOL, (cid, rel)


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["q_mode"] == "std"])
def test_one_cell_shift_fails_every_comparison(cid):
    """Negative control: numpy's own G with every window moved by one cell
    fails the bit-exact, the 1e-10 and the float32 comparison on every window
    whose cells span SPREAD or more, so each of them can see an off-by-one."""
    case = case_by_id(cid)
    op = make_operator(case)
    rows, res = numpy_results(cid, "float64")
    G, _, v = res[0]
    shifted = [(lo + 1, hi + 1) if hi < op.N else (lo - 1, hi - 1) for lo, hi in zip(op.win_lo, op.win_hi)]
    Gs = burgers_numpy(op, rows[0], windows=shifted)[0]
    wide = [j for j, (lo, hi) in enumerate(zip(op.win_lo, op.win_hi)) if hi - lo >= 2 and np.ptp(v[lo:hi]) >= SPREAD]
    if op.N >= 64:
        assert wide, cid
    for j in wide:
        assert Gs[j] != G[j], (cid, j)
        assert not np.isclose(Gs[j], G[j], rtol=1e-10, atol=1e-12), (cid, j)
        assert _rel(Gs[j:j + 1], G[j:j + 1])[0] > F32_TOL, (cid, j, _rel(Gs[j:j + 1], G[j:j + 1])[0])


def test_library_refuses_exactly_the_grid_sizes_without_a_layout():
    """The library's argument check (it runs before anything reaches a device,
    as in test_abi_validation.py) refuses every N from 2 to 540 for which
    `layout` finds no (cells per lane, group size), and says which N it takes."""
    import ctypes as C

    from ip_mcmc_amd import _abi, _lib
    from test_abi_validation import DUMMY, _model, _sweep

    h = _lib.lib()

    def refused(N, lanes=0):
        m = _model(kind=_abi.MODEL_BURGERS, k=3, q=5, dim=N)
        m.n_windows, m.win_lo, m.win_hi = 5, DUMMY, DUMMY
        s = _sweep(k=3)
        s.lanes_per_chain = lanes
        rc = h.ipmc_pcn_sweep(C.byref(m), C.byref(s), None)
        assert rc == _abi.ERR_UNSUPPORTED, (N, lanes, rc)
        return h.ipmc_last_error().decode()

    bad = [N for N in range(2, 541) if layout(N) is None]
    assert {6, 260, 516, 520} <= set(bad) and not {4, 256, 264, 512} & set(bad)
    assert set(range(2, 541)) - set(bad) == set(range(4, 257, 4)) | set(range(8, 513, 8))
    for N in bad:
        msg = refused(N)
        assert f"N={N} " in msg and "multiple of 8 and at most 512, or a multiple of 4 and at most 256" in msg, msg
    for N, lanes in ((256, 16), (512, 32), (136, 16), (64, 64), (12, 8)):
        assert layout(N, lanes) is None
        assert f"N={N} lanes_per_chain={lanes} " in refused(N, lanes)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("arith", ["reference", "fma"])
@pytest.mark.parametrize("N", [8, 264])
def test_cfl_iteration_cap(orc, N, arith, dtype):
    """max_iter = the iterations the base state needs: the uncapped result bit
    for bit; one fewer: G = NaN and Phi = +inf."""
    case = case_by_id(f"N{N}-std-cfl-{arith}-nu0")
    free = make_operator(case)
    u = input_rows(free, dtype)[:1]
    need = burgers_numpy(free, u[0])[1]
    want = orc.forward(free, u, dtype)
    assert np.isfinite(want).all() and need >= 2
    if dtype == np.float32:  # the float32 run's own count, from the oracle
        finite = [m for m in range(need - 3, need + 4)
                  if np.isfinite(orc.forward(make_operator(case, max_iter=m), u, dtype)).all()]
        assert finite and finite[0] > need - 3 and finite == list(range(finite[0], need + 4)), (need, finite)
        need = finite[0]
    y, ginv = np.zeros(free.q), np.ones(free.q)
    capped = make_operator(case, max_iter=need - 1)
    assert np.isnan(orc.forward(capped, u, dtype)).all()
    assert np.isposinf(orc.potential(capped, u, y, ginv, dtype)).all()
    exact = make_operator(case, max_iter=need)
    assert np.array_equal(orc.forward(exact, u, dtype), want)
    assert np.array_equal(orc.potential(exact, u, y, ginv, dtype), orc.potential(free, u, y, ginv, dtype))

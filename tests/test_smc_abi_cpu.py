"""Argument checks of the tempered-SMC entry points (include/ipmc.h: ipmc_smc_workspace, ipmc_temper_sums,
ipmc_temper_cumweights, ipmc_systematic_ancestors, ipmc_gather_rows), on the CPU: every call fails
validation, is a no-op or only computes a size before anything reaches the device
(tests/test_rank_abi_cpu.py's style; the pointers are dummies)."""
import ctypes

import numpy as np
import pytest

from ip_mcmc_amd import _abi, _hostlib, _lib, smc

DUMMY = 0x10000  # a non-NULL "device pointer"; never dereferenced by these calls
DUMMY2 = 0x40000000  # a second one, far from the first
F64, F32 = _abi.F64, _abi.F32
INV = _abi.ERR_INVALID


@pytest.fixture(scope="module")
def h():
    return _lib.lib()


def _status(h, rc, code, text):
    assert rc == code, (rc, h.ipmc_last_error())
    assert text in h.ipmc_last_error().decode()


def _workspace(h, n, nd):
    out = ctypes.c_int64(-1)
    assert h.ipmc_smc_workspace(n, nd, ctypes.byref(out)) == _abi.OK, h.ipmc_last_error()
    return out.value


def _deltas(*v):
    return np.array(v, dtype=np.float64)


def test_constants_and_abi_version(h):
    assert h.ipmc_abi_version() == _abi.ABI_VERSION == 13  # the entry points are additive
    assert _abi.SMC_BLOCK == smc.SMC_BLOCK == 1024 and _abi.SMC_MAX_DELTAS == smc.MAX_DELTAS == 64
    assert _hostlib.lib().ipmc_host_abi_version() == _hostlib.ABI_VERSION == 1


def test_smc_workspace_checks(h):
    f = h.ipmc_smc_workspace
    out = ctypes.c_int64(-1)
    ref = ctypes.byref(out)
    _status(h, f(-1, 15, ref), INV, "negative size")
    _status(h, f(100, -1, ref), INV, "negative size")
    _status(h, f(100, 0, ref), INV, "outside [1, 64]")
    _status(h, f(100, 65, ref), INV, "outside [1, 64]")
    _status(h, f(100, 15, None), INV, "NULL pointer")
    assert out.value == -1  # no failing call wrote a size
    assert f(0, 1, ref) == _abi.OK and out.value == 0  # no particle: nothing is needed
    sizes = [_workspace(h, n, 15) for n in (1, 1024, 1025, 2049, 1 << 20)]
    assert sizes[0] == sizes[1] > 0 and sizes == sorted(sizes) and sizes[2] > sizes[1]
    assert _workspace(h, 5000, 64) > _workspace(h, 5000, 15) > _workspace(h, 5000, 1) >= 2 * 5 * 8


def test_temper_sums_checks(h):
    f = h.ipmc_temper_sums
    d = _deltas(0.1, 0.2, 0.3)
    big = 1 << 40

    def args(phi=DUMMY, dtype=F64, n=5000, ref=1.0, deltas=d.ctypes.data, nd=3, s1=DUMMY, s2=DUMMY, ws=DUMMY,
             ws_bytes=big):
        return (phi, dtype, n, ref, deltas, nd, s1, s2, ws, ws_bytes, None)

    _status(h, f(*args(n=-1)), INV, "negative size")
    _status(h, f(*args(nd=-1)), INV, "negative size")
    _status(h, f(*args(ws_bytes=-1)), INV, "negative size")
    _status(h, f(*args(nd=0)), INV, "outside [1, 64]")
    _status(h, f(*args(nd=65)), INV, "outside [1, 64]")
    _status(h, f(*args(dtype=5)), INV, "bad dtype")
    _status(h, f(*args(phi=None)), INV, "NULL pointer")
    _status(h, f(*args(deltas=None)), INV, "NULL pointer")
    _status(h, f(*args(s1=None)), INV, "NULL pointer")
    _status(h, f(*args(s2=None)), INV, "NULL pointer")
    _status(h, f(*args(ws=None)), INV, "NULL pointer")
    need = _workspace(h, 5000, 3)
    _status(h, f(*args(ws_bytes=need - 1)), INV, f"ipmc_smc_workspace asks for {need}")
    _status(h, f(*args(ws_bytes=0)), INV, f"ipmc_smc_workspace asks for {need}")
    for bad in (-0.5, np.nan, np.inf):
        b = _deltas(0.1, bad, 0.3)
        _status(h, f(*args(deltas=b.ctypes.data)), INV, "deltas[1] is not a finite number >= 0")
    assert f(*args(phi=None, n=0, deltas=None, s1=None, s2=None, ws=None, ws_bytes=0)) == _abi.OK  # no-op


def test_temper_cumweights_checks(h):
    f = h.ipmc_temper_cumweights
    big = 1 << 40

    def args(phi=DUMMY, dtype=F64, n=5000, ref=1.0, delta=0.5, cum=DUMMY, ws=DUMMY, ws_bytes=big):
        return (phi, dtype, n, ref, delta, cum, ws, ws_bytes, None)

    _status(h, f(*args(n=-1)), INV, "negative size")
    _status(h, f(*args(ws_bytes=-1)), INV, "negative size")
    _status(h, f(*args(dtype=5)), INV, "bad dtype")
    _status(h, f(*args(phi=None)), INV, "NULL pointer")
    _status(h, f(*args(cum=None)), INV, "NULL pointer")
    _status(h, f(*args(ws=None)), INV, "NULL pointer")
    need = _workspace(h, 5000, 1)
    _status(h, f(*args(ws_bytes=need - 1)), INV, f"ipmc_smc_workspace asks for {need}")
    for bad in (-0.5, float("nan"), float("inf")):
        _status(h, f(*args(delta=bad)), INV, "delta is not a finite number >= 0")
    assert f(*args(phi=None, n=0, cum=None, ws=None, ws_bytes=0)) == _abi.OK  # no-op


def test_systematic_ancestors_checks(h):
    f = h.ipmc_systematic_ancestors

    def args(cum=DUMMY, n=5000, u=0.5, n_out=5000, anc=DUMMY):
        return (cum, n, u, n_out, anc, None)

    _status(h, f(*args(n=-1)), INV, "negative size")
    _status(h, f(*args(n_out=-1)), INV, "negative size")
    for bad in (1.0, -1e-9, 1.5, float("nan")):
        _status(h, f(*args(u=bad)), INV, "u outside [0, 1)")
    _status(h, f(*args(cum=None)), INV, "NULL pointer")
    _status(h, f(*args(anc=None)), INV, "NULL pointer")
    assert f(*args(cum=None, n=0, anc=None)) == _abi.OK  # no particle: a no-op
    assert f(*args(n_out=0, anc=None)) == _abi.OK  # no offspring


def test_gather_rows_checks(h):
    f = h.ipmc_gather_rows

    def args(src=DUMMY, dtype=F64, n_src=100, k=40, s_stride=40, idx=DUMMY, n_out=100, dst=DUMMY2, d_stride=40):
        return (src, dtype, n_src, k, s_stride, idx, n_out, dst, d_stride, None)

    _status(h, f(*args(n_src=-1)), INV, "negative size")
    _status(h, f(*args(n_out=-1)), INV, "negative size")
    _status(h, f(*args(k=-1)), INV, "negative size")
    _status(h, f(*args(s_stride=-40)), INV, "negative size")
    _status(h, f(*args(d_stride=-40)), INV, "negative size")
    _status(h, f(*args(k=0)), INV, "outside [1, 256]")
    _status(h, f(*args(k=257, s_stride=300, d_stride=300)), INV, "outside [1, 256]")
    _status(h, f(*args(s_stride=39)), INV, "stride is below k")
    _status(h, f(*args(d_stride=39)), INV, "stride is below k")
    _status(h, f(*args(dtype=5)), INV, "bad dtype")
    _status(h, f(*args(src=None)), INV, "NULL pointer")
    _status(h, f(*args(idx=None)), INV, "NULL pointer")
    _status(h, f(*args(dst=None)), INV, "NULL pointer")
    _status(h, f(*args(dst=DUMMY)), INV, "overlaps")  # in place
    _status(h, f(*args(dst=DUMMY + 99 * 40 * 8)), INV, "overlaps")  # the last source row
    _status(h, f(*args(dst=DUMMY - 8)), INV, "overlaps")
    _status(h, f(*args(n_src=1 << 62, s_stride=1 << 40)), INV, "overflows")
    assert f(*args(src=None, idx=None, n_out=0, dst=None)) == _abi.OK  # no row: a no-op

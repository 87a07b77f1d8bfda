"""Argument checks of the pooled sort and rank-score entry points
(include/ipmc.h: ipmc_sort_workspace, ipmc_pooled_sort, ipmc_rank_scores), on
the CPU: every call fails validation, is a no-op or only computes a size
before anything reaches the device (tests/test_convergence_abi_cpu.py's style;
the pointers are dummies)."""
import ctypes

import pytest

from ip_mcmc_amd import _abi, _lib, ranks

DUMMY = 0x10000  # a non-NULL "device pointer"; never dereferenced by these calls
F64, F32 = _abi.F64, _abi.F32
INV = _abi.ERR_INVALID


@pytest.fixture(scope="module")
def h():
    return _lib.lib()


def _status(h, rc, code, text):
    assert rc == code, (rc, h.ipmc_last_error())
    assert text in h.ipmc_last_error().decode()


def _workspace(h, C, n, k, dtype=F64):
    out = ctypes.c_int64(-1)
    assert h.ipmc_sort_workspace(C, n, k, dtype, ctypes.byref(out)) == _abi.OK, h.ipmc_last_error()
    return out.value


def test_abi_version_and_tile_constant(h):
    assert h.ipmc_abi_version() == _abi.ABI_VERSION == 13
    assert _abi.SORT_TILE == ranks.SORT_TILE == 4096


def test_sort_workspace_checks(h):
    f = h.ipmc_sort_workspace
    out = ctypes.c_int64(-1)
    ref = ctypes.byref(out)
    _status(h, f(-1, 20, 3, F64, ref), INV, "negative size")
    _status(h, f(4, -20, 3, F64, ref), INV, "negative size")
    _status(h, f(4, 20, -3, F64, ref), INV, "negative size")
    _status(h, f(4, 20, 0, F64, ref), INV, "outside [1, 256]")
    _status(h, f(4, 20, 257, F64, ref), INV, "outside [1, 256]")
    _status(h, f(4, 20, 3, 5, ref), INV, "bad dtype")
    _status(h, f(4, 20, 3, F64, None), INV, "NULL pointer")
    _status(h, f(1 << 16, 1 << 16, 3, F64, ref), INV, "2^32")  # S = 2^32: one too many for uint32
    _status(h, f(1 << 40, 1 << 40, 3, F64, ref), INV, "2^32")  # the product does not fit int64 either
    assert out.value == -1  # no failing call wrote a size
    assert f((1 << 32) - 1, 1, 1, F64, ref) == _abi.OK and out.value > 0  # the largest S
    assert f(0, 20, 3, F64, ref) == _abi.OK and out.value == 0  # no chain: nothing to do


def test_sort_workspace_is_positive_and_monotone(h):
    sizes = [_workspace(h, C, 100, 3) for C in (1, 2, 41, 42, 1000, 65536)]  # S = 4 100 / 4 200: a tile more
    assert sizes[0] > 0
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    by_k = [_workspace(h, 8, 100, k) for k in (1, 2, 3, 40, 255, 256)]
    assert by_k == sorted(by_k) and len(set(by_k)) == len(by_k)
    # a second key (8 bytes) and permutation (4 bytes) buffer at the least
    assert _workspace(h, 8, 100, 3) >= 12 * 800 * 3
    assert _workspace(h, 8, 100, 3, F32) > 0


def test_pooled_sort_checks(h):
    f = h.ipmc_pooled_sort
    big = 1 << 40

    def args(x=DUMMY, dtype=F64, C=4, n=20, k=3, s_chain=60, s_t=3, s_var=1, center=None, srt=DUMMY, perm=DUMMY,
             ws=DUMMY, ws_bytes=big):
        return (x, dtype, C, n, k, s_chain, s_t, s_var, center, srt, perm, ws, ws_bytes, None)

    _status(h, f(*args(C=-1)), INV, "negative size")
    _status(h, f(*args(n=-20)), INV, "negative size")
    _status(h, f(*args(k=-3)), INV, "negative size")
    _status(h, f(*args(s_chain=-60)), INV, "negative size")
    _status(h, f(*args(s_t=-3)), INV, "negative size")
    _status(h, f(*args(s_var=-1)), INV, "negative size")
    _status(h, f(*args(ws_bytes=-1)), INV, "negative size")
    _status(h, f(*args(k=0)), INV, "outside [1, 256]")
    _status(h, f(*args(k=257)), INV, "outside [1, 256]")
    _status(h, f(*args(dtype=5)), INV, "bad dtype")
    _status(h, f(*args(x=None)), INV, "NULL pointer")
    _status(h, f(*args(srt=None)), INV, "NULL pointer")
    _status(h, f(*args(perm=None)), INV, "NULL pointer")
    _status(h, f(*args(ws=None)), INV, "NULL pointer")
    _status(h, f(*args(C=1 << 16, n=1 << 16)), INV, "2^32")
    _status(h, f(*args(C=1 << 40, n=1 << 40)), INV, "2^32")
    need = _workspace(h, 4, 20, 3)
    _status(h, f(*args(ws_bytes=need - 1)), INV, f"ipmc_sort_workspace asks for {need}")
    _status(h, f(*args(ws_bytes=0)), INV, f"ipmc_sort_workspace asks for {need}")
    _status(h, f(*args(dtype=F32, ws_bytes=_workspace(h, 4, 20, 3, F32) - 1)), INV, "ipmc_sort_workspace asks for")
    assert f(*args(x=None, C=0, srt=None, perm=None, ws=None, ws_bytes=0)) == _abi.OK  # no chain: nothing to do
    assert f(*args(n=0, ws_bytes=_workspace(h, 4, 0, 3))) == _abi.OK  # no sample either


def test_rank_scores_checks(h):
    f = h.ipmc_rank_scores

    def args(srt=DUMMY, perm=DUMMY, k=3, C=4, n=20, mode=1, out=DUMMY, o_chain=60, o_t=3, o_var=1, ws=None,
             ws_bytes=0):
        return (srt, perm, k, C, n, mode, out, o_chain, o_t, o_var, ws, ws_bytes, None)

    _status(h, f(*args(C=-1)), INV, "negative size")
    _status(h, f(*args(n=-20)), INV, "negative size")
    _status(h, f(*args(k=-3)), INV, "negative size")
    _status(h, f(*args(o_chain=-60)), INV, "negative size")
    _status(h, f(*args(o_t=-3)), INV, "negative size")
    _status(h, f(*args(o_var=-1)), INV, "negative size")
    _status(h, f(*args(ws_bytes=-1)), INV, "negative size")  # it needs no workspace: any size >= 0 is enough
    _status(h, f(*args(k=0)), INV, "outside [1, 256]")
    _status(h, f(*args(k=257)), INV, "outside [1, 256]")
    _status(h, f(*args(mode=2)), INV, "mode = 2")
    _status(h, f(*args(mode=-1)), INV, "mode = -1")
    _status(h, f(*args(srt=None)), INV, "NULL pointer")
    _status(h, f(*args(perm=None)), INV, "NULL pointer")
    _status(h, f(*args(out=None)), INV, "NULL pointer")
    _status(h, f(*args(C=1 << 16, n=1 << 16)), INV, "2^32")
    assert f(*args(srt=None, perm=None, C=0, out=None)) == _abi.OK  # no chain: nothing to do
    assert f(*args(n=0)) == _abi.OK

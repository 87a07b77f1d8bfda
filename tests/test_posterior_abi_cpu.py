"""Argument checks of the pooled-histogram entry points (include/ipmc.h:
ipmc_minmax, ipmc_hist1d, ipmc_histdd), on the CPU: every call fails
validation or is a no-op before anything reaches the device
(tests/test_convergence_abi_cpu.py's style; the data pointers are dummies)."""
import ctypes

import pytest

from ip_mcmc_amd import _abi, _lib

DUMMY = 0x10000  # a non-NULL "device pointer"; never dereferenced by these calls
F64 = _abi.F64
INV = _abi.ERR_INVALID


@pytest.fixture(scope="module")
def h():
    return _lib.lib()


def _status(h, rc, code, text):
    assert rc == code, (rc, h.ipmc_last_error())
    assert text in h.ipmc_last_error().decode()


def test_abi_version_is_unchanged(h):
    assert h.ipmc_abi_version() == _abi.ABI_VERSION == 13


def test_minmax_checks(h):
    f = h.ipmc_minmax

    def args(x=DUMMY, dtype=F64, C=4, n=20, k=3, s=(60, 3, 1), lo=DUMMY, hi=DUMMY, scratch=DUMMY):
        return (x, dtype, C, n, k, *s, lo, hi, scratch, None)

    _status(h, f(*args(C=-1)), INV, "negative size")
    _status(h, f(*args(n=-20)), INV, "negative size")
    _status(h, f(*args(k=-3)), INV, "negative size")
    _status(h, f(*args(s=(60, -3, 1))), INV, "negative size")
    _status(h, f(*args(k=0)), INV, "outside [1, 256]")
    _status(h, f(*args(k=257)), INV, "outside [1, 256]")
    _status(h, f(*args(dtype=5)), INV, "bad dtype")
    _status(h, f(*args(x=None)), INV, "NULL pointer")
    _status(h, f(*args(lo=None)), INV, "NULL pointer")
    _status(h, f(*args(hi=None)), INV, "NULL pointer")
    _status(h, f(*args(scratch=None)), INV, "NULL pointer")
    assert f(*args(x=None, C=0, lo=None, hi=None, scratch=None)) == _abi.OK  # no chain: nothing to do


def test_hist1d_checks(h):
    f = h.ipmc_hist1d

    def args(x=DUMMY, dtype=F64, C=4, n=20, k=3, s=(60, 3, 1), B=20, edges=DUMMY, counts=DUMMY, below=DUMMY,
             above=DUMMY):
        return (x, dtype, C, n, k, *s, B, edges, counts, below, above, None)

    _status(h, f(*args(C=-1)), INV, "negative size")
    _status(h, f(*args(n=-1)), INV, "negative size")
    _status(h, f(*args(s=(-60, 3, 1))), INV, "negative size")
    _status(h, f(*args(k=0)), INV, "outside [1, 256]")
    _status(h, f(*args(k=300)), INV, "outside [1, 256]")
    _status(h, f(*args(dtype=-1)), INV, "bad dtype")
    _status(h, f(*args(B=0)), INV, "bins = 0 outside [1, 4096]")
    _status(h, f(*args(B=-20)), INV, "outside [1, 4096]")
    _status(h, f(*args(B=4097)), INV, "bins = 4097 outside [1, 4096]")
    for name in ("x", "edges", "counts", "below", "above"):
        _status(h, f(*args(**{name: None})), INV, "NULL pointer")
    assert f(*args(x=None, C=0, edges=None, counts=None, below=None, above=None)) == _abi.OK


def test_histdd_checks(h):
    f = h.ipmc_histdd

    def args(x=DUMMY, dtype=F64, C=4, n=20, k=3, s=(60, 3, 1), nd=3, comp=(0, 1, 2), bins=(20, 20, 20), edges=DUMMY,
             counts=DUMMY):
        c = None if comp is None else ctypes.addressof(keep.setdefault(("c", comp), (ctypes.c_int32 * 4)(*comp)))
        b = None if bins is None else ctypes.addressof(keep.setdefault(("b", bins), (ctypes.c_int32 * 4)(*bins)))
        return (x, dtype, C, n, k, *s, nd, c, b, edges, counts, None)

    keep = {}  # the host arrays stay alive for the calls
    _status(h, f(*args(C=-1)), INV, "negative size")
    _status(h, f(*args(s=(60, 3, -1))), INV, "negative size")
    _status(h, f(*args(k=0)), INV, "outside [1, 256]")
    _status(h, f(*args(k=257)), INV, "outside [1, 256]")
    _status(h, f(*args(dtype=2)), INV, "bad dtype")
    _status(h, f(*args(nd=0)), INV, "nd = 0 outside [1, 4]")
    _status(h, f(*args(nd=5)), INV, "nd = 5 outside [1, 4]")
    for name in ("x", "comp", "bins", "edges", "counts"):
        _status(h, f(*args(**{name: None})), INV, "NULL pointer")
    _status(h, f(*args(comp=(0, 1, 3))), INV, "comp[2] = 3 outside [0, k = 3)")
    _status(h, f(*args(comp=(-1, 1, 2))), INV, "comp[0] = -1 outside")
    _status(h, f(*args(bins=(20, 0, 20))), INV, "bins = 0 outside [1, 4096]")
    _status(h, f(*args(bins=(20, 20, 4097))), INV, "bins = 4097 outside [1, 4096]")
    _status(h, f(*args(bins=(256, 256, 257))), INV, "cells exceed 2^24")  # one row of cells too many
    _status(h, f(*args(k=4, nd=4, comp=(0, 1, 2, 3), bins=(4096, 4096, 4096, 4096))), INV, "cells exceed 2^24")
    assert f(*args(x=None, C=0, edges=None, counts=None)) == _abi.OK

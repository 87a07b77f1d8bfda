"""Argument checks of the cross-chain convergence entry points (include/ipmc.h),
on the CPU: every call fails validation or is a no-op before anything reaches
the device (tests/test_abi_validation.py's style; the pointers are dummies)."""
import pytest

from ip_mcmc_amd import _abi, _lib

DUMMY = 0x10000  # a non-NULL "device pointer"; never dereferenced by these calls
F64 = _abi.F64


@pytest.fixture(scope="module")
def h():
    return _lib.lib()


def _status(h, rc, code, text):
    assert rc == code, (rc, h.ipmc_last_error())
    assert text in h.ipmc_last_error().decode()


def test_abi_version_is_unchanged(h):
    assert h.ipmc_abi_version() == _abi.ABI_VERSION == 13


def test_split_stats_checks(h):
    f = h.ipmc_split_stats
    ok = (DUMMY, F64, 4, 20, 3, 60, 3, 1, DUMMY, DUMMY, None)
    inv = _abi.ERR_INVALID
    _status(h, f(DUMMY, F64, -1, 20, 3, 60, 3, 1, DUMMY, DUMMY, None), inv, "negative size")
    _status(h, f(DUMMY, F64, 4, -20, 3, 60, 3, 1, DUMMY, DUMMY, None), inv, "negative size")
    _status(h, f(DUMMY, F64, 4, 20, -3, 60, 3, 1, DUMMY, DUMMY, None), inv, "negative size")
    _status(h, f(DUMMY, F64, 4, 20, 3, 60, -3, 1, DUMMY, DUMMY, None), inv, "negative size")
    _status(h, f(DUMMY, F64, 4, 3, 3, 9, 3, 1, DUMMY, DUMMY, None), inv, "len >= 4")
    _status(h, f(DUMMY, F64, 4, 20, 0, 60, 3, 1, DUMMY, DUMMY, None), inv, "outside [1, 256]")
    _status(h, f(DUMMY, F64, 4, 20, 257, 5140, 257, 1, DUMMY, DUMMY, None), inv, "outside [1, 256]")
    _status(h, f(DUMMY, 5, 4, 20, 3, 60, 3, 1, DUMMY, DUMMY, None), inv, "bad dtype")
    _status(h, f(None, *ok[1:]), inv, "NULL pointer")
    _status(h, f(*ok[:8], None, DUMMY, None), inv, "NULL pointer")
    _status(h, f(*ok[:8], DUMMY, None, None), inv, "NULL pointer")
    _status(h, f(DUMMY, F64, 1 << 23, 20, 3, 60, 3, 1, DUMMY, DUMMY, None), inv, "chains per call")
    assert f(None, F64, 0, 20, 3, 60, 3, 1, None, None, None) == _abi.OK  # no chain: nothing to do


def test_mean_acov_checks(h):
    f = h.ipmc_mean_acov
    inv = _abi.ERR_INVALID

    def args(x=DUMMY, dtype=F64, C=4, n=20, k=3, mean=DUMMY, L=9, bc=1024, out=DUMMY):
        return (x, dtype, C, n, k, n * k, k, 1, mean, L, bc, out, None)

    _status(h, f(*args(C=-1)), inv, "negative size")
    _status(h, f(*args(L=-1)), inv, "negative size")
    _status(h, f(*args(n=2, L=0)), inv, "len >= 4")
    _status(h, f(*args(k=300)), inv, "outside [1, 256]")
    _status(h, f(*args(dtype=9)), inv, "bad dtype")
    _status(h, f(*args(L=10)), inv, "exceeds len/2 - 1 = 9")
    _status(h, f(*args(n=21, L=10)), inv, "exceeds len/2 - 1 = 9")  # the odd sample does not count
    _status(h, f(*args(n=20000, L=10000)), inv, "exceeds len/2 - 1 = 9999")  # the long-series path too
    _status(h, f(*args(bc=0)), inv, "block_chains must be positive")
    _status(h, f(*args(bc=-4)), inv, "block_chains must be positive")
    _status(h, f(*args(x=None)), inv, "NULL pointer")
    _status(h, f(*args(mean=None)), inv, "NULL pointer")
    _status(h, f(*args(out=None)), inv, "NULL pointer")
    assert f(*args(x=None, C=0, mean=None, out=None)) == _abi.OK


def test_moments_stats_checks(h):
    f = h.ipmc_moments_stats
    inv = _abi.ERR_INVALID
    _status(h, f(DUMMY, DUMMY, -1, 3, 100, DUMMY, DUMMY, None), inv, "negative size")
    _status(h, f(DUMMY, DUMMY, 8, -3, 100, DUMMY, DUMMY, None), inv, "negative size")
    _status(h, f(DUMMY, DUMMY, 8, 3, 1, DUMMY, DUMMY, None), inv, "n >= 2")
    _status(h, f(None, DUMMY, 8, 3, 100, DUMMY, DUMMY, None), inv, "NULL pointer")
    _status(h, f(DUMMY, None, 8, 3, 100, DUMMY, DUMMY, None), inv, "NULL pointer")
    _status(h, f(DUMMY, DUMMY, 8, 3, 100, None, DUMMY, None), inv, "NULL pointer")
    _status(h, f(DUMMY, DUMMY, 8, 3, 100, DUMMY, None, None), inv, "NULL pointer")
    assert f(None, None, 0, 3, 100, None, None, None) == _abi.OK


def test_centered_sq_block_sums_checks(h):
    f = h.ipmc_centered_sq_block_sums
    inv = _abi.ERR_INVALID
    _status(h, f(DUMMY, -1, 3, 3, DUMMY, 1024, DUMMY, None), inv, "bad shape")
    _status(h, f(DUMMY, 8, 3, 2, DUMMY, 1024, DUMMY, None), inv, "bad shape")
    _status(h, f(DUMMY, 8, 3, 3, DUMMY, 0, DUMMY, None), inv, "bad shape")
    _status(h, f(None, 8, 3, 3, DUMMY, 1024, DUMMY, None), inv, "NULL pointer")
    _status(h, f(DUMMY, 8, 3, 3, None, 1024, DUMMY, None), inv, "NULL pointer")
    _status(h, f(DUMMY, 8, 3, 3, DUMMY, 1024, None, None), inv, "NULL pointer")
    assert f(None, 0, 3, 3, None, 1024, None, None) == _abi.OK

"""Argument checks of ipmc_scatter (include/ipmc.h), on the CPU: every call
fails validation or is a no-op before anything reaches the device
(tests/test_posterior_abi_cpu.py's style; the data pointers are dummies)."""
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


def _args(x=DUMMY, dtype=F64, C=4, n=20, k=3, s=(60, 3, 1), center=DUMMY, mode=0, block=2, out=DUMMY, dsum=DUMMY):
    return (x, dtype, C, n, k, *s, center, mode, block, out, dsum, None)


def test_abi_version_is_unchanged(h):
    assert h.ipmc_abi_version() == _abi.ABI_VERSION == 13


def test_scatter_is_declared_and_bound(h):
    assert "ipmc_scatter" in _abi.SIGNATURES and hasattr(h, "ipmc_scatter")
    assert (_abi.CENTER_SHARED, _abi.CENTER_SPLIT) == (0, 1)


def test_scatter_sizes_and_strides(h):
    f = h.ipmc_scatter
    _status(h, f(*_args(C=-1)), INV, "negative size")
    _status(h, f(*_args(n=-20)), INV, "negative size")
    _status(h, f(*_args(k=-3)), INV, "negative size")
    _status(h, f(*_args(s=(-60, 3, 1))), INV, "negative size")
    _status(h, f(*_args(s=(60, -3, 1))), INV, "negative size")
    _status(h, f(*_args(s=(60, 3, -1))), INV, "negative size")
    _status(h, f(*_args(k=0)), INV, "outside [1, 256]")
    _status(h, f(*_args(k=257)), INV, "outside [1, 256]")


def test_scatter_dtype_and_pointers(h):
    f = h.ipmc_scatter
    _status(h, f(*_args(dtype=5)), INV, "bad dtype")
    _status(h, f(*_args(dtype=-1)), INV, "bad dtype")
    for name in ("x", "center", "out"):
        _status(h, f(*_args(**{name: None})), INV, "NULL pointer")


def test_scatter_center_mode_and_block(h):
    f = h.ipmc_scatter
    _status(h, f(*_args(mode=2)), INV, "bad center_mode")
    _status(h, f(*_args(mode=-1)), INV, "bad center_mode")
    _status(h, f(*_args(block=0)), INV, "block_chains = 0 < 1")
    _status(h, f(*_args(block=-4)), INV, "block_chains = -4 < 1")


def test_scatter_lengths(h):
    f = h.ipmc_scatter
    _status(h, f(*_args(n=0)), INV, "len >= 1")  # the shared centre uses every row: there must be one
    _status(h, f(*_args(n=3, mode=1)), INV, "len >= 4")  # a split chain needs two samples
    _status(h, f(*_args(C=1 << 30, n=1 << 24, k=256, s=(1 << 32, 256, 1))), INV, "more than 1e18 values")


def test_scatter_accepts_a_null_dsum(h):
    """The length checks come after the pointer checks: a call with dsum_out == NULL
    that reaches them has passed the pointer checks."""
    f = h.ipmc_scatter
    _status(h, f(*_args(dsum=None, n=0)), INV, "len >= 1")
    _status(h, f(*_args(dsum=None, n=3, mode=1)), INV, "len >= 4")
    _status(h, f(*_args(dsum=None, out=None, n=0)), INV, "NULL pointer")


def test_scatter_no_chain_is_a_no_op(h):
    f = h.ipmc_scatter
    assert f(*_args(x=None, C=0, center=None, out=None, dsum=None)) == _abi.OK
    assert f(*_args(x=None, C=0, k=0, mode=7, block=0, center=None, out=None, dsum=None)) == _abi.OK

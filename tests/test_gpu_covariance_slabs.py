"""ipmc_scatter past its first slab and on partial tile pairs.

The shapes of tests/test_gpu_covariance.py have few rows: set against the
kernel's geometry (csrc/ipmc_cov.hip, restated in geometry() below) almost
none of them leaves the first slab, and every multi-tile one has k = 256, four
full 64-wide tiles.  The shapes here are the smallest that give several slabs
per block with a short last one, chain boundaries inside slabs and, for
k > 64, a last tile narrower than the others and of a width that is no
multiple of 4.

  nt         ceil(k / 64)
  tw         ceil(k / nt) rounded up to a multiple of 4
  slab rows  6144 // tw (nt == 1) or 4096 // tw (nt > 1); 2048 // tw, at most 768, with 256 lanes
  P          (tw/4)² for an off-diagonal tile pair, (tw/4)(tw/4 + 1)/2 for a diagonal one
  G          min(lanes // P, 64)

Exact integers: the samples are integers in [-5, 5] plus arange(k) % 7, the
shared centre is arange(k) % 3 and the split centres are integers in [-2, 2],
so |x - c| <= 13, every product is at most 169 and every sum is below
169 · 844 < 2^18: exact in f64 (and the samples in f32) whatever the order of
the adds.  The kernel has to give numpy's integers, entry by entry; a lost or
doubled row at a slab seam, a misplaced tile or thread tile, or a wrong
mirror changes an integer.  Outputs are filled with NaN first, so that an
entry the kernel does not write shows as well.

The 64-bit row index of a block of more than 2^31 rows is not reachable by a
test of a few seconds and stays untested."""
import functools

import numpy as np
import pytest

from ip_mcmc_amd import _abi
import test_gpu_covariance as base
from test_covariance_cpu import SLAB_IDS, SLAB_SHAPES, make_samples
from test_gpu_covariance import _scatter, on_gpu

pytestmark = pytest.mark.gpu

LAYOUTS = ["time_vars", "vars_time"]
DTYPES = [np.float64, np.float32]
MODES = ["shared_dsum", "shared", "split"]

# (C, n, k, block) -> slabs in each block (shared centre and split centres alike): n is odd wherever
# it can be, so that the split chains drop the last row of each chain
TABLE = {
    (11, 19, 256, 11): [4],   # 209 rows, slabs of 64: the pair kernel in its steady state, 3 full + 17
    (8, 24, 256, 8): [3],     # 192 rows: exactly 3 slabs, no short one
    (7, 53, 65, 7): [4],      # 371 rows, slabs of 113: tiles of 36 and 29 columns
    (5, 61, 129, 5): [4],     # 305 rows, slabs of 93: tiles of 44, 44 and 41 columns
    (9, 29, 200, 4): [2, 2, 1],  # 116, 116 and 29 rows, slabs of 78: tw = 52, last tile 44, a last block of one chain
    (3, 71, 255, 3): [4],     # 213 rows, slabs of 64: last tile 63 columns
    (6, 87, 64, 6): [6],      # 522 rows, slabs of 96: a single tile at full width, P = 136, G = 7
    (9, 57, 40, 9): [4],      # 513 rows, slabs of 153: the headline k
    (4, 211, 12, 4): [2],     # 844 rows, slabs of 512
    (4, 211, 5, 4): [2],      # 844 rows, slabs of 768: two thread tiles, 64 groups
}
SLAB_ROWS = {256: 64, 65: 113, 129: 93, 200: 78, 255: 64, 64: 96, 40: 153, 12: 512, 5: 768}
SHAPES = list(TABLE)
IDS = ["-".join(str(v) for v in s) for s in SHAPES]
BY_K = {s[2]: s for s in SHAPES if s != (8, 24, 256, 8)}

STALE = ("the slab geometry restated in this test no longer gives the number of slabs that the shapes were chosen "
         "for: re-derive the shapes (and geometry()) from csrc/ipmc_cov.hip.  This says nothing about whether the "
         "kernel is right.")


def geometry(k, lanes=1024, tile=None):
    """(nt, tw, slab rows) of ipmc_scatter for k components, restated from the table above;
    lanes = 256 is IPMC_COV_THREADS=256, tile is IPMC_COV_TILE (a single tile widened)."""
    nt = -(-k // 64)
    tw = (-(-k // nt) + 3) // 4 * 4
    if tile is not None and nt == 1 and tw < tile // 4 * 4 <= 64:
        tw = tile // 4 * 4
    if lanes == 256:
        return nt, tw, min(2048 // tw, 768)
    return nt, tw, (6144 if nt == 1 else 4096) // tw


def slabs(shape, split, lanes=1024, tile=None):
    """Slabs in each block of `shape`: the split centres use 2 (n // 2) rows of a chain."""
    C, n, k, block = shape
    sr = geometry(k, lanes, tile)[2]
    rows = 2 * (n // 2) if split else n
    return [-(-min(block, C - c0) * rows // sr) for c0 in range(0, C, block)]


def test_the_shapes_give_the_slabs_they_were_chosen_for():
    assert [geometry(k)[:2] for k in (65, 129, 200, 255, 256, 64, 40, 12, 5, 3)] == [
        (2, 36), (3, 44), (4, 52), (4, 64), (4, 64), (1, 64), (1, 40), (1, 12), (1, 8), (1, 4)], STALE
    for shape, want in TABLE.items():
        assert geometry(shape[2])[2] == SLAB_ROWS[shape[2]], (shape, STALE)
        for split in (False, True):
            assert slabs(shape, split) == want, (shape, split, STALE)
    # 256 lanes: slabs of 2048 // tw rows; one 64-wide tile: slabs of 96 rows
    for k, sr, want, want_split in ((256, 32, 7, 7), (65, 56, 7, 7), (40, 51, 11, 10), (5, 256, 4, 4)):
        assert geometry(k, lanes=256)[2] == sr and slabs(BY_K[k], False, lanes=256) == [want], (k, STALE)
        assert slabs(BY_K[k], True, lanes=256) == [want_split], (k, STALE)
    for k, want in ((40, 6), (5, 9)):
        assert geometry(k, tile=64) == (1, 64, 96) and slabs(BY_K[k], False, tile=64) == [want], (k, STALE)
        assert slabs(BY_K[k], True, tile=64) == [want], (k, STALE)
    # every k on (3, 67, k, 3): two slabs or more from k = 29, three or more from k = 81 (slabs of 113
    # and 102 rows for k = 65..80 hold the 201 rows in two)
    for k in range(1, 257):
        for split in (False, True):
            n_slabs = slabs((3, 67, k, 3), split)[0]
            assert n_slabs >= (3 if k >= 81 else 2 if k >= 29 else 1), (k, split, STALE)


def integer_case(shape, pad=0):
    """The integer samples of `shape` and their reference, read-only:
    x (C, n + pad, k) float64 of which the rows [pad:] are the samples, the shared centre, the
    split centres (2C, k), and per block (S, D) about the shared centre and S about the split ones,
    d.T @ d and d.sum(0) in numpy float64."""
    C, n, k, block = shape
    rng = np.random.default_rng(1000 * k + n)
    x = rng.integers(-5, 6, size=(C, n + pad, k)).astype(np.float64)
    x += (np.arange(k) % 7)[None, None, :]  # means that differ between components: an asymmetric pattern
    center = np.arange(k, dtype=np.float64) % 3
    mu = rng.integers(-2, 3, size=(2 * C, k)).astype(np.float64)
    xs, N = x[:, pad:], n // 2
    shared_S, shared_D, split_S = [], [], []
    for c0 in range(0, C, block):
        c1 = min(C, c0 + block)
        d = (xs[c0:c1] - center).reshape(-1, k)
        shared_S.append(d.T @ d)
        shared_D.append(d.sum(axis=0))
        d = np.concatenate([xs[c0:c1, :N] - mu[c0:c1, None], xs[c0:c1, N:2 * N] - mu[C + c0:C + c1, None]],
                           axis=1).reshape(-1, k)
        split_S.append(d.T @ d)
    out = (x, center, mu, np.stack(shared_S), np.stack(shared_D), np.stack(split_S))
    for a in out:
        a.setflags(write=False)
    assert np.abs(out[3]).max() < 2**53 and np.abs(out[5]).max() < 2**53
    return out


# the named shapes are shared by the tests below: their reference is computed once
cached_integer_case = functools.lru_cache(maxsize=None)(integer_case)


def device_samples(x, layout, dtype, pad=0):
    """x (C, n + pad, k) on the device in `layout` and `dtype`, and its view without the first
    `pad` samples of every chain (the tensor itself when pad = 0)."""
    a = x.astype(dtype)
    assert np.array_equal(a.astype(np.float64), x)  # small integers are exact in f32
    t = on_gpu(a.transpose(0, 2, 1) if layout == "vars_time" else a)
    if pad == 0:
        return t, t
    return t, (t[:, :, pad:] if layout == "vars_time" else t[:, pad:])


def assert_exact(got, want, what):
    assert got.shape == want.shape, what
    for b in range(got.shape[0]):
        bad = np.argwhere(~(got[b] == want[b]))  # NaN (never written) counts as wrong
        if len(bad):
            e = tuple(int(i) for i in bad[0])
            pytest.fail(f"{what}, block {b}: {len(bad)} of {got[b].size} entries differ from numpy's integers, "
                        f"the first at {e}: got {got[b][e]!r}, want {want[b][e]!r}")


def check_integers(shape, layout, dtype, mode, pad=0, case=cached_integer_case):
    """One launch of ipmc_scatter on the integer samples of `shape` against numpy, bit for bit."""
    C, n, k, block = shape
    x, center, mu, shared_S, shared_D, split_S = case(shape, pad)
    whole, t = device_samples(x, layout, dtype, pad)
    if pad:  # a burn-in slice, passed by its strides: not contiguous, no copy, chains that do not follow one another
        assert not t.is_contiguous()
        assert t.data_ptr() == whole.data_ptr() + pad * whole.element_size() * (k if layout == "time_vars" else 1)
        assert t.stride() == whole.stride() and t.stride(0) == (n + pad) * k
        assert t.stride(0) != n * t.stride(1 if layout == "time_vars" else 2)  # so ipmc_scatter does not collapse the chains
    what = f"k={k} {layout} {np.dtype(dtype).name} {mode} shape={shape} pad={pad}"
    if mode == "split":
        got, ds = _scatter(t, on_gpu(mu.copy()), _abi.CENTER_SPLIT, block, with_dsum=False, layout=layout)
        want = split_S
    else:
        got, ds = _scatter(t, on_gpu(center.copy()), _abi.CENTER_SHARED, block, with_dsum=mode == "shared_dsum",
                           layout=layout)
        want = shared_S
    assert_exact(got, want, what + " scatter")
    if mode == "shared_dsum":
        assert_exact(ds, shared_D, what + " dsum")
    else:
        assert ds is None
    for b in range(got.shape[0]):
        assert np.array_equal(got[b], got[b].T), (what, b)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_integers_across_slabs_and_partial_tiles(shape, layout, dtype, mode):
    check_integers(shape, layout, dtype, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k", [65, 40])
def test_integers_of_a_burn_in_slice_in_place(k, layout, dtype, mode):
    """x[:, 3:] of a larger tensor (x[:, :, 3:] for vars_time), as posterior_covariance passes a
    view: stride_chain != len * stride_t, so the shared centre takes the per-row chain / sample
    decomposition too, with chain boundaries inside the second and third slab."""
    check_integers(BY_K[k], layout, dtype, mode, pad=3)


@pytest.mark.parametrize("k0", range(1, 257, 32))
def test_integers_for_every_k(k0):
    """(3, 67, k, 3) for every k: every (nt, tw, tg, P, G) the dispatcher can produce."""
    for k in range(k0, k0 + 32):
        case = integer_case((3, 67, k, 3))
        for mode in ("shared_dsum", "split"):
            check_integers((3, 67, k, 3), "time_vars", np.float64, mode, case=lambda shape, pad: case)


# ------------------------------------------------------------- the environment switches
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k", [256, 65, 40, 5])
def test_integers_with_256_lane_workgroups(k, layout, dtype, mode, monkeypatch):
    """IPMC_COV_THREADS=256 (read on every call): 8 loads per lane in flight, slabs of 2048 // tw rows."""
    monkeypatch.setenv("IPMC_COV_THREADS", "256")
    check_integers(BY_K[k], layout, dtype, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k", [40, 5])
def test_integers_with_one_64_wide_tile(k, layout, dtype, mode, monkeypatch):
    """IPMC_COV_TILE=64: a tile wider than k needs (P = 136, G = 7, slabs of 96 rows)."""
    monkeypatch.setenv("IPMC_COV_TILE", "64")
    check_integers(BY_K[k], layout, dtype, mode)


@pytest.mark.parametrize("switch", [("IPMC_COV_THREADS", "256"), ("IPMC_COV_TILE", "64")], ids=["threads", "tile"])
def test_the_switches_reach_the_kernel(switch, monkeypatch):
    """The two tests above would pass with a switch that is not read.  On samples that are not
    integers the switches change G (k = 40: 18 groups by default, 4 with 256 lanes, 7 with a 64-wide
    tile) and with it the order of the adds: some of the 1 600 sums of 513 products round differently,
    while the result stays within the device-against-host bar."""
    C, n, k, block = BY_K[40]
    t = on_gpu(make_samples(C, n, k, seed=40))
    center = on_gpu(np.asarray(t[0, 0].cpu()))
    plain, _ = _scatter(t, center, _abi.CENTER_SHARED, block)
    monkeypatch.setenv(*switch)
    other, _ = _scatter(t, center, _abi.CENTER_SHARED, block)
    assert not np.array_equal(plain, other)
    base.assert_cov_close(other[0], plain[0], 1e-10)


# ------------------------------------------------------------------- the public API
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SLAB_SHAPES, ids=SLAB_IDS)
def test_api_device_equals_host_definition(shape, layout, dtype):
    """posterior_covariance and multivariate_rhat on the device against the host definition with the
    bars of tests/test_gpu_covariance.py, on the multi-tile shapes above (and k = 65 once more with
    the default block); tests/test_covariance_cpu.py holds the host within 1e-12 of np.cov on them.

    Bn of (3, 71, 255, 3), vars_time, f64 was 9.14e-10 from the host's while the split-chain means were
    plain sums: with N = 35 >= 32 samples of unit stride ipmc_split_stats adds over the lanes of a wave,
    the host in sample order, the means differed by 5 ulp, and Bn of chain means that are 1e5 standard
    deviations large and spread by 5e-7 of their size multiplies that by 2 |μ| / spread.  Both sides
    now sum a mean about the series' first sample, which rounds the same value in any order."""
    assert shape[:3] in [s[:3] for s in SHAPES]
    base.test_device_equals_host_definition(shape, layout, dtype)

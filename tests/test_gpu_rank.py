"""The pooled sort, the rank scores and the rank-normalised diagnostics on the
device (ipmc_pooled_sort, ipmc_rank_scores; ranks.py) against numpy / scipy and
the host definition.

Comparison rules of tests/test_gpu_convergence.py: float outputs rtol 1e-10 /
atol 1e-12; sorted values, permutations, average ranks, lag_used, truncated
and pooled quantiles exactly.  ESS contains a discrete stop, so every ESS case
first asserts on the host reference that each evaluated |P_j| > 1e-6, for each
of the four transformed series.
"""
import ctypes
import warnings

import numpy as np
import pytest
from scipy.special import ndtri
from scipy.stats import rankdata

from ip_mcmc_amd import _abi, convergence, pooled_quantiles, rank_convergence, rank_normalize
from ip_mcmc_amd import diagnostics as D

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-10, 1e-12
FLOAT_KEYS = ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail")
EXACT_KEYS = ("median", "q_lo", "q_hi", "lag_used", "truncated", "n_chains", "n_samples", "n_split")
P_CLEAR = 1e-6
T = _abi.SORT_TILE  # keys of one workgroup's tile (IPMC_SORT_TILE)


def ar1(C, n, k, phi, seed, offset=8.0, scale=0.01):
    """AR(1) chains around `offset` with spread ~`scale` (θ = 8 + u: the normal case), (C, n, k)."""
    rng = np.random.default_rng(seed)
    e = rng.normal(size=(C, n, k))
    x = np.empty((C, n, k))
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return offset + scale * x + 0.2 * scale * rng.normal(size=(C, 1, k))


def ties(x, seed, grid=0.002):
    rng = np.random.default_rng(seed); C, n, k = x.shape; out = np.empty_like(x)
    for c in range(C):
        keep = rng.random(n) < 0.3; keep[0] = True
        out[c] = x[c, np.maximum.accumulate(np.where(keep, np.arange(n), 0))]
    return np.round(out / grid) * grid


def quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


def on_gpu(x, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to("cuda")


# ----------------------------------------------------------------- the sort
def device_sort(t, C, n, k, strides, center=None):
    """ipmc_pooled_sort on the device tensor t with element strides (chain, t, var) -> numpy
    (sorted (k, S) float64, perm (k, S) uint32)."""
    import torch

    from ip_mcmc_amd import device as dev
    from ip_mcmc_amd._lib import call

    S = C * n
    dtype = dev.abi_dtype(t.dtype)
    need = ctypes.c_int64(0)
    call("ipmc_sort_workspace", C, n, k, dtype, ctypes.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=t.device)
    srt = torch.full((k, S), -7.0, dtype=torch.float64, device=t.device)
    perm = torch.full((k, S), -1, dtype=torch.int32, device=t.device)
    cen = None if center is None else on_gpu(np.asarray(center, dtype=np.float64))
    call("ipmc_pooled_sort", t.data_ptr(), dtype, C, n, k, *strides, None if cen is None else cen.data_ptr(),
         srt.data_ptr(), perm.data_ptr(), ws.data_ptr(), need.value, dev.stream_handle(t.device))
    return srt.cpu().numpy(), perm.cpu().numpy().view(np.uint32)


def check_sort(x, got, center=None):
    """x (C, n, k) float64 (the widened values); got = device_sort's result."""
    C, n, k = x.shape
    pooled = x.reshape(C * n, k)
    if center is not None:
        pooled = np.abs(pooled - np.asarray(center))
    srt, perm = got
    assert srt.shape == perm.shape == (k, C * n)
    for v in range(k):
        order = np.argsort(pooled[:, v], kind="stable")
        assert np.array_equal(perm[v], order.astype(np.uint32)), f"permutation of component {v}"
        # == on the values: -0.0 equals +0.0 (the sign of a zero is unspecified), NaN matches NaN
        assert np.array_equal(srt[v], pooled[order, v], equal_nan=True), f"sorted values of component {v}"
        assert np.array_equal(srt[v], np.sort(pooled[:, v]), equal_nan=True)


def varying_key_bytes(values):
    """The byte positions (0 = lowest) in which the sort keys of the float64 `values` differ: the
    passes that run.  The key map of the kernel, restated: the sign bit flipped for a non-negative
    value, every bit for a negative one (after -0 -> +0; no NaN here)."""
    v = np.asarray(values, dtype=np.float64).ravel() + 0.0  # -0.0 + 0.0 = +0.0
    assert not np.isnan(v).any()
    b = v.view(np.uint64)
    key = np.where(b >> np.uint64(63), ~b, b ^ np.uint64(1 << 63))
    diff = np.bitwise_or.reduce(key ^ key[0])
    return {p for p in range(8) if (int(diff) >> (8 * p)) & 0xFF}


def sort_time_vars(x, dtype=None, center=None):
    C, n, k = x.shape
    t = on_gpu(x, dtype)
    return device_sort(t, C, n, k, (n * k, k, 1), center)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("S", [1, T - 1, T, T + 1, 3 * T + 17])
def test_sort_sizes_around_the_tile(S, k):
    x = np.random.default_rng(100 + k).normal(size=(1, S, k))
    check_sort(x, sort_time_vars(x))


def test_sort_layouts_and_a_view():
    import torch

    C, n, k = 5, 1000, 3  # S = 5 000: two tiles
    x = ar1(C, n, k, 0.5, 110)
    check_sort(x, sort_time_vars(x))
    tv = on_gpu(x.transpose(0, 2, 1))  # (C, k, n)
    check_sort(x, device_sort(tv, C, n, k, (k * n, 1, n)))
    wide = on_gpu(ar1(C, 2 * n, k + 2, 0.5, 111))  # every other sample of the middle components, in place
    view = wide[:, ::2, 1:k + 1]
    assert not view.is_contiguous()
    s_chain, s_t, s_var = view.stride()
    got = device_sort(view, C, n, k, (s_chain, s_t, s_var))
    check_sort(view.cpu().numpy(), got)
    assert torch.equal(view, wide[:, ::2, 1:k + 1])  # the input is read only


@pytest.mark.parametrize("layout", ["time_vars", "vars_time"])
def test_sort_f32_input(layout):
    C, n, k = 3, 1500, 3
    x32 = ar1(C, n, k, 0.5, 112, offset=1.0, scale=0.5).astype(np.float32)
    if layout == "time_vars":
        got = sort_time_vars(x32)
    else:
        got = device_sort(on_gpu(x32.transpose(0, 2, 1)), C, n, k, (k * n, 1, n))
    check_sort(x32.astype(np.float64), got)
    c = np.array([1.0, 0.9, 1.2])  # the fold happens in double on the widened values
    check_sort(x32.astype(np.float64), sort_time_vars(x32, center=c), center=c)
    for v in range(k):  # both signs: the low key bytes are 0x00 and 0xFF, every pass runs
        assert varying_key_bytes(x32[:, :, v].astype(np.float64)) == set(range(8))


@pytest.mark.parametrize("layout", ["time_vars", "vars_time"])
def test_sort_positive_f32_input_skips_the_low_passes(layout):
    """theta = 8 + u as f32: the three lowest key bytes are zero and the highest is the same for every
    sample, so passes 0 to 2 are skipped, passes 3 to 6 run and pass 7 is skipped.  Rounded to f32 the
    AR(1) values tie now and then, which is where the order the running passes keep shows."""
    C, n, k = 3, 1500, 3  # S = 4 500: two tiles
    x32 = ar1(C, n, k, 0.5, 116).astype(np.float32)
    x64 = x32.astype(np.float64)
    for v in range(k):
        assert varying_key_bytes(x64[:, :, v]) == {3, 4, 5, 6}
    assert len(np.unique(x32[:, :, 0])) < C * n  # ties
    if layout == "time_vars":
        got = sort_time_vars(x32)
    else:
        got = device_sort(on_gpu(x32.transpose(0, 2, 1)), C, n, k, (k * n, 1, n))
    check_sort(x64, got)


def test_sort_special_columns():
    S = 3 * T + 17
    rng = np.random.default_rng(113)
    cols = []
    cols.append(np.full(S, 8.25))  # S equal values: every pass is skipped
    run = rng.normal(size=S)
    run[T - 5:3 * T + 2] = 0.125  # a run of equal values from the first tile into the fourth
    cols.append(run)
    mixed = rng.normal(size=S)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, -1e-310, -1.0, 1.0])
    where = rng.choice(S, size=4 * len(special), replace=False)
    mixed[where] = np.tile(special, 4)
    cols.append(mixed)
    nans = rng.normal(size=S)
    nans[rng.choice(S, size=37, replace=False)] = np.nan
    nans[[0, T, S - 1]] = np.array([np.nan, -np.nan, np.float64(np.nan)])
    payload = np.array([0x7FF0000000000001, 0xFFF8000000000123], dtype=np.uint64).view(np.float64)
    nans[[5, 2 * T + 1]] = payload  # a signalling and a negative NaN with a payload
    cols.append(nans)
    low = (np.uint64(0x4020000000000000) + rng.integers(0, 256, size=S).astype(np.uint64)).view(np.float64)
    cols.append(low)  # keys that differ in the lowest byte only
    signs = np.where(rng.random(S) < 0.5, 1.5, -1.5) * np.where(rng.random(S) < 0.5, 1.0, 2.0 ** 600)
    cols.append(signs)  # four values of both signs: a negative key is the complement, every byte differs
    top = rng.choice(np.array([2.0 ** -512, 1.0, 2.0 ** 512]), size=S)
    cols.append(top)  # keys 0x9FF0.., 0xBFF0.., 0xDFF0..: only the highest byte differs, passes 0 to 6 are skipped
    high = rng.choice(np.array([1.0, 1.5, 2.0 ** 512, 1.5 * 2.0 ** 512]), size=S)
    cols.append(high)  # keys 0xBFF0.., 0xBFF8.., 0xDFF0.., 0xDFF8..: the two highest bytes differ
    ends = (rng.choice(np.array([1.0, 2.0 ** 512]), size=S).view(np.uint64)
            + rng.integers(0, 256, size=S).astype(np.uint64)).view(np.float64)
    cols.append(ends)  # the lowest and the highest byte differ: pass 0 runs, 1 to 6 are skipped, pass 7 runs
    widened = (8.0 + 0.01 * rng.normal(size=S)).astype(np.float32).astype(np.float64)
    cols.append(widened)  # f32 values as doubles: passes 0 to 2 skipped, then running passes
    x = np.stack(cols, axis=1)[None]  # (1, S, 10)
    assert np.array_equal(low.view(np.uint64) >> np.uint64(8), np.full(S, 0x40200000000000, dtype=np.uint64))
    want = {0: set(), 4: {0}, 5: set(range(8)), 6: {7}, 7: {6, 7}, 8: {0, 7}, 9: {3, 4, 5, 6}}
    for v, passes in want.items():  # the passes that run are those the column was built for
        assert varying_key_bytes(x[0, :, v]) == passes, v
    check_sort(x, sort_time_vars(x))
    # |x - c|: ties at zero, NaN stays NaN, inf - c
    c = np.array([8.25, 0.125, 0.0, 0.1, 8.0, 0.0, 1.0, 1.0, 1.0, 8.0])
    with np.errstate(invalid="ignore"):
        check_sort(x, sort_time_vars(x, center=c), center=c)


def test_sort_twice_gives_the_same_bits():
    x = ties(ar1(4, 1200, 3, 0.5, 114), 115)
    a, b = sort_time_vars(x), sort_time_vars(x)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])


# ------------------------------------------------------- ranks and scores
# shape (C, n, k), seed: the smallest shapes that reach each code path
SHAPES = [
    ((3, 64, 40), 41),  # k neither a power of two nor a wave multiple, odd C
    ((1, 200, 2), 42),  # one chain
    ((8, 101, 3), 43),  # odd n: the last sample is dropped
    ((2, 16, 256), 44),  # the largest k
    ((5, 32, 1), 45),  # the smallest k
    ((6, 700, 2), 46),  # S = 4 200: two tiles of the sort, five of the rank scores
    ((40, 300, 3), 47),  # S = 12 000: three tiles
]
TIE_SHAPES = [((4, 120, 3), 51), ((8, 101, 3), 52), ((3, 64, 40), 53)]


def fixture(shape, seed, tied):
    x = ar1(*shape, 0.5, seed)
    return ties(x, seed) if tied else x


ALL_FIXTURES = [(s, seed, False) for s, seed in SHAPES] + [(s, seed, True) for s, seed in TIE_SHAPES]


def used(x):
    return x[:, :2 * (x.shape[1] // 2)]


def ref_ranks(u):
    C, m, k = u.shape
    return rankdata(u.reshape(C * m, k), method="average", axis=0).reshape(C, m, k)


def ref_scores(u):
    return ndtri((ref_ranks(u) - 3 / 8) / (u.shape[0] * u.shape[1] + 1 / 4))


@pytest.mark.parametrize("shape,seed,tied", ALL_FIXTURES)
def test_rank_normalize_on_the_device(shape, seed, tied):
    x = fixture(shape, seed, tied)
    u = used(x)
    t = on_gpu(x)
    ranks = rank_normalize(t, scores=False, backend="device")
    assert ranks.is_cuda and tuple(ranks.shape) == u.shape
    assert np.array_equal(ranks.cpu().numpy(), ref_ranks(u))
    np.testing.assert_allclose(rank_normalize(t, backend="device").cpu().numpy(), ref_scores(u), rtol=RTOL, atol=ATOL)
    med = np.median(u.reshape(-1, u.shape[2]), axis=0)
    folded = np.abs(u - med)
    assert np.array_equal(rank_normalize(t, fold=True, scores=False, backend="device").cpu().numpy(), ref_ranks(folded))
    np.testing.assert_allclose(rank_normalize(t, fold=True, backend="device").cpu().numpy(), ref_scores(folded),
                               rtol=RTOL, atol=ATOL)
    # numpy in, vars_time layout, device backend: the same bits
    again = rank_normalize(x.transpose(0, 2, 1), scores=False, layout="vars_time", backend="device")
    assert np.array_equal(again.cpu().numpy(), ranks.cpu().numpy())


@pytest.mark.parametrize("shape,seed,tied", ALL_FIXTURES)
def test_pooled_quantiles_on_the_device(shape, seed, tied):
    x = fixture(shape, seed, tied)
    q = [0.0, 0.05, 1 / 3, 0.5, 0.95, 1.0]
    want = np.quantile(x.reshape(-1, x.shape[2]), q, axis=0).T  # all n samples
    assert np.array_equal(pooled_quantiles(on_gpu(x), q, backend="device"), want)
    assert np.array_equal(pooled_quantiles(on_gpu(x), q, backend="device", component_slab=2), want)


# ------------------------------------------------------- rank_convergence
def clear_pairs(series, L):
    """Assert on the host that no evaluated pair sum of convergence(series) is within P_CLEAR of zero."""
    ref = quiet(convergence, series, max_lag=L, backend="host")
    N = ref["n_split"]
    mean, W, Bn, acov = D._host_parts(np.ascontiguousarray(series, dtype=np.float64), L)
    rho = D._rho(W, Bn, acov, N)
    for v in np.flatnonzero(W > 0):
        last = ref["lag_used"][v] // 2 if ref["truncated"][v] else ref["lag_used"][v] // 2 - 1
        P = np.array([rho[2 * j, v] + rho[2 * j + 1, v] for j in range(last + 1)])
        assert np.abs(P).min() > P_CLEAR, (v, P)


def reference(x64, max_lag=None, tail=(0.05, 0.95)):
    """The host definition on float64 (C, n, k), after the |P_j| guard on each of the four series."""
    ref = quiet(rank_convergence, x64, max_lag=max_lag, tail=tail, backend="host")
    u = used(np.asarray(x64, dtype=np.float64))
    N = u.shape[1] // 2
    L = min(N - 1, 1000) if max_lag is None else max_lag
    keep = ~np.isnan(u).any(axis=(0, 1))  # a component with a NaN sample has no series to guard
    u = u[:, :, keep]
    if u.shape[2]:
        for series in (ref_scores(u), ref_scores(np.abs(u - ref["median"][keep])),
                       (u <= ref["q_lo"][keep]).astype(np.float64), (u <= ref["q_hi"][keep]).astype(np.float64)):
            clear_pairs(series, L)
    return ref


def assert_same(got, ref):
    assert set(got) == set(ref)
    for key in FLOAT_KEYS:
        np.testing.assert_allclose(got[key], ref[key], rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=key)
    for key in EXACT_KEYS:
        assert np.array_equal(got[key], ref[key], equal_nan=True), (key, got[key], ref[key])


def assert_same_bits(a, b):
    for key in FLOAT_KEYS + EXACT_KEYS:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


@pytest.mark.parametrize("shape,seed,tied", ALL_FIXTURES)
def test_rank_convergence_equals_host_definition(shape, seed, tied):
    x = fixture(shape, seed, tied)
    ref = reference(x)
    got = quiet(rank_convergence, on_gpu(x), backend="device")
    assert_same(got, ref)
    assert_same_bits(got, quiet(rank_convergence, x, backend="device"))  # numpy in: the same bits


def test_component_slabs_and_repeat_calls_give_the_same_bits():
    x = ar1(3, 64, 40, 0.5, 41)
    t = on_gpu(x)
    whole = quiet(rank_convergence, t, backend="device")
    assert_same_bits(whole, quiet(rank_convergence, t, backend="device"))
    for slab in (1, 7):
        assert_same_bits(whole, quiet(rank_convergence, t, backend="device", component_slab=slab))
    z = rank_normalize(t, backend="device")
    for slab in (1, 7):
        assert np.array_equal(z.cpu().numpy(), rank_normalize(t, backend="device", component_slab=slab).cpu().numpy())
    tv = on_gpu(x.transpose(0, 2, 1))
    assert_same_bits(whole, quiet(rank_convergence, tv, layout="vars_time", backend="device", component_slab=7))
    tied = on_gpu(ties(ar1(40, 300, 3, 0.5, 47), 47))
    assert_same_bits(quiet(rank_convergence, tied, backend="device"), quiet(rank_convergence, tied, backend="device"))


def test_nan_and_constant_components():
    x = ar1(4, 120, 4, 0.5, 54)
    x[:, :, 1] = 8.0
    x[2, 17, 3] = np.nan
    ref = reference(x)
    got = quiet(rank_convergence, on_gpu(x), backend="device")
    assert_same(got, ref)
    for key in FLOAT_KEYS:
        assert np.isnan(got[key][[1, 3]]).all() and np.isfinite(got[key][[0, 2]]).all(), key
    assert got["median"][1] == 8.0 and np.isnan(got["median"][3])
    clean = quiet(rank_convergence, on_gpu(x[:, :, [0, 2]]), backend="device")
    for key in FLOAT_KEYS:  # the other components are unaffected (the order of the kernels' sums depends on k)
        np.testing.assert_allclose(got[key][[0, 2]], clean[key], rtol=RTOL, atol=ATOL, err_msg=key)
    z = rank_normalize(on_gpu(x), backend="device").cpu().numpy()
    assert np.isnan(z[2, 17, 3]) and np.isnan(z).sum() == 1
    r = rank_normalize(on_gpu(x), scores=False, backend="device").cpu().numpy()
    assert np.array_equal(r[:, :, 1], np.full((4, 120), 240.5))  # one run over the whole segment


def test_f32_tensor():
    x32 = ties(ar1(4, 120, 3, 0.5, 55, offset=1.0, scale=0.5), 56, grid=0.05).astype(np.float32)
    x64 = x32.astype(np.float64)
    t = on_gpu(x32)
    assert_same(quiet(rank_convergence, t, backend="device"), reference(x64))
    assert np.array_equal(rank_normalize(t, scores=False, backend="device").cpu().numpy(), ref_ranks(x64))
    q = [0.05, 0.5, 0.95]
    assert np.array_equal(pooled_quantiles(t, q, backend="device"), np.quantile(x64.reshape(-1, 3), q, axis=0).T)


def test_one_warning_per_call_on_the_device():
    t = on_gpu(ar1(4, 200, 3, 0.9, 57))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = rank_convergence(t, max_lag=3, backend="device")
    assert len(w) == 1 and "component(s) [0, 1, 2]" in str(w[0].message)
    assert not r["truncated"].any() and (r["lag_used"] == 4).all()


def _linear_sampler():
    """Stuart (2010) example 2.1's shape: G(u) = <g, u>, k = 2, scalar noise, prior N(0, I), pCN."""
    from ip_mcmc_amd import (ConstSteppCNProposer, CountedAccepter, EvolutionPotential, GaussianDistribution,
                             LinearOperator, MCMCSampler, pCNAccepter)

    g, gamma = np.array([3.0, 1.0]), 0.5
    y = np.array([g @ np.array([2.0, 7.0]) + 0.3])
    pot = EvolutionPotential(LinearOperator(g), y, GaussianDistribution(0, gamma**2))
    prior = GaussianDistribution(np.zeros(2), np.eye(2))
    return MCMCSampler(ConstSteppCNProposer(0.25, prior), CountedAccepter(pCNAccepter(pot)), 20261)


def test_end_to_end_linear_problem():
    u0 = 5.0 * np.random.default_rng(37).normal(size=(256, 2))  # dispersed starts
    early = _linear_sampler().run(u0, n_samples=20, burn_in=0, sample_interval=1)
    late = _linear_sampler().run(u0, n_samples=200, burn_in=2000, sample_interval=5)
    r_early = quiet(rank_convergence, early, backend="device")["rhat"]
    r_late = quiet(rank_convergence, late, backend="device")["rhat"]
    assert (r_early > r_late).all(), f"rhat without burn-in {r_early} vs after 2000 steps of burn-in {r_late}"

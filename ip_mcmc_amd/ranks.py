"""Rank-normalised convergence diagnostics and exact pooled quantiles.

  rank_normalize(samples)      average ranks / normal scores over all chains' pooled samples
  pooled_quantiles(samples, q) np.quantile of the pooled samples, exactly
  rank_convergence(samples)    rank-normalised split-R̂ (bulk, folded), bulk- and tail-ESS
                               (Vehtari, Gelman, Simpson, Carpenter, Bürkner 2021)

All three rest on one sort of the C·n pooled samples of each component:
ipmc_pooled_sort (a stable segmented radix sort that reads the strided samples
in place) and ipmc_rank_scores (average ranks over tie runs, Φ⁻¹ by AS241) on
the device, a stable argsort and scipy's ndtri on the host.

Definition.  x is (C, n, k), N = n // 2, the used samples are t < 2N of every
chain (an odd last sample is dropped, as in convergence()), S = C·2N.  The
average rank r of a sample among the S pooled ones of its component counts
ties by the mean of their positions; its normal score is
z = Φ⁻¹((r − 3/8)/(S + 1/4)).  Each part of rank_convergence is convergence()'s
definition (diagnostics: split chains, W, B, Geyer's sum) applied to a
transformed copy of the samples:

  rhat_bulk, ess_bulk   z of x
  rhat_tail             z of |x − median|, the median pooled over the used samples
  rhat                  max(rhat_bulk, rhat_tail)
  ess_tail              min of the ESS of the 0/1 series x <= q_lo and x <= q_hi,
                        q the pooled `tail` quantiles of the used samples
"""
import ctypes
import warnings

import numpy as np
import torch

from . import device as dev
from ._lib import call
from .diagnostics import (_check_layout, _check_lengths, _device_parts, _device_samples, _finish, _host_parts,
                          _host_samples, _on_device)

SORT_TILE = 4096  # IPMC_SORT_TILE (include/ipmc.h): keys of one workgroup's tile of the sort
MEMORY_SHARE = 0.25  # of the free device memory: what one slab of components may take
# device bytes per pooled sample of one component while a slab is sorted: sorted 8 + permutation 4, the
# sort's second buffers 12 and its tile counts 0.25 (the transformed series, 8 k S, is whole and comes on top)
SLAB_BYTES_PER_SAMPLE = 25


# ------------------------------------------------------------------ quantiles
def _quantile_plan(S, q):
    """np.quantile's default (linear) method over S sorted values: the virtual index (S - 1) q, the
    positions of its two neighbouring order statistics and the weight of the upper one."""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or not ((q >= 0) & (q <= 1)).all():
        raise ValueError("quantiles must be a scalar or a 1-D sequence in [0, 1]")
    virtual = (S - 1) * q
    lo = np.floor(virtual).astype(np.int64)
    gamma = virtual - lo
    lo = np.clip(lo, 0, S - 1)
    return lo, np.minimum(lo + 1, S - 1), gamma


def _interpolate(lo_vals, hi_vals, gamma, last):
    """(k, len(q)) quantiles from the neighbouring order statistics (k, len(q)) each.  The interpolation
    is numpy's own: np.quantile of the pair [lo, hi] at gamma has the virtual index gamma and applies the
    same lerp to the same three numbers.  last (k,): the largest sorted value; NaN there (NaN sorts last)
    makes the component's quantiles NaN, as np.quantile does."""
    out = np.empty(lo_vals.shape)
    for i, g in enumerate(gamma):
        out[:, i] = np.quantile(np.stack([lo_vals[:, i], hi_vals[:, i]], axis=1), g, axis=1)
    out[np.isnan(last)] = np.nan
    return out


def _quantiles_of_sorted(srt, q):
    """srt: (k, S) ascending, numpy or device tensor -> (k, len(q)) float64 numpy; a few elements per
    component leave the device."""
    S = srt.shape[1]
    lo, hi, gamma = _quantile_plan(S, q)
    idx = np.concatenate([lo, hi, [S - 1]])
    if isinstance(srt, torch.Tensor):
        got = srt[:, torch.from_numpy(idx).to(srt.device)].cpu().numpy()
    else:
        got = srt[:, idx]
    m = len(lo)
    return _interpolate(got[:, :m], got[:, m:2 * m], gamma, got[:, -1])


# --------------------------------------------------------------------- host
def _host_ranks(x):
    """x float64 (C, m, k) -> (average ranks (C, m, k), sorted values (k, C·m)).  Ties (==) share the mean
    of their positions; a NaN sample sorts last and has rank NaN."""
    C, m, k = x.shape
    S = C * m
    pooled = x.reshape(S, k)
    order = np.argsort(pooled, axis=0, kind="stable")
    srt = np.take_along_axis(pooled, order, axis=0)
    pos = np.arange(S)[:, None]
    edge = srt[1:] != srt[:-1]  # a run ends before position j + 1
    start, end = np.ones((S, k), dtype=bool), np.ones((S, k), dtype=bool)
    start[1:], end[:-1] = edge, edge
    a = np.maximum.accumulate(np.where(start, pos, 0), axis=0)
    b = np.minimum.accumulate(np.where(end, pos, S - 1)[::-1], axis=0)[::-1]
    r = (a + b) / 2 + 1.0
    r[np.isnan(srt)] = np.nan
    ranks = np.empty((S, k))
    np.put_along_axis(ranks, order, r, axis=0)
    return ranks.reshape(C, m, k), np.ascontiguousarray(srt.T)


def _host_scores(ranks, S):
    from scipy.special import ndtri  # lazily, as covariance.py: scipy is needed on the host path alone

    return ndtri((ranks - 0.375) / (S + 0.25))


# ------------------------------------------------------------------- device
def _geometry(t, layout):
    """-> (C, n, k, stride_chain, stride_t, stride_var) of a contiguous 3-D tensor."""
    C, a, b = t.shape
    n, k, s_t, s_var = (a, b, b, 1) if layout == "time_vars" else (b, a, 1, b)
    return C, n, k, a * b, s_t, s_var


def _default_slab(t, S, k):
    free, _ = torch.cuda.mem_get_info(t.device)
    return int(max(1, min(k, (MEMORY_SHARE * free) // (SLAB_BYTES_PER_SAMPLE * max(S, 1)))))


def _slabs(t, S, k, component_slab):
    slab = _default_slab(t, S, k) if component_slab is None else int(component_slab)
    if slab < 1:
        raise ValueError("component_slab must be positive")
    return [(v0, min(slab, k - v0)) for v0 in range(0, k, slab)]


def _sort_slab(t, layout, length, v0, ks, center=None):
    """ipmc_pooled_sort of components [v0, v0 + ks) over the samples t < length of every chain, read in
    place: (sorted (ks, S) float64, permutation (ks, S) int32 holding the uint32 pooled indices)."""
    C, _, _, s_chain, s_t, s_var = _geometry(t, layout)
    S = C * length
    dtype = dev.abi_dtype(t.dtype)
    need = ctypes.c_int64(0)
    call("ipmc_sort_workspace", C, length, ks, dtype, ctypes.byref(need))
    ws = torch.empty(max(need.value, 1), dtype=torch.uint8, device=t.device)
    srt = torch.empty((ks, S), dtype=torch.float64, device=t.device)
    perm = torch.empty((ks, S), dtype=torch.int32, device=t.device)
    cen = None
    if center is not None:
        cen = torch.from_numpy(np.ascontiguousarray(center, dtype=np.float64)).to(t.device)
    call("ipmc_pooled_sort", t.data_ptr() + v0 * s_var * t.element_size(), dtype, C, length, ks, s_chain, s_t, s_var,
         None if cen is None else cen.data_ptr(), srt.data_ptr(), perm.data_ptr(), ws.data_ptr(), need.value,
         dev.stream_handle(t.device))
    return srt, perm


def _scores_slab(srt, perm, C, length, mode, out, v0):
    """ipmc_rank_scores into components [v0, v0 + ks) of out, a contiguous (C, length, K) float64 tensor."""
    s_chain, s_t, s_var = out.stride()
    call("ipmc_rank_scores", srt.data_ptr(), perm.data_ptr(), srt.shape[0], C, length, mode,
         out.data_ptr() + v0 * s_var * out.element_size(), s_chain, s_t, s_var, None, 0, dev.stream_handle(out.device))


def _used(t, layout):
    """-> (C, n, k, N): the geometry and the split length of the samples that count."""
    C, n, k = _geometry(t, layout)[:3]
    if C < 1:
        raise ValueError("rank statistics need at least one chain")
    return C, n, k, _check_lengths(n, None)[0]


# ------------------------------------------------------------------- public
def rank_normalize(samples, fold=False, scores=True, layout="time_vars", backend="auto", device=None,
                   component_slab=None):
    """Normal scores z = Φ⁻¹((r − 3/8)/(S + 1/4)) of the average ranks r of every used sample among the
    S = C·2N pooled ones of its component (N = n // 2; an odd last sample is dropped), as float64
    (C, 2N, k) whatever the layout given; scores=False returns the ranks themselves.  fold=True ranks
    |x − pooled median| (the median of the used samples).  Inputs, layout, backend and device are
    convergence()'s; the result is a CUDA tensor on the device backend and numpy on the host backend.
    A NaN sample has a NaN result."""
    _check_layout(layout)
    if not _on_device(backend):
        x = _host_samples(samples, layout)
        if x.shape[0] < 1:
            raise ValueError("rank statistics need at least one chain")
        N = _check_lengths(x.shape[1], None)[0]
        x = np.ascontiguousarray(x[:, :2 * N])
        if fold:
            x = np.abs(x - _quantiles_of_sorted(_host_ranks(x)[1], 0.5)[:, 0])
        ranks = _host_ranks(x)[0]
        return _host_scores(ranks, x.shape[0] * 2 * N) if scores else ranks
    t = _device_samples(samples, device)
    C, n, k, N = _used(t, layout)
    out = torch.empty((C, 2 * N, k), dtype=torch.float64, device=t.device)
    for v0, ks in _slabs(t, C * 2 * N, k, component_slab):
        srt, perm = _sort_slab(t, layout, 2 * N, v0, ks)
        if fold:
            srt, perm = _sort_slab(t, layout, 2 * N, v0, ks, center=_quantiles_of_sorted(srt, 0.5)[:, 0])
        _scores_slab(srt, perm, C, 2 * N, 1 if scores else 0, out, v0)
    return out


def pooled_quantiles(samples, q, layout="time_vars", backend="auto", device=None, component_slab=None):
    """The quantiles q (a scalar or a sequence in [0, 1]) of each component over all n samples of all
    chains: float64 numpy (k, len(q)), equal to np.quantile(pooled, q, axis=0).T exactly (the two
    neighbouring order statistics of each quantile come from the sort, numpy interpolates).  A component
    with a NaN sample has NaN quantiles."""
    _check_layout(layout)
    if not _on_device(backend):
        x = _host_samples(samples, layout)
        C, n, k = x.shape
        if C * n < 1:
            raise ValueError("pooled_quantiles needs at least one sample")
        return _quantiles_of_sorted(np.ascontiguousarray(np.sort(x.reshape(C * n, k), axis=0).T), q)
    t = _device_samples(samples, device)
    C, n, k = _geometry(t, layout)[:3]
    if C * n < 1:
        raise ValueError("pooled_quantiles needs at least one sample")
    return np.concatenate([_quantiles_of_sorted(_sort_slab(t, layout, n, v0, ks)[0], q)
                           for v0, ks in _slabs(t, C * n, k, component_slab)], axis=0)


def _finish_quiet(parts, C, n_used, N, L):
    """convergence()'s _finish without its "max_lag ... ended the autocorrelation sum" warning (any other
    warning passes); the components it would have named come back, for the one warning of the call.
    `short` restates _finish's rule for naming a component, W > 0 and not truncated (a comment there
    points here)."""
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=r"convergence: max_lag=.* ended the autocorrelation sum")
        r = _finish(*parts, C, n_used, N, L)
    short = (parts[1] > 0) & ~r["truncated"] if L is not None else None
    return r, short


def _check_tail(tail):
    lo, hi = (float(v) for v in tail)
    if not 0.0 <= lo <= hi <= 1.0:
        raise ValueError("tail must be two probabilities (lo, hi) with 0 <= lo <= hi <= 1")
    return lo, hi


def rank_convergence(samples, max_lag=None, tail=(0.05, 0.95), layout="time_vars", backend="auto", device=None,
                     block_chains=1024, component_slab=None):
    """Rank-normalised split-R̂ with bulk- and tail-ESS per component (the definition at the top of the
    module): each part is convergence()'s definition on a transformed copy of the used samples.

    samples, max_lag, layout, backend, device and block_chains are convergence()'s.  tail: the two pooled
    quantile levels of the tail indicators.  component_slab: components sorted per call on the device;
    by default as many as keep the sort's outputs and workspace within MEMORY_SHARE of the free device
    memory (beside them one (C, 2N, k) float64 buffer holds each transformed series in turn).  Every
    component is independent and the sums run over whole series: no result depends on it.

    Returns a dict of numpy (k,): rhat_bulk, rhat_tail, rhat = max of the two, ess_bulk, ess_tail,
    median, q_lo, q_hi (float64), the bulk run's lag_used (int64) and truncated (bool); and n_chains,
    n_samples, n_split.  A component whose transformed series has W == 0 (a constant component: all its
    ranks tie) has nan there, as in convergence(); a component with a NaN sample has nan in every float
    output and leaves the others as they are.  Components of any ESS part whose pair sum reached
    max_lag before turning negative are named in one warning."""
    _check_layout(layout)
    q_levels = (0.5,) + _check_tail(tail)
    on_device = _on_device(backend)
    if on_device:
        t = _device_samples(samples, device)
        C, n, k, N = _used(t, layout)
    else:
        x = _host_samples(samples, layout)
        C, n, k = x.shape
        if C < 1:
            raise ValueError("rank statistics need at least one chain")
        N = _check_lengths(n, None)[0]
        x = np.ascontiguousarray(x[:, :2 * N])
    L = _check_lengths(n, max_lag)[1]
    m, S = 2 * N, C * 2 * N
    if on_device:
        # The sorts go slab by slab; each transformed series is whole, (C, 2N, k) in one buffer used four
        # times, so that the sums of convergence()'s kernels (whose order is a function of k) do not
        # depend on the slabs.
        z = torch.empty((C, m, k), dtype=torch.float64, device=t.device)
        slabs = _slabs(t, S, k, component_slab)
        qv, last = np.empty((k, 3)), np.empty(k)
        for v0, ks in slabs:
            srt, perm = _sort_slab(t, layout, m, v0, ks)
            qv[v0:v0 + ks] = _quantiles_of_sorted(srt, q_levels)
            last[v0:v0 + ks] = srt[:, -1].cpu().numpy()
            _scores_slab(srt, perm, C, m, 1, z, v0)
        bulk = _device_parts(z, "time_vars", L, block_chains)
        for v0, ks in slabs:
            srt, perm = _sort_slab(t, layout, m, v0, ks, center=qv[v0:v0 + ks, 0])
            _scores_slab(srt, perm, C, m, 1, z, v0)
        del srt, perm
        folded = _device_parts(z, "time_vars", None, block_chains)
        xs = t[:, :m] if layout == "time_vars" else t[:, :, :m].transpose(1, 2)
        below = []
        for j in (1, 2):  # f32 samples are widened by the comparison with the float64 edges; 0.0 / 1.0 series
            z.copy_(xs <= torch.from_numpy(np.ascontiguousarray(qv[:, j])).to(t.device))
            below.append(_device_parts(z, "time_vars", L, block_chains))
        has_nan = np.isnan(last)
    else:
        ranks, srt = _host_ranks(x)
        qv = _quantiles_of_sorted(srt, q_levels)
        has_nan = np.isnan(srt[:, -1])
        bulk = _host_parts(np.ascontiguousarray(_host_scores(ranks, S)), L)
        folded = _host_parts(np.ascontiguousarray(_host_scores(_host_ranks(np.abs(x - qv[:, 0]))[0], S)), None)
        below = [_host_parts(np.ascontiguousarray((x <= qv[:, j]).astype(np.float64)), L) for j in (1, 2)]
    rb, sb = _finish_quiet(bulk, C, m, N, L)
    rf, _ = _finish_quiet(folded, C, m, N, None)
    tails = [_finish_quiet(p, C, m, N, L) for p in below]
    nan = np.where(has_nan, np.nan, 0.0)  # added to a float output: nan for a component with a NaN sample
    out = {"rhat_bulk": rb["rhat"] + nan, "ess_bulk": rb["ess"] + nan, "rhat_tail": rf["rhat"] + nan,
           "ess_tail": np.minimum(tails[0][0]["ess"], tails[1][0]["ess"]) + nan,
           "median": qv[:, 0].copy(), "q_lo": qv[:, 1].copy(), "q_hi": qv[:, 2].copy(),
           "lag_used": rb["lag_used"], "truncated": rb["truncated"]}
    short = (sb | tails[0][1] | tails[1][1]) & ~has_nan
    out["rhat"] = np.maximum(out["rhat_bulk"], out["rhat_tail"])
    out.update(n_chains=C, n_samples=n, n_split=N)
    if short.any():
        warnings.warn(f"rank_convergence: max_lag={L} ended the autocorrelation sum before a negative pair for "
                      f"component(s) {np.flatnonzero(short).tolist()}: tau is a lower and ess an upper bound there "
                      "(raise max_lag or run longer chains)", stacklevel=2)
    return out

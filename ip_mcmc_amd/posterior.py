"""The pooled posterior's shape, on the device where the samples are.

  support(samples)                          per-component (min, max) over all chains and samples
  marginal_histograms(samples, bins, range) np.histogram per component: counts, edges, below, above, n
  histogramdd(samples, bins, range, components)   np.histogramdd over up to four components
  hist_quantiles(hist, q)                   quantiles from a marginal histogram (host)
  wasserstein_to_point(counts, intervals, point)  W1 between a binned posterior and a point mass (host)
  wasserstein_1d(counts_a, counts_b, interval)    W1 between two 1-D histograms on the same ticks (host)
  wasserstein_distance(d1, d2, intervals)   helpers.wasserstein_distance (helpers.py:57-77) where it has a
                                            closed form; two general N-D histograms raise NotImplementedError

This is the binning of the reference's last two studies
(report/scripts/burgers/burgers_wasserstein_chain.py:169-188 and
burgers_wasserstein_grid.py): intervals from the data's min and max, then
np.histogramdd(chain.T, bins=20, range=intervals), then helpers.py:57-77's
distance to the histogram of one point, the ground truth.  The reference
solves that transport problem with POT's ot.emd2; transport to a point mass
needs no solver (all mass moves to the point), so the distance here is the
closed form Σ p(cell) ‖tick(cell) − tick(cell*)‖₂ on the reference's ticks.

Definition (backend="host", numpy; the device kernels ipmc_minmax, ipmc_hist1d
and ipmc_histdd give the same integers):

  edges   np.linspace(lo, hi, B + 1) for a component with range (lo, hi) and B bins
  range   None = the data's own min and max per component; lo == hi becomes
          (lo - 0.5, hi + 0.5) (numpy's rule)
  bins    x is in bin b iff edges[b] <= x < edges[b + 1]; the last bin also holds
          x == edges[B]; x < edges[0] is below, x > edges[B] above, NaN nowhere
  f32 samples are widened to f64 before any comparison; edges are f64; counts int64

which is np.searchsorted(edges, x, "right") - 1 with the right edge folded in,
and equals np.histogram / np.histogramdd count for count.  A joint histogram
drops a sample when any selected component is outside its range.

Inputs are those of diagnostics.convergence: numpy arrays, a memory-mapped
sample_file or a CUDA tensor (never copied: a burn-in slice or a transposed
view goes to the kernels by its strides), shaped (C, n, k) or (n, k), or
(C, k, n) with layout="vars_time".  A host input goes to the device in chunks
of whole chains of at most chunk_bytes; counts add exactly and min / max
combine, so a sample file larger than the device's memory works and no result
depends on the chunking.
"""
import ctypes

import numpy as np
import torch

from . import device as dev
from ._lib import call
from .diagnostics import _check_layout, _is_cuda, _on_device

MINMAX_GROUPS = 1024  # IPMC_MINMAX_GROUPS (include/ipmc.h)
MAX_BINS = 4096
MAX_CELLS = 1 << 24
DEFAULT_CHUNK_BYTES = 1 << 30


# ------------------------------------------------------------------ inputs
def _as3d(samples):
    """samples -> (3-D numpy array or CUDA tensor, no copy); (n, k) becomes one chain."""
    if _is_cuda(samples):
        x = samples
        if x.dtype not in (torch.float32, torch.float64):
            x = x.double()
        if x.dim() == 2:
            x = x.unsqueeze(0)
        ndim = x.dim()
    else:
        x = samples.detach().numpy() if isinstance(samples, torch.Tensor) else np.asanyarray(samples)
        if x.dtype not in (np.float32, np.float64):
            x = x.astype(np.float64)
        if x.ndim == 2:
            x = x[None]
        ndim = x.ndim
    if ndim != 3:
        raise ValueError(f"samples must be (C, n, k) or (n, k), got shape {tuple(samples.shape)}")
    return x


def _shape(x, layout):
    """(C, n, k) of a 3-D input in `layout`."""
    C, a, b = x.shape
    return (C, a, b) if layout == "time_vars" else (C, b, a)


def _chain_chunks(x, layout, chunk_bytes):
    """Slices of whole chains of a host (C, ., .) array, each at most chunk_bytes (at least one chain)."""
    C = x.shape[0]
    per_chain = max(1, x.shape[1] * x.shape[2] * x.dtype.itemsize)
    step = max(1, int(chunk_bytes) // per_chain)
    for c0 in range(0, C, step):
        yield x[c0:c0 + step]


def _device_chunks(x, layout, device, chunk_bytes):
    """CUDA tensors of whole chains: the input itself, or a host input chunk by chunk."""
    if _is_cuda(x):
        yield x
        return
    d = dev.resolve_device(device)
    for part in _chain_chunks(x, layout, chunk_bytes):
        a = np.ascontiguousarray(part)
        if not a.flags.writeable:  # a read-only memory map
            a = a.copy()
        yield torch.from_numpy(a).to(d)


def _geom(t, layout):
    """The strided geometry of the C-ABI for a 3-D CUDA tensor: (ptr, dtype, C, n, k, s_chain, s_t, s_var)."""
    C, n, k = _shape(t, layout)
    s0, s1, s2 = t.stride()
    s_t, s_var = (s1, s2) if layout == "time_vars" else (s2, s1)
    if min(s0, s1, s2) < 0:
        raise ValueError("samples with negative strides are not supported")
    return (t.data_ptr(), dev.abi_dtype(t.dtype), C, n, k, s0, s_t, s_var)


def _host_cnk(part, layout):
    """float64 (C, n, k) view or copy of a host chunk."""
    a = np.asarray(part, dtype=np.float64)
    return a.transpose(0, 2, 1) if layout == "vars_time" else a


# -------------------------------------------------------------- definition
def _edges(lo, hi, bins):
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"histogram range ({lo}, {hi}) is not finite")
    if lo > hi:
        raise ValueError(f"histogram range ({lo}, {hi}): max must be larger than min")
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, int(bins) + 1)


def _bin_index(x, edges):
    """Bin of every x (float64) among edges[0..B]: 0..B-1, B = below, B + 1 = above, -1 = NaN."""
    B = len(edges) - 1
    b = np.searchsorted(edges, x, "right") - 1
    b[x == edges[B]] = B - 1
    b[x < edges[0]] = B
    b[x > edges[B]] = B + 1
    b[np.isnan(x)] = -1
    return b


def _check_bins(b):
    b = int(b)
    if b < 1 or b > MAX_BINS:
        raise ValueError(f"bins = {b} outside [1, {MAX_BINS}]")
    return b


def _ranges(rng, k, what):
    """range argument -> (k, 2) float64 or None."""
    if rng is None:
        return None
    r = np.asarray(rng, dtype=np.float64)
    if r.shape == (2,):
        r = np.broadcast_to(r, (k, 2))
    if r.shape != (k, 2):
        raise ValueError(f"range must be (lo, hi) or one (lo, hi) per {what}: shape ({k}, 2), got {r.shape}")
    return r


# ----------------------------------------------------------------- support
def _support_device(chunks, layout, k):
    lo, hi = np.full(k, np.inf), np.full(k, -np.inf)
    for t in chunks:
        f64 = dict(dtype=torch.float64, device=t.device)
        out = torch.empty((2, k), **f64)
        scratch = torch.empty(2 * MINMAX_GROUPS * k, **f64)
        call("ipmc_minmax", *_geom(t, layout), out[0].data_ptr(), out[1].data_ptr(), scratch.data_ptr(),
             dev.stream_handle(t.device))
        o = out.cpu().numpy()
        lo, hi = np.minimum(lo, o[0]), np.maximum(hi, o[1])
    return np.stack([lo, hi], axis=1)


def _support_host(chunks, layout, k):
    lo, hi = np.full(k, np.inf), np.full(k, -np.inf)
    for part in chunks:
        a = _host_cnk(part, layout).reshape(-1, k)
        if a.shape[0] == 0:
            continue
        with np.errstate(invalid="ignore"):
            fin = ~np.isnan(a)
            lo = np.minimum(lo, np.where(fin, a, np.inf).min(axis=0))
            hi = np.maximum(hi, np.where(fin, a, -np.inf).max(axis=0))
    return np.stack([lo, hi], axis=1)


def _support(x, layout, on_device, device, chunk_bytes):
    k = _shape(x, layout)[2]
    if on_device:
        return _support_device(_device_chunks(x, layout, device, chunk_bytes), layout, k)
    return _support_host(_chain_chunks(x, layout, chunk_bytes), layout, k)


def _prepare(samples, layout, backend, chunk_bytes):
    _check_layout(layout)
    on_device = _on_device(backend)
    x = _as3d(samples)
    if _is_cuda(x) and not on_device:
        x = x.cpu().numpy()
    if chunk_bytes <= 0:
        raise ValueError("chunk_bytes must be positive")
    return x, on_device


def support(samples, layout="time_vars", backend="auto", device=None, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """Per-component (min, max) over all chains and samples: float64 (k, 2).
    NaN is skipped; a component with no comparable sample gives (+inf, -inf)."""
    x, on_device = _prepare(samples, layout, backend, chunk_bytes)
    return _support(x, layout, on_device, device, chunk_bytes)


# --------------------------------------------------------------- marginals
def marginal_histograms(samples, bins=20, range=None, layout="time_vars", backend="auto", device=None,
                        chunk_bytes=DEFAULT_CHUNK_BYTES):
    """np.histogram(samples[..., v], bins, range) for every component v, pooled over all chains.

    bins: one int B (1..4096).  range: None (each component's own min and max),
    one (lo, hi) for all components or a (k, 2) array.
    Returns {"counts": int64 (k, B), "edges": float64 (k, B + 1), "below": int64 (k,),
    "above": int64 (k,), "n": samples per component (C * n)}; NaN samples are in none of them."""
    x, on_device = _prepare(samples, layout, backend, chunk_bytes)
    C, n, k = _shape(x, layout)
    B = _check_bins(bins)
    r = _ranges(range, k, "component")
    if r is None:
        r = _support(x, layout, on_device, device, chunk_bytes)
        if C * n == 0:
            r = np.zeros((k, 2))  # numpy's range for no data: (0, 1)
            r[:, 1] = 1.0
        elif not np.all(np.isfinite(r)):
            raise ValueError("range=None needs at least one finite sample per component and no infinite ones")
    edges = np.stack([_edges(lo, hi, B) for lo, hi in r])
    counts = np.zeros((k, B), dtype=np.int64)
    below, above = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
    if on_device:
        for t in _device_chunks(x, layout, device, chunk_bytes):
            e = torch.from_numpy(edges).to(t.device)
            i64 = dict(dtype=torch.int64, device=t.device)
            out = torch.empty(k * B + 2 * k, **i64)
            c, lo, hi = out[:k * B], out[k * B:k * B + k], out[k * B + k:]
            call("ipmc_hist1d", *_geom(t, layout), B, e.data_ptr(), c.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                 dev.stream_handle(t.device))
            o = out.cpu().numpy()
            counts += o[:k * B].reshape(k, B)
            below += o[k * B:k * B + k]
            above += o[k * B + k:]
    else:
        for part in _chain_chunks(x, layout, chunk_bytes):
            a = _host_cnk(part, layout).reshape(-1, k)
            for v in np.arange(k):
                b = _bin_index(np.ascontiguousarray(a[:, v]), edges[v])
                full = np.bincount(b[b >= 0], minlength=B + 2)
                counts[v] += full[:B]
                below[v] += full[B]
                above[v] += full[B + 1]
    return {"counts": counts, "edges": edges, "below": below, "above": above, "n": C * n}


# ------------------------------------------------------------------- joint
def histogramdd(samples, bins=20, range=None, components=None, layout="time_vars", backend="auto", device=None,
                chunk_bytes=DEFAULT_CHUNK_BYTES):
    """np.histogramdd over the selected components of the pooled samples.

    components: up to four component indices, default all when k <= 4.
    bins: one int or one per selected component (each 1..4096, at most 2^24 cells in all).
    range: None (the data's min and max per selected component) or one (lo, hi) per selected component.
    Returns (counts, edges) shaped like numpy's: counts int64 of shape bins, edges a list of
    float64 arrays.  A sample counts iff every selected component is inside its range."""
    x, on_device = _prepare(samples, layout, backend, chunk_bytes)
    C, n, k = _shape(x, layout)
    if components is None:
        if k > 4:
            raise ValueError(f"histogramdd needs components= (at most 4 of the k = {k})")
        components = tuple(np.arange(k).tolist())
    comp = [int(c) for c in components]
    nd = len(comp)
    if nd < 1 or nd > 4:
        raise ValueError(f"histogramdd takes 1 to 4 components, got {nd}")
    if any(c < 0 or c >= k for c in comp):
        raise ValueError(f"components {comp} outside [0, k = {k})")
    nb = [_check_bins(b) for b in (np.broadcast_to(np.asarray(bins), (nd,)).tolist())]
    cells = int(np.prod(nb, dtype=np.int64))
    if cells > MAX_CELLS:
        raise ValueError(f"{cells} cells exceed 2^24")
    r = _ranges(range, nd, "selected component")
    if r is None:
        full = _support(x, layout, on_device, device, chunk_bytes)
        if C * n == 0:
            full = np.zeros((k, 2))
            full[:, 1] = 1.0
        r = full[comp]
        if not np.all(np.isfinite(r)):
            raise ValueError("range=None needs at least one finite sample per component and no infinite ones")
    edges = [_edges(lo, hi, b) for (lo, hi), b in zip(r, nb)]
    counts = np.zeros(cells, dtype=np.int64)
    if on_device:
        c_comp, c_bins = (ctypes.c_int32 * nd)(*comp), (ctypes.c_int32 * nd)(*nb)
        for t in _device_chunks(x, layout, device, chunk_bytes):
            e = torch.from_numpy(np.concatenate(edges)).to(t.device)
            out = torch.empty(cells, dtype=torch.int64, device=t.device)
            call("ipmc_histdd", *_geom(t, layout), nd, ctypes.addressof(c_comp), ctypes.addressof(c_bins),
                 e.data_ptr(), out.data_ptr(), dev.stream_handle(t.device))
            counts += out.cpu().numpy()
    else:
        for part in _chain_chunks(x, layout, chunk_bytes):
            a = _host_cnk(part, layout).reshape(-1, k)
            keep = np.ones(a.shape[0], dtype=bool)
            idx = []
            for c, e, b in zip(comp, edges, nb):
                bi = _bin_index(np.ascontiguousarray(a[:, c]), e)
                keep &= (bi >= 0) & (bi < b)
                idx.append(bi)
            flat = np.ravel_multi_index([bi[keep] for bi in idx], nb)
            counts += np.bincount(flat, minlength=cells)
    return counts.reshape(nb), edges


# --------------------------------------------------------------- quantiles
def hist_quantiles(hist, q):
    """Per-component quantiles from marginal_histograms' result: linear inside the
    bin where the cumulative in-range count crosses q * total.  Exact to one bin
    width (the samples' positions inside a bin are not kept); below / above and
    NaN samples do not count.  q scalar -> (k,), q (m,) -> (k, m); nan for a
    component without in-range samples.  Host."""
    counts, edges = np.asarray(hist["counts"]), np.asarray(hist["edges"])
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if np.any((qs < 0) | (qs > 1)):
        raise ValueError("quantiles must be in [0, 1]")
    k, B = counts.shape
    out = np.full((k, len(qs)), np.nan)
    for v in np.arange(k):
        cum = np.cumsum(counts[v])
        total = cum[-1]
        if total == 0:
            continue
        for j, qq in enumerate(qs):
            target = qq * total
            b = min(int(np.searchsorted(cum, target, "left")), B - 1)
            while counts[v, b] == 0 and b < B - 1:  # q = 0 with empty leading bins
                b += 1
            before = cum[b] - counts[v, b]
            frac = (target - before) / counts[v, b] if counts[v, b] else 0.0
            out[v, j] = edges[v, b] + min(max(frac, 0.0), 1.0) * (edges[v, b + 1] - edges[v, b])
    return out[:, 0] if np.ndim(q) == 0 else out


# ------------------------------------------------------------- Wasserstein
def _ticks(counts, intervals):
    """The reference's ticks (helpers.py:69-72): np.linspace(lo, hi, B) per axis -- B ticks
    across the interval, not the bin centres."""
    iv = np.asarray(intervals, dtype=np.float64).reshape(-1, 2)
    if iv.shape[0] != counts.ndim:
        raise ValueError(f"{counts.ndim}-D counts need {counts.ndim} intervals, got {iv.shape[0]}")
    return iv, [np.linspace(iv[d, 0], iv[d, 1], counts.shape[d]) for d in np.arange(counts.ndim)]


def _probabilities(counts):
    c = np.asarray(counts, dtype=np.float64)
    total = c.sum()
    if not total > 0 or np.any(c < 0):
        raise ValueError("a histogram needs non-negative counts with a positive sum")
    return c / total


def _w1_to_cell(counts, ticks, cell):
    """Σ p(c) ‖tick(c) − tick(cell)‖₂ for a target given by its cell index."""
    p = _probabilities(counts)
    dist2 = np.zeros(p.shape)
    for d in np.arange(p.ndim):
        shape = [1] * p.ndim
        shape[d] = -1
        dist2 = dist2 + ((ticks[d] - ticks[d][cell[d]]) ** 2).reshape(shape)
    return float((p * np.sqrt(dist2)).sum())


def wasserstein_to_point(counts, intervals, point):
    """W1 (Euclidean ground metric) between the binned posterior `counts` (N-D, any
    normalisation) on `intervals` (N, 2) and the histogram of the single `point`, as
    helpers.wasserstein_distance(d1, ground_truth, intervals) computes it: the mass of every
    cell moves to the cell that holds the point, Σ p(cell) ‖tick(cell) − tick(cell*)‖₂."""
    p = _probabilities(counts)
    iv, ticks = _ticks(p, intervals)
    pt = np.atleast_1d(np.asarray(point, dtype=np.float64))
    if pt.shape != (p.ndim,):
        raise ValueError(f"point must have {p.ndim} coordinates")
    cell = []
    for d in np.arange(p.ndim):
        b = int(_bin_index(pt[d:d + 1], _edges(iv[d, 0], iv[d, 1], p.shape[d]))[0])
        if b < 0 or b >= p.shape[d]:
            raise ValueError(f"point coordinate {d} = {pt[d]} is outside its interval [{iv[d, 0]}, {iv[d, 1]}]")
        cell.append(b)
    return _w1_to_cell(p, ticks, cell)


def wasserstein_1d(counts_a, counts_b, interval):
    """W1 between two 1-D histograms on the same B ticks np.linspace(lo, hi, B): the CDF form
    Σ_i |A_i − B_i| (tick_{i+1} − tick_i) over the cumulative probabilities."""
    a, b = _probabilities(np.ravel(counts_a)), _probabilities(np.ravel(counts_b))
    if a.shape != b.shape:
        raise ValueError("the two histograms need the same number of bins")
    _, (t,) = _ticks(a, interval)
    return float((np.abs(np.cumsum(a) - np.cumsum(b))[:-1] * np.diff(t)).sum())


def wasserstein_distance(d1, d2, intervals):
    """helpers.wasserstein_distance (helpers.py:57-77) without an LP solver: 1-D histograms by
    the CDF form, an N-D histogram against a point mass (one non-zero cell, as the reference's
    ground truth) by the closed form.  Two general N-D histograms need an optimal-transport
    linear program and are out of scope: NotImplementedError."""
    a, b = np.asarray(d1), np.asarray(d2)
    if a.shape != b.shape:
        raise ValueError("the two histograms need one shape")
    if a.ndim == 1:
        return wasserstein_1d(a, b, intervals)
    for hist, other in ((a, b), (b, a)):
        if np.count_nonzero(other) == 1:
            _, ticks = _ticks(other, intervals)
            cell = np.argwhere(other)[0]
            return _w1_to_cell(hist, ticks, cell)
    raise NotImplementedError("W1 between two general N-D histograms needs an optimal-transport linear program "
                              "(the reference uses POT's ot.emd2); only 1-D pairs and an N-D histogram against "
                              "a point mass are implemented")

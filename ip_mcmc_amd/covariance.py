"""Second moments between components, on the device where the samples are.

  posterior_covariance(samples)   mean, covariance and correlation matrix of the pooled posterior
  multivariate_rhat(samples)      within- and between-chain covariance of the split chains and the
                                  multivariate potential scale reduction (Brooks & Gelman 1998)

diagnostics.convergence and posterior.marginal_histograms look at one component
at a time.  A linear-Gaussian posterior keeps its information in the
off-diagonal entries (Σ = Σ₀ − Σ₀g gᵀΣ₀/(γ² + gᵀΣ₀g)), and chains that disagree
only along a narrow direction of a strongly correlated posterior pass every
per-component R̂: both need the k × k matrices.

Definition (backend="host", numpy float64; the device kernel ipmc_scatter
computes the same sums and differs only in the order of the adds).  x is
(C, n, k), N = n // 2, and the split chains are diagnostics.convergence's:
M = 2C of them, first halves of all chains, then second halves, an odd last
sample dropped; μ_m are their means.

posterior_covariance pools all R = C n rows (the odd last sample included), as
a corrected two-pass:

  a     the mean of the μ_m (n >= 4; shorter chains have no split chains and a is the first row)
  D     Σ_r (x_r − a),   S = Σ_r (x_r − a)(x_r − a)ᵀ
  mean  a + D/R
  cov   (S − D Dᵀ/R)/(R − 1)      = np.cov(x.reshape(-1, k), rowvar=False)
  corr  cov/sqrt(diag ⊗ diag)      = np.corrcoef; the diagonal is exactly 1

a is within rounding of the mean (or half a sample off for odd n), so the
correction D Dᵀ/R is tiny and nothing cancels: components of 10⁵ standard
deviations keep fifteen digits where Σ x xᵀ − (Σx)(Σx)ᵀ/R keeps five.  A
component whose variance is zero has nan in its row and column of corr; a NaN
sample makes only the rows and columns of its component NaN.

multivariate_rhat (n >= 4):

  W           (1/M) Σ_m Σ_{t<N} (x_mt − μ_m)(x_mt − μ_m)ᵀ/(N − 1)
  Bn          the covariance (ddof 1) of the M × k matrix of the μ_m about their mean
  rhat        sqrt((N − 1)/N + diag(Bn)/diag(W))       convergence()'s split-R̂
  lambda_max  the largest λ of Bn v = λ W v             (host, k × k)
  rhat_mv     sqrt((N − 1)/N + lambda_max)

S and the split scatter are summed in blocks of block_chains consecutive whole
chains, each block from zero, and the blocks are added in block order; a host
input goes to the device in chunks of whole blocks, so no result depends on
the chunking, and two calls give the same bits.
"""
import numpy as np
import torch

from . import _abi
from . import device as dev
from ._lib import call
from .diagnostics import SUM_BLOCK, _check_layout, _is_cuda, _on_device, _ordered_col_sums, _pivot_mean, _seq_sum
from .posterior import DEFAULT_CHUNK_BYTES, _as3d, _geom, _host_cnk, _shape

PARTIAL_BYTES = 256 << 20  # the block partials [nb, k, k] stay below this with the default block


def default_block_chains(C, k):
    """Chains per block when block_chains is None: max(1, min(1024, C // 256)), doubled until the
    partial sums ceil(C / block) k² 8 bytes fit 256 MiB.  A function of (C, k) alone."""
    b = max(1, min(1024, C // 256))
    while -(-C // b) * k * k * 8 > PARTIAL_BYTES:
        b *= 2
    return b


def _block(block_chains, C, k):
    if block_chains is None:
        return default_block_chains(C, k)
    b = int(block_chains)
    if b < 1:
        raise ValueError("block_chains must be positive")
    return b


def _prepare(samples, layout, backend, chunk_bytes):
    _check_layout(layout)
    on_device = _on_device(backend)
    x = _as3d(samples)
    if _is_cuda(x) and not on_device:
        x = x.cpu().numpy()
    if chunk_bytes <= 0:
        raise ValueError("chunk_bytes must be positive")
    return x, on_device


def _block_chunks(x, chunk_bytes, block):
    """Slices of a host (C, ., .) array: whole blocks of `block` chains, at most chunk_bytes
    (at least one block), so that no block straddles two chunks."""
    C = x.shape[0]
    per_chain = max(1, x.shape[1] * x.shape[2] * x.dtype.itemsize)
    step = max(block, int(chunk_bytes) // per_chain // block * block)
    for c0 in range(0, C, step):
        yield x[c0:c0 + step]


def _device_chunks(x, device, chunk_bytes, block):
    """CUDA tensors of whole blocks of chains: the input itself (never copied), or a host input chunk by chunk."""
    if _is_cuda(x):
        yield x
        return
    d = dev.resolve_device(device)
    for part in _block_chunks(x, chunk_bytes, block):
        a = np.ascontiguousarray(part)
        if not a.flags.writeable:  # a read-only memory map
            a = a.copy()
        yield torch.from_numpy(a).to(d)


def _sym(S):
    """The lower triangle mirrored: [i, j] and [j, i] hold the same bits."""
    return np.tril(S) + np.tril(S, -1).T


# --------------------------------------------------------------- definition
def _host_split_means(x, layout, block):
    """μ_m (M, k): first halves of all chains, then second halves."""
    N = _shape(x, layout)[1] // 2
    first, second = [], []
    for c0 in range(0, x.shape[0], block):
        # one memory order, as diagnostics._host_samples (numpy adds a strided axis in sample order and a
        # contiguous one pairwise), and diagnostics' means about the first sample
        xb = np.ascontiguousarray(_host_cnk(x[c0:c0 + block], layout))
        first.append(_pivot_mean(xb[:, :N]))
        second.append(_pivot_mean(xb[:, N:2 * N]))
    return np.concatenate(first + second, axis=0)


def _host_scatter(x, layout, block, center=None, mu=None):
    """(S, D) about the shared `center` over all rows, or S about the split-chain means `mu`
    over the split chains' rows (D is None); dᵀd per block, the blocks added in block order."""
    C, n, k = _shape(x, layout)
    N = n // 2
    S, D = np.zeros((k, k)), np.zeros(k)
    for c0 in range(0, C, block):
        xb = _host_cnk(x[c0:c0 + block], layout)
        if mu is None:
            d = (xb - center).reshape(-1, k)
            D = D + d.sum(axis=0)
        else:
            c1 = c0 + xb.shape[0]
            d = np.concatenate([xb[:, :N] - mu[c0:c1, None, :], xb[:, N:2 * N] - mu[C + c0:C + c1, None, :]],
                               axis=1).reshape(-1, k)
        S = S + _sym(d.T @ d)
    return S, (D if mu is None else None)


def _host_rows_scatter(rows, center):
    """Σ (rows − center)(rows − center)ᵀ in blocks of SUM_BLOCK rows, the blocks in order."""
    k = rows.shape[1]
    S = np.zeros((k, k))
    for r0 in range(0, rows.shape[0], SUM_BLOCK):
        d = rows[r0:r0 + SUM_BLOCK] - center
        S = S + _sym(d.T @ d)
    return S


# ------------------------------------------------------------------- device
def _scatter_call(t_geom, center, mode, block, with_dsum, device):
    """ipmc_scatter on one geometry: block partials (nb, k, k) and (nb, k) or None, on the device."""
    C, k = t_geom[2], t_geom[4]
    nb = -(-C // block)
    f64 = dict(dtype=torch.float64, device=device)
    part = torch.empty((nb, k * k), **f64)
    dsum = torch.empty((nb, k), **f64) if with_dsum else None
    call("ipmc_scatter", *t_geom, center.data_ptr(), mode, int(block), part.data_ptr(), dev.ptr(dsum),
         dev.stream_handle(device))
    return part, dsum


def _device_split_means(x, layout, device, chunk_bytes, block):
    """μ_m (M, k) on the device (ipmc_split_stats per chunk) and the device it is on."""
    first, second = [], []
    for t in _device_chunks(x, device, chunk_bytes, block):
        geom = _geom(t, layout)
        c, k = geom[2], geom[4]
        f64 = dict(dtype=torch.float64, device=t.device)
        mean_m, var_m = torch.empty((2 * c, k), **f64), torch.empty((2 * c, k), **f64)
        call("ipmc_split_stats", *geom, mean_m.data_ptr(), var_m.data_ptr(), dev.stream_handle(t.device))
        first.append(mean_m[:c])
        second.append(mean_m[c:])
    return torch.cat(first + second, dim=0)


def _block_order_sum(parts):
    """Device block partials [(nb_i, w), ...] in block order -> (w,) on the host."""
    return _ordered_col_sums(torch.cat(parts, dim=0) if len(parts) > 1 else parts[0])[0]


def _to_device(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


# ---------------------------------------------------------------- covariance
def posterior_covariance(samples, layout="time_vars", backend="auto", device=None,
                         chunk_bytes=DEFAULT_CHUNK_BYTES, block_chains=None):
    """Mean, covariance (ddof 1) and correlation matrix of the pooled posterior: every sample of
    every chain, np.cov(x.reshape(-1, k), rowvar=False) and np.corrcoef by the corrected two-pass
    of the module's definition.

    samples: (C, n, k) -- MCMCSampler.run's keep="samples" output, a memory-mapped sample_file or a
    CUDA tensor (never copied: a burn-in slice or a transposed view goes to the kernel by its
    strides; f32 is widened on load) -- or (C, k, n) with layout="vars_time"; (n, k) is one chain.
    backend: "auto" (the device when there is one), "device" or "host" (numpy).
    chunk_bytes: a host input goes to the device in chunks of whole blocks of at most this size, twice
    (the split-chain means, then the scatter).
    block_chains: chains per partial sum, default default_block_chains(C, k).

    Returns {"mean": (k,), "cov": (k, k), "corr": (k, k), "n": C n}, float64 numpy.  cov is bitwise
    symmetric; corr has a diagonal of exactly 1 and nan in the row and column of a component
    of zero variance.  Needs at least two samples in all."""
    x, on_device = _prepare(samples, layout, backend, chunk_bytes)
    C, n, k = _shape(x, layout)
    R = C * n
    if R < 2:
        raise ValueError(f"posterior_covariance needs at least 2 samples, got {R}")
    if k < 1:
        raise ValueError("posterior_covariance needs at least one component")
    block = _block(block_chains, C, k)
    split = n >= 4
    if on_device:
        if split:
            mu = _device_split_means(x, layout, device, chunk_bytes, block)
            a = _ordered_col_sums(mu)[0] / mu.shape[0]
        else:
            first = x[0, 0, :] if layout == "time_vars" else x[0, :, 0]
            a = (first.double().cpu().numpy() if _is_cuda(x) else np.asarray(first, dtype=np.float64)).copy()
        parts, dsums = [], []
        for t in _device_chunks(x, device, chunk_bytes, block):
            p, d = _scatter_call(_geom(t, layout), _to_device(a, t.device), _abi.CENTER_SHARED, block, True, t.device)
            parts.append(p)
            dsums.append(d)
        S = _block_order_sum(parts).reshape(k, k)
        D = _block_order_sum(dsums)
    else:
        if split:
            a = _host_split_means(x, layout, block).mean(axis=0)
        else:
            a = _host_cnk(x[:1], layout)[0, 0].copy()
        S, D = _host_scatter(x, layout, block, center=a)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = a + D / R
        cov = (S - _sym(np.outer(D, D)) / R) / (R - 1)
        var = np.diag(cov)
        sd = np.sqrt(np.where(var > 0, var, np.nan))
        corr = np.clip(cov / np.outer(sd, sd), -1.0, 1.0)
    corr[np.diag_indices(k)] = np.where(np.isnan(sd), np.nan, 1.0)
    return {"mean": mean, "cov": cov, "corr": corr, "n": R}


# ------------------------------------------------------------------- R-hat
def _lambda_max(Bn, W):
    """The largest generalised eigenvalue of Bn v = λ W v; nan unless W is positive definite."""
    if not (np.all(np.isfinite(Bn)) and np.all(np.isfinite(W))):
        return np.nan
    try:
        from scipy.linalg import eigh
    except ImportError:  # the same through W's Cholesky factor: L⁻¹ Bn L⁻ᵀ
        try:
            L = np.linalg.cholesky(W)
        except np.linalg.LinAlgError:
            return np.nan
        A = np.linalg.solve(L, np.linalg.solve(L, Bn).T)
        return float(np.linalg.eigvalsh(0.5 * (A + A.T))[-1])
    k = W.shape[0]
    try:
        return float(eigh(Bn, W, eigvals_only=True, subset_by_index=[k - 1, k - 1])[0])
    except np.linalg.LinAlgError:
        return np.nan


def multivariate_rhat(samples, layout="time_vars", backend="auto", device=None, block_chains=None,
                      chunk_bytes=DEFAULT_CHUNK_BYTES):
    """Within- and between-chain covariance of the split chains and the multivariate R̂
    (the module's definition): {"W": (k, k), "Bn": (k, k), "rhat": (k,), "lambda_max", "rhat_mv"}.

    rhat is convergence()'s split-R̂ per component.  rhat_mv = sqrt((N − 1)/N + λ_max) is Brooks &
    Gelman's multivariate potential scale reduction factor without their (M + 1)/M factor, dropped
    so that it matches the per-component definition: rhat_mv >= max(rhat) (the per-component ratio
    is the generalised Rayleigh quotient of a unit vector), with equality for k = 1.  Chains that
    disagree only along a narrow direction of a correlated posterior show in rhat_mv and in no
    component of rhat.  A W that is not positive definite (a constant component, fewer than k + 1
    samples) gives nan for lambda_max and rhat_mv.  Inputs, backend, chunking and block_chains as
    posterior_covariance; needs n >= 4 samples per chain."""
    x, on_device = _prepare(samples, layout, backend, chunk_bytes)
    C, n, k = _shape(x, layout)
    if C < 1 or k < 1:
        raise ValueError("multivariate_rhat needs at least one chain and one component")
    if n < 4:
        raise ValueError(f"multivariate_rhat needs at least 4 samples per chain (a split chain needs 2), got {n}")
    N, M = n // 2, 2 * C
    block = _block(block_chains, C, k)
    if on_device:
        parts, first, second = [], [], []
        for t in _device_chunks(x, device, chunk_bytes, block):
            geom = _geom(t, layout)
            c = geom[2]
            f64 = dict(dtype=torch.float64, device=t.device)
            mean_m, var_m = torch.empty((2 * c, k), **f64), torch.empty((2 * c, k), **f64)
            call("ipmc_split_stats", *geom, mean_m.data_ptr(), var_m.data_ptr(), dev.stream_handle(t.device))
            parts.append(_scatter_call(geom, mean_m, _abi.CENTER_SPLIT, block, False, t.device)[0])
            first.append(mean_m[:c])
            second.append(mean_m[c:])
        mu = torch.cat(first + second, dim=0)
        S = _block_order_sum(parts).reshape(k, k)
        centre = _ordered_col_sums(mu)[0] / M
        # the M x k chain means as M chains of one sample each, about their mean
        p, _ = _scatter_call((mu.data_ptr(), _abi.F64, M, 1, k, k, k, 1), _to_device(centre, mu.device),
                             _abi.CENTER_SHARED, SUM_BLOCK, False, mu.device)
        SB = _block_order_sum([p]).reshape(k, k)
    else:
        mu = _host_split_means(x, layout, block)
        S, _ = _host_scatter(x, layout, block, mu=mu)
        SB = _host_rows_scatter(mu, mu.mean(axis=0))
    W = S / (M * (N - 1))
    Bn = SB / (M - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        w, b = np.diag(W), np.diag(Bn)
        rhat = np.where(w > 0, np.sqrt((N - 1) / N + b / w), np.nan)
        lam = _lambda_max(Bn, W)
        rhat_mv = float(np.sqrt((N - 1) / N + lam))
    return {"W": W, "Bn": Bn, "rhat": rhat, "lambda_max": lam, "rhat_mv": rhat_mv}

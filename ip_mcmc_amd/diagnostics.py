"""Chain diagnostics on the device.

  autocorr(x, max_lag)            batched MCMCSampler.autocorr (sampler.py:43-54)
  autocorrelation(samples, tau)   helpers.autocorrelation (report/scripts/helpers.py:41-54)
  chain_autocorr(samples, lag)    per chain and component, for run()'s (C, n_samples, k) output
  burn_in_lengths(chains)         batched len_burn_in (burgers/utilities.py:134-167), ipmc_burn_in kernel
  len_burn_in / uncorrelated_sample_spacing / clean_samples   utilities.py:134-195, reference signatures

The autocorrelations call libipmc's ``ipmc_autocorr`` kernel (one workgroup
per series, the series staged in LDS); results agree with the reference's
np.correlate formula to rounding (the summation order differs).  Burn-in
detection calls ``ipmc_burn_in``, which keeps np.cumsum's and np.mean's
summation orders, so its moving averages and decisions equal the
reference's bit for bit.

Across chains (nothing in the reference: it runs one chain):

  convergence(samples)            split-R̂, ESS, MCSE, τ per component over (C, n, k) samples
  split_rhat(samples)             the R̂ part alone (no autocovariance kernel)
  moments_convergence(moments)    non-split R̂ and the across-chain standard error from keep="moments" sums

The definition is the numpy code below (backend="host", float64); the device
path (ipmc_split_stats, ipmc_mean_acov, ipmc_moments_stats and the fixed-order
block sums) computes the same quantities where the samples are, and differs
from it only in summation order.
"""
import warnings

import numpy as np
import torch

from . import device as dev
from ._lib import call


def _series_tensor(x, device=None):
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x
    return torch.as_tensor(np.asarray(x, dtype=np.float64)).to(dev.resolve_device(device))


def autocorr(x, max_lag=None, device=None):
    """Normalised autocorrelation of every series along the last axis of x
    (numpy or device tensor, shape (..., n)); returns (..., max_lag) float64,
    numpy for numpy input.  max_lag defaults to n (the reference returns all n lags)."""
    numpy_in = not (isinstance(x, torch.Tensor) and x.is_cuda)
    t = _series_tensor(x, device)
    if t.dtype not in (torch.float32, torch.float64):
        t = t.double()
    shape = tuple(t.shape)
    n = shape[-1]
    lag = n if max_lag is None else int(max_lag)
    flat = t.reshape(-1, n).contiguous()
    out = torch.empty((flat.shape[0], lag), dtype=torch.float64, device=flat.device)
    call("ipmc_autocorr", flat.data_ptr(), dev.abi_dtype(flat.dtype), flat.shape[0], n, n, 1, lag, out.data_ptr(),
         dev.stream_handle(flat.device))
    out = out.reshape(shape[:-1] + (lag,))
    return out.cpu().numpy() if numpy_in else out


def autocorrelation(samples, tau_max, device=None):
    """helpers.autocorrelation (helpers.py:41-54): samples (n_vars, N) -> (n_vars, tau_max),
    the autocorrelation averaged over the N // tau_max consecutive windows of tau_max samples."""
    a = np.asarray(samples, dtype=np.float64)
    avg_over = int(len(a[0, :]) / tau_max)
    assert avg_over > 0, "Not enough samples to compute autocorrelationwith specified length"
    windows = a[:, : avg_over * tau_max].reshape(a.shape[0], avg_over, tau_max)
    ac_w = autocorr(windows, tau_max, device)  # (n_vars, avg_over, tau_max)
    ac = np.zeros((a.shape[0], tau_max))
    for i in range(avg_over):  # the reference's accumulation order
        ac += ac_w[:, i, :]
    return ac / avg_over


def chain_autocorr(samples, max_lag=None, device=None):
    """(C, n_samples, k) samples from MCMCSampler.run -> (C, k, max_lag) autocorrelations."""
    t = _series_tensor(samples, device)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    return autocorr(t.transpose(1, 2).contiguous(), max_lag, device) if isinstance(samples, torch.Tensor) else (
        autocorr(t.transpose(1, 2).contiguous(), max_lag, device).cpu().numpy())


# ------------------------------------------------------------------ burn-in
def burn_in_lengths(chains, avg_window=50, accepted_change=0.03, layout="vars_time", device=None):
    """len_burn_in (burgers/utilities.py:134-167) for a batch of chains on the device.

    chains: (C, n_vars, n) with layout='vars_time' (the reference's x, one per
    chain), or run()'s (C, n_samples, k) output with layout='time_vars'.
    Returns int64 (C,) (numpy for numpy input)."""
    numpy_in = not (isinstance(chains, torch.Tensor) and chains.is_cuda)
    t = _series_tensor(chains, device)
    if t.dtype not in (torch.float32, torch.float64):
        t = t.double()
    if t.dim() == 2:
        t = t.unsqueeze(0)
    t = t.contiguous()
    C, a, b = t.shape
    if layout == "vars_time":
        n_vars, n, s_var, s_t = a, b, b, 1
    elif layout == "time_vars":
        n, n_vars, s_var, s_t = a, b, 1, b
    else:
        raise ValueError("layout must be 'vars_time' or 'time_vars'")
    if n < avg_window:
        raise ValueError(f"len_burn_in needs at least avg_window={avg_window} samples, got {n}")
    words = (n + 31) // 32
    flags = torch.empty(max(1, C * words), dtype=torch.int32, device=t.device)
    out = torch.empty(C, dtype=torch.int64, device=t.device)
    call("ipmc_burn_in", t.data_ptr(), dev.abi_dtype(t.dtype), C, n_vars, n, a * b, s_var, s_t, int(avg_window),
         float(accepted_change), flags.data_ptr(), out.data_ptr(), dev.stream_handle(t.device))
    return out.cpu().numpy() if numpy_in else out


def len_burn_in(x, device=None):
    """Reference signature (utilities.py:134): x (n_vars, n) -> burn-in index (int)."""
    return int(burn_in_lengths(np.asarray(x, dtype=np.float64)[None], device=device)[0])


def uncorrelated_sample_spacing(x, device=None):
    """utilities.py:169-186: grow tau by 1.5x from 10 until the variable-averaged
    windowed autocorrelation first drops to <= 0.001; returns that lag.  Keeps
    the reference's early exit value len(x) (the number of variables)
    when the series is too short to decorrelate."""
    x = np.asarray(x, dtype=np.float64)
    tau = 10
    while True:
        if 2 > int(len(x[0, :]) / tau):
            return len(x)
        tau = int(tau * 1.5)
        ac = autocorrelation(x, tau, device)
        avg_ac = np.mean(ac, axis=0)
        idx = np.argwhere(avg_ac <= 0.001)
        if len(idx) > 0:
            return idx[0][0]


def clean_samples(x, device=None):
    """utilities.py:189-195: drop the burn-in, then keep every spacing-th sample."""
    x_ = np.copy(np.asarray(x, dtype=np.float64))
    x_ = x_[:, len_burn_in(x_, device):]
    return x_[:, :: uncorrelated_sample_spacing(x_, device)]


# ------------------------------------------------------- across chains
# Definition (Gelman et al. BDA3 §11.4-11.5 / Stan's split-R̂ and ESS, without
# rank normalisation).  x is (C, n, k); N = n // 2; chain c gives the split
# chains x[c, :N] and x[c, N:2N] (an odd last sample is dropped), ordered
# [first halves of all chains, then second halves], M = 2C of them.
#   μ_m, γ_m(t) = (1/N) Σ_{i<N-t} (x_i - μ_m)(x_{i+t} - μ_m), s²_m = γ_m(0) N/(N-1)
#   W = mean_m s²_m,  B/N = var_m(μ_m) (ddof 1),  var⁺ = (N-1)/N W + B/N
#   rhat = sqrt(var⁺ / W)
#   ρ_t = 1 - (W - mean_m γ_m(t) N/(N-1)) / var⁺,  t = 0 .. L = max_lag
#   P_j = ρ_2j + ρ_2j+1: stop at the first P_j < 0 (truncated) or when
#   2j + 1 > L (not truncated); before adding, P_j <- min(P_j, P_j-1)
#   tau = -1 + 2 Σ P_j,  ess = min(M N / tau, M N log10(M N)),  mcse = sqrt(var⁺ / ess)
# Every sum is centred (two passes): chain means of 8 with spreads of 0.01 are
# the normal case (θ = 8 + u), where Σx² - (Σx)²/n would lose the variance.
SUM_BLOCK = 1024  # chains per fixed-order block sum (device.block_sums), as for the posterior mean


def _is_cuda(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _on_device(backend):
    if backend == "auto":
        return torch.cuda.is_available()
    if backend in ("device", "host"):
        return backend == "device"
    raise ValueError("backend must be 'auto', 'device' or 'host'")


def _check_layout(layout):
    if layout not in ("time_vars", "vars_time"):
        raise ValueError("layout must be 'vars_time' or 'time_vars'")


def _check_lengths(n, max_lag):
    """-> (N, L) for chains of n samples."""
    if n < 4:
        raise ValueError(f"convergence needs at least 4 samples per chain (a split chain needs 2), got {n}")
    N = n // 2
    L = min(N - 1, 1000) if max_lag is None else int(max_lag)
    if L < 0 or L > N - 1:
        raise ValueError(f"max_lag={L} outside [0, N - 1 = {N - 1}] for split chains of {N} samples")
    return N, L


def _host_samples(samples, layout):
    """-> float64 (C, n, k) view or copy on the host."""
    a = samples.detach().cpu().numpy() if isinstance(samples, torch.Tensor) else np.asarray(samples)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError(f"samples must be (C, n, k) or (n, k), got shape {a.shape}")
    # one memory order, so numpy's sums (and the bits) do not depend on the layout given
    return np.ascontiguousarray(a.transpose(0, 2, 1) if layout == "vars_time" else a)


def _pivot_mean(S):
    """Means over axis 1 of (M, N, k), summed about each series' first sample: x_0 + Σ (x_t − x_0)/N.
    The differences are spread-sized, so the sum's rounding is far below an ulp of a mean that is
    many spreads large (θ = 8 + u; 10⁵ standard deviations in the tests), and any order of the adds
    rounds the same value: B/N, the variance of such means, multiplies a change of a mean by
    2 |mean| / spread.  ipmc_split_stats sums the same way."""
    x0 = S[:, :1]
    return x0[:, 0] + (S - x0).mean(axis=1)


def _host_parts(x, max_lag=None):
    """The sums of the definition on float64 (C, n, k): (mean (k,), W (k,),
    B/N (k,), mean_m γ_m(t) (max_lag + 1, k) or None when max_lag is None)."""
    C, n, k = x.shape
    N, M = n // 2, 2 * C
    S = np.concatenate([x[:, :N], x[:, N:2 * N]], axis=0)  # (M, N, k)
    mu = _pivot_mean(S)
    d = S - mu[:, None, :]
    s2 = (d * d).sum(axis=1) / (N - 1)
    mean = mu.mean(axis=0)
    W = s2.mean(axis=0)
    Bn = ((mu - mean) ** 2).sum(axis=0) / (M - 1)
    acov = None
    if max_lag is not None:
        acov = np.empty((max_lag + 1, k))
        for t in range(max_lag + 1):
            acov[t] = ((d[:, :N - t] * d[:, t:]).sum(axis=1) / N).mean(axis=0)
    return mean, W, Bn, acov


def _rho(W, Bn, acov, N):
    """ρ_t (L + 1, k) of the definition (nan where W == 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        varp = (N - 1) / N * W + Bn
        return 1.0 - (W - acov * (N / (N - 1))) / varp


def _geyer(rho, ok):
    """Geyer's initial monotone sequence over the pairs of ρ (L + 1, k), for
    the components with ok set: (Σ P_j, lag_used, truncated)."""
    L, k = rho.shape[0] - 1, rho.shape[1]
    total, prev = np.zeros(k), np.full(k, np.inf)
    lag_used, truncated = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=bool)
    active = ok.copy()
    j = 0
    while active.any():
        if 2 * j + 1 > L:
            lag_used[active] = 2 * j
            break
        P = rho[2 * j] + rho[2 * j + 1]
        stop = active & ~(P >= 0)
        truncated[stop] = True
        lag_used[stop] = 2 * j
        active &= ~stop
        P = np.minimum(P, prev)
        total[active] += P[active]
        prev[active] = P[active]
        j += 1
    return total, lag_used, truncated


def _finish(mean, W, Bn, acov, C, n, N, L):
    M = 2 * C
    ok = W > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        varp = (N - 1) / N * W + Bn
        rhat = np.where(ok, np.sqrt(varp / W), np.nan)
        out = {"mean": mean, "sd": np.sqrt(varp), "rhat": rhat}
        if acov is not None:
            total, lag_used, truncated = _geyer(_rho(W, Bn, acov, N), ok)
            tau = np.where(ok, -1.0 + 2.0 * total, np.nan)
            cap = M * N * np.log10(M * N)
            # tau <= 0 (a first pair below zero) has no finite-variance reading: report the cap
            ess = np.where(ok, np.where(tau > 0, np.minimum(M * N / np.where(tau > 0, tau, 1.0), cap), cap), np.nan)
            out.update(ess=ess, mcse=np.sqrt(varp / ess), tau=tau, lag_used=lag_used, truncated=truncated)
            # ranks._finish_quiet filters this warning by its text and restates this rule (ok & ~truncated)
            # to name the components of its parts in one warning: change the three together
            short = np.flatnonzero(ok & ~truncated)
            if len(short):
                warnings.warn(f"convergence: max_lag={L} ended the autocorrelation sum before a negative pair for "
                              f"component(s) {short.tolist()}: tau is a lower and ess an upper bound there "
                              "(raise max_lag or run longer chains)", stacklevel=4)
    out.update(n_chains=C, n_samples=n, n_split=N)
    return out


def _device_samples(samples, device):
    """-> contiguous f32/f64 3-D device tensor (CUDA tensors are not copied when contiguous)."""
    if _is_cuda(samples):
        t = samples
    else:
        a = samples.detach().numpy() if isinstance(samples, torch.Tensor) else np.asarray(samples)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        a = np.ascontiguousarray(a)
        if not a.flags.writeable:  # a read-only memory map
            a = a.copy()
        t = torch.from_numpy(a).to(dev.resolve_device(device))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.double()
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError(f"samples must be (C, n, k) or (n, k), got shape {tuple(t.shape)}")
    return t.contiguous()


def _seq_sum(block_sums):
    """(0 + S_0) + S_1 + ... over the rows of a small host array, in row order."""
    acc = np.zeros(block_sums.shape[1])
    for s in block_sums:
        acc = acc + s
    return acc


def _ordered_col_sums(*rows):
    """Column sums of device f64 [n, w] arrays over the chain axis in the fixed
    order of the posterior mean: blocks of SUM_BLOCK rows from zero in row order
    on the device (ipmc_block_sums), the block sums in block order on the host."""
    parts = [dev.block_sums(r, SUM_BLOCK) for r in rows]  # all queued before the first copy waits
    return [_seq_sum(p.cpu().numpy()) for p in parts]


def _centered_sq_sum(rows, center):
    """Σ_r (rows[r] - center)² per column in the same fixed order (ipmc_centered_sq_block_sums)."""
    n, k = rows.shape
    c = torch.from_numpy(np.ascontiguousarray(center, dtype=np.float64)).to(rows.device)
    out = torch.empty(((n + SUM_BLOCK - 1) // SUM_BLOCK, k), dtype=torch.float64, device=rows.device)
    call("ipmc_centered_sq_block_sums", rows.data_ptr(), n, k, rows.stride(0), c.data_ptr(), SUM_BLOCK,
         out.data_ptr(), dev.stream_handle(rows.device))
    return _seq_sum(out.cpu().numpy())


def _device_parts(t, layout, L, block_chains):
    """_host_parts on the device: t contiguous (C, n, k) or (C, k, n); L None skips the autocovariances."""
    C, a, b = t.shape
    n, k, s_t, s_var = (a, b, b, 1) if layout == "time_vars" else (b, a, 1, b)
    M, N = 2 * C, n // 2
    stream = dev.stream_handle(t.device)
    f64 = dict(dtype=torch.float64, device=t.device)
    mean_m, var_m = torch.empty((M, k), **f64), torch.empty((M, k), **f64)
    geom = (t.data_ptr(), dev.abi_dtype(t.dtype), C, n, k, a * b, s_t, s_var)
    call("ipmc_split_stats", *geom, mean_m.data_ptr(), var_m.data_ptr(), stream)
    partial = None
    if L is not None:  # queued behind the stats; nothing waits on the host in between
        if block_chains <= 0:
            raise ValueError("block_chains must be positive")
        nb = (M + block_chains - 1) // block_chains
        partial = torch.empty((nb, (L + 1) * k), **f64)
        call("ipmc_mean_acov", *geom, mean_m.data_ptr(), L, int(block_chains), partial.data_ptr(), stream)
    sum_mean, sum_var = _ordered_col_sums(mean_m, var_m)
    mean, W = sum_mean / M, sum_var / M
    Bn = _centered_sq_sum(mean_m, mean) / (M - 1)
    acov = None
    if partial is not None:
        acov = (_ordered_col_sums(partial)[0] / M).reshape(L + 1, k)
    return mean, W, Bn, acov


def _convergence(samples, max_lag, with_acov, layout, backend, device, block_chains):
    _check_layout(layout)
    if _on_device(backend):
        t = _device_samples(samples, device)
        C, n = t.shape[0], t.shape[1 if layout == "time_vars" else 2]
    else:
        x = _host_samples(samples, layout)
        C, n = x.shape[0], x.shape[1]
    if C < 1:
        raise ValueError("convergence needs at least one chain")
    N, L = _check_lengths(n, max_lag)
    if not with_acov:
        L = None
    parts = _device_parts(t, layout, L, block_chains) if _on_device(backend) else _host_parts(x, L)
    return _finish(*parts, C, n, N, L)


def convergence(samples, max_lag=None, layout="time_vars", backend="auto", device=None, block_chains=1024):
    """Split-R̂, effective sample size and Monte-Carlo standard error per
    component over all chains (the definition above).

    samples: (C, n, k) -- MCMCSampler.run's keep="samples" output, a memory-
    mapped sample_file, or a CUDA tensor (not copied when contiguous; f32 is
    widened on load) -- or (C, k, n) with layout="vars_time"; (n, k) is one chain.
    max_lag: L, default min(N - 1, 1000), at most N - 1 (N = n // 2).
    backend: "auto" (the device when there is one), "device" or "host" (numpy).
    block_chains: split chains per autocovariance partial sum on the device.
    Few long chains leave the GPU idle at the default (one workgroup per block,
    component and 256 lags); a smaller block adds workgroups and changes only
    the summation order.

    Returns a dict of float64 numpy (k,): mean, sd (sqrt var⁺), rhat, ess,
    mcse, tau; lag_used (int64), truncated (bool); and n_chains, n_samples,
    n_split.  A constant component (W == 0) has nan rhat, ess, mcse and tau.
    Components whose pair sum reaches max_lag before turning negative have
    truncated False and are named in one warning.  On the device every sum has
    a fixed order: two calls on the same input give the same bits."""
    return _convergence(samples, max_lag, True, layout, backend, device, block_chains)


def split_rhat(samples, layout="time_vars", backend="auto", device=None):
    """convergence()'s rhat alone, float64 (k,): the autocovariance kernel does not run."""
    return _convergence(samples, 0, False, layout, backend, device, 1024)["rhat"]


def moments_convergence(moments):
    """Non-split R̂ and the across-chain standard error of the posterior mean
    from the per-chain sums of run(keep="moments"): {"sum_u", "sum_u2", "n"},
    sums (C, k) as host arrays or device tensors (results="device":
    ipmc_moments_stats and the fixed-order block sums, nothing but (k,)
    results leaves the device).

      var_c = (sum_u2 - sum_u²/n)/(n-1),  W = mean_c var_c,  B/n = var_c(sum_u/n) (ddof 1)
      rhat = sqrt(((n-1)/n W + B/n)/W),   se = sd_c(sum_u/n)/sqrt(C)

    Returns {"mean", "se", "rhat"}, float64 numpy (k,).  The sums are all the
    sampler keeps, so var_c is the one-pass form: its relative error is about
    (mean/sd)² 2⁻⁵³ (θ = 8 + u with sd 0.01 loses six of sixteen digits; a mean
    10⁸ sd away loses all).  It does not see a drift every chain shares:
    that is what the split in convergence() is for."""
    su, su2, n = moments["sum_u"], moments["sum_u2"], int(moments["n"])
    if n < 2:
        raise ValueError(f"moments_convergence needs n >= 2 steps, got {n}")
    if tuple(su.shape) != tuple(su2.shape) or len(su.shape) != 2 or su.shape[0] < 2:
        raise ValueError("moments_convergence needs sum_u and sum_u2 of one shape (C, k) with C >= 2 chains")
    C, k = su.shape
    if _is_cuda(su):
        su, su2 = su.double().contiguous(), su2.double().contiguous()
        f64 = dict(dtype=torch.float64, device=su.device)
        mean_c, var_c = torch.empty((C, k), **f64), torch.empty((C, k), **f64)
        call("ipmc_moments_stats", su.data_ptr(), su2.data_ptr(), C, k, n, mean_c.data_ptr(), var_c.data_ptr(),
             dev.stream_handle(su.device))
        sum_mean, sum_var = _ordered_col_sums(mean_c, var_c)
        mean, W = sum_mean / C, sum_var / C
        Bn = _centered_sq_sum(mean_c, mean) / (C - 1)
    else:
        su, su2 = np.asarray(su, dtype=np.float64), np.asarray(su2, dtype=np.float64)
        mean_c = su / n
        var_c = (su2 - su ** 2 / n) / (n - 1)
        mean, W = mean_c.mean(axis=0), var_c.mean(axis=0)
        Bn = ((mean_c - mean) ** 2).sum(axis=0) / (C - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rhat = np.where(W > 0, np.sqrt(((n - 1) / n * W + Bn) / W), np.nan)
    return {"mean": mean, "se": np.sqrt(Bn) / np.sqrt(C), "rhat": rhat}

"""Tempered sequential Monte Carlo over the ensemble.

  TemperedSMC(prior, potential, beta).run(n_particles, ...)   prior -> posterior, with the evidence
  tempering_sums(phi, phi_ref, deltas)     Σ w and Σ w² of the weights exp(−δ(Φ − Φ_ref)) per candidate δ
  next_temperature(phi, t, target)         the adaptive step of the ladder (a 16-way search on the ESS)
  systematic_resample(phi, phi_ref, δ, U)  the ancestors of systematic resampling

The particles are the sampler's chains.  They start as draws from the prior;
the temperature t rises from 0 to 1 in steps δ chosen so that the importance
weights w_c = exp(−δ Φ(u_c)) keep the effective sample size
ESS = (Σ w)² / Σ w² at ess_frac·C; each stage resamples the particles by their
weights and then moves every one with K pCN steps that leave
π_t ∝ exp(−tΦ)·prior invariant: MCMCSampler on the caller's potential with its
noise covariance divided by t, whose Φ is tΦ.  The product of the stages' mean
weights estimates the evidence Z = E_prior[exp(−Φ)].

Reweighting, the search, resampling and the row gather of the states run on
the device (ipmc_temper_sums, ipmc_temper_cumweights,
ipmc_systematic_ancestors, ipmc_gather_rows; Φ_ref through ipmc_minmax), so a
composition the kernels can run stays in HBM from the prior to the posterior;
only a few doubles per stage reach the host (Φ_ref, the sums, U).  On a machine
without a GPU, and for a composition MCMCSampler runs through its host step (a
Python forward map, a non-diagonal noise), the same operations come from
libipmc_host.so, bit for bit (ipmc_host_temper_sums, ...).

A stage evaluates the forward map K + 2 times per particle: K in the sweeps,
once for Φ₁ = Φ at t = 1 of the stage's particles (the weights) and once for the
run's own Φ_t(u₀).  Deriving Φ₁ from the run's cached Φ_t would save one, and
change bits.
"""
import ctypes
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np
import torch

from . import _abi
from . import device as dev
from ._lib import UnsupportedOnDevice, call
from .accepter import ConstrainAccepter, CountedAccepter, StandardRWAccepter, _unwrap_accepter, pCNAccepter
from .diagnostics import _on_device
from .distribution import GaussianDistribution
from .potential import EvolutionPotential
from .proposer import ConstSteppCNProposer
from .rng import resolve_rng
from .sampler import MCMCSampler

SMC_BLOCK = _abi.SMC_BLOCK
MAX_DELTAS = _abi.SMC_MAX_DELTAS
SEARCH_ROUNDS = 10  # rounds of the search for the next temperature
SEARCH_POINTS = 15  # interior points lo + (hi − lo)·j/16 of one round: one ipmc_temper_sums call
MINMAX_GROUPS = 1024  # IPMC_MINMAX_GROUPS


# ------------------------------------------------------------------ backends
class _HostOps:
    """The resampling pieces from libipmc_host.so, on numpy arrays."""

    on_device = False

    def __init__(self):
        self.d2h_bytes = 0

    def phi_array(self, phi):
        if isinstance(phi, torch.Tensor):
            phi = phi.detach().cpu().numpy()
        a = np.asarray(phi)
        return np.ascontiguousarray(a if a.dtype == np.float32 else a.astype(np.float64, copy=False)).reshape(-1)

    def phi_min(self, phi):
        with np.errstate(invalid="ignore"):
            return float(np.fmin.reduce(phi.astype(np.float64))) if phi.size else float("nan")  # NaN is skipped

    def count_finite(self, phi):
        return int(np.isfinite(phi).sum())

    def sums(self, phi, phi_ref, deltas):
        from . import _hostlib

        return _hostlib.temper_sums(phi, phi_ref, deltas)

    def cumweights(self, phi, phi_ref, delta):
        from . import _hostlib

        return _hostlib.temper_cumweights(phi, phi_ref, delta)

    def ancestors(self, cum, u, n_out):
        from . import _hostlib

        return _hostlib.systematic_ancestors(cum, u, n_out)

    def gather(self, x, anc):
        return np.ascontiguousarray(x[anc])

    def uniform(self, seed, step):
        from . import _hostlib

        return float(_hostlib.uniforms(seed, 0, 1, step)[0])

    def host(self, x):
        return np.array(x, copy=True)


class _DeviceOps:
    """The same pieces from libipmc.so, on device tensors; only scalars reach the host."""

    on_device = True

    def __init__(self, device=None):
        self.device = dev.resolve_device(device)
        self.d2h_bytes = 0  # what these calls themselves copied to the host
        self._ws = None

    def _stream(self):
        return dev.stream_handle(self.device)

    def _workspace(self, n, n_deltas):
        need = ctypes.c_int64(0)
        call("ipmc_smc_workspace", n, n_deltas, ctypes.byref(need))
        if self._ws is None or self._ws.numel() < need.value:
            self._ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device=self.device)
        return self._ws, need.value

    def _to_host(self, t):
        self.d2h_bytes += t.numel() * t.element_size()
        return t.cpu().numpy()

    def phi_array(self, phi):
        if isinstance(phi, torch.Tensor):
            t = phi.to(self.device)
        else:
            a = np.asarray(phi)
            a = np.ascontiguousarray(a if a.dtype == np.float32 else a.astype(np.float64))
            t = torch.from_numpy(a if a.flags.writeable else a.copy()).to(self.device)
        if t.dtype not in (torch.float32, torch.float64):
            t = t.double()
        return t.contiguous().reshape(-1)

    def phi_min(self, phi):
        n = phi.shape[0]
        if n == 0:
            return float("nan")
        out = torch.empty((2, 1), dtype=torch.float64, device=self.device)
        scratch = torch.empty(2 * MINMAX_GROUPS, dtype=torch.float64, device=self.device)
        call("ipmc_minmax", phi.data_ptr(), dev.abi_dtype(phi.dtype), n, 1, 1, 1, 1, 1, out[0].data_ptr(),
             out[1].data_ptr(), scratch.data_ptr(), self._stream())
        return float(self._to_host(out)[0, 0])

    def count_finite(self, phi):
        return int(torch.isfinite(phi).sum().item())  # an error message's number: not on the product path

    def sums(self, phi, phi_ref, deltas):
        d = np.ascontiguousarray(np.atleast_1d(deltas), dtype=np.float64)
        nd, n = d.shape[0], phi.shape[0]
        out = torch.zeros((2, nd), dtype=torch.float64, device=self.device)
        ws, nbytes = self._workspace(n, nd)
        call("ipmc_temper_sums", phi.data_ptr(), dev.abi_dtype(phi.dtype), n, float(phi_ref), d.ctypes.data, nd,
             out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), nbytes, self._stream())
        o = self._to_host(out)
        return o[0].copy(), o[1].copy()

    def cumweights(self, phi, phi_ref, delta):
        n = phi.shape[0]
        cum = torch.empty(n, dtype=torch.float64, device=self.device)
        ws, nbytes = self._workspace(n, 1)
        call("ipmc_temper_cumweights", phi.data_ptr(), dev.abi_dtype(phi.dtype), n, float(phi_ref), float(delta),
             cum.data_ptr(), ws.data_ptr(), nbytes, self._stream())
        return cum

    def ancestors(self, cum, u, n_out):
        anc = torch.full((int(n_out),), -1, dtype=torch.int64, device=self.device)
        call("ipmc_systematic_ancestors", cum.data_ptr(), cum.shape[0], float(u), int(n_out), anc.data_ptr(),
             self._stream())
        return anc

    def gather(self, x, anc):
        x = x.contiguous()
        out = torch.empty((anc.shape[0], x.shape[1]), dtype=x.dtype, device=x.device)
        call("ipmc_gather_rows", x.data_ptr(), dev.abi_dtype(x.dtype), x.shape[0], x.shape[1], x.stride(0),
             anc.data_ptr(), anc.shape[0], out.data_ptr(), out.stride(0), self._stream())
        return out

    def uniform(self, seed, step):
        return float(self._to_host(dev.uniforms(seed, 0, 1, step, self.device))[0])

    def host(self, x):
        return x.cpu().numpy()  # records and the final copy: not counted in d2h_bytes


def _ops(backend, device, phi=None):
    if backend == "auto" and isinstance(phi, torch.Tensor) and phi.is_cuda:
        return _DeviceOps(phi.device)
    return _DeviceOps(device) if _on_device(backend) else _HostOps()


# -------------------------------------------------------------------- pieces
def _sums_chunked(ops, phi, phi_ref, deltas):
    d = np.ascontiguousarray(np.atleast_1d(deltas), dtype=np.float64)
    if d.ndim != 1:
        raise ValueError("deltas must be a scalar or one-dimensional")
    if not (np.isfinite(d) & (d >= 0)).all():
        raise ValueError("every delta must be a finite number >= 0")
    s1, s2 = np.zeros(d.shape[0]), np.zeros(d.shape[0])
    if phi.shape[0] == 0:
        return s1, s2
    for j0 in range(0, d.shape[0], MAX_DELTAS):
        s1[j0:j0 + MAX_DELTAS], s2[j0:j0 + MAX_DELTAS] = ops.sums(phi, phi_ref, d[j0:j0 + MAX_DELTAS])
    return s1, s2


def _reference(ops, phi, phi_ref, what):
    if phi_ref is not None:
        return float(phi_ref)
    ref = ops.phi_min(phi)
    if not np.isfinite(ref):
        raise ValueError(f"{what}: no potential is finite (none of the {phi.shape[0]} particles has a valid forward map)")
    return ref


def tempering_sums(phi, phi_ref, deltas, backend="auto", device=None):
    """(s1, s2), float64 numpy (len(deltas),): s1[j] = Σ_c w_c(δ_j) and s2[j] = Σ_c w_c(δ_j)² of the weights
    w_c(δ) = exp(−δ(Φ_c − Φ_ref)) (0 where Φ_c is not finite), each summed inside blocks of 1 024 particles
    in particle order and then over the blocks in block order: the same bits on either backend.  phi: (n,)
    float32 or float64, numpy or a device tensor; phi_ref: the smallest finite Φ (None: it is looked up)."""
    ops = _ops(backend, device, phi)
    p = ops.phi_array(phi)
    return _sums_chunked(ops, p, _reference(ops, p, phi_ref, "tempering_sums"), deltas)


@dataclass
class TemperStep:
    """next_temperature's result: the increment, the temperature it leads to, ESS(δ) with its sums s1 and
    s2, the upper end of the last bracket (ESS there is below the target; None on the final step), whether
    the step reaches t = 1, and Φ_ref."""
    delta: float
    t_next: float
    ess: float
    s1: float
    s2: float
    upper: Optional[float]
    final: bool
    phi_ref: float


def _ess(s1, s2):
    with np.errstate(invalid="ignore", divide="ignore"):
        return s1 * s1 / s2


def _next_temperature(ops, phi, t, target, phi_ref, stage=None):
    t = float(t)
    if not 0.0 <= t < 1.0:
        raise ValueError("t must be in [0, 1)")
    full = 1.0 - t
    s1, s2 = ops.sums(phi, phi_ref, np.array([full]))
    if _ess(s1[0], s2[0]) >= target:
        return TemperStep(full, 1.0, float(_ess(s1[0], s2[0])), float(s1[0]), float(s2[0]), None, True, phi_ref)
    lo, hi = 0.0, full
    best = None  # (s1, s2) at lo
    for _ in range(SEARCH_ROUNDS):
        pts = lo + (hi - lo) * (np.arange(1, SEARCH_POINTS + 1) / (SEARCH_POINTS + 1.0))
        s1, s2 = ops.sums(phi, phi_ref, pts)
        ok = np.flatnonzero(_ess(s1, s2) >= target)
        if ok.size:
            j = int(ok[-1])
            best = (float(s1[j]), float(s2[j]))
            lo, hi = float(pts[j]), (float(pts[j + 1]) if j + 1 < SEARCH_POINTS else hi)
        else:
            hi = float(pts[0])
    if lo == 0.0 or t + lo == t:
        where = "" if stage is None else f" at stage {stage}"
        raise RuntimeError(
            f"tempered SMC{where}: no temperature increment keeps ESS >= {target:g}: {ops.count_finite(phi)} of the "
            f"{phi.shape[0]} particles have a finite potential (too few valid particles cannot reach the target; "
            "lower ess_frac or use more particles)")
    return TemperStep(lo, min(t + lo, 1.0), float(_ess(best[0], best[1])), best[0], best[1], hi, False, phi_ref)


def next_temperature(phi, t, target, phi_ref=None, backend="auto", device=None):
    """The step of the adaptive ladder from temperature t (a TemperStep): δ = 1 − t where ESS(1 − t) >= target;
    else ten rounds of a 16-way search on [0, 1 − t], each evaluating the 15 points lo + (hi − lo)·j/16 in one
    pass over phi: the new bracket starts at the largest point whose ESS is still >= target (at lo if none is)
    and ends at the next point; δ = the last lo.  Raises if that is 0."""
    ops = _ops(backend, device, phi)
    p = ops.phi_array(phi)
    return _next_temperature(ops, p, t, float(target), _reference(ops, p, phi_ref, "next_temperature"))


def systematic_resample(phi, phi_ref, delta, u, n_out=None, backend="auto", device=None):
    """Ancestors (int64 (n_out,), non-decreasing; numpy on the host backend, a device tensor on the device
    backend) of systematic resampling by the weights w_c(δ): offspring i descends from the smallest c whose
    cumulative weight exceeds (i + u)·total/n_out, 0 <= u < 1.  A particle of weight 0 is never an ancestor."""
    ops = _ops(backend, device, phi)
    p = ops.phi_array(phi)
    ref = _reference(ops, p, phi_ref, "systematic_resample")
    if not 0.0 <= float(u) < 1.0:
        raise ValueError("u must be in [0, 1)")
    if not (np.isfinite(delta) and delta >= 0):
        raise ValueError("delta must be a finite number >= 0")
    cum = ops.cumweights(p, ref, float(delta))
    return ops.ancestors(cum, float(u), p.shape[0] if n_out is None else int(n_out))


# -------------------------------------------------------------------- driver
@dataclass
class SMCResult:
    """particles (C, k) with equal weights and phi (C,) = Φ at t = 1 of them (device tensors with
    results="device" on the device tier, else numpy); temperatures (S + 1,), ess (S,) = ESS(δ) of each
    stage's weights, log_evidence = Σ log_evidence_increments (S,), accept_rate (S,) of the stages' pCN
    steps, n_stages = S; last_path: "device" or "host", the tier the mutation ran on; driver_d2h_bytes:
    what the driver's own device calls copied to the host (scalars); record: per stage, with record=True,
    a dict of phi, particles (before resampling), u, delta, ancestors and resampled (the particles after the
    gather) as numpy."""
    particles: Any
    phi: Any
    temperatures: np.ndarray
    ess: np.ndarray
    log_evidence: float
    log_evidence_increments: np.ndarray
    accept_rate: np.ndarray
    n_stages: int
    last_path: str
    driver_d2h_bytes: int = 0
    record: Optional[list] = None


def _unwrap_potential(potential):
    acc = potential
    while True:
        layers, acc = _unwrap_accepter(acc)
        if any(isinstance(lay, ConstrainAccepter) for lay in layers):
            raise NotImplementedError("TemperedSMC: ConstrainAccepter is not supported (a truncated prior needs "
                                      "rejection at the prior draw)")
        if isinstance(acc, StandardRWAccepter):
            raise NotImplementedError("TemperedSMC: random-walk accepters are not supported (the mutation is pCN)")
        if not isinstance(acc, pCNAccepter):
            break
        acc = acc.theta
    if not isinstance(acc, EvolutionPotential):
        raise TypeError(f"TemperedSMC: potential must be an EvolutionPotential, not {type(acc).__name__}")
    if not isinstance(acc.rho, GaussianDistribution):
        raise TypeError("TemperedSMC: the potential's noise must be a GaussianDistribution (the stage at temperature "
                        "t divides its covariance by t)")
    return acc


def _unwrap_prior(prior):
    kind = getattr(prior, "kind", None)
    if kind == "rw":
        raise NotImplementedError("TemperedSMC: random-walk proposers are not supported (pCN leaves the tempered "
                                  "posterior invariant on function-space priors)")
    if kind == "pcn":
        prior = prior.w
    if not isinstance(prior, GaussianDistribution):
        raise TypeError(f"TemperedSMC: prior must be a GaussianDistribution, not {type(prior).__name__}")
    return prior


class TemperedSMC:
    """Tempered SMC with pCN mutations: prior is the pCN proposer's GaussianDistribution (its covariance is
    used; the particles are perturbations around its mean, as the chains are), potential an
    EvolutionPotential with Gaussian noise, beta the pCN step, a float or a callable
    (stage, t, previous_accept_rate) -> float (previous_accept_rate is None at stage 0)."""

    def __init__(self, prior, potential, beta=0.25, rng=0, dtype=np.float64, device=None, chain_offset=0,
                 process_group=None):
        if chain_offset != 0 or process_group is not None:
            raise NotImplementedError("TemperedSMC: chain_offset != 0 or a process group is not supported "
                                      "(resampling across ranks needs an all-to-all)")
        self.prior = _unwrap_prior(prior)
        self.potential = _unwrap_potential(potential)
        if not callable(beta) and not 0 <= float(beta) <= 1:
            raise ValueError("beta has to be in [0, 1]")
        self.beta = beta
        self.rng = rng
        self.dtype = dtype
        self.device = device

    def _tier(self):
        """"device" where MCMCSampler runs the fused kernels for this composition, else "host"."""
        try:
            self.potential.device_terms()
        except UnsupportedOnDevice:
            return "host"
        return "device"

    def _tempered(self, t):
        rho = self.potential.rho
        return EvolutionPotential(self.potential.G, self.potential.y,
                                  GaussianDistribution(rho.mean, rho.covariance / t))

    def _prior_draw(self, n, tier, rng):
        from . import hostloop

        block = (rng.seed, 0, n, rng.step, 1, self.prior.k)  # one step of n chains at the stream's position
        if tier == "host":
            T = np.float64 if dev.torch_dtype(self.dtype) == dev.F64 else np.float32
            w, _ = hostloop.DRAWS["w"](*block, T, *self.prior.sqrt_factors(), self.device)
            return w[0].astype(np.float64)
        w, _ = hostloop._draws_on_device(*block, self.dtype, *self.prior.sqrt_factors(), self.device, log_r=False,
                                         shared_prior=True)
        return w[0]

    def _phi1(self, u, tier):
        if tier == "device":
            return self.potential.phi_device(u)
        return np.asarray(self.potential(u), dtype=np.float64).reshape(-1) - self.potential.rho.log_normaliser()

    def run(self, n_particles=65536, steps_per_stage=10, ess_frac=0.5, max_stages=1000, results="device",
            record=False, backend="auto", resampling="systematic"):
        """Run the ladder from the prior (t = 0) to the posterior (t = 1) and return an SMCResult.

        The definition: the particles are one ipmc_pcn_draws block at the stream's current step
        (the stream advances by one); per stage Φ₁ = Φ of the particles, Φ_ref its smallest finite value,
        δ = next_temperature(Φ₁, t, ess_frac·C), the evidence increment log(s1(δ)/C) − δ·Φ_ref, systematic
        resampling with U = the accept uniform of chain 0 at the stream's current step (the stream advances
        by one), the gather of the states, then MCMCSampler(ConstSteppCNProposer(β, prior),
        CountedAccepter(pCNAccepter(potential at t))).run(u, 1, 0, K, keep="last"), which advances the stream
        itself.  Two forward-map evaluations per particle and stage come on top of the K of the sweeps (Φ₁
        and the run's Φ_t(u₀)).

        backend: where the reweighting, search and resampling run: "auto" follows the tier (the device for a
        composition the kernels run, libipmc_host.so for the host step), "device" / "host" force one; the
        results are the same bits.  results: "device" leaves particles and phi in HBM on the device tier,
        "host" copies them at the end.  record=True keeps every stage's Φ₁, particles, U, δ and ancestors on
        the host (tests and small runs)."""
        if resampling != "systematic":
            raise NotImplementedError(f"TemperedSMC: resampling={resampling!r} is not supported (systematic only)")
        if results not in ("host", "device"):
            raise ValueError("results must be 'host' or 'device'")
        C, K = int(n_particles), int(steps_per_stage)
        if C < 1 or K < 0:
            raise ValueError("n_particles must be positive and steps_per_stage >= 0")
        if not 0.0 < ess_frac <= 1.0:
            raise ValueError("ess_frac must be in (0, 1]")
        tier = self._tier()
        if backend == "auto":
            ops = _DeviceOps(self.device) if tier == "device" else _HostOps()
        else:
            ops = _DeviceOps(self.device) if _on_device(backend) else _HostOps()
        self.rng = rng = resolve_rng(self.rng)
        target = float(ess_frac) * C

        u = self._prior_draw(C, tier, rng)
        rng.advance(1)
        t, stage, prev_rate = 0.0, 0, None
        temps, ess, incs, rates, rec = [0.0], [], [], [], ([] if record else None)
        phi = self._phi1(u, tier)
        while t < 1.0:
            if stage >= max_stages:
                raise RuntimeError(f"tempered SMC: t = {t} after max_stages = {max_stages} stages")
            p = ops.phi_array(phi)
            ref = _reference(ops, p, None, f"tempered SMC at stage {stage}")
            step = _next_temperature(ops, p, t, target, ref, stage)
            incs.append(float(np.log(step.s1 / C) - step.delta * ref))
            ess.append(step.ess)
            U = ops.uniform(rng.seed, rng.step)
            rng.advance(1)
            anc = ops.ancestors(ops.cumweights(p, ref, step.delta), U, C)
            if record:
                rec.append({"phi": ops.host(p), "particles": _to_numpy(u), "u": U, "delta": step.delta,
                            "ancestors": ops.host(anc)})
            u = _gather(u, anc, ops)
            if record:
                rec[-1]["resampled"] = _to_numpy(u)
            t = step.t_next
            beta = float(self.beta(stage, t, prev_rate)) if callable(self.beta) else float(self.beta)
            counted = CountedAccepter(pCNAccepter(self._tempered(t)))
            sampler = MCMCSampler(ConstSteppCNProposer(beta, self.prior), counted, rng, dtype=self.dtype,
                                  device=self.device)
            out = sampler.run(u, n_samples=1, burn_in=0, sample_interval=K, keep="last", results="device")
            if sampler.last_path != tier and not (tier == "host" and sampler.last_path.startswith("host")):
                raise RuntimeError(f"tempered SMC: the mutation ran on {sampler.last_path!r}, expected {tier!r}")
            u = out.to(dev.torch_dtype(self.dtype)) if tier == "device" else np.asarray(out, dtype=np.float64)
            calls = float(np.sum(counted.calls))
            prev_rate = float(np.sum(counted.accepts)) / calls if calls > 0 else float("nan")
            rates.append(prev_rate)
            temps.append(t)
            stage += 1
            phi = self._phi1(u, tier)
        if results == "host" and tier == "device":
            u, phi = u.double().cpu().numpy(), phi.double().cpu().numpy()
        incs = np.array(incs, dtype=np.float64)
        return SMCResult(u, phi, np.array(temps), np.array(ess), float(np.sum(incs)), incs, np.array(rates), stage,
                         tier, int(ops.d2h_bytes), rec)


def _to_numpy(x):
    return x.detach().cpu().numpy().copy() if isinstance(x, torch.Tensor) else np.array(x, copy=True)


def _gather(u, anc, ops):
    """The rows u[anc], where the particles are: ipmc_gather_rows for device particles, numpy for host ones
    (the ancestors are moved if the pieces ran on the other side)."""
    if isinstance(u, torch.Tensor):
        if not isinstance(anc, torch.Tensor):
            anc = torch.from_numpy(np.ascontiguousarray(anc)).to(u.device)
        return (ops if ops.on_device else _DeviceOps(u.device)).gather(u, anc)
    if isinstance(anc, torch.Tensor):
        anc = anc.cpu().numpy()
    return np.ascontiguousarray(u[anc])

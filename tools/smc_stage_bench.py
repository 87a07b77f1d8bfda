"""One SMC stage at the headline ensemble (65 536 x 40, f64) on one GPU: the reweighting, the search for
the next temperature, the cumulative weights, the ancestors and the gather on the device (HIP-event times
after warm-up calls, median / min / max; the calls that return sums end in their small synchronising
copy), beside Phi_1 of the ensemble, a sweep of 1 and of 10 pCN steps (Lorenz-96, 200 RK4 steps), and the
wall time of the same stage resampled on the host through a D2H and H2D of the states, which is what the
device path avoids (both give the same particles, asserted).

  python tools/smc_stage_bench.py [out.jsonl]      (default profiles/r13/smc_stage.jsonl)

Writes one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ip_mcmc_amd import (ConstSteppCNProposer, CountedAccepter, EvolutionPotential, GaussianDistribution,  # noqa: E402
                         Lorenz96Operator, MCMCSampler, _hostlib, pCNAccepter)
from ip_mcmc_amd import smc  # noqa: E402

C, K = 65536, 40
dev = torch.device("cuda", 0)
op = Lorenz96Operator(K, 8.0, dt=0.005, n_steps=200)
y = op(0.3 * np.random.default_rng(0).standard_normal(K))
pot = EvolutionPotential(op, y, GaussianDistribution(np.zeros(K), 0.1**2 * np.eye(K)))
prior = GaussianDistribution(np.zeros(K), np.eye(K))
u = torch.from_numpy(np.random.default_rng(1).standard_normal((C, K))).to(dev)
phi = pot.phi_device(u)
ops = smc._DeviceOps(dev)
target = 0.5 * C


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        out.append(a.elapsed_time(b))
    out.sort()
    return {"median_ms": out[len(out) // 2], "min_ms": out[0], "max_ms": out[-1]}


ref = ops.phi_min(phi)
step = smc._next_temperature(ops, phi, 0.0, target, ref, 0)
cum = ops.cumweights(phi, ref, step.delta)
anc = ops.ancestors(cum, 0.37, C)
pts = np.linspace(0, 1, 17)[1:16]
res = {"shape": [C, K], "dtype": "f64", "delta": step.delta, "ess": step.ess,
       "distinct_ancestors": int(torch.unique(anc).numel())}
res["phi_min"] = timed(lambda: ops.phi_min(phi))
res["temper_sums_15"] = timed(lambda: ops.sums(phi, ref, pts))
res["search_11_calls"] = timed(lambda: smc._next_temperature(ops, phi, 0.0, target, ref, 0), reps=10)
res["cumweights"] = timed(lambda: ops.cumweights(phi, ref, step.delta))
res["ancestors"] = timed(lambda: ops.ancestors(cum, 0.37, C))
res["gather"] = timed(lambda: ops.gather(u, anc))
res["gather_GBps"] = 2 * C * K * 8 / res["gather"]["median_ms"] / 1e6
perm = torch.randperm(C, device=dev)
res["gather_random_permutation"] = timed(lambda: ops.gather(u, perm))
res["phi1_potential"] = timed(lambda: pot.phi_device(u), reps=5)


def device_stage():
    r = ops.phi_min(phi)
    s = smc._next_temperature(ops, phi, 0.0, target, r, 0)
    a = ops.ancestors(ops.cumweights(phi, r, s.delta), 0.37, C)
    return ops.gather(u, a)


def host_stage():
    """The same stage with the resampling on the host: Φ and the states cross PCIe, numpy gathers."""
    p = phi.cpu().numpy()
    x = u.cpu().numpy()
    hops = smc._HostOps()
    r = hops.phi_min(p)
    s = smc._next_temperature(hops, p, 0.0, target, r, 0)
    a = hops.ancestors(hops.cumweights(p, r, s.delta), 0.37, C)
    return torch.from_numpy(np.ascontiguousarray(x[a])).to(dev)


def wall(fn, reps=5):
    fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return {"median_ms": out[len(out) // 2], "min_ms": out[0], "max_ms": out[-1]}


assert torch.equal(device_stage(), host_stage())
res["stage_resampling_device_wall"] = wall(device_stage)
res["stage_resampling_host_wall"] = wall(host_stage)

acc = CountedAccepter(pCNAccepter(pot))
sampler = MCMCSampler(ConstSteppCNProposer(0.1, prior), acc, 3)


def sweep(n):
    return sampler.run(u, n_samples=1, burn_in=0, sample_interval=n, keep="last", results="device")


sweep(1)
for n in (1, 10):
    ts = []
    for _ in range(5):
        sweep(n)
        ts.append(sampler.last_run_timing["sweeps_gpu_ms"])
    ts.sort()
    res[f"sweep_{n}_steps_gpu_ms"] = ts[len(ts) // 2]
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "r13", "smc_stage.jsonl")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(json.dumps(res) + "\n")
print(json.dumps(res, indent=1))

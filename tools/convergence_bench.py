"""Time of the cross-chain convergence diagnostics on the device, beside the host path (one GPU).

  python tools/convergence_bench.py [--out profiles/r7/convergence_diag.jsonl] [case ...]

split_rhat   split_rhat on (65 536, 20, 40) f64: the README's "65 536 x 20 samples" case
convergence  convergence on (1 024, 5 000, 3) f64 with max_lag=500: the Burgers study's shape,
             at the default block_chains=1024 and at block_chains=64
moments      moments_convergence on (65 536, 40) device sums (keep="moments", results="device")

Each case runs in a child process of its own under `timeout` (the parent never
opens the GPU and stops at the first case that fails) and appends one JSON line
to --out.  Device times are HIP-event times after warm-up calls, median / min /
max over the repetitions; an API call ends in the synchronising copy of its
(k,) results, so its event time is the whole call.  Beside each: the host
path (numpy, backend="host") on the same input, once; and for the stats kernel
(ipmc_split_stats alone) the time of one read of its input at the 6.29 TB/s a
streaming copy reaches on the MI355X.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STREAM_TBPS = 6.29  # measured float4 copy rate of the MI355X's HBM (8.0 TB/s by specification)
CASES = ("split_rhat", "convergence", "moments")
CASE_TIMEOUT_S = {"split_rhat": 300, "convergence": 420, "moments": 120}


def ensemble(C, n, k, phi, seed):
    """θ = 8 + u: AR(1) chains of spread ~0.01 around 8, (C, n, k) float64."""
    rng = np.random.default_rng(seed)
    x = np.empty((C, n, k))
    x[:, 0] = rng.normal(size=(C, k)) / np.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        x[:, t] = phi * x[:, t - 1] + rng.normal(size=(C, k))
    return 8.0 + 0.01 * x


def host_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn, warmup, reps):
    """HIP-event times of fn() after `warmup` untimed calls: median, min, max over `reps`."""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median": float(np.median(times)), "min": min(times), "max": max(times), "reps": reps}


def stats_kernel(t):
    """ipmc_split_stats alone on the contiguous (C, n, k) device tensor t."""
    import torch

    from ip_mcmc_amd import device as dev
    from ip_mcmc_amd._lib import call

    C, n, k = t.shape
    mean = torch.empty((2 * C, k), dtype=torch.float64, device=t.device)
    var = torch.empty_like(mean)
    stream = dev.stream_handle(t.device)
    return lambda: call("ipmc_split_stats", t.data_ptr(), dev.abi_dtype(t.dtype), C, n, k, n * k, k, 1,
                        mean.data_ptr(), var.data_ptr(), stream)


def acov_kernel(t, max_lag, block_chains):
    """ipmc_mean_acov alone (the means from one ipmc_split_stats call)."""
    import torch

    from ip_mcmc_amd import device as dev
    from ip_mcmc_amd._lib import call

    C, n, k = t.shape
    mean = torch.empty((2 * C, k), dtype=torch.float64, device=t.device)
    var = torch.empty_like(mean)
    stream = dev.stream_handle(t.device)
    geom = (t.data_ptr(), dev.abi_dtype(t.dtype), C, n, k, n * k, k, 1)
    call("ipmc_split_stats", *geom, mean.data_ptr(), var.data_ptr(), stream)
    nb = (2 * C + block_chains - 1) // block_chains
    partial = torch.empty((nb, max_lag + 1, k), dtype=torch.float64, device=t.device)
    return lambda: call("ipmc_mean_acov", *geom, mean.data_ptr(), max_lag, block_chains, partial.data_ptr(), stream)


def one_read(t):
    nbytes = t.numel() * t.element_size()
    return {"input_bytes": nbytes, "stream_TBps": STREAM_TBPS, "one_read_ms": nbytes / (STREAM_TBPS * 1e12) * 1e3}


def run_case(name):
    import warnings

    import torch

    from ip_mcmc_amd import convergence, moments_convergence, split_rhat
    from ip_mcmc_amd import device as dev

    dev.require_gpu()  # a measurement without the GPU fails; it does not fall back
    warnings.simplefilter("ignore")
    rec = {"case": name, "gpu": torch.cuda.get_device_name(0), "dtype": "float64"}
    if name == "split_rhat":
        x = ensemble(65536, 20, 40, 0.5, 1)
        t = torch.from_numpy(x).to("cuda")
        rec["shape"] = list(x.shape)
        rec["device_ms"] = event_ms(lambda: split_rhat(t, backend="device"), 3, 20)
        rec["stats_kernel_ms"] = event_ms(stats_kernel(t), 3, 20)
        rec.update(one_read(t))
        rec["stats_kernel_over_one_read"] = rec["stats_kernel_ms"]["median"] / rec["one_read_ms"]
        rec["host_ms"] = host_ms(lambda: split_rhat(x, backend="host"))
        # the whole of convergence() on the same ensemble (N = 10: the in-place autocovariance kernel)
        rec["convergence_device_ms"] = event_ms(lambda: convergence(t, backend="device"), 2, 5)
        rec["convergence_host_ms"] = host_ms(lambda: convergence(x, backend="host"))
        got, ref = split_rhat(t, backend="device"), split_rhat(x, backend="host")
        rec["max_rel_diff_vs_host"] = float(np.max(np.abs(got - ref) / ref))
    elif name == "convergence":
        x = ensemble(1024, 5000, 3, 0.9, 2)
        t = torch.from_numpy(x).to("cuda")
        rec["shape"], rec["max_lag"] = list(x.shape), 500
        for bc in (1024, 64):
            rec[f"device_ms_block{bc}"] = event_ms(
                lambda: convergence(t, max_lag=500, backend="device", block_chains=bc), 2, 5)
            rec[f"acov_kernel_ms_block{bc}"] = event_ms(acov_kernel(t, 500, bc), 1, 5)
        rec["stats_kernel_ms"] = event_ms(stats_kernel(t), 3, 20)
        rec.update(one_read(t))
        rec["stats_kernel_over_one_read"] = rec["stats_kernel_ms"]["median"] / rec["one_read_ms"]
        ref = {}
        rec["host_ms"] = host_ms(lambda: ref.update(convergence(x, max_lag=500, backend="host")))
        got = convergence(t, max_lag=500, backend="device")
        rec["max_rel_diff_vs_host"] = {key: float(np.max(np.abs(got[key] - ref[key]) / np.abs(ref[key])))
                                       for key in ("rhat", "ess", "mcse")}
        rec["rhat_max"], rec["ess_min"] = float(got["rhat"].max()), float(got["ess"].min())
    elif name == "moments":
        x = ensemble(65536, 50, 40, 0.5, 3)
        m = {"sum_u": x.sum(axis=1), "sum_u2": (x * x).sum(axis=1), "n": 50}
        d = {"sum_u": torch.from_numpy(m["sum_u"]).to("cuda"), "sum_u2": torch.from_numpy(m["sum_u2"]).to("cuda"),
             "n": 50}
        rec["shape"] = list(m["sum_u"].shape)
        rec["device_ms"] = event_ms(lambda: moments_convergence(d), 3, 20)
        rec["host_ms"] = host_ms(lambda: moments_convergence(m))
        got, ref = moments_convergence(d), moments_convergence(m)
        rec["max_rel_diff_vs_host"] = {key: float(np.max(np.abs(got[key] - ref[key]) / np.abs(ref[key])))
                                       for key in ("mean", "se", "rhat")}
    else:
        raise SystemExit(f"unknown case {name!r} (one of {', '.join(CASES)})")
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r7", "convergence_diag.jsonl"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        line = json.dumps(run_case(args.child))
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        return 0
    for name in args.cases:
        if name not in CASES:
            raise SystemExit(f"unknown case {name!r} (one of {', '.join(CASES)})")
    for name in args.cases:  # every GPU step under its own time limit; nothing runs after a failure
        rc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT_S[name]), sys.executable,
                             os.path.abspath(__file__), "--child", name, "--out", args.out]).returncode
        if rc != 0:
            print(f"convergence_bench: case {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

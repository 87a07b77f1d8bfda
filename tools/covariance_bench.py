"""Time of the pooled posterior covariance and the multivariate R-hat on the device (one GPU),
beside a clone of the same input, torch.cov on the same tensor and the numpy host path.

  python tools/covariance_bench.py [--out profiles/r9/posterior_cov.jsonl] [case ...]

cases:
  ensemble  (65 536, 20, 40) f64: config 3's sample array (419 MB); 5 FLOP per byte, borderline
  burgers   (1 024, 5 000, 3) f64: the Burgers studies' sample array (123 MB); bandwidth
  config5   (16 384, 4, 256) f64: a config-5 ensemble (134 MB); 32 FLOP per byte, compute -- but a block
            of 64 chains has only 256 rows, and the block partials are as large as the input
  config5_long  (256, 1 024, 256) f64 (537 MB): the same k with 1 024 rows per block

Each case runs in a child process of its own under `timeout` (the parent never opens the
GPU and stops at the first case that fails) and appends one JSON line to --out.  Device
times are HIP-event times after warm-up calls, median / min / max over the repetitions:
ipmc_scatter alone with its buffers prepared (about a shared centre with the row sums, and
about the split-chain means), and the two API calls on the device tensor (they end in the
synchronising copy of their small results).  Yardsticks, in the same process:
tensor.clone() of the same input, which reads the data once and also writes it (the kernel
reads it once; clone_ms / kernel_ms is reported); the FP64 rate R k (k + 1) / time as a
fraction of the 78.6 TFLOP/s peak; torch.cov on the same tensor (an independent
implementation, not a bar); np.cov and backend="host" on the host copy, once.
ipmc_scatter is also timed with one 64-wide tile where the default is narrower
(IPMC_COV_TILE=64; k <= 60) and with workgroups of 256 lanes instead of 1 024
(IPMC_COV_THREADS=256): the alternatives the tile width and the workgroup size were
chosen against.
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

SHAPES = {"ensemble": (65536, 20, 40), "burgers": (1024, 5000, 3), "config5": (16384, 4, 256),
          "config5_long": (256, 1024, 256)}
CASES = tuple(SHAPES)
CASE_TIMEOUT_S = 420
FP64_PEAK = 78.6e12


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


def kernels(t, block):
    """ipmc_scatter alone on the contiguous (C, n, k) device tensor t, in both centre modes."""
    import torch

    from ip_mcmc_amd import _abi
    from ip_mcmc_amd import device as dev
    from ip_mcmc_amd import posterior as P
    from ip_mcmc_amd._lib import call

    C, n, k = t.shape
    geom = P._geom(t, "time_vars")
    stream = dev.stream_handle(t.device)
    f64 = dict(dtype=torch.float64, device=t.device)
    nb = -(-C // block)
    mean_m, var_m = torch.empty((2 * C, k), **f64), torch.empty((2 * C, k), **f64)
    call("ipmc_split_stats", *geom, mean_m.data_ptr(), var_m.data_ptr(), stream)
    centre = mean_m.mean(dim=0).contiguous()
    part, dsum = torch.empty((nb, k, k), **f64), torch.empty((nb, k), **f64)
    keep = (mean_m, var_m, centre, part, dsum)
    return {
        "shared": lambda: call("ipmc_scatter", *geom, centre.data_ptr(), _abi.CENTER_SHARED, block, part.data_ptr(),
                               dsum.data_ptr(), stream),
        "split": lambda: call("ipmc_scatter", *geom, mean_m.data_ptr(), _abi.CENTER_SPLIT, block, part.data_ptr(),
                              None, stream),
        "split_stats": lambda: call("ipmc_split_stats", *geom, mean_m.data_ptr(), var_m.data_ptr(), stream),
    }, keep


def run_case(name):
    import torch

    from ip_mcmc_amd import device as dev
    from ip_mcmc_amd import multivariate_rhat, posterior_covariance
    from ip_mcmc_amd.covariance import default_block_chains

    dev.require_gpu()  # a measurement without the GPU fails; it does not fall back
    shape = SHAPES[name]
    C, n, k = shape
    rng = np.random.default_rng(1)
    x = 8.0 + 0.1 * rng.normal(size=shape)
    x[..., 1:] += 0.05 * x[..., :-1]
    t = torch.from_numpy(x).to("cuda")
    nbytes = t.numel() * t.element_size()
    block = default_block_chains(C, k)
    flop = C * n * k * (k + 1)
    rec = {"case": name, "gpu": torch.cuda.get_device_name(0), "dtype": "float64", "shape": list(shape),
           "input_bytes": nbytes, "block_chains": block, "blocks": -(-C // block), "flop": flop}

    rec["clone_ms"] = event_ms(lambda: t.clone(), 3, 20)
    clone = rec["clone_ms"]["median"]
    rec["clone_read_TBps"] = nbytes / clone * 1e-9

    kern, keep = kernels(t, block)
    for key, fn in kern.items():
        tag = f"ipmc_scatter_{key}" if key != "split_stats" else "ipmc_split_stats"
        rec[tag + "_ms"] = event_ms(fn, 3, 20)
        ms = rec[tag + "_ms"]["median"]
        rec[tag + "_rate_over_clone"] = clone / ms
        if key != "split_stats":
            rec[tag + "_fp64_peak_fraction"] = flop / (ms * 1e-3) / FP64_PEAK
    if k <= 60:
        os.environ["IPMC_COV_TILE"] = "64"
        rec["ipmc_scatter_shared_tile64_ms"] = event_ms(kern["shared"], 3, 20)
        del os.environ["IPMC_COV_TILE"]
    os.environ["IPMC_COV_THREADS"] = "256"
    rec["ipmc_scatter_shared_threads256_ms"] = event_ms(kern["shared"], 3, 20)
    del os.environ["IPMC_COV_THREADS"]

    api = {
        "posterior_covariance": lambda: posterior_covariance(t, backend="device"),
        "multivariate_rhat": lambda: multivariate_rhat(t, backend="device"),
    }
    for key, fn in api.items():
        rec[key + "_device_ms"] = event_ms(fn, 2, 10)

    flat = t.reshape(-1, k)
    rec["torch_cov_ms"] = event_ms(lambda: torch.cov(flat.T), 2, 10)
    got = posterior_covariance(t, backend="device")
    tc = torch.cov(flat.T).cpu().numpy().reshape(k, k)

    ref = {}
    rec["numpy_cov_host_ms"] = host_ms(lambda: ref.update(c=np.cov(x.reshape(-1, k), rowvar=False)))
    rec["posterior_covariance_host_ms"] = host_ms(lambda: ref.update(h=posterior_covariance(x, backend="host")))
    rec["multivariate_rhat_host_ms"] = host_ms(lambda: ref.update(r=multivariate_rhat(x, backend="host")))
    scale = np.sqrt(np.outer(np.diag(ref["c"]), np.diag(ref["c"])))
    rec["device_vs_numpy_max_rel"] = float((np.abs(got["cov"] - ref["c"]) / scale).max())
    rec["torch_cov_vs_numpy_max_rel"] = float((np.abs(tc - ref["c"]) / scale).max())
    rec["rhat_mv_device"] = multivariate_rhat(t, backend="device")["rhat_mv"]
    rec["rhat_mv_host"] = ref["r"]["rhat_mv"]
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r9", "posterior_cov.jsonl"))
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
        rc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT_S), sys.executable, os.path.abspath(__file__),
                             "--child", name, "--out", args.out]).returncode
        if rc != 0:
            print(f"covariance_bench: case {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

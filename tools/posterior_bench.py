"""Time of the pooled posterior histograms on the device (one GPU), beside a clone of the
same input and the numpy host path.

  python tools/posterior_bench.py [--out profiles/r8/posterior_hist.jsonl] [case ...]

cases: {ensemble, burgers}_{spread, onebin}
  ensemble  (65 536, 20, 40) f64: config 3's sample array (419 MB); histogramdd takes components (0, 1, 2)
  burgers   (1 024, 5 000, 3) f64: the Burgers studies' sample array (123 MB)
  spread    Gaussian samples, range = their support: the adds spread over the bins
  onebin    every sample 0.25 in the range (-1, 1.5): one counter per component (one joint
            cell) takes every add -- the worst contention

Each case runs in a child process of its own under `timeout` (the parent never opens the
GPU and stops at the first case that fails) and appends one JSON line to --out.  Device
times are HIP-event times after warm-up calls, median / min / max over the repetitions:
for support, marginal_histograms and histogramdd the whole API call on the device tensor
(it ends in the synchronising copy of its small result), and the C entry point alone
(ipmc_minmax, ipmc_hist1d, ipmc_histdd with their buffers prepared: for the last two the
zeroing of the result and the kernel).  The yardstick, in the same process: tensor.clone()
of the same input, which reads the data once and also writes it; every kernel reads it once,
and its rate is reported as a fraction of the clone's (clone_ms / kernel_ms).  ipmc_hist1d is
also timed with its LDS counters not replicated (IPMC_HIST_COPIES=1: plain LDS adds).
The numpy host path (backend="host") runs once on the same input.
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

SHAPES = {"ensemble": (65536, 20, 40), "burgers": (1024, 5000, 3)}
CASES = tuple(f"{s}_{d}" for s in SHAPES for d in ("spread", "onebin"))
CASE_TIMEOUT_S = 420
BINS = 20
LO, HI = -1.0, 1.5


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


def kernels(t, edges1d, comp, edgesdd):
    """The three C entry points alone on the contiguous (C, n, k) device tensor t."""
    import ctypes

    import torch

    from ip_mcmc_amd import device as dev
    from ip_mcmc_amd import posterior as P
    from ip_mcmc_amd._lib import call

    C, n, k = t.shape
    geom = P._geom(t, "time_vars")
    stream = dev.stream_handle(t.device)
    f64 = dict(dtype=torch.float64, device=t.device)
    i64 = dict(dtype=torch.int64, device=t.device)
    mm, scratch = torch.empty((2, k), **f64), torch.empty(2 * P.MINMAX_GROUPS * k, **f64)
    e1 = torch.from_numpy(edges1d).to(t.device)
    counts, below, above = torch.empty((k, BINS), **i64), torch.empty(k, **i64), torch.empty(k, **i64)
    nd = len(comp)
    c_comp, c_bins = (ctypes.c_int32 * nd)(*comp), (ctypes.c_int32 * nd)(*([BINS] * nd))
    edd = torch.from_numpy(np.concatenate(edgesdd)).to(t.device)
    cells = torch.empty(BINS**nd, **i64)
    keep = (mm, scratch, e1, counts, below, above, c_comp, c_bins, edd, cells)
    return {
        "minmax": lambda: call("ipmc_minmax", *geom, mm[0].data_ptr(), mm[1].data_ptr(), scratch.data_ptr(), stream),
        "hist1d": lambda: call("ipmc_hist1d", *geom, BINS, e1.data_ptr(), counts.data_ptr(), below.data_ptr(),
                               above.data_ptr(), stream),
        "histdd": lambda: call("ipmc_histdd", *geom, nd, ctypes.addressof(c_comp), ctypes.addressof(c_bins),
                               edd.data_ptr(), cells.data_ptr(), stream),
    }, keep


def run_case(name):
    import torch

    from ip_mcmc_amd import device as dev
    from ip_mcmc_amd import histogramdd, marginal_histograms, support

    dev.require_gpu()  # a measurement without the GPU fails; it does not fall back
    shape_name, data = name.rsplit("_", 1)
    shape = SHAPES[shape_name]
    k = shape[2]
    comp = (0, 1, 2)
    if data == "spread":
        x = np.random.default_rng(1).normal(size=shape)
        rng = None
    else:
        x = np.full(shape, 0.25)
        rng = (LO, HI)
    t = torch.from_numpy(x).to("cuda")
    nbytes = t.numel() * t.element_size()
    rec = {"case": name, "gpu": torch.cuda.get_device_name(0), "dtype": "float64", "shape": list(shape),
           "bins": BINS, "components_dd": list(comp), "input_bytes": nbytes}
    rdd = None if rng is None else [rng] * 3

    rec["clone_ms"] = event_ms(lambda: t.clone(), 3, 20)
    clone = rec["clone_ms"]["median"]
    rec["clone_read_TBps"] = nbytes / clone * 1e-9

    api = {
        "support": lambda: support(t, backend="device"),
        "marginal_histograms": lambda: marginal_histograms(t, bins=BINS, range=rng, backend="device"),
        "histogramdd": lambda: histogramdd(t, bins=BINS, range=rdd, components=comp, backend="device"),
    }
    for key, fn in api.items():
        rec[key + "_device_ms"] = event_ms(fn, 2, 10)

    h = marginal_histograms(t, bins=BINS, range=rng, backend="device")
    H, edd = histogramdd(t, bins=BINS, range=rdd, components=comp, backend="device")
    kern, keep = kernels(t, h["edges"], comp, edd)
    for key, fn in kern.items():
        rec[f"ipmc_{key}_ms"] = event_ms(fn, 3, 20)
        rec[f"ipmc_{key}_rate_over_clone"] = clone / rec[f"ipmc_{key}_ms"]["median"]
    os.environ["IPMC_HIST_COPIES"] = "1"
    rec["ipmc_hist1d_one_copy_ms"] = event_ms(kern["hist1d"], 3, 20)
    rec["ipmc_hist1d_one_copy_rate_over_clone"] = clone / rec["ipmc_hist1d_one_copy_ms"]["median"]
    del os.environ["IPMC_HIST_COPIES"]

    ref = {}
    rec["support_host_ms"] = host_ms(lambda: ref.update(s=support(x, backend="host")))
    rec["marginal_histograms_host_ms"] = host_ms(
        lambda: ref.update(h=marginal_histograms(x, bins=BINS, range=rng, backend="host")))
    rec["histogramdd_host_ms"] = host_ms(
        lambda: ref.update(H=histogramdd(x, bins=BINS, range=rdd, components=comp, backend="host")[0]))
    rec["equal_to_host"] = bool(np.array_equal(h["counts"], ref["h"]["counts"]) and np.array_equal(H, ref["H"])
                                and np.array_equal(support(t, backend="device"), ref["s"]))
    rec["largest_count_share"] = float(h["counts"].max() / (shape[0] * shape[1]))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r8", "posterior_hist.jsonl"))
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
            print(f"posterior_bench: case {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

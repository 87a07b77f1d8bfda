"""Time of the pooled sort, the rank scores and rank_convergence on the device (one GPU), beside
torch.sort of the same (k, S) float64 tensor.

  python tools/rank_bench.py [--out profiles/r12/rank_bench.jsonl] [case ...]

cases:
  ensemble      (65 536, 100, 40) f64: the headline ensemble's sample array (2.1 GB), S = 6 553 600 per component
  ensemble_f32  the same samples as f32 (1.05 GB): the three lowest bytes of every key are zero
  burgers       (1 024, 5 000, 3) f64: a Burgers study's sample array (123 MB), S = 5 120 000, small k

Each case runs in a child process of its own under `timeout` (the parent never opens the GPU and
stops at the first case that fails) and appends one JSON line to --out.  Device times are HIP-event
times after warm-up calls, median / min / max over the repetitions: ipmc_pooled_sort alone with its
buffers prepared, ipmc_rank_scores alone (normal scores) on its result, and the whole
rank_convergence on the device tensor (it ends in synchronising copies of small results).
The samples are 8 + 0.1 N(0, 1) (theta = 8 + u: the highest key byte is the same for every sample,
so one pass is skipped; f32 input skips the three lowest as well).  The passes that run are worked
out from the values by the sort's definition, with torch on the device (a pass runs for a component
iff that byte of the 64-bit key differs between two of its samples): nothing of the library's
workspace is read back.  From them the bytes the sort moves are computed: per key 8 (f32: 4) read
and 12 written by the key pass, 32 per pass that runs (the count reads the key, the scatter reads
and writes key and index), 16 or 24 by the last kernel (24 after an odd number of passes, when the
permutation ended in the workspace); bytes / time is reported as a fraction of the 8 TB/s HBM peak.
Yardstick, in the same process: torch.sort(stable=True) along the last axis of the (k, S) float64
tensor of the same values (an independent implementation that returns 64-bit indices).
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"ensemble": ((65536, 100, 40), "float64"), "ensemble_f32": ((65536, 100, 40), "float32"),
          "burgers": ((1024, 5000, 3), "float64")}
CASES = tuple(SHAPES)
CASE_TIMEOUT_S = 420
HBM_PEAK = 8.0e12  # bytes per second


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


def passes_that_run(t):
    """(k, 8) bool, on the host: pass p of component v runs iff byte p of the sort key (the sign bit
    flipped for a non-negative double, every bit for a negative one; -0 is +0) differs between two
    samples of component v of the (C, n, k) device tensor t (no NaN)."""
    import torch

    k = t.shape[2]
    b = (t.double().reshape(-1, k) + 0.0).view(torch.int64)
    key = torch.where(b < 0, ~b, b ^ torch.iinfo(torch.int64).min)
    diff = key ^ key[:1]
    return torch.stack([(((diff >> (8 * p)) & 0xFF) != 0).any(dim=0) for p in range(8)], dim=1).cpu().numpy()


def run_case(name):
    import torch

    from ip_mcmc_amd import device as dev
    from ip_mcmc_amd import rank_convergence
    from ip_mcmc_amd._lib import call

    dev.require_gpu()  # a measurement without the GPU fails; it does not fall back
    shape, dtype = SHAPES[name]
    C, n, k = shape
    S = C * n
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    t = torch.randn(shape, generator=gen, device="cuda", dtype=torch.float64).mul_(0.1).add_(8.0)
    if dtype == "float32":
        t = t.float()
    abi = dev.abi_dtype(t.dtype)
    stream = dev.stream_handle(t.device)
    rec = {"case": name, "gpu": torch.cuda.get_device_name(0), "dtype": dtype, "shape": list(shape), "S": S,
           "input_bytes": t.numel() * t.element_size()}

    need = ctypes.c_int64(0)
    call("ipmc_sort_workspace", C, n, k, abi, ctypes.byref(need))
    rec["workspace_bytes"] = need.value
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    srt = torch.empty((k, S), dtype=torch.float64, device="cuda")
    perm = torch.empty((k, S), dtype=torch.int32, device="cuda")
    z = torch.empty((C, n, k), dtype=torch.float64, device="cuda")

    def sort():
        call("ipmc_pooled_sort", t.data_ptr(), abi, C, n, k, n * k, k, 1, None, srt.data_ptr(), perm.data_ptr(),
             ws.data_ptr(), need.value, stream)

    def scores():
        call("ipmc_rank_scores", srt.data_ptr(), perm.data_ptr(), k, C, n, 1, z.data_ptr(), n * k, k, 1, None, 0, stream)

    rec["ipmc_pooled_sort_ms"] = event_ms(sort, 2, 10)
    rec["ipmc_rank_scores_ms"] = event_ms(scores, 2, 10)
    runs = passes_that_run(t)
    ran = int(runs.sum())  # passes summed over the components
    item = t.element_size()
    ended_in_workspace = int((runs.sum(axis=1) % 2 == 1).sum())  # the buffers alternate with every pass that runs
    moved = S * (k * (item + 12) + ran * 32 + (k - ended_in_workspace) * 16 + ended_in_workspace * 24)
    sort_s = rec["ipmc_pooled_sort_ms"]["median"] * 1e-3
    rec.update(passes_run_per_component=ran / k, sort_bytes_moved=moved, sort_TBps=moved / sort_s * 1e-12,
               sort_hbm_peak_fraction=moved / sort_s / HBM_PEAK, sort_Mkeys_per_s=S * k / sort_s * 1e-6)
    scores_moved = S * k * (8 + 4 + 8)
    rec["rank_scores_TBps"] = scores_moved / (rec["ipmc_rank_scores_ms"]["median"] * 1e-3) * 1e-12

    # the same values as a (k, S) float64 tensor, as torch.sort wants them
    flat = t.double().reshape(S, k).t().contiguous()
    rec["torch_sort_ms"] = event_ms(lambda: torch.sort(flat, dim=1, stable=True), 2, 10)
    rec["sort_over_torch_sort"] = rec["ipmc_pooled_sort_ms"]["median"] / rec["torch_sort_ms"]["median"]
    want, index = torch.sort(flat, dim=1, stable=True)
    rec["equals_torch_sort"] = bool(torch.equal(want, srt) and torch.equal(index.int(), perm))
    del flat, want, index, ws, z
    torch.cuda.empty_cache()

    import warnings

    def whole():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return rank_convergence(t, backend="device")

    rec["rank_convergence_ms"] = event_ms(whole, 1, 5)
    r = whole()
    rec["rhat_max"], rec["ess_bulk_min"], rec["ess_tail_min"] = (float(r["rhat"].max()), float(r["ess_bulk"].min()),
                                                                 float(r["ess_tail"].min()))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r12", "rank_bench.jsonl"))
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
            print(f"rank_bench: case {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

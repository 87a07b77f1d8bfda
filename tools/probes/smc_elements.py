"""ancestors_kernel and normal_kernel at the headline ensemble (65 536 x 40) through ipmc_systematic_ancestors
and ipmc_normal: HIP-event times of 20 calls after 3 warm-up calls, as tools/smc_stage_bench.py takes them.
Prints one JSON line; IPMC_LIB_PATH selects the library, the label names it in the line.

  python tools/probes/smc_elements.py [label]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ip_mcmc_amd import device as D, smc  # noqa: E402

C, K = 65536, 40
dev = torch.device("cuda", 0)
ops = smc._DeviceOps(dev)
phi = torch.from_numpy(20.0 + 5.0 * np.random.default_rng(0).standard_normal(C)).to(dev)
cum = ops.cumweights(phi, ops.phi_min(phi), 0.3)


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


res = {"lib": sys.argv[1] if len(sys.argv) > 1 else "in-tree", "shape": [C, K],
       "distinct_ancestors": int(torch.unique(ops.ancestors(cum, 0.37, C)).numel())}
res["ancestors"] = timed(lambda: ops.ancestors(cum, 0.37, C))
res["normal_f64"] = timed(lambda: D.normals(7, 0, C, 3, K, torch.float64, dev))
res["normal_f32"] = timed(lambda: D.normals(7, 0, C, 3, K, torch.float32, dev))
print(json.dumps(res), flush=True)

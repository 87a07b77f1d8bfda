"""A plain `bench.py --gpus 1 --steps K --warmup W` run: value's leg only (no
kernel leg, roofline, extras, parity or CPU baseline: those are --full's), K
timed steps, and with --dump-outputs the arrays the timed run returned -- the
same bits as the same run_sharded call made here, in another process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

CHAINS, STEPS, WARMUP = 2048, 3, 1


def test_plain_run_is_lean_and_dumps_what_it_computed(tmp_path):
    import torch

    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
           str(WARMUP), "--chains", str(CHAINS), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and not line["full"]
    assert line["unit"] == "pCN steps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert "2 048 chains" in line["metric"] and line["value"] > 0
    e2e = line["extra"]["run_e2e_moments"]
    assert e2e["steps"] == STEPS and line["value"] == e2e["pcn_steps_per_s"]
    assert abs(line["ms_per_step"] * STEPS / 1e3 - e2e["wall_s"]) < 1e-9
    assert abs(line["value"] - CHAINS * 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
    # nothing beside value's leg
    assert set(line["extra"]) == {"run_e2e_moments"}
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["parity"] is None
    assert "kernel leg" not in r.stderr and "host buffers" not in r.stderr

    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(got) == {"u", "phi", "accepts", "sum_u", "sum_u2", "mean", "chain_rows", "chain_ids"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum((out / f).stat().st_size for f in os.listdir(out)) < 64e6
    assert np.array_equal(got["chain_ids"], np.arange(CHAINS))
    assert got["u"].shape == (CHAINS, 40) and got["mean"].shape == (40,)
    assert got["accepts"].sum() == round(line["accept_rate"] * CHAINS * STEPS)

    # the same run here: the timed path's result, bit for bit
    sys.path.insert(0, REPO)
    import bench

    _, res = bench.timed_run(bench.make_problem("cfg3"), np.float64, torch.device("cuda", 0), CHAINS, STEPS, 0, 1,
                             gather="mean")
    for key in ("u", "sum_u", "sum_u2"):
        assert np.array_equal(got[key], res[key].double().cpu().numpy().reshape(CHAINS, 40)), key
    assert np.array_equal(got["phi"], res["phi"]) and np.array_equal(got["accepts"], res["accepts"])
    assert np.array_equal(got["mean"], res["mean"])

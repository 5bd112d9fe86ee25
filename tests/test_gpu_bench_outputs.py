"""A plain `bench.py --gpus 1 --steps K --warmup W` run and its --dump-outputs.

One child process runs the benchmark for two timed steps with --dump-outputs: the line carries the
headline figure and ms_per_step, the legs of --full are absent (null), and DIR/rgb.npy, DIR/depth.npy
hold float32 arrays of every ray of the frame, equal bit for bit to what the timed path returns for
the last step's seed (warmup + steps - 1) when this process renders it with the same arguments:
the dump is the output of the measured path and repeats from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    import bench
    import nerfmi
    from nerfmi import cameras, frames
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=REPO, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["higher_is_better"] is True
    assert line["unit"] == "rays/s" and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(bench.H * bench.W / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["cpu_baseline"] is None and line["f32_exact"] is None and line["train"] is None

    assert sorted(os.listdir(out)) == ["depth.npy", "rgb.npy"]
    rgb, depth = np.load(out / "rgb.npy"), np.load(out / "depth.npy")
    assert rgb.dtype == np.float32 and depth.dtype == np.float32
    assert rgb.shape == (bench.H * bench.W, 3) and depth.shape == (bench.H * bench.W,)
    assert np.isfinite(rgb).all() and np.isfinite(depth).all()

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = nerfmi.NeRF(nerfmi.Config()).to(dev).eval()
    torch.manual_seed(1)
    app = torch.randn(100, 32)[0].to(dev)
    with torch.no_grad():
        r, d = frames.render_path_frames(model, bench.workload("chair", 1, "weak"), bench.H, bench.W,
                                         cameras.synthetic_focal(bench.W), 2.0, 6.0, bench.N_COARSE, bench.N_FINE,
                                         appearance_embedding=app, perturb=True, hierarchical=True, seed=2)
    assert np.array_equal(r.reshape(-1, 3).cpu().numpy(), rgb)
    assert np.array_equal(d.reshape(-1).cpu().numpy(), depth)

"""GPU: `bench.py --dump-outputs DIR` writes what the last timed step computed, and `--steps` decides which step that is.

The headline frame is rendered again in this process - the turntable pose and jitter seed of step warmup + steps - 1 - and
must equal the dumped arrays bit for bit; the nerf training workload's dump carries the step's outputs and parameters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.timeout(600)
def test_dump_is_the_frame_of_the_last_timed_step(tmp_path):
    import bench
    from mirender import dist as mdist
    steps, warmup = 2, 1
    line = run_bench("--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path))
    assert line["steps"] == steps and line["warmup"] == warmup
    # a plain run is lean: what takes runs of its own waits for --full
    assert not {"frame64", "train", "cpu_baseline", "gpu_over_cpu", "psnr_vs_ref"} & set(line), sorted(line)
    assert line["roofline"]["launches"] == 2 * steps
    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("rgb", "depth", "acc")}
    assert sorted(os.listdir(tmp_path)) == ["acc.npy", "depth.npy", "rgb.npy"]
    assert got["rgb"].shape == (bench.H, bench.W, 3) and got["depth"].shape == got["acc"].shape == (bench.H, bench.W, 1)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_MAX_BYTES

    dev = torch.device("cuda", 0)
    coarse, fine = bench.make_models(dev)
    i = warmup + steps - 1
    theta = float(np.linspace(-180, 180, 41)[:-1][i])
    want = mdist.render_image_dist(bench.W, bench.H, 1.3875 * bench.W, bench.pose_degrees(4.0, theta, -30.0), bench.NEAR,
                                   bench.FAR, coarse, fine, bench.NC, bench.NF, seed=1000 + i)
    for name, w in zip(("rgb", "depth", "acc"), want):
        assert np.array_equal(got[name], w.cpu().numpy()), name


@pytest.mark.timeout(600)
def test_training_workload_dump_holds_outputs_loss_and_parameters(tmp_path):
    import bench
    line = run_bench("--workload", "nerf_train", "--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path))
    assert line["steps"] == 1
    coarse, fine = bench.make_models("cpu")
    n_params = sum(p.numel() for m in (coarse, fine) for p in m.parameters())
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"rgb_c", "depth_c", "acc_c", "rgb_f", "depth_f", "acc_f", "loss", "params"}
    assert got["rgb_f"].shape == (1024, 3) and got["loss"].shape == () and got["params"].shape == (n_params,)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())

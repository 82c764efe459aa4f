#!/usr/bin/env python3
"""Time of one training step with an occupancy grid against the same step without one (DESIGN.md 4.8 "Training with a grid").

    python tools/bench_occupancy_train.py [--rays 1024] [--repeats 5] [--warmup 2] [--steps 10] [--cases ones,quarter,twentieth]
                                          [--pose] [--out FILE.json]

The step of nerf/train_nerf.py at 1 024 rays, 64 + 128 samples, on bench.py's NeRF pair: forward, nerf_loss, backward,
FusedAdam.  With a grid the forward is mirender.occupancy_train.render_rays, without one render_core.render_rays (the plain
training path) on the same fields in the same process; the two alternate.  A repeat is `--steps` steps between two
synchronisations, reported per step.  Grids are from_dense at 128^3 over (-4, 4)^3: all ones and the two balls of
tools/bench_occupancy.py (radii 1.032 and 0.504: about a quarter / a twentieth of an 800 x 800 frame's samples).  Per case: the
evaluated counts of the timed batch, evaluated / n (2 Nc + Nf), step ms (median, min, max over the warmed repeats) with and
without the grid, and their ratio.  One JSON line per case; --out writes them all to a file.

--pose: the same step with a gradient to the rays as well (rays.requires_grad: mirender.pose.render_rays(grid=), DESIGN.md 4.8
"Gradients to the rays"), next to the step with the grid and without that gradient, and the ungridded pose.render_rays step;
the three alternate.  Per case: pose_grid_step_ms, grid_step_ms, pose_plain_step_ms and the ray gradient's share of the
gridded step.

--no-baseline skips the plain steps (for a kernel trace of one case: rocprofv3 --kernel-trace --stats -- python
tools/bench_occupancy_train.py --cases twentieth --no-baseline --repeats 2).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "msra-practice-project_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.bench_occupancy import HI, LO, NC, NEAR, FAR, NF, RES, ball  # noqa: E402

RADII = {"quarter": 1.032, "twentieth": 0.504}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--cases", default="ones,quarter,twentieth")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--pose", action="store_true", help="time the steps with a gradient to the rays")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import bench
    from mirender import occupancy, occupancy_train, ops, pose, render_core, train
    dev = torch.device("cuda", 0)
    coarse, fine = bench.make_models(dev)
    for m in (coarse, fine):
        for p in m.parameters():
            p.requires_grad_(True)
    opt = train.FusedAdam([coarse, fine], lr=5e-4, betas=(0.9, 0.999))
    n = a.rays
    w = 800
    rays_all = ops.gen_rays(w, w, 1.3875 * w, bench.pose_degrees(4.0, 0.0, -30.0), dev)
    idx = torch.randperm(w * w, generator=torch.Generator().manual_seed(0))[:n].to(dev)
    rays = rays_all[idx].contiguous()
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    alpha = torch.ones(n, device=dev)
    total = n * (2 * NC + NF)

    rays_req = rays.clone().requires_grad_(True)

    def steps(grid, to_rays=False):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        counts = None
        for k in range(a.steps):
            if to_rays:
                rays_req.grad = None
                out = pose.render_rays(rays_req, NEAR, FAR, coarse, fine, NC, NF, grid=grid, seed=k)
            elif grid is None:
                out = render_core.render_rays(rays, NEAR, FAR, coarse, fine, NC, NF, seed=k)
            else:
                out, counts = occupancy_train.render_rays(rays, NEAR, FAR, coarse, fine, NC, NF, grid=grid, seed=k, return_counts=True)
            loss, _ = train.nerf_loss(out, target, alpha, use_alpha=False, use_fine_model=True)
            opt.zero_grad()
            loss.backward()
            opt.step()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / a.steps, counts

    results = []
    for case in [c for c in a.cases.split(",") if c]:
        dense = np.ones((RES,) * 3, bool) if case == "ones" else ball(RADII[case])
        grid = occupancy.OccupancyGrid.from_dense(dense, LO, HI, dev)
        with_grid, without, counts = [], [], None
        pose_grid, pose_plain = [], []
        for i in range(a.warmup + a.repeats):
            t_plain = None if a.no_baseline else steps(None)[0]
            t_grid, counts = steps(grid)
            t_pose = (steps(grid, True)[0], None if a.no_baseline else steps(None, True)[0]) if a.pose else None
            if i >= a.warmup:
                with_grid.append(t_grid)
                if t_plain is not None:
                    without.append(t_plain)
                if t_pose:
                    pose_grid.append(t_pose[0])
                    if t_pose[1] is not None:
                        pose_plain.append(t_pose[1])
        evaluated = [int(v) for v in counts[0].tolist()]
        rec = {"case": case, "rays": n, "samples": [NC, NF], "grid_resolution": RES, "ball_radius": RADII.get(case),
               "evaluated": evaluated, "evaluated_fraction": sum(evaluated) / total, "repeats": a.repeats, "steps_per_repeat": a.steps,
               "grid_step_ms": {"median": statistics.median(with_grid), "min": min(with_grid), "max": max(with_grid)}}
        if without:
            rec["plain_step_ms"] = {"median": statistics.median(without), "min": min(without), "max": max(without)}
            rec["ratio_grid_over_plain"] = rec["grid_step_ms"]["median"] / rec["plain_step_ms"]["median"]
        if pose_grid:
            rec["pose_grid_step_ms"] = {"median": statistics.median(pose_grid), "min": min(pose_grid), "max": max(pose_grid)}
            rec["ray_gradient_ms"] = rec["pose_grid_step_ms"]["median"] - rec["grid_step_ms"]["median"]
        if pose_plain:
            rec["pose_plain_step_ms"] = {"median": statistics.median(pose_plain), "min": min(pose_plain), "max": max(pose_plain)}
            rec["ratio_pose_grid_over_pose_plain"] = rec["pose_grid_step_ms"]["median"] / rec["pose_plain_step_ms"]["median"]
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

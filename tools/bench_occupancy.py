#!/usr/bin/env python3
"""Frame time of render_image with an occupancy grid against the same frame without one.

    python tools/bench_occupancy.py [--size 800] [--repeats 5] [--warmup 2] [--cases ones,quarter,twentieth] [--out FILE.json]

One W x W frame (64 + 128 samples) of bench.py's NeRF pair through render_core.render_image, seeded jitter.  The run without
a grid is the plain path (windowed sigma-only coarse pass, deferred colour branch) on the same fields in the same process;
its repeats alternate with the grid's.  Grids are from_dense at 128^3 over (-4, 4)^3: all ones, and two balls about the
origin whose radii are found by bisection on the evaluated count so that about a quarter / a twentieth of the frame's
n (2 Nc + Nf) samples are evaluated.  Per case: frame ms (median, min, max over the warmed repeats), the evaluated counts,
evaluated / n (2 Nc + Nf), and the ratio grid frame time / no-grid frame time.  Prints one JSON line per case and, with --out,
writes them all to a file.

--no-baseline skips the runs without a grid (for a kernel trace of one case: rocprofv3 --kernel-trace --stats -- python
tools/bench_occupancy.py --cases twentieth --no-baseline --repeats 2; the mark kernel is occupancy_mark_rays_kernel, the list
forward the nerf_fwd_kernel instance whose last template argument is true).
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

NEAR, FAR, NC, NF = 2.0, 6.0, 64, 128
LO, HI, RES = (-4.0,) * 3, (4.0,) * 3, 128
SEED = 0


def ball(radius):
    c = (np.arange(RES, dtype=np.float64) + 0.5) * ((HI[0] - LO[0]) / RES) + LO[0]
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    return x * x + y * y + z * z <= radius * radius


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="ones,quarter,twentieth")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import bench
    from mirender import fields, occupancy, ops, render_core
    dev = torch.device("cuda", 0)
    coarse, fine = bench.make_models(dev)
    pf_c, pf_f = fields.as_packed_field(coarse), fields.as_packed_field(fine)
    w = h = a.size
    n = w * h
    focal, pose = 1.3875 * w, bench.pose_degrees(4.0, 0.0, -30.0)
    total = n * (2 * NC + NF)

    def counts_of(grid):
        with torch.no_grad():
            rays = ops.gen_rays(w, h, focal, pose, dev)
            _, c = ops.render_rays_occupancy(pf_c, pf_f, rays, NEAR, FAR, NC, NF, grid, None, SEED, coarse_outputs=False)
        return [int(v) for v in c.tolist()]

    def grid_of(dense):
        return occupancy.OccupancyGrid.from_dense(dense, LO, HI, dev)

    def ball_for(target):
        lo_r, hi_r = 0.0, 4.0 * 3 ** 0.5
        for _ in range(10):                                   # the evaluated fraction grows with the radius
            mid = 0.5 * (lo_r + hi_r)
            if sum(counts_of(grid_of(ball(mid)))) / total < target:
                lo_r = mid
            else:
                hi_r = mid
        return 0.5 * (lo_r + hi_r)

    def frame(grid):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        render_core.render_image(w, h, focal, pose, NEAR, FAR, coarse, fine, NC, NF, seed=SEED, grid=grid)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    results = []
    for case in [c for c in a.cases.split(",") if c]:
        radius = None
        if case == "ones":
            dense = np.ones((RES,) * 3, bool)
        else:
            radius = ball_for({"quarter": 0.25, "twentieth": 0.05}[case])
            dense = ball(radius)
        grid = grid_of(dense)
        counts = counts_of(grid)
        with_grid, without = [], []
        for i in range(a.warmup + a.repeats):
            t_plain = None if a.no_baseline else frame(None)
            t_grid = frame(grid)
            if i >= a.warmup:
                with_grid.append(t_grid)
                if t_plain is not None:
                    without.append(t_plain)
        rec = {"case": case, "size": a.size, "samples": [NC, NF], "grid_resolution": RES, "ball_radius": radius,
               "cells_occupied": float(dense.mean()), "evaluated": counts, "evaluated_fraction": sum(counts) / total,
               "repeats": a.repeats, "grid_ms": {"median": statistics.median(with_grid), "min": min(with_grid), "max": max(with_grid)}}
        if without:
            rec["no_grid_ms"] = {"median": statistics.median(without), "min": min(without), "max": max(without)}
            rec["ratio_grid_over_no_grid"] = rec["grid_ms"]["median"] / rec["no_grid_ms"]["median"]
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

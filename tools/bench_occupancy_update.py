#!/usr/bin/env python3
"""What it costs to keep an occupancy grid current while the field trains (DESIGN.md 4.8 "Live grid").

    python tools/bench_occupancy_update.py [--repeats 5] [--warmup 2] [--rows 262144] [--steps 10] [--out FILE.json]

All in one process on bench.py's NeRF pair, every figure the median (min .. max) of `--repeats` warmed repeats, in ms between
two device events:

    from_field        OccupancyGrid.from_field(resolution=128, supersample=2): the rebuild a live grid replaces
    sweep             LiveOccupancyGrid.update(model) at 128^3: every cell at one jittered point
    partial           LiveOccupancyGrid.update(model, cells=rows), and the same four stages called one by one with an event
                      between them: draw, field evaluation, fold, pack
    plain / grid step the 1 024-ray 64 + 128 training step of tools/bench_occupancy_train.py without a grid and with its
                      "quarter" grid (`--steps` steps per repeat, reported per step)

Whether an update at a given period pays is arithmetic on these figures; nothing here is tuned to a target.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "msra-practice-project_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.bench_occupancy import HI, LO, NC, NEAR, FAR, NF, RES, ball  # noqa: E402
from tools.bench_occupancy_train import RADII  # noqa: E402


def summary(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=1 << 18)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import bench
    from mirender import _lib, fields, occupancy, occupancy_train, ops, render_core, train
    dev = torch.device("cuda", 0)
    coarse, fine = bench.make_models(dev)
    pf = fields.as_packed_field(fine)

    def timed(fn, marks=1):
        """fn(mark) calls mark() after each of its `marks` stages: the warmed repeats' ms per stage, [marks][repeats]."""
        out = [[] for _ in range(marks)]
        for i in range(a.warmup + a.repeats):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(marks + 1)]
            at = iter(ev[1:])
            ev[0].record()
            fn(lambda: next(at).record())
            torch.cuda.synchronize(dev)
            if i >= a.warmup:
                for k in range(marks):
                    out[k].append(ev[k].elapsed_time(ev[k + 1]))
        return out

    def once(fn):
        def run(mark):
            fn()
            mark()
        return summary(timed(run)[0])

    rec = {"grid_resolution": RES, "cells": RES ** 3, "partial_rows": a.rows, "repeats": a.repeats, "unit": "ms"}
    rec["from_field_128_supersample_2"] = once(lambda: occupancy.OccupancyGrid.from_field(fine, LO, HI, resolution=RES, threshold=0.01,
                                                                                          supersample=2, dilate=1))
    live = occupancy.LiveOccupancyGrid(LO, HI, RES, dev, dilate=1)
    rec["sweep_update"] = once(lambda: live.update(fine))
    rec["occupied_fraction_after_sweeps"] = live.occupied_fraction()
    rec["partial_update"] = once(lambda: live.update(fine, cells=a.rows))

    # the partial update's four stages, as update() issues them (one batch per 64^3 rows)
    g, rows, batch = live.grid, a.rows, 64 ** 3
    pdims, plo, pcell = live._dims[1], live._lo[1], live._cell[1]
    ids = torch.empty(rows, dtype=torch.int32, device=dev)
    sigma = torch.empty(rows, dtype=torch.float32, device=dev)
    pts = torch.empty((rows, 6), dtype=torch.float32, device=dev)

    def stages(mark):
        with torch.no_grad():
            for head in range(0, rows, batch):
                count = min(batch, rows - head)
                _lib.call("mi_occupancy_draw_points", dev, _lib.ptr(g.bits), pdims, plo, pcell, live.seed, live.updates & 0xFFFFFFFF, 1,
                          head, count, rows - rows // 2, _lib.ptr(ids[head:head + count]), _lib.ptr(pts[head:head + count]))
            mark()
            for head in range(0, rows, batch):
                count = min(batch, rows - head)
                sigma[head:head + count] = fields.eval_points(pf, pts[head:head + count])[:, 3]
            mark()
            _lib.call("mi_occupancy_density_update", dev, _lib.ptr(sigma), _lib.ptr(ids), rows, pdims, live.decay, _lib.ptr(live.density),
                      _lib.ptr(live._ws), live._ws_bytes)
            mark()
            _lib.call("mi_occupancy_density_pack", dev, _lib.ptr(live.density), pdims, live.threshold, int(live.relative), live.dilate,
                      _lib.ptr(g.bits), _lib.ptr(live._ws), live._ws_bytes)
            mark()
            live.updates += 1
    for name, ms in zip(("draw", "field_eval", "fold", "pack"), timed(stages, 4)):
        rec["partial_" + name] = summary(ms)
    rec["ns_per_point_field_eval"] = rec["partial_field_eval"]["median"] * 1e6 / rows

    # the training step it sits next to: tools/bench_occupancy_train.py's, plain and with the "quarter" grid
    for m in (coarse, fine):
        for p in m.parameters():
            p.requires_grad_(True)
    opt = train.FusedAdam([coarse, fine], lr=5e-4, betas=(0.9, 0.999))
    n, w = 1024, 800
    rays_all = ops.gen_rays(w, w, 1.3875 * w, bench.pose_degrees(4.0, 0.0, -30.0), dev)
    rays = rays_all[torch.randperm(w * w, generator=torch.Generator().manual_seed(0))[:n].to(dev)].contiguous()
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    alpha = torch.ones(n, device=dev)
    quarter = occupancy.OccupancyGrid.from_dense(ball(RADII["quarter"]), LO, HI, dev)

    def steps(grid):
        for k in range(a.steps):
            if grid is None:
                out = render_core.render_rays(rays, NEAR, FAR, coarse, fine, NC, NF, seed=k)
            else:
                out = occupancy_train.render_rays(rays, NEAR, FAR, coarse, fine, NC, NF, grid=grid, seed=k)
            loss, _ = train.nerf_loss(out, target, alpha, use_alpha=False, use_fine_model=True)
            opt.zero_grad()
            loss.backward()
            opt.step()
    for name, grid in (("plain_step", None), ("grid_step_quarter", quarter)):
        s = once(lambda: steps(grid))
        rec[name] = {k: v / a.steps for k, v in s.items()}
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

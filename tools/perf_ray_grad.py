#!/usr/bin/env python3
"""Cost of the gradient to the rays: the 1 024-ray, 64+128 NeRF training step (render_rays forward + backward on a coarse
and a fine field) with and without `mirender.pose`'s ray gradients.  Not a test.

    python tools/perf_ray_grad.py [--iters 30] [--warmup 5] [--once MODE] [--json PATH]

Timing: device events around whole steps, after warm-up, the two variants interleaved so that clock drift hits both; the
median and the spread over the iterations are reported.  `--once plain|rays` runs a few steps of one variant and nothing
else: the program to put under `rocprofv3 --kernel-trace --stats` (input_grad_pe_kernel and composite_bwd_rays_kernel are
the added kernels; their bytes per point follow from the rows they read: dA of the three consuming layers + the two
encoding rows)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "msra-practice-project_amd"))

from mirender import fields, pose, render_core  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--once", choices=["plain", "rays"])
    ap.add_argument("--json")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n, nc, nf, near, far = 1024, 64, 128, 2.0, 6.0
    coarse, fine = fields.NeRF().to(dev), fields.NeRF().to(dev)
    o = torch.randn(n, 3, device=dev)
    o = 4.0 * o / o.norm(dim=1, keepdim=True)
    rays = torch.stack([o, -o / 4.0 + 0.1 * torch.randn(n, 3, device=dev)], 1).contiguous()
    target = torch.rand(n, 3, device=dev)

    def step(mode):
        r = rays.clone().requires_grad_(mode == "rays")
        fn = pose.render_rays if mode == "rays" else render_core.render_rays
        out = fn(r, near, far, coarse, fine, nc, nf, seed=3)
        loss = torch.mean((out[3] - target) ** 2) + torch.mean((out[0] - target) ** 2)
        loss.backward()
        for p in list(coarse.parameters()) + list(fine.parameters()):
            p.grad = None

    if args.once:
        for _ in range(3):
            step(args.once)
        torch.cuda.synchronize()
        return
    times = {"plain": [], "rays": []}
    for i in range(args.warmup + args.iters):
        for mode in ("plain", "rays"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(mode)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                times[mode].append(a.elapsed_time(b))
    res = {m: dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t)) for m, t in times.items()}
    res["ratio_rays_over_plain"] = res["rays"]["median_ms"] / res["plain"]["median_ms"]
    res["config"] = dict(rays=n, n_coarse=nc, n_fine=nf, kind="nerf coarse + fine", iters=args.iters, warmup=args.warmup)
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

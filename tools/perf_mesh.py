#!/usr/bin/env python3
"""Marching cubes on the device (mirender.mesh), timed on HIP events:

    python tools/perf_mesh.py [--n 512]

1. an analytic sphere on an n^3 grid, 2. -sigma of a FilmSirenNeRF on create_mesh's n^3 grid, and 3. the
pi_GAN/extract_mesh.py call end to end (create_mesh N=n, max_batch=65536), split into grid and marching-cubes time.
Achieved GB/s counts the bytes the design must move: three sweeps of the volume (count, vertices, faces), the 2-byte
vertex tag written once and read once, and the output arrays."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "msra-practice-project_amd")]

import torch  # noqa: E402

from mirender import mesh, pigan  # noqa: E402
from mirender.grid import density_grid  # noqa: E402
from oracle import synth  # noqa: E402

HBM_TBS = 6.3      # achievable HBM rate of MI355X_MICROARCH.md


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best, out


def mc_record(name, vol, level, spacing=(1.0, 1.0, 1.0)):
    ms, (v, f, n, val) = timed(lambda: mesh.marching_cubes(vol, level, spacing))
    nbytes = 3 * vol.numel() * 4 + 2 * vol.numel() * 2 + v.numel() * 4 * 2 + val.numel() * 4 + f.numel() * 4
    rec = dict(case=name, shape=list(vol.shape), verts=len(v), faces=len(f), mc_ms=ms, bytes=nbytes,
               gbs=nbytes / ms / 1e6, frac_of_hbm=nbytes / ms / 1e6 / (HBM_TBS * 1e3))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    args = ap.parse_args()
    n, dev = args.n, torch.device("cuda", 0)
    ax = torch.arange(n, device=dev, dtype=torch.float32) - (n - 1) / 2
    sphere = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - 0.4 * n
    mc_record(f"sphere {n}^3", sphere, 0.0)
    del sphere

    gen = pigan.Generator(256, 64).to(dev)
    sd = synth.state_dict("film_siren_nerf", seed=11, sharp=True)
    gen.film_siren_nerf.load_state_dict(sd)
    z = torch.randn(1, 256, generator=torch.Generator().manual_seed(0)).to(dev)
    with torch.no_grad():
        gen.set_film_params(gen.get_mapping(z)[0])
        torch.cuda.synchronize()
        t0 = time.time()
        sdf = density_grid(gen.film_siren_nerf, n, 65536)
        torch.cuda.synchronize()
        grid_s = time.time() - t0
    level = -20.0 if float(sdf.min()) <= -20.0 else float(sdf.quantile(0.05)) if sdf.numel() < 2 ** 24 else float(sdf.min()) * 0.5
    rec = mc_record(f"film_siren_nerf -sigma {n}^3 level {level:g}", sdf, level, (0.2 / (n - 1),) * 3)
    print(json.dumps(dict(case="density_grid", n=n, max_batch=65536, grid_s=grid_s,
                          mc_share_of_grid=rec["mc_ms"] / 1e3 / grid_s)), flush=True)
    del sdf
    with tempfile.TemporaryDirectory() as tmp:
        torch.cuda.synchronize()
        t0 = time.time()
        v, f = mesh.create_mesh(gen, os.path.join(tmp, "mesh"), N=n, max_batch=65536, level=level, z=z)
        torch.cuda.synchronize()
        total = time.time() - t0
    print(json.dumps(dict(case="create_mesh end to end", N=n, max_batch=65536, total_s=total, verts=len(v),
                          faces=len(f))), flush=True)


if __name__ == "__main__":
    main()

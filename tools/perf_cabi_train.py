#!/usr/bin/env python3
"""One training step of render_rays through the C-ABI pair (mi_render_rays_train + mi_render_rays_backward) and through
mirender's autograd (autograd.render_rays_train + backward), timed on device events:

    python tools/perf_cabi_train.py [--steps 5] [--warmup 2]

Cases: C4, the pi_GAN generator step (32 images of 128 x 128, 12 + 24 samples, FilmSirenNeRF, one field for both
passes), and the nerf step (1 024 rays, 64 + 128 samples, NeRF coarse + fine).  The loss is a fixed weighting of the six
outputs, so the step is render_rays' forward and backward and nothing else.  The kernels are the same ones on both
paths; the pair runs them without Python between the launches.  Every (case, path) runs in a child process of its own
under `timeout -k 10`; the table goes to profiles/perf_cabi_train.log."""
import argparse
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "msra-practice-project_amd")]
LOG = os.path.join(ROOT, "profiles", "perf_cabi_train.log")
CASES = {"c4": dict(kind=2, shared=True, w=128, h=128, nc=12, nf=24, groups=32),
         "nerf1024": dict(kind=0, shared=False, w=32, h=32, nc=64, nf=128, groups=1)}


def _helpers():
    """Case / cotangents / autograd_step of tests/test_gpu_cabi_train.py: the same inputs the bit-equality tests use."""
    spec = importlib.util.spec_from_file_location("cabi_train_cases", os.path.join(ROOT, "tests", "test_gpu_cabi_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_one(name, path, steps, warmup):
    import torch
    from mirender import _lib, autograd as A
    T = _helpers()
    c = CASES[name]
    case = T.Case(c["kind"], c["shared"], c["w"], c["h"], c["nc"], c["nf"], c["groups"])
    cots = case.cotangents()
    if path == "autograd":
        def step():
            T.autograd_step(case, cots)
    else:
        lib = _lib.load()
        dev = T.dev()
        pf_c, pf_f, n, nc, nf = case.pf_c, case.pf_f, case.n, case.nc, case.nf
        rp_c, rp_f = A._max_points_per_chunk(pf_c), A._max_points_per_chunk(pf_f)
        groups = case.groups if T.is_film(case.kind) else 1
        shared = int(case.shared)
        ws_bytes = lib.mi_render_workspace_bytes(n, nc, nf) + (lib.mi_render_shared_field_extra_bytes(n, nc, nf) if shared else 0)
        full = lib.mi_render_train_saved_bytes(case.kind, case.kind, shared, n, nc, nf)
        bw_bytes = lib.mi_render_backward_workspace_bytes(case.kind, case.kind, shared, groups, n // groups, nc, nf, rp_c, rp_f)
        free, _ = torch.cuda.mem_get_info(dev)
        # keep what autograd's forward would keep: up to SAVE_FINE_BYTES, within what is free next to the backward
        saved_bytes = max(0, min(full, A.SAVE_FINE_BYTES, free - ws_bytes - bw_bytes - A.RESERVE_FIXED_BYTES))
        ws, sv, bw = (torch.empty(max(int(b), 1), dtype=torch.uint8, device=dev) for b in (ws_bytes, saved_bytes, bw_bytes))
        outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in T.OUT_SHAPES(n)]
        grads = [[torch.empty_like(p) for p in pf.params] for pf in case.fields()]
        g_film = None if case.film is None else torch.empty_like(case.film)
        arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
        par = lambda pf: arr([p.detach() for p in pf.params]) if T.is_film(case.kind) else None  # noqa: E731
        written = ctypes.c_int()

        def step():
            stream = _lib.stream_ptr(dev)
            packed_c, packed_f = pf_c.refresh(), pf_f.refresh()
            _lib.check(lib.mi_render_rays_train(case.kind, _lib.ptr(packed_c), case.kind, _lib.ptr(packed_f),
                                                _lib.ptr(case.film), _lib.ptr(case.rays), groups, n // groups, case.near,
                                                case.far, nc, nf, _lib.ptr(case.z_lin), _lib.ptr(case.u_lin), None,
                                                case.seed, 0, *[_lib.ptr(o) for o in outs], _lib.ptr(ws), ws_bytes, rp_c,
                                                rp_f, _lib.ptr(sv), saved_bytes, stream), "mi_render_rays_train")
            _lib.check(lib.mi_render_rays_backward(
                case.kind, _lib.ptr(packed_c), _lib.ptr(pf_c.refresh_bwd()), par(pf_c), case.kind, _lib.ptr(packed_f),
                _lib.ptr(pf_f.refresh_bwd()), par(pf_f), _lib.ptr(case.film), _lib.ptr(case.rays), groups, n // groups, nc,
                nf, rp_c, rp_f, _lib.ptr(ws), ws_bytes, _lib.ptr(sv), saved_bytes, *[_lib.ptr(t) for t in cots],
                arr(grads[0]), arr(grads[-1]) if not shared else None, _lib.ptr(g_film), _lib.ptr(bw), bw_bytes,
                ctypes.byref(written), stream), "mi_render_rays_backward")
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    print(json.dumps(dict(case=name, path=path, steps=steps, median_ms=times[len(times) // 2], min_ms=times[0],
                          max_ms=times[-1])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--one", nargs=2, metavar=("CASE", "PATH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return run_one(args.one[0], args.one[1], args.steps, args.warmup)
    rows = []
    for name in CASES:
        for path in ("autograd", "pair"):
            cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--one", name, path]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:           # a fault or a time limit: report it and start nothing more on the GPU
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(f"{name} / {path}: exit status {r.returncode}")
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "w") as f:
        f.write(f"render_rays training step (forward + backward), {args.steps} timed steps after {args.warmup} warm-up, "
                "device events, median [min, max] ms; the autograd step also clones its gradients and synchronises once "
                "(tests/test_gpu_cabi_train.py:autograd_step)\n")
        for name in CASES:
            by = {r["path"]: r for r in rows if r["case"] == name}
            line = f"{name:9s} " + "  ".join(f"{p}: {by[p]['median_ms']:.2f} [{by[p]['min_ms']:.2f}, {by[p]['max_ms']:.2f}]"
                                             for p in ("autograd", "pair"))
            line += f"  pair/autograd {by['pair']['median_ms'] / by['autograd']['median_ms']:.3f}"
            f.write(line + "\n")
            print(line)


if __name__ == "__main__":
    main()

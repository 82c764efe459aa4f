#!/usr/bin/env python3
"""One SHA-256 per output tensor of every instance of the fused field-MLP forward, on one MI355X.

    python tools/fwd_hashes.py > hashes.txt

The evidence that a change which may move the forward kernels' machine code (another split of their translation units, a
compiler flag) left their arithmetic alone: run it at the parent and at the branch and compare the outputs line for line.
Inputs are seeded (oracle/synth.py, tests/film_depth_util.py for the FiLM depths) with the sharp density head, so sigma is
exactly 0 at some points and positive at others.  Cases:

  * every fixed kind, and FiLM depths 4 and 12 with and without the direction;
  * point form with M = 1, 127, 128, 129, 257; ray form with 43 rays x 3 samples (129 points; the FiLM kinds: 2 images of 129
    points each, so a tile boundary falls inside a group);
  * for each: the inference instance (raw) and the training instance (raw and every saved region);
  * the kinds with a sigma-only instance: mi_render_rays without rgb_c at the same sizes in rays (M and 43 rays x 3 coarse
    samples, the fewest the fine sampler takes: the sigma-only instance over 3, 381, 384, 387, 771 and 129 points) and at
    33 rays x 16 coarse samples (the windowed instance: 3 ragged tiles of 16 rays, 2 windows); depth_c, acc_c and the fine
    outputs;
  * NeRF, TinyNeRF: mi_field_eval_rays_deferred at 43 x 3 (the trunk-and-spill instance and the colour-branch kernel);
  * NeRF, SirenNeRF, TinyNeRF: the list-driven inference and training instances at 43 x 3 over a half-occupied 4^3 grid with the
    ordered mark; the saved buffer is prefilled with a constant and the first `count` rows of every region are hashed."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "msra-practice-project_amd"), ROOT):
    sys.path.insert(0, p)

import bwd_gates as G  # noqa: E402
import film_depth_util as FD  # noqa: E402
from mirender import _lib, fields, occupancy, ops  # noqa: E402
from oracle import render_ref as R, synth  # noqa: E402

DEV = torch.device("cuda", 0)
FIXED = ["nerf", "siren_nerf", "film_siren_nerf", "film_siren_nerf_nodir", "tiny_nerf"]
DEPTHS = [(4, False), (4, True), (12, False), (12, True)]
SIGMA_KINDS = ["nerf", "siren_nerf", "tiny_nerf"]      # a sigma-only instance, a list-driven pair
DEFER_KINDS = ["nerf", "tiny_nerf"]
POINTS = (1, 127, 128, 129, 257)
N_RAYS, N_SAMPLES = 43, 3
FILL = 7.0                                             # what a buffer holds where a kernel must not write


def emit(case, name, t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    print(f"{hashlib.sha256(a.tobytes()).hexdigest()}  {case} {name} {list(a.shape)}", flush=True)


def packed(name, seed):
    """(PackedField, FiLM layers or 0) of a kind name: a fixed kind of oracle/synth.py or a depth name of tests/bwd_gates.py."""
    depth = G.depth_of(name)
    if name in FIXED:
        model = fields.field_from_state_dict(synth.state_dict(name, seed=seed, sharp=True, bias_jitter=0.05), DEV)
    else:
        L, use_dir = depth
        model = fields.FilmSirenNeRF(hidden_layers=L, use_dir=use_dir)
        model.load_state_dict(FD.state_dict(L, use_dir, seed=seed, head="sharp"))
        model = model.to(DEV)
    return fields.as_packed_field(model), (depth[0] if depth else 0)


def rays_of(n, film):
    pose = synth.pose_radians(1.0, 0.2, -0.1) if film else synth.pose_degrees(4.0, 20.0, -30.0)
    r = torch.from_numpy(R.rays_from_camera(40, 40, 180.0 if film else 55.0, pose))
    return r[(torch.arange(n) * 1600 // n + 20) % 1600].contiguous().to(DEV)


def regions(name, acts, rows, count=None):
    layout = G.ACTS[name]
    for key, t in G.regions(layout, acts, rows).items():
        yield key, (t if count is None else t[:count])


def field_cases(name):
    lib = _lib.load()
    pf, L = packed(name, 5)
    k, stream = pf.kind, _lib.stream_ptr(DEV)
    per_point = lib.mi_field_train_acts_floats(k)
    assert per_point == G.floats_per_point(G.ACTS[name]), name

    def both(case, groups, rows, infer, train):
        film = FD.film_rows(groups, L, seed=100 + L).to(DEV) if L else None
        raw = torch.full((rows, 4), FILL, device=DEV)
        _lib.check(infer(_lib.ptr(film), _lib.ptr(raw)), case)
        emit(case, "infer.raw", raw)
        raw = torch.full((rows, 4), FILL, device=DEV)
        acts = torch.full((per_point * rows,), FILL, device=DEV)
        _lib.check(train(_lib.ptr(film), _lib.ptr(raw), _lib.ptr(acts)), case)
        emit(case, "train.raw", raw)
        for key, t in regions(name, acts, rows):
            emit(case, "train.saved." + key, t)

    for m in POINTS:
        x = FD.sample_points(m, seed=40 + m).to(DEV)
        both(f"{name} points M={m}", 1, m,
             lambda f, raw: lib.mi_field_eval_points(k, _lib.ptr(pf.refresh()), f, _lib.ptr(x), 1, m, raw, stream),
             lambda f, raw, acts: lib.mi_field_eval_points_train(k, _lib.ptr(pf.refresh()), f, _lib.ptr(x), 1, m, raw, acts, stream))
    groups = 2 if L else 1
    n = N_RAYS * groups
    rays = rays_of(n, bool(L))
    near, far = (0.5, 1.5) if L else (2.0, 6.0)
    z = ops.sample_coarse(n, near, far, N_SAMPLES, DEV, synth.t_rand(n, N_SAMPLES, seed=9).to(DEV))
    both(f"{name} rays {groups}x{N_RAYS}x{N_SAMPLES}", groups, n * N_SAMPLES,
         lambda f, raw: lib.mi_field_eval_rays(k, _lib.ptr(pf.refresh()), f, _lib.ptr(rays), _lib.ptr(z), groups, N_RAYS, N_SAMPLES,
                                               raw, stream),
         lambda f, raw, acts: lib.mi_field_eval_rays_train(k, _lib.ptr(pf.refresh()), f, _lib.ptr(rays), _lib.ptr(z), groups, N_RAYS,
                                                           N_SAMPLES, raw, acts, stream))


def sigma_only_cases(name):
    """mi_render_rays with rgb_c = NULL and two different fields: the coarse pass is the sigma-only instance, windowed when it
    has more than one window of samples."""
    lib = _lib.load()
    pf_c, _ = packed(name, 5)
    pf_f, _ = packed(name, 6)
    for n, nc, nf in [(m, N_SAMPLES, 2) for m in POINTS + (N_RAYS,)] + [(33, 16, 4)]:
        rays, tr = rays_of(n, False), synth.t_rand(n, nc, seed=9).to(DEV)
        ws_bytes = lib.mi_render_workspace_bytes(n, nc, nf)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        outs = [None] + [torch.full(s, FILL, device=DEV) for s in ((n,), (n,), (n, 3), (n,), (n,))]
        zl, ul = ops.linspace_table(2.0, 6.0, nc, DEV), ops.linspace_table(0.0, 1.0, nf, DEV)
        _lib.check(lib.mi_render_rays(pf_c.kind, _lib.ptr(pf_c.refresh()), pf_f.kind, _lib.ptr(pf_f.refresh()), None, _lib.ptr(rays),
                                      1, n, 2.0, 6.0, nc, nf, _lib.ptr(zl), _lib.ptr(ul), _lib.ptr(tr), 0, 0,
                                      *[_lib.ptr(o) for o in outs], _lib.ptr(ws), ws_bytes, _lib.stream_ptr(DEV)), "mi_render_rays")
        for key, t in zip(("depth_c", "acc_c", "rgb_f", "depth_f", "acc_f"), outs[1:]):
            emit(f"{name} render sigma-only {n}x{nc}+{nf}", key, t)


def deferred_case(name):
    lib = _lib.load()
    pf, _ = packed(name, 5)
    n, s = N_RAYS, N_SAMPLES
    rays = rays_of(n, False)
    z = ops.sample_coarse(n, 2.0, 6.0, s, DEV, synth.t_rand(n, s, seed=9).to(DEV))
    nbytes = lib.mi_render_deferred_colour_extra_bytes(n, 1, s - 1)
    extra = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    raw = torch.full((n, s, 4), FILL, device=DEV)
    _lib.check(lib.mi_field_eval_rays_deferred(pf.kind, _lib.ptr(pf.refresh()), None, _lib.ptr(rays), _lib.ptr(z), 1, n, s,
                                               _lib.ptr(raw), _lib.ptr(extra), nbytes, _lib.stream_ptr(DEV)),
               "mi_field_eval_rays_deferred")
    emit(f"{name} deferred {n}x{s}", "raw", raw)


def list_cases(name):
    lib = _lib.load()
    pf, _ = packed(name, 5)
    n, s, k, stream = N_RAYS, N_SAMPLES, pf.kind, _lib.stream_ptr(DEV)
    rays = rays_of(n, False)
    z = ops.sample_coarse(n, 2.0, 6.0, s, DEV, synth.t_rand(n, s, seed=9).to(DEV))
    i = np.arange(4)
    dense = (i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2 == 0          # half of the 4^3 cells
    grid = occupancy.OccupancyGrid.from_dense(dense, (-4.0,) * 3, (4.0,) * 3, DEV)
    d = (ctypes.c_int * 3)(*grid.dims)
    lo = (ctypes.c_float * 3)(*[float(v) for v in grid.lo])
    inv = (ctypes.c_float * 3)(*[float(v) for v in grid.inv_cell])
    case = f"{name} list {n}x{s}"
    for train in (False, True):
        lst = torch.full((lib.mi_occupancy_ordered_list_ints(n, s),), -1, dtype=torch.int32, device=DEV)
        count = torch.zeros(1, dtype=torch.int32, device=DEV)
        raw = torch.full((n, s, 4), FILL, device=DEV)
        _lib.check(lib.mi_occupancy_mark_rays_ordered(_lib.ptr(grid.bits), d, lo, inv, _lib.ptr(rays), _lib.ptr(z), n, s, _lib.ptr(lst),
                                                      _lib.ptr(count), _lib.ptr(raw), stream), "mi_occupancy_mark_rays_ordered")
        c = int(count.item())
        assert 0 < c < n * s, c
        if not train:
            emit(case, "list", lst[:c])
            _lib.check(lib.mi_field_eval_rays_list(k, _lib.ptr(pf.refresh()), _lib.ptr(rays), _lib.ptr(z), n, s, _lib.ptr(lst),
                                                   _lib.ptr(count), _lib.ptr(raw), stream), "mi_field_eval_rays_list")
            emit(case, "infer.raw", raw)
        else:
            acts = torch.full((lib.mi_field_train_acts_floats(k) * n * s,), FILL, device=DEV)
            _lib.check(lib.mi_field_eval_rays_list_train(k, _lib.ptr(pf.refresh()), _lib.ptr(rays), _lib.ptr(z), n, s, _lib.ptr(lst),
                                                         _lib.ptr(count), _lib.ptr(raw), _lib.ptr(acts), stream),
                       "mi_field_eval_rays_list_train")
            emit(case, "train.raw", raw)
            for key, t in regions(name, acts, n * s, c):
                emit(case, "train.saved." + key, t)


def main():
    with torch.no_grad():
        for name in FIXED + [G.depth_name(L, use_dir) for L, use_dir in DEPTHS]:
            field_cases(name)
        for name in SIGMA_KINDS:
            sigma_only_cases(name)
        for name in DEFER_KINDS:
            deferred_case(name)
        for name in SIGMA_KINDS:
            list_cases(name)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()

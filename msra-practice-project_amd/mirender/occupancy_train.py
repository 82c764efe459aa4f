"""Training with an occupancy grid: render_rays(..., grid=) with a graph to the two fields' parameters.

    from mirender import occupancy_train
    outs = occupancy_train.render_rays(rays, near, far, coarse, fine, 64, 128, grid=grid, seed=step)
    loss(outs).backward()

An opt-in surface, as mirender.pose is for ray gradients: render_core.render_rays(..., grid=) keeps refusing calls that need
gradients.  The rule is the inference rule (mirender.occupancy): a sample whose point lies in an unoccupied
cell, or outside the grid's box, has raw = 0 and is not evaluated - forward or backward.  A listed sample contributes to the
parameter gradients exactly what it contributes without a grid, an unlisted one nothing.

What that means for a training loop: A CELL THAT IS EMPTY IN THE GRID GETS NO GRADIENT AND CANNOT FILL UP UNTIL THE GRID IS
REBUILT.  Warm-up steps without a grid, the grid's `dilate` and the rebuild period are the caller's policy
(examples/train_nerf_occupancy.py shows one).

From C: mi_render_rays_occupancy_train / mi_render_rays_occupancy_backward (include/mi_render.h).  NeRF, SirenNeRF and
TinyNeRF fields; not built: FiLM kinds, generic callables, render_image_dist.  Gradients to the rays with a grid are
mirender.pose's: pose.render_rays(grid=) runs this module's forward and mi_render_rays_occupancy_backward_rays.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib, fields, ops, render_core


def _check_kept(ctx):
    """MI_DEBUG_GUARDS=1: the two buffers the forward keeps for the backward, after either call wrote or read them."""
    _lib.check_guard(ctx.ws_g, "occupancy training workspace (mi_render_occupancy_train_extra_bytes)")
    _lib.check_guard(ctx.saved_g, "occupancy training saved rows (mi_render_occupancy_train_saved_bytes)")


class _OccupancyRenderFn(torch.autograd.Function):
    """One call of the pair over n rays: forward keeps the workspace (z, raw, weights, the two lists and counts) and the
    compact saved rows; backward hands the six cotangents to mi_render_rays_occupancy_backward - to its _rays form, which also
    gives dL/d(rays), exactly when the rays the Function was applied to require grad (mirender.pose's calls: render_rays of
    this module detaches them)."""

    @staticmethod
    def forward(ctx, pf_c, pf_f, rays, near, far, nc, nf, grid, t_rand, seed, ray0, clip, *params):
        dev = pf_c.device
        n = rays.shape[0]
        # clip = (probes, pad): the bounds lie behind what the backward reads
        ws_bytes = ops._occupancy_workspace_bytes(True, clip, n, nc, nf)
        sv_bytes = _lib.query("mi_render_occupancy_train_saved_bytes", pf_c.kind, pf_f.kind, n, nc, nf)
        # owned by this call (not the shared inference workspace): the backward reads both
        ws, ctx.ws_g = _lib.guarded(ws_bytes, torch.uint8, dev)
        saved, ctx.saved_g = _lib.guarded(sv_bytes, torch.uint8, dev)
        outs, counts = ops._occupancy_forward(True, clip, pf_c, pf_f, rays, near, far, nc, nf, grid, t_rand, seed, ray0, ws,
                                              ws_bytes, saved)
        _check_kept(ctx)
        ctx.pf_c, ctx.pf_f, ctx.shared, ctx.n, ctx.nc, ctx.nf = pf_c, pf_f, pf_c is pf_f, n, nc, nf
        ctx.versions = fields.versions_of(pf_c, pf_f)
        ctx.rays, ctx.ws, ctx.saved, ctx.counts = rays, ws, saved, counts
        ctx.mark_non_differentiable(counts)
        return (*outs, counts)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_rgb_c, g_depth_c, g_acc_c, g_rgb_f, g_depth_f, g_acc_f, _g_counts=None):
        pf_c, pf_f, n, nc, nf = ctx.pf_c, ctx.pf_f, ctx.n, ctx.nc, ctx.nf
        fields.check_versions(ctx.versions, "render_rays backward", pf_c, pf_f)
        dev = pf_c.device
        # under once_differentiable the cotangents carry no graph, and a detach each is time on this step's clock
        gs = [_lib.f32c(g, dev, detach=False) for g in (g_rgb_c, g_depth_c, g_acc_c, g_rgb_f, g_depth_f, g_acc_f)]
        grads_c = [torch.empty_like(p) for p in pf_c.params]
        grads_f = None if ctx.shared else [torch.empty_like(p) for p in pf_f.params]
        bws_bytes = _lib.query("mi_render_occupancy_backward_workspace_bytes", pf_c.kind, pf_f.kind, int(ctx.shared), n, nc,
                               nf)
        bws, bws_g = _lib.guarded(bws_bytes, torch.uint8, dev)
        written = ctypes.c_int(0)
        g_rays, ray_args = None, ()
        if ctx.needs_input_grad[2]:
            # the _rays form: the same launches, plus the ray parts behind each composite and each field, which overwrite g_rays
            # in full; it takes the live parameters as mi_field_input_grad_rays does
            g_rays = torch.empty_like(ctx.rays)
            src_c, src_f = pf_c._sources(), None if ctx.shared else pf_f._sources()
            ray_args = (_lib.ptr_array(src_c), len(src_c), None if src_f is None else _lib.ptr_array(src_f),
                        0 if src_f is None else len(src_f), _lib.ptr(g_rays))
        _lib.call("mi_render_rays_occupancy_backward" + ("" if g_rays is None else "_rays"), dev, pf_c.kind,
                  _lib.ptr(pf_c.refresh_bwd()), pf_f.kind, None if ctx.shared else _lib.ptr(pf_f.refresh_bwd()), int(ctx.shared),
                  _lib.ptr(ctx.rays), n, nc, nf, _lib.ptr(ctx.ws), ctx.ws.numel(), _lib.ptr(ctx.saved), ctx.saved.numel(),
                  *[_lib.ptr(g) for g in gs], _lib.ptr_array(grads_c), None if grads_f is None else _lib.ptr_array(grads_f),
                  _lib.ptr(bws), bws_bytes, ctypes.byref(written), *ray_args)
        _check_kept(ctx)
        _lib.check_guard(bws_g, "occupancy backward workspace (mi_render_occupancy_backward_workspace_bytes)")
        gc = tuple(grads_c) if written.value & 1 else (None,) * len(grads_c)
        gf = () if ctx.shared else (tuple(grads_f) if written.value & 2 else (None,) * len(grads_f))
        return (None, None, g_rays) + (None,) * 9 + gc + gf


def _check(grid, pf_c, pf_f, rays, rays_may_need_grad=False):
    """What training with an occupancy grid is not built for (fields.refuse_grid_call) and, between its refusals, this
    module's own.  rays_may_need_grad: mirender.pose's call, which produces that gradient."""
    def own():
        if not rays_may_need_grad and _lib.wants_grad(rays):
            raise _lib.MiRenderError("occupancy_train.render_rays is not built for gradients to the rays (an opt-in of "
                                     "mirender.pose: pose.render_rays(grid=))")
        if grid is None:
            raise _lib.MiRenderError("occupancy_train.render_rays needs grid= (without one, call render_core.render_rays)")
    fields.refuse_grid_call("training", grid, pf_c, pf_f, own)


def render_rays(rays, near, far, coarse_model, fine_model, coarse_sample_num, fine_sample_num, *, grid, t_rand=None,
                seed=None, ray0=0, max_points=None, return_counts=False, clip_probes=None, clip_pad=1):
    """render_core.render_rays(..., grid=) with a graph to the two fields' parameters: (rgb_c, depth_c, acc_c, rgb_f, depth_f,
    acc_f); with return_counts=True (not part of render_core's signature: the example and the benchmark report it) also an
    int32 device tensor [calls, 2] of the samples each pass evaluated, under no_grad too.

    max_points: the rays are cut into consecutive calls of at most max_points // (2 Nc + Nf) rays (the samples a call
    evaluates at worst; its saved rows and workspaces are sized for them) and autograd sums the calls' gradients.  `ray0`
    keeps the seeded jitter keyed by the absolute ray index, so the cut does not change a sample.
    clip_probes (None: off), clip_pad: render_core.render_rays' keywords - each ray's range is first clipped to the grid and
    both passes sample inside it (mi_render_rays_occupancy_clip_train); the backward is the same call, it reads the depths.
    Under torch.no_grad() (or with no parameter that requires a gradient) this is render_core.render_rays(grid=).
    A cell that is empty in `grid` gets no gradient and cannot fill up until the caller rebuilds the grid.
    Not built: FiLM kinds, generic callables, render_image_dist; gradients to the rays: pose.render_rays(grid=)."""
    seed = render_core._call_seed(seed, t_rand, "occupancy_train.render_rays")
    pf_c, pf_f = fields.as_packed_field(coarse_model), fields.as_packed_field(fine_model)
    _check(grid, pf_c, pf_f, rays)
    dev = pf_c.device
    nc, nf = int(coarse_sample_num), int(fine_sample_num)
    if not fields.needs_graph(None, pf_c, pf_f):
        with torch.no_grad():                       # one call, so counts is [1, 2] ([0, 2] without rays)
            return render_core._render_rays(rays, near, far, coarse_model, fine_model, nc, nf, t_rand=t_rand, seed=seed,
                                            ray0=ray0, grid=grid, return_counts=return_counts, clip_probes=clip_probes,
                                            clip_pad=clip_pad)
    rays = ops._f32c(torch.as_tensor(rays), dev).reshape(-1, 2, 3)
    if rays.shape[0] == 0:                          # no rays: render_core's empty outputs, hanging off the parameters
        outs = render_core.render_rays(rays, near, far, coarse_model, fine_model, nc, nf, t_rand=t_rand, seed=seed, ray0=ray0)
        return (outs, torch.zeros((0, 2), dtype=torch.int32, device=dev)) if return_counts else outs
    outs, counts = _render_calls(pf_c, pf_f, rays, near, far, nc, nf, grid, t_rand, seed, ray0, max_points,
                                 clip_probes, clip_pad)
    return (outs, counts) if return_counts else outs


def _render_calls(pf_c, pf_f, rays, near, far, nc, nf, grid, t_rand, seed, ray0, max_points, clip_probes, clip_pad):
    """The calls of one render_rays over rays [n,2,3] (n > 0, fp32 on the fields' device): consecutive slices of at most
    max_points // (2 Nc + Nf) rays through _OccupancyRenderFn (whose backward reaches the rays when they require grad:
    mirender.pose's call): (the six outputs, the counts [calls, 2])."""
    dev = pf_c.device
    n = rays.shape[0]
    seed = render_core._call_seed(seed, t_rand)              # render_rays / pose.render_rays resolved it on entry: then as given
    t_rand = ops._t_rand(t_rand, n, nc, dev)
    params = fields.pair_params(pf_c, pf_f)
    clip = None if clip_probes is None else (int(clip_probes), int(clip_pad))
    step = n if not max_points else max(1, int(max_points) // (2 * nc + nf))
    pieces, counts = [], []
    for r0 in range(0, n, max(step, 1)):
        r1 = min(n, r0 + step)
        res = _OccupancyRenderFn.apply(pf_c, pf_f, rays[r0:r1].contiguous(), float(near), float(far), nc, nf, grid,
                       None if t_rand is None else t_rand[r0:r1].contiguous(), int(seed or 0), int(ray0) + r0, clip, *params)
        pieces.append(res[:6])
        counts.append(res[6])
    outs = pieces[0] if len(pieces) == 1 else tuple(torch.cat([p[k] for p in pieces]) for k in range(6))
    return outs, torch.stack(counts)

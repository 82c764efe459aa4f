"""Gradients to rays: opt-in camera pose refinement on the fused path.

The reference's renderer is plain torch, so `pts = o + d z`, `view = d / |d|` and `dists * |d|` (nerf/render.py:93,122,
134,143) carry a gradient back to `rays`, and from there to a camera pose - what pose refinement, calibration and the
inversion of an image with unknown pose differentiate.  The drop-in functions (render_core.render_rays, raw_to_outputs,
run_network, autograd.composite / field_eval_*) keep refusing geometric inputs that require grad: on the reference's own
training path nothing asks for that gradient, and producing it costs an extra pass over the per-layer gradient rows.  A
script that wants it says so by calling this module instead:

    rays = pose.get_rays(W, H, focal, c2w)                     # c2w: device tensor [3,4] | [4,4], may require grad
    outs = pose.render_rays(rays, near, far, coarse, fine, Nc, Nf, seed=0)
    loss(outs).backward()                                       # c2w.grad, and the parameters' gradients as ever

Outputs, parameter gradients and FiLM-table gradients are the bits render_core.render_rays gives; the gradient to the rays
comes from mi_composite_bwd_rays and mi_field_input_grad_rays (csrc/ray_grad.hip), range by range inside the same backward.
The depths carry no gradient to the rays: the stratified ones do not depend on them, the resampled ones are detached
(render.py:141) and the sort only permutes.

With an occupancy grid (`grid=`, optionally `clip_probes=`; NeRF, SirenNeRF and TinyNeRF fields): the forward is
occupancy_train's, the backward mi_render_rays_occupancy_backward_rays.  The rule: an unlisted sample's raw
is the constant 0 and sends the rays nothing; a listed sample sends them exactly what it sends without a grid; occupancy and
the clipped bounds are piecewise constant in the rays and carry no gradient.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib, autograd, fields, occupancy_train, ops, render_core


class _GetRaysFn(torch.autograd.Function):
    """get_rays (nerf/render.py:7-23): rays_d = dirs . R^T, rays_o = t.  Forward mi_gen_rays; backward to c2w."""

    @staticmethod
    def forward(ctx, c2w, width, height, focal, ray0, n):
        ctx.geom = (width, height, focal, ray0, n)
        ctx.c2w_shape, ctx.c2w_dtype = tuple(c2w.shape), c2w.dtype
        return ops.gen_rays(width, height, focal, c2w.detach().cpu().numpy(), c2w.device, ray0, n)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_rays):
        width, height, focal, ray0, n = ctx.geom
        dev = g_rays.device
        k = torch.arange(ray0, ray0 + n, device=dev)
        px, py = (k % width).to(torch.float32), (k // width).to(torch.float32)
        dirs = torch.stack([(px - width * 0.5) / float(focal), -(py - height * 0.5) / float(focal), -torch.ones_like(px)], -1)
        g = g_rays.to(torch.float64)
        g_c2w = torch.zeros(ctx.c2w_shape, dtype=torch.float64, device=dev)
        g_c2w[:3, :3] = g[:, 1].t() @ dirs.to(torch.float64)          # g_R[r][c] = sum_rays g_d[r] dirs[c]
        g_c2w[:3, 3] = g[:, 0].sum(0)                                   # g_t = sum_rays g_o
        return g_c2w.to(ctx.c2w_dtype), None, None, None, None, None


def get_rays(width, height, focal, c2w, *, ray0: int = 0, n: int | None = None) -> torch.Tensor:
    """Rays [n,2,3] of a pinhole camera in render_image's flattened order, the bits of ops.gen_rays, with a graph to
    `c2w` (a device tensor [3,4] or [4,4]).  `ray0` / `n` select a range of the frame's rays.  `focal` gets no gradient."""
    if not isinstance(c2w, torch.Tensor) or not c2w.is_cuda:
        raise _lib.MiRenderError("pose.get_rays needs c2w as a tensor on a ROCm device (the pose being refined)")
    if c2w.dim() != 2 or c2w.shape[1] != 4 or c2w.shape[0] not in (3, 4):
        raise _lib.MiRenderError(f"pose.get_rays: c2w must be [3,4] or [4,4], got {tuple(c2w.shape)}")
    width, height = int(width), int(height)
    n = width * height - int(ray0) if n is None else int(n)
    if isinstance(focal, torch.Tensor):
        focal = float(focal)
    return _GetRaysFn.apply(c2w, width, height, focal, int(ray0), n)


def _fused_pair(coarse_model, fine_model, what: str):
    pf_c, pf_f = fields.as_packed_field(coarse_model), fields.as_packed_field(fine_model)
    if pf_c is None or pf_f is None:
        raise _lib.MiRenderError(
            f"{what} differentiates through the fused field kernels and needs both models to be fused kinds; for any other "
            "callable use render_core.render_rays (the generic path), whose own torch ops already carry the gradient to the rays")
    return pf_c, pf_f


def _not_wanted(rays, render, *args, **kw):
    """The prelude of both forms of render_rays: rays whose gradient nobody asks for (or none at all) go, detached, to the
    module this one extends - `render`'s outputs then; None when the graph is to reach the rays."""
    if _lib.wants_grad(rays) and rays.numel():
        return None
    return render(rays.detach() if isinstance(rays, torch.Tensor) else rays, *args, **kw)


def _render_rays_grid(rays, near, far, coarse_model, fine_model, nc, nf, grid, t_rand, seed, film, ray0, clip_probes, clip_pad,
                      max_points):
    """render_rays with a grid: occupancy_train's checks but the one on the rays, and its calls on rays that keep their graph,
    whose backward is then the _rays form."""
    if film is not None:
        raise _lib.MiRenderError("pose.render_rays: film= with grid= is not built (training with an occupancy grid is not "
                                 "built for FiLM kinds)")
    pf_c, pf_f = fields.as_packed_field(coarse_model), fields.as_packed_field(fine_model)
    occupancy_train._check(grid, pf_c, pf_f, rays, rays_may_need_grad=True)
    outs = _not_wanted(rays, occupancy_train.render_rays, near, far, coarse_model, fine_model, nc, nf, grid=grid, t_rand=t_rand,
                       seed=seed, ray0=ray0, max_points=max_points, clip_probes=clip_probes, clip_pad=clip_pad)
    if outs is not None:
        return outs
    rays = _lib.f32c(rays, pf_c.device, detach=False).reshape(-1, 2, 3)
    return occupancy_train._render_calls(pf_c, pf_f, rays, near, far, nc, nf, grid, None if t_rand is None else t_rand.detach(),
                                         seed, ray0, max_points, clip_probes, clip_pad)[0]


def render_rays(rays, near, far, coarse_model, fine_model, coarse_sample_num, fine_sample_num, *,
                t_rand=None, seed=None, film=None, ray0=0, grid=None, clip_probes=None, clip_pad=1, max_points=None):
    """render_core.render_rays (same arguments, same six outputs bit for bit, same gradients to the parameters and the
    FiLM table) whose graph additionally reaches `rays` [N,2,3].

    grid= (an OccupancyGrid; clip_probes / clip_pad / max_points as occupancy_train.render_rays takes them): the outputs and
    parameter gradients of occupancy_train.render_rays, and the gradient to the rays under the same rule - only the samples in
    occupied cells send one.  NeRF, SirenNeRF and TinyNeRF fields; film= is refused.  The calls that max_points cuts the rays
    into are disjoint ray slices, so the cut changes no bit of rays.grad."""
    seed = render_core._call_seed(seed, t_rand, "pose.render_rays")
    if grid is not None:
        return _render_rays_grid(rays, near, far, coarse_model, fine_model, int(coarse_sample_num), int(fine_sample_num), grid,
                                 t_rand, seed, film, ray0, clip_probes, clip_pad, max_points)
    if clip_probes is not None or max_points is not None:
        raise _lib.MiRenderError("pose.render_rays: clip_probes= and max_points= belong to grid= (there is no grid to clip to)")
    pf_c, pf_f = _fused_pair(coarse_model, fine_model, "pose.render_rays")
    outs = _not_wanted(rays, render_core.render_rays, near, far, coarse_model, fine_model, coarse_sample_num, fine_sample_num,
                       t_rand=t_rand, seed=seed, film=film, ray0=ray0)
    if outs is not None:
        return outs
    rays = _lib.f32c(rays, pf_c.device, detach=False).reshape(-1, 2, 3)
    film = fields.resolve_film(film, (pf_c, coarse_model), (pf_f, fine_model))
    # autograd.render_rays_train's call, but on rays that keep their graph: the backward then also gives dL/d(rays)
    return autograd._RenderRaysFn.apply(pf_c, pf_f, rays, float(near), float(far), int(coarse_sample_num),
                                        int(fine_sample_num), film, None if t_rand is None else t_rand.detach(), int(seed or 0),
                                        int(ray0), *fields.pair_params(pf_c, pf_f))


def render_image_tensor(width, height, focal, c2w, near, far, coarse_model, fine_model, coarse_sample_num,
                        fine_sample_num, chunk=None, *, t_rand=None, seed=None, grid=None, clip_probes=None, clip_pad=1):
    """render_core.render_image_tensor (rgb of the fine pass [H,W,3]) with a graph to `c2w`: get_rays and render_rays of
    this module over the frame's chunks, the jitter keyed by each chunk's first ray like render_core._render_image_device.
    grid= / clip_probes= / clip_pad=: render_rays' keywords, handed to every chunk."""
    seed = render_core._call_seed(seed, t_rand, "pose.render_image_tensor")
    width, height = int(width), int(height)
    total = width * height
    step = render_core.MAX_RAYS_PER_LAUNCH if not chunk else max(int(chunk), 2)
    parts = []
    for i in range(0, total, step):
        m = min(step, total - i)
        rays = get_rays(width, height, focal, c2w, ray0=i, n=m)
        outs = render_rays(rays, near, far, coarse_model, fine_model, coarse_sample_num, fine_sample_num,
                           t_rand=None if t_rand is None else t_rand[i:i + m], seed=seed, ray0=i, grid=grid,
                           clip_probes=clip_probes, clip_pad=clip_pad)
        parts.append(outs[3])
    return (parts[0] if len(parts) == 1 else torch.cat(parts)).reshape(height, width, 3)


def field_eval_points(pf_or_module, x, film=None):
    """network(x [M,6]) -> [M,4] (nerf/render.py:73) on the fused kernels with a gradient to x as well as to the
    parameters and the FiLM table.  `pf_or_module`: a fused module or its PackedField."""
    pf = fields.as_packed_field(pf_or_module)
    if pf is None:
        raise _lib.MiRenderError("pose.field_eval_points needs a fused field kind; any other module differentiates through "
                                 "its own forward")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != 6:
        raise _lib.MiRenderError(f"expected inputs [M,6], got {tuple(getattr(x, 'shape', ()))}")
    film = fields.resolve_film(film, (pf, pf_or_module))
    if not _lib.wants_grad(x) or x.shape[0] == 0:
        return autograd.field_eval_points(pf, x.detach(), film)
    # autograd.field_eval_points' call, but on points that keep their graph: the backward then also gives dL/dx
    return autograd._FieldFn.apply(pf, _lib.f32c(x, pf.device, detach=False), None, film, *pf.params).reshape(-1, 4)

"""Stage-level wrappers over the C ABI (one function per reference stage).

Every function takes/returns torch tensors on a ROCm device and launches on the calling
thread's current stream; nothing here computes in PyTorch.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from . import _lib
from ._lib import f32c as _f32c, ptr as _p
from .fields import PackedField, film_groups, is_film


@functools.lru_cache(maxsize=64)
def _linspace_table(start: float, end: float, steps: int, device_str: str):
    """torch.linspace evaluated on the CPU (as the reference's CPU path does: render.py:35,123) and
    uploaded once, so depths match the CPU oracle bit for bit."""
    # device="cpu" explicitly: the reference scripts set the CUDA default tensor type (nerf/train_nerf.py:11), under
    # which a bare factory call would evaluate the table with the device's linspace instead
    return torch.linspace(start, end, steps=steps, dtype=torch.float32, device="cpu").to(device_str)


def linspace_table(start, end, steps, device):
    if steps <= 0:
        return None
    return _linspace_table(float(start), float(end), int(steps), str(device))


def _lin_tables(near, far, n_coarse, n_fine, device, exact_linspace=True):
    """(z_lin, u_lin): the coarse depths' and the inverse CDF's linspace tables, (None, None) when the kernels are to
    evaluate them."""
    if not exact_linspace:
        return None, None
    return linspace_table(near, far, n_coarse, device), linspace_table(0.0, 1.0, n_fine, device)


def _t_rand(t_rand, n, n_coarse, device):
    """The injected jitter as the library reads it, checked against the call's shape (None stays None)."""
    if t_rand is None:
        return None
    t_rand = _f32c(torch.as_tensor(t_rand), device)
    if tuple(t_rand.shape) != (n, n_coarse):
        raise _lib.MiRenderError(f"t_rand must be [{n},{n_coarse}]")
    return t_rand


def _render_outputs(n, device, coarse_outputs=True):
    """The six outputs of a render call (rgb, depth, acc of the coarse, then of the fine pass), None in the coarse slots
    when they are not wanted."""
    return [torch.empty(s, dtype=torch.float32, device=device) if coarse_outputs or k >= 3 else None
            for k, s in enumerate(((n, 3), (n,), (n,), (n, 3), (n,), (n,)))]


def gen_rays(width: int, height: int, focal, c2w, device, ray0: int = 0, n: int | None = None) -> torch.Tensor:
    """get_rays (nerf/render.py:7-23) generated on the device in render_image's flattened order
    (render.py:151-154).  Returns rays [n,2,3]."""
    n = width * height - ray0 if n is None else n
    c2w = np.ascontiguousarray(np.asarray(c2w)[:3, :4], dtype=np.float32)
    # NumPy >= 2 promotion: an np.float64 focal promotes the whole expression to fp64 (pi_GAN/modules.py:127),
    # a Python float keeps it fp32 (nerf/show_nerf.py:16)
    f64 = isinstance(focal, np.floating) and np.dtype(type(focal)) == np.float64
    rays = torch.empty((n, 2, 3), dtype=torch.float32, device=device)
    _lib.call("mi_gen_rays", device, int(width), int(height), float(focal),
              c2w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), int(ray0), int(n), _p(rays), int(f64))
    return rays


def sample_coarse(n: int, near: float, far: float, n_coarse: int, device, t_rand=None, seed: int = 0,
                  exact_linspace: bool = True, ray0: int = 0) -> torch.Tensor:
    """Stratified depths z[n,Nc] (render.py:123-132).  t_rand[n,Nc] injects the jitter; otherwise an
    in-kernel Philox stream keyed by (``seed``, ``ray0`` + ray index, sample) is used, ``ray0`` being the index of
    the first ray in the caller's full ray list (so the jitter of a frame does not depend on how it is split)."""
    z = torch.empty((n, n_coarse), dtype=torch.float32, device=device)
    t_rand = _t_rand(t_rand, n, n_coarse, device)
    zl = linspace_table(near, far, n_coarse, device) if exact_linspace else None
    _lib.call("mi_sample_coarse", device, n, float(near), float(far), n_coarse, _p(zl), _p(t_rand), _lib.seed64(seed),
              int(ray0), _p(z))
    return z


def composite(raw: torch.Tensor, z: torch.Tensor, rays: torch.Tensor, want_weights: bool = True):
    """raw_to_outputs (render.py:78-103): returns rgb[n,3], depth[n], acc[n], weights[n,S]|None."""
    dev = raw.device
    n, s = z.shape
    raw, z, rays = _f32c(raw, dev), _f32c(z, dev), _f32c(rays, dev)
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    depth = torch.empty((n,), dtype=torch.float32, device=dev)
    acc = torch.empty((n,), dtype=torch.float32, device=dev)
    w = torch.empty((n, s), dtype=torch.float32, device=dev) if want_weights else None
    _lib.call("mi_composite", dev, n, s, _p(raw), _p(z), _p(rays), _p(rgb), _p(depth), _p(acc), _p(w))
    return rgb, depth, acc, w


def sample_fine(z_coarse: torch.Tensor, weights: torch.Tensor, near: float, far: float, n_fine: int,
                want_samples: bool = False, exact_linspace: bool = True):
    """sample_pdf(mids, weights[...,1:-1], Nf) + detach + sort(cat) (render.py:140-142).
    Returns z_fine[n,Nc+Nf] (and z_samples[n,Nf] when asked)."""
    dev = z_coarse.device
    n, nc = z_coarse.shape
    z_coarse, weights = _f32c(z_coarse, dev), _f32c(weights, dev)
    z_fine = torch.empty((n, nc + n_fine), dtype=torch.float32, device=dev)
    zs = torch.empty((n, n_fine), dtype=torch.float32, device=dev) if want_samples else None
    zl, ul = _lin_tables(near, far, nc, n_fine, dev, exact_linspace)
    _lib.call("mi_sample_fine", dev, n, float(near), float(far), nc, n_fine, _p(zl), _p(ul), _p(z_coarse), _p(weights),
              _p(zs), _p(z_fine))
    return (z_fine, zs) if want_samples else z_fine


def sample_fine_pos(z_coarse: torch.Tensor, weights: torch.Tensor, near: float, far: float, n_fine: int,
                    exact_linspace: bool = True):
    """sample_fine that also says where every input went: (z_fine [n,Nc+Nf], z_samples [n,Nf], pos [n,Nc+Nf] int32 with
    pos[e] = index in z_fine of z_coarse[e] (e < Nc) or z_samples[e - Nc]).  For one field shared by both passes."""
    dev = z_coarse.device
    n, nc = z_coarse.shape
    z_coarse, weights = _f32c(z_coarse, dev), _f32c(weights, dev)
    z_fine = torch.empty((n, nc + n_fine), dtype=torch.float32, device=dev)
    zs = torch.empty((n, n_fine), dtype=torch.float32, device=dev)
    pos = torch.empty((n, nc + n_fine), dtype=torch.int32, device=dev)
    zl, ul = _lin_tables(near, far, nc, n_fine, dev, exact_linspace)
    _lib.call("mi_sample_fine_pos", dev, n, float(near), float(far), nc, n_fine, _p(zl), _p(ul), _p(z_coarse),
              _p(weights), _p(zs), _p(z_fine), _p(pos))
    return z_fine, zs, pos


def occupancy_clip_rays(grid, rays: torch.Tensor, near: float, far: float, probes: int, pad: int = 1) -> torch.Tensor:
    """Each ray's sampling range clipped to `grid` (mi_occupancy_clip_rays): bounds [n,2] = (near_r, far_r).  `probes` probes at
    the midpoints of equal bins of [near, far] are tested like samples of a pass; the range runs from `pad` bins in front of the
    first occupied probe to `pad` bins behind the last one, clamped to [near, far]; a ray without an occupied probe keeps
    (near, far).  A structure thinner than (far - near) / probes between two probes can be missed: a step of at most half a
    cell along the ray is a sound default, probes >= 2 (far - near) |d| max(inv_cell)."""
    dev = grid.device
    rays = _f32c(rays, dev).reshape(-1, 2, 3)
    n = rays.shape[0]
    bounds = torch.empty((n, 2), dtype=torch.float32, device=dev)
    _lib.call("mi_occupancy_clip_rays", dev, _p(grid.bits), *grid.c_args(), _p(rays), n, float(near), float(far), int(probes),
              int(pad), _p(bounds))
    return bounds


def sample_coarse_bounds(bounds: torch.Tensor, n_coarse: int, t_rand=None, seed: int = 0, ray0: int = 0) -> torch.Tensor:
    """sample_coarse over a range per ray, bounds [n,2] (mi_sample_coarse_bounds): the same arithmetic, the linspace of ray r
    evaluated in the kernel from bounds[r]."""
    dev = bounds.device
    bounds = _f32c(bounds, dev)
    n = bounds.shape[0]
    z = torch.empty((n, n_coarse), dtype=torch.float32, device=dev)
    t_rand = _t_rand(t_rand, n, n_coarse, dev)
    _lib.call("mi_sample_coarse_bounds", dev, n, _p(bounds), int(n_coarse), _p(t_rand), _lib.seed64(seed), int(ray0), _p(z))
    return z


def sample_fine_bounds(bounds: torch.Tensor, z_coarse: torch.Tensor, weights: torch.Tensor, n_fine: int, want_pos: bool = True,
                       exact_linspace: bool = True):
    """sample_fine_pos over a range per ray, bounds [n,2] (mi_sample_fine_bounds): (z_fine, z_samples, pos); with
    want_pos=False the two optional outputs are not written and z_fine alone comes back."""
    dev = z_coarse.device
    n, nc = z_coarse.shape
    bounds, z_coarse, weights = _f32c(bounds, dev), _f32c(z_coarse, dev), _f32c(weights, dev)
    z_fine = torch.empty((n, nc + n_fine), dtype=torch.float32, device=dev)
    zs = torch.empty((n, n_fine), dtype=torch.float32, device=dev) if want_pos else None
    pos = torch.empty((n, nc + n_fine), dtype=torch.int32, device=dev) if want_pos else None
    ul = linspace_table(0.0, 1.0, n_fine, dev) if exact_linspace else None
    _lib.call("mi_sample_fine_bounds", dev, n, _p(bounds), nc, int(n_fine), _p(ul), _p(z_coarse), _p(weights), _p(zs), _p(z_fine),
              _p(pos))
    return (z_fine, zs, pos) if want_pos else z_fine


def merge_raw(raw_c: torch.Tensor, raw_s: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """raw_fine [n,Nc+Nf,4] in sorted order from the coarse pass's raw [n,Nc,4] and the field at z_samples [n,Nf,4]."""
    dev = raw_c.device
    n, nc = raw_c.shape[0], raw_c.shape[1]
    nf = pos.shape[1] - nc
    raw_f = torch.empty((n, nc + nf, 4), dtype=torch.float32, device=dev)
    _lib.call("mi_merge_raw", dev, n, nc, nf, _p(raw_c), _p(raw_s) if nf else None, _p(pos), _p(raw_f))
    return raw_f


def split_grad(g_raw_f: torch.Tensor, pos: torch.Tensor, nc: int, g_raw_c: torch.Tensor | None = None):
    """The transpose of merge_raw: (g_raw_coarse [n,Nc,4] - added onto `g_raw_c` in place when given -, g_raw_samples
    [n,Nf,4])."""
    dev = g_raw_f.device
    n, s = pos.shape
    nf = s - nc
    acc = g_raw_c is not None
    if g_raw_c is None:
        g_raw_c = torch.empty((n, nc, 4), dtype=torch.float32, device=dev)
    g_s = torch.empty((n, nf, 4), dtype=torch.float32, device=dev)
    _lib.call("mi_split_grad", dev, n, nc, nf, _p(g_raw_f), _p(pos), _p(g_raw_c), int(acc), _p(g_s) if nf else None)
    return g_raw_c, g_s


def sample_pdf(bins: torch.Tensor, weights: torch.Tensor, n_samples: int) -> torch.Tensor:
    """sample_pdf(bins[n,nb], weights[n,nb-1], N) -> [n,N] (render.py:27-56), any bins."""
    dev = bins.device
    bins, weights = _f32c(bins, dev), _f32c(weights, dev)
    n, nb = bins.shape
    if tuple(weights.shape) != (n, nb - 1):
        raise _lib.MiRenderError("weights must be [n, len(bins)-1]")
    out = torch.empty((n, n_samples), dtype=torch.float32, device=dev)
    ul = linspace_table(0.0, 1.0, n_samples, dev)
    _lib.call("mi_sample_pdf", dev, n, nb, n_samples, _p(bins), _p(weights), _p(ul), _p(out))
    return out


def field_eval_rays(pf: PackedField, rays: torch.Tensor, z: torch.Tensor, film=None) -> torch.Tensor:
    """run_network on points o + d*z with view dirs d/|d| (render.py:122,134-135), fused.  raw[n,S,4]."""
    dev = pf.device
    rays, z = _f32c(rays, dev), _f32c(z, dev)
    n, s = z.shape
    film, groups, rpg = film_groups(pf, film, n)
    raw = torch.empty((n, s, 4), dtype=torch.float32, device=dev)
    _lib.call("mi_field_eval_rays", dev, pf.kind, _p(pf.refresh()), _p(film), _p(rays), _p(z), groups, rpg, s, _p(raw))
    return raw


class _Workspace:
    """Grow-only scratch for mi_render_rays (no allocation inside the library), one per (device, stream): launches
    on one stream are ordered, so they can share it; concurrent callers (DataParallel's thread per GPU,
    pi_GAN/train.py:50, or user threads on their own streams) never do.  Eager calls only: a call under stream capture
    neither reads nor fills this cache (_workspace), so no graph ever holds the address of a buffer kept here."""
    bufs: dict = {}

    @classmethod
    def release(cls, device=None):
        """Drop the scratch of `device` (all devices if None): it only grows otherwise (3.4 GB after an 800x800 frame).
        Safe at any time between calls, captured graphs included: a captured call's scratch is a buffer of the graph's own
        memory pool, not one of these, so dropping or growing the cache takes nothing from under a replay.  The next eager
        render_rays allocates what it needs."""
        want = None if device is None else cls._name(device)
        for key in [k for k in cls.bufs if want is None or k[0] == want]:
            del cls.bufs[key]

    @staticmethod
    def _name(device) -> str:
        """'cuda', 'cuda:0', torch.device('cuda'), 0 -> 'cuda:<index>' (the current device where none is given)."""
        d = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        return str(d)

    @classmethod
    def get(cls, device, nbytes):
        key = (cls._name(device), torch.cuda.current_stream(device).cuda_stream)
        b = cls.bufs.get(key)
        if b is None or b.numel() < nbytes:
            b = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            cls.bufs[key] = b
        return b


def _workspace(device, nbytes):
    """(workspace of at least `nbytes`, what _lib.check_guard takes after the call): the cached one of this (device,
    stream); with MI_DEBUG_GUARDS=1 a fresh one of exactly `nbytes` with a sentinel tail, so an overrun cannot hide in
    what an earlier, larger call left behind.
    Under stream capture: a fresh buffer of exactly `nbytes` that the cache never sees.  The graph's private pool owns it
    like any temporary of a captured torch op.  A cached buffer's address baked into a graph would be freed under the graph
    by the next larger call on the stream or by _Workspace.release(), and the following replay would write into memory the
    allocator has handed to someone else."""
    if _lib.guards_on():
        return _lib.guarded(nbytes, torch.uint8, device)
    if _lib.capturing():
        return torch.empty(int(nbytes), dtype=torch.uint8, device=device), None
    return _Workspace.get(device, nbytes), None


def render_rays_fused(pf_c: PackedField, pf_f: PackedField, rays: torch.Tensor, near: float, far: float,
                      n_coarse: int, n_fine: int, film=None, t_rand=None, seed: int = 0, exact_linspace: bool = True,
                      ray0: int = 0, coarse_outputs: bool = True):
    """render_rays (render.py:106-147) as one C-ABI call: six launches on the current stream.
    Returns the reference's 6-tuple.  coarse_outputs=False: the caller discards the coarse pass's outputs, which come back
    as None; with two different fields the library then runs the coarse field's sigma-only forward (mi_render_rays).
    The fine outputs are the same bits either way."""
    dev = pf_c.device
    rays = _f32c(rays, dev).reshape(-1, 2, 3)
    n = rays.shape[0]
    film, groups, rpg = film_groups(pf_c if is_film(pf_c.kind) else pf_f, film, n)
    t_rand = _t_rand(t_rand, n, n_coarse, dev)
    outs = _render_outputs(n, dev, coarse_outputs)
    ws_bytes = _lib.query("mi_render_workspace_bytes", n, n_coarse, n_fine)
    if pf_c is pf_f and n_fine > 0:
        # one field for both passes: with room for z_samples / their raw values / the merge positions the library evaluates
        # the Nf new depths only (mi_render_rays, include/mi_render.h); without it the plain path, same results
        ws_bytes += _lib.query("mi_render_shared_field_extra_bytes", n, n_coarse, n_fine)
    elif _lib.load().mi_field_has_deferred_colour(pf_f.kind) == 1:
        # two fields: with room for one chunk's live list the library runs the fine pass's colour branch on the points with
        # sigma > 0 only (0 bytes with Nf = 0); without it the whole forward, same results.  The list is min(n * S, 2^22)
        # rows of 1 028 bytes: 4.02 GiB from 21 846 rays of 192 samples on, kept with the workspace between calls
        ws_bytes += _lib.query("mi_render_deferred_colour_extra_bytes", n, n_coarse, n_fine)
    ws, ws_g = _workspace(dev, ws_bytes)
    zl, ul = _lin_tables(near, far, n_coarse, n_fine, dev, exact_linspace)
    _lib.call("mi_render_rays", dev, pf_c.kind, _p(pf_c.refresh()), pf_f.kind, _p(pf_f.refresh()), _p(film), _p(rays),
              groups, rpg, float(near), float(far), n_coarse, n_fine, _p(zl), _p(ul), _p(t_rand), _lib.seed64(seed),
              int(ray0), *[_p(o) for o in outs], _p(ws), ws_bytes)
    _lib.check_guard(ws_g, "mi_render_rays workspace (mi_render_workspace_bytes)")
    return tuple(outs)


def render_rays_occupancy(pf_c: PackedField, pf_f: PackedField, rays: torch.Tensor, near: float, far: float,
                          n_coarse: int, n_fine: int, grid, t_rand=None, seed: int = 0, ray0: int = 0,
                          coarse_outputs: bool = True, clip_probes=None, clip_pad: int = 1):
    """render_rays with an occupancy grid (mi_render_rays_occupancy): a sample whose point lies in an unoccupied cell of
    `grid` (mirender.occupancy.OccupancyGrid), or outside its box, counts as raw = 0 and is not evaluated; everything else is
    render_rays_fused.  Returns (the 6-tuple, counts): counts is a device int32 [2], the samples the coarse and the fine pass
    evaluated.  coarse_outputs=False: the coarse slots come back as None.
    clip_probes (None: today's call): every ray's sampling range is first clipped to the grid with that many probes and
    `clip_pad` bins of margin (occupancy_clip_rays), and both samplers place their depths inside it
    (mi_render_rays_occupancy_clip)."""
    dev = pf_c.device
    if is_film(pf_c.kind) or is_film(pf_f.kind):
        raise _lib.MiRenderError("rendering with an occupancy grid is not built for FiLM fields")
    rays = _f32c(rays, dev).reshape(-1, 2, 3)
    n = rays.shape[0]
    t_rand = _t_rand(t_rand, n, n_coarse, dev)
    clip = None if clip_probes is None else (int(clip_probes), int(clip_pad))
    ws_bytes = _occupancy_workspace_bytes(False, clip, n, n_coarse, n_fine)
    ws, ws_g = _workspace(dev, ws_bytes)
    outs, counts = _occupancy_forward(False, clip, pf_c, pf_f, rays, near, far, n_coarse, n_fine, grid, t_rand, seed, ray0, ws,
                                      ws_bytes, coarse_outputs=coarse_outputs)
    _lib.check_guard(ws_g, "mi_render_rays_occupancy workspace (mi_render_occupancy_extra_bytes)")
    return tuple(outs), counts


def _occupancy_workspace_bytes(train: bool, clip, n, n_coarse, n_fine) -> int:
    """Bytes of the workspace of a grid-driven forward: the render workspace, the lists of the inference or of the training
    call, and with `clip` the rays' bounds behind them (which the backward of a clipped training call reads past)."""
    extra = "mi_render_occupancy_train_extra_bytes" if train else "mi_render_occupancy_extra_bytes"
    nbytes = _lib.query("mi_render_workspace_bytes", n, n_coarse, n_fine) + _lib.query(extra, n, n_coarse, n_fine)
    if clip is not None:
        nbytes += _lib.query("mi_render_occupancy_clip_extra_bytes", n)
    return nbytes


def _occupancy_forward(train: bool, clip, pf_c, pf_f, rays, near, far, n_coarse, n_fine, grid, t_rand, seed, ray0, ws, ws_bytes,
                       saved=None, coarse_outputs=True):
    """The one call site of mi_render_rays_occupancy / _clip / _train / _clip_train: (the six outputs, counts int32 [2]).
    rays [n,2,3] and t_rand as the library reads them; clip: (probes, pad), which take z_lin's place, or None; ws of
    ws_bytes = _occupancy_workspace_bytes(train, clip, ...) and, with train, `saved` of mi_render_occupancy_train_saved_bytes:
    the caller's buffers, whose lifetime and guards stay the caller's."""
    dev = pf_c.device
    n = rays.shape[0]
    outs = _render_outputs(n, dev, coarse_outputs)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    zl, ul = _lin_tables(near, far, n_coarse, n_fine, dev)
    _lib.call("mi_render_rays_occupancy" + ("" if clip is None else "_clip") + ("_train" if train else ""), dev, pf_c.kind,
              _p(pf_c.refresh()), pf_f.kind, _p(pf_f.refresh()), _p(rays), n, float(near), float(far), n_coarse, n_fine,
              *((_p(zl),) if clip is None else clip), _p(ul), _p(t_rand), _lib.seed64(seed), int(ray0), _p(grid.bits),
              *grid.c_args(), *[_p(o) for o in outs], _p(counts), _p(ws), ws_bytes,
              *((_p(saved), saved.numel()) if train else ()))
    return outs, counts


def render_rays_occupancy_clip(pf_c: PackedField, pf_f: PackedField, rays: torch.Tensor, near: float, far: float, n_coarse: int,
                               n_fine: int, grid, probes: int, pad: int = 1, t_rand=None, seed: int = 0, ray0: int = 0,
                               coarse_outputs: bool = True):
    """mi_render_rays_occupancy_clip under its own name: render_rays_occupancy(..., clip_probes=probes, clip_pad=pad).  The
    training call, mi_render_rays_occupancy_clip_train, is mirender.occupancy_train.render_rays(..., clip_probes=)."""
    return render_rays_occupancy(pf_c, pf_f, rays, near, far, n_coarse, n_fine, grid, t_rand, seed, ray0, coarse_outputs,
                                 clip_probes=int(probes), clip_pad=pad)

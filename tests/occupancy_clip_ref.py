"""Clipping each ray's sampling range to an occupancy grid: the rule restated in numpy / torch fp32 on the CPU (IEEE, every
operation rounded on its own), shared by tests/test_occupancy_clip_host.py (which counts cases by hand and plants the mistakes
the comparison must reject) and tests/test_gpu_occupancy_clip.py (which holds the kernel and every layer above it to it).

The rule (include/mi_render.h "clipping"): M probes per ray at the midpoints of M equal bins of [near, far],
h = (far - near) / float(M), t_k = near + (float(k) + 0.5f) * h, the probe's point p = o + d * t_k and its occupancy exactly
as the mark rule has them (tests/occupancy_render_ref.py).  With k0 / k1 the least / greatest occupied probe,
a = max(k0 - pad, 0), b = min(k1 + 1 + pad, M), near_r = near + float(a) * h, far_r = far if b == M else near + float(b) * h;
a ray without an occupied probe keeps (near, far).

With per-ray bounds the two samplers keep their arithmetic; only their linspace is linspace_at(near_r, far_r, Nc, i), the
in-kernel ATen formula restated below.  The fine sampler itself is restated in tests/sampler_ref.py.
"""
import numpy as np
import torch

import occupancy_render_ref as ref
from oracle import render_ref as R, synth

F = np.float32

# planted mistakes (clip_bounds(plant=...)): what a wrong kernel would compute
PLANTS = ("k1_not_k1_plus_1", "probes_at_bin_edges", "pad_not_clamped", "hi_inclusive")


def probe_depths(near, far, probes, plant=None) -> np.ndarray:
    """float32 [M]: t_k = near + (float(k) + 0.5f) * h."""
    near, far = F(near), F(far)
    h = (far - near) / F(probes)
    k = np.arange(probes, dtype=np.float32)
    if plant == "probes_at_bin_edges":
        return (near + k * h).astype(np.float32)
    return (near + (k + F(0.5)) * h).astype(np.float32)


def _occupied_hi_inclusive(p, lo, inv_cell, dense):
    """The planted inside test 0 <= t <= G (the cell clamped into the grid)."""
    dense = torch.from_numpy(np.ascontiguousarray(np.asarray(dense, dtype=bool)))
    dims = torch.tensor(dense.shape)
    t = (p - torch.from_numpy(np.asarray(lo, F).reshape(3))) * torch.from_numpy(np.asarray(inv_cell, F).reshape(3))
    inside = ((t >= 0) & (t <= dims.to(torch.float32))).all(-1)
    c = torch.minimum(torch.floor(torch.nan_to_num(t)).to(torch.int64).clamp(min=0), dims - 1)
    return inside & dense[c[..., 0], c[..., 1], c[..., 2]]


def probe_mask(rays, near, far, lo, inv_cell, dense, probes, plant=None) -> np.ndarray:
    """bool [n,M]: which probes are occupied."""
    rays = torch.as_tensor(rays).detach().cpu().to(torch.float32).reshape(-1, 2, 3)
    t = torch.from_numpy(probe_depths(near, far, probes, plant))[None, :].expand(rays.shape[0], -1).contiguous()
    if plant == "hi_inclusive":
        return _occupied_hi_inclusive(ref.points(rays, t), lo, inv_cell, dense).numpy()
    return ref.occupied_mask(rays, t, lo, inv_cell, dense).numpy()


def first_last(mask: np.ndarray):
    """(k0, k1, hit) per ray: the least and greatest occupied probe (0 where none is), and whether any is."""
    m = mask.shape[1]
    hit = mask.any(1)
    k0 = np.argmax(mask, 1)
    k1 = m - 1 - np.argmax(mask[:, ::-1], 1)
    return np.where(hit, k0, 0), np.where(hit, k1, 0), hit


def bounds_from(k0, k1, hit, near, far, probes, pad, plant=None) -> np.ndarray:
    near, far = F(near), F(far)
    h = (far - near) / F(probes)
    a, b = k0 - pad, k1 + 1 + pad
    if plant == "k1_not_k1_plus_1":
        b = k1 + pad
    if plant != "pad_not_clamped":
        a, b = np.maximum(a, 0), np.minimum(b, probes)
    near_r = (near + a.astype(np.float32) * h).astype(np.float32)
    far_r = np.where(b == probes, far, (near + b.astype(np.float32) * h).astype(np.float32)).astype(np.float32)
    out = np.stack([np.where(hit, near_r, near), np.where(hit, far_r, far)], 1).astype(np.float32)
    return out


def clip_bounds(rays, near, far, lo, inv_cell, dense, probes, pad, plant=None) -> np.ndarray:
    """float32 [n,2]: (near_r, far_r) of every ray."""
    k0, k1, hit = first_last(probe_mask(rays, near, far, lo, inv_cell, dense, probes, plant))
    return bounds_from(k0, k1, hit, near, far, probes, pad, plant)


# ---- the samplers with bounds -------------------------------------------------------------------------------------------------
def linspace_at(start, end, steps: int) -> np.ndarray:
    """float32 [n,steps]: linspace(start[r], end[r], steps) by ATen's scalar formula (symmetric halves), start / end float32 [n]."""
    start, end = np.asarray(start, F).reshape(-1, 1), np.asarray(end, F).reshape(-1, 1)
    if steps <= 1:
        return np.repeat(start, max(steps, 0), 1)
    step = ((end - start) / F(steps - 1)).astype(np.float32)
    i = np.arange(steps)
    front = (start + step * i.astype(np.float32)[None, :]).astype(np.float32)
    back = (end - step * (steps - i - 1).astype(np.float32)[None, :]).astype(np.float32)
    return np.where((i < steps // 2)[None, :], front, back).astype(np.float32)


def sample_coarse_bounds(bounds, nc: int, t_rand) -> np.ndarray:
    """float32 [n,Nc]: sample_coarse's stratified depths over each ray's own linspace (render.py:123-132)."""
    b = np.asarray(bounds, F)
    lin = linspace_at(b[:, 0], b[:, 1], nc)
    mids = (F(0.5) * (lin[:, 1:] + lin[:, :-1])).astype(np.float32)
    lower = np.concatenate([lin[:, :1], mids], 1)
    upper = np.concatenate([mids, lin[:, -1:]], 1)
    u = np.asarray(torch.as_tensor(t_rand).cpu().numpy(), F)
    return (lower + (upper - lower).astype(np.float32) * u).astype(np.float32)


def sample_fine_bounds(bounds, z_coarse, weights, nf: int):
    """(z_samples [n,Nf], z_fine [n,Nc+Nf]) torch fp32: sample_pdf over each ray's own bin mids, then sort(cat)
    (render.py:140-142), as tests/sampler_ref.py restates the kernel bit for bit (u: the torch.linspace table mirender passes)."""
    import sampler_ref                                      # (it imports this module for linspace_at)
    u = torch.linspace(0.0, 1.0, nf).numpy() if nf else None                     # the u table mirender injects
    zs, zf, _ = sampler_ref.sample_fine_bounds(np.asarray(bounds, F), torch.as_tensor(z_coarse).cpu().float().numpy(),
                                               torch.as_tensor(weights).cpu().float().numpy(), nf, u)
    return torch.from_numpy(zs), torch.from_numpy(zf)


# ---- the inputs of tests/test_gpu_occupancy_clip.py, built here so that the host test can check them on the CPU ---------------
NEAR, FAR = 2.0, 6.0
BOX = ((-4.0,) * 3, (4.0,) * 3)              # holds every sample of the camera's rays (camera at radius 4, depths 2..6)
SMALL = ((-1.5,) * 3, (1.5,) * 3)            # a box the rays partly leave
CLIP_N = (1, 5, 37, 130)
CLIP_M = (1, 63, 64, 65, 192)
CLIP_PAD = (0, 1, 3)
CLIP_GRIDS = [("random", (5, 7, 3), BOX), ("random", (16, 16, 16), BOX), ("zeros", (16, 16, 16), BOX), ("ones", (5, 7, 3), BOX),
              ("ones", (16, 16, 16), SMALL), ("random", (16, 16, 16), SMALL), ("ones", (16, 16, 16), BOX)]


def case_dense(name: str, dims) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(31))
    if name == "zeros":
        return np.zeros(dims, bool)
    if name == "ones":
        return np.ones(dims, bool)
    return rng.random(dims) < 0.3


N_SPECIAL = 6


def case_rays(n: int) -> torch.Tensor:
    """n rays on the CPU.  From the seventh ray on, rays spread over a 40x40 view (focal 55) of the volume.  In front of them:
    ray 0      along +x with its probe 10 of 64 exactly on the face x = 4 of BOX (t_10 = 2 + 10.5 / 16, origin 4 - t_10: every
               term a dyadic rational, so the sum is exact): outside under `t < G`, inside under a planted `t <= G`;
    ray 1      a NaN direction;
    rays 2-4   pointing away from the volume (minus three times a view direction, from radius 4 outwards): they miss every grid;
    ray 5      along -z through the middle of SMALL."""
    cam = torch.from_numpy(R.rays_from_camera(40, 40, 55.0, synth.pose_degrees(4.0, 20.0, -30.0)))
    special = torch.zeros(N_SPECIAL, 2, 3)
    special[0, 0] = torch.tensor([4.0 - (2.0 + 10.5 / 16.0), 0.125, 0.125])
    special[0, 1] = torch.tensor([1.0, 0.0, 0.0])
    special[1, 0] = cam[0, 0]
    special[1, 1] = torch.tensor([float("nan"), 0.0, 1.0])
    for j, i in ((2, 0), (3, 799), (4, 1599)):
        special[j, 0] = cam[i, 0]
        special[j, 1] = -3.0 * cam[i, 1]
    special[5, 0] = torch.tensor([0.0625, 0.0625, 4.0])
    special[5, 1] = torch.tensor([0.0, 0.0, -1.0])
    m = max(n - N_SPECIAL, 0)
    idx = (torch.arange(m) * 1600 // max(m, 1) + 20) % 1600
    return torch.cat([special, cam[idx]])[:n].contiguous()


def clip_cases(n_values=CLIP_N):
    """Every (n, M, grid name, dims, box) of the kernel test; the pads are applied to each."""
    for n in n_values:
        for m in CLIP_M:
            for name, dims, box in CLIP_GRIDS:
                yield n, m, name, dims, box


def case_bounds(n, m, name, dims, box, pad, plant=None) -> np.ndarray:
    return clip_bounds(case_rays(n), NEAR, FAR, F(box[0]), ref.inv_cell_of(box[0], box[1], dims), case_dense(name, dims), m, pad,
                       plant)


# ---- the gradient cases of the clipped training pair: tests/occupancy_train_ref.py's cases at the clipped depths ---------------
CLIP_TRAIN_PROBES, CLIP_TRAIN_PAD = 32, 1


def train_case_bounds(case: str) -> np.ndarray:
    """The bounds of occupancy_train_ref.GRAD_CASES[case]'s rays under its grid."""
    import occupancy_train_ref as tref
    *_, gname, dims, box = tref.GRAD_CASES[case]
    return clip_bounds(tref.case_rays(), tref.NEAR, tref.FAR, F(box[0]), ref.inv_cell_of(box[0], box[1], dims),
                       tref.case_dense(gname, dims), CLIP_TRAIN_PROBES, CLIP_TRAIN_PAD)


def train_oracle_depths(case: str):
    """(z_c, mask_c, z_f, mask_f) of the case from the fp32 oracle alone, as occupancy_train_ref.oracle_depths has them,
    with the coarse depths and the bin mids taken over each ray's clipped range."""
    import occupancy_train_ref as tref
    from oracle import fields as ofields
    kind, _sc, _sf, _sharp, nc, nf, *_ = tref.GRAD_CASES[case]
    sd_c, _ = tref.case_state_dicts(case)
    rays = tref.case_rays()
    rd = rays[:, 1]
    b = train_case_bounds(case)
    z_c = torch.from_numpy(sample_coarse_bounds(b, nc, tref.case_t_rand(nc)))
    m_c = tref.case_mask(case, rays, z_c)
    with torch.no_grad():
        raw = R.query_field(R.points_on_rays(rays[:, 0], rd, z_c), rd / torch.norm(rd, dim=-1, keepdim=True),
                            ofields.make_field(kind, sd_c))
        raw = torch.where(m_c[..., None], raw, torch.zeros(()))
        w_c = R.composite(raw, z_c, rd)[3]
    _, z_f = sample_fine_bounds(b, z_c, w_c, nf)
    return z_c, m_c, z_f, tref.case_mask(case, rays, z_f)

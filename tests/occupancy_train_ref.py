"""Training with an occupancy grid: the reference gradients, on the CPU under torch autograd.

One pass of render_rays under the rule of DESIGN.md 4.8: the oracle field at every sample of the injected depths, then
`where(mask, raw, 0)` between the field and the composite (the mask is tests/occupancy_render_ref.py's restatement of "which
samples are occupied"), then the oracle composite, then the three cotangents of the pass.  A masked sample's raw is the
constant 0, so autograd sends it nothing: exactly the rule "an unlisted sample contributes nothing to any parameter gradient".
The resampled depths of the fine pass are detached in the reference (render.py:141), so each pass is differentiated alone,
from its own depths and cotangents.

Shared by tests/test_occupancy_train_host.py (which checks the reference and plants the mistakes the GPU gate must reject)
and tests/test_gpu_occupancy_train.py.
"""
import numpy as np
import torch

import occupancy_render_ref as ref
from oracle import fields as ofields, parity, render_ref as R, synth


def param_names(kind: str, sd: dict) -> list:
    """The state dict's keys in the order of the field's parameter list (weight, bias per layer)."""
    from mirender import fields
    kid = {v: k for k, v in fields.KIND_NAMES.items()}[kind]
    out = []
    for key, _ in fields.SPECS[kid]:
        out += [key + ".weight", key + ".bias"]
    assert sorted(out) == sorted(sd), (sorted(out), sorted(sd))
    return out


def pass_grads(kind: str, sd: dict, rays: torch.Tensor, z: torch.Tensor, mask, cot, dtype=torch.float64) -> dict:
    """{parameter name: gradient (float64)} of sum(rgb * cot[0]) + sum(depth * cot[1]) + sum(acc * cot[2]) for one pass over
    rays [n,2,3] at depths z [n,S] with the bool mask [n,S] (None: no grid); also "__outs__": (rgb, depth, acc)."""
    rays, z = rays.detach().cpu(), z.detach().cpu()
    req = {k: v.detach().cpu().clone().to(dtype).requires_grad_(True) for k, v in sd.items()}
    ro, rd = rays[:, 0].to(dtype), rays[:, 1].to(dtype)
    pts, view = R.points_on_rays(ro, rd, z.to(dtype)), rd / torch.norm(rd, dim=-1, keepdim=True)
    raw = R.query_field(pts, view, ofields.make_field(kind, req))
    if mask is not None:
        raw = torch.where(torch.as_tensor(mask).cpu()[..., None], raw, torch.zeros((), dtype=dtype))
    rgb, depth, acc, _ = R.composite(raw, z.to(dtype), rd)
    loss = (rgb * cot[0].cpu().to(dtype)).sum() + (depth * cot[1].cpu().to(dtype)).sum() + (acc * cot[2].cpu().to(dtype)).sum()
    loss.backward()
    out = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double() for k, v in req.items()}
    out["__outs__"] = (rgb.detach(), depth.detach(), acc.detach())
    return out


def shifted(mask: torch.Tensor) -> torch.Tensor:
    """A planted mistake: the mask moved by one sample along each ray (the first sample takes the last one's bit)."""
    return torch.roll(torch.as_tensor(mask), 1, dims=1)


# ---- the device rule of the counted weight-gradient kernels (DESIGN.md 4.8 "Training with a grid") -----------------------
def counted_slab_len(count: int, n_slabs: int) -> int:
    """Slab length the counted dW kernels derive on the device: the host plans n_slabs from the CAPACITY (bwd_gates.group_plan)
    and the device cuts the `count` rows it has into that many equal slabs of whole 32-point stages."""
    return ((count + n_slabs - 1) // n_slabs + 31) // 32 * 32


# ---- the gradient cases of tests/test_gpu_occupancy_train.py, built here so that the host test can put the same cases through
# the same gates on the CPU -------------------------------------------------------------------------------------------------
NEAR, FAR = 2.0, 6.0
BOX = ((-4.0,) * 3, (4.0,) * 3)              # holds every sample of the rays below (camera at radius 4, depths 2..6)
SMALL = ((-1.5,) * 3, (1.5,) * 3)            # a box the rays partly leave
BIG = ((-8.0,) * 3, (8.0,) * 3)
N_RAYS = 24
# name: (kind, coarse seed, fine seed (the same: one shared field), sigma head variant, Nc, Nf, grid, its dims, its box).
# The head variants are those tests/test_gpu_train.py gates with these tolerances (sharp = True / False); the seeds are kept
# only if the fp32 oracle under the mask stays inside the hard gates against its fp64 self (test_occupancy_train_host.py).
GRAD_CASES = {
    "nerf_random": ("nerf", 5, 6, True, 12, 24, "random", (16, 16, 16), BOX),
    "tiny_nerf_box": ("tiny_nerf", 5, 6, False, 5, 3, "ones", (16, 16, 16), SMALL),
    "siren_nerf_random": ("siren_nerf", 5, 6, True, 9, 5, "random", (16, 16, 16), BOX),
    "nerf_shared_random": ("nerf", 5, 5, False, 12, 24, "random", (16, 16, 16), BOX),
    "nerf_shared_ones": ("nerf", 5, 5, True, 12, 24, "ones", (4, 4, 4), BIG),
}


def case_rays(n: int = N_RAYS) -> torch.Tensor:
    """n rays spread over a 40x40 view (focal 55) of the volume, on the CPU."""
    r = torch.from_numpy(R.rays_from_camera(40, 40, 55.0, synth.pose_degrees(4.0, 20.0, -30.0)))
    idx = (torch.arange(n) * 1600 // n + 20) % 1600
    return r[idx].contiguous()


def case_dense(name: str, dims) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(31))
    if name == "zeros":
        return np.zeros(dims, bool)
    if name == "ones":
        return np.ones(dims, bool)
    return rng.random(dims) < 0.3


def case_cots(n: int = N_RAYS, seed: int = 4) -> list:
    """The six output cotangents (CPU)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(sh, generator=g) for sh in ((n, 3), (n,), (n,), (n, 3), (n,), (n,))]


def case_t_rand(nc: int, n: int = N_RAYS) -> torch.Tensor:
    return synth.t_rand(n, nc, seed=9)


def case_state_dicts(case: str):
    kind, sc, sf, sharp, *_ = GRAD_CASES[case]
    return tuple(synth.state_dict(kind, seed=s, sharp=sharp, bias_jitter=0.05) for s in (sc, sf))


def case_mask(case: str, rays, z):
    *_, gname, dims, box = GRAD_CASES[case]
    return ref.occupied_mask(rays, z, np.float32(box[0]), ref.inv_cell_of(box[0], box[1], dims), case_dense(gname, dims))


def oracle_depths(case: str):
    """(z_c, mask_c, z_f, mask_f) of the case from the fp32 oracle alone: render.py's sampling with the masked coarse raw."""
    kind, _sc, _sf, _sharp, nc, nf, *_ = GRAD_CASES[case]
    sd_c, _ = case_state_dicts(case)
    rays = case_rays()
    ro, rd = rays[:, 0], rays[:, 1]
    z_c, mids = R.stratified_z(rays.shape[0], NEAR, FAR, nc, case_t_rand(nc))
    m_c = case_mask(case, rays, z_c)
    with torch.no_grad():
        raw = R.query_field(R.points_on_rays(ro, rd, z_c), rd / torch.norm(rd, dim=-1, keepdim=True), ofields.make_field(kind, sd_c))
        raw = torch.where(m_c[..., None], raw, torch.zeros(()))
        w_c = R.composite(raw, z_c, rd)[3]
        z_f = z_c if nf == 0 else torch.sort(torch.cat([z_c, R.sample_pdf(mids, w_c[..., 1:-1], nf)], -1), -1).values
    return z_c, m_c, z_f, case_mask(case, rays, z_f)


def case_refs(case: str, z_c, m_c, z_f, m_f) -> dict:
    """{dtype: [per field {parameter name: gradient}]} of the case at the given depths and masks: the coarse pass from the
    first three cotangents, the fine pass from the last three; one shared field gets their sum."""
    kind, sc, sf, *_ = GRAD_CASES[case]
    sd_c, sd_f = case_state_dicts(case)
    rays, cots = case_rays(), case_cots()
    names = param_names(kind, sd_c)
    out = {}
    for dt in (torch.float32, torch.float64):
        rc = pass_grads(kind, sd_c, rays, z_c, m_c, cots[:3], dt)
        rf = pass_grads(kind, sd_f, rays, z_f, m_f, cots[3:], dt)
        out[dt] = [{k: rc[k] + rf[k] for k in names}] if sc == sf else [{k: rc[k] for k in names}, {k: rf[k] for k in names}]
    return out


def case_gates(kind: str) -> dict:
    smooth = kind == "siren_nerf"            # sin activations have no derivative switches
    return dict(tol=parity.GRAD_TOL_SMOOTH if smooth else parity.GRAD_TOL_RELU,
                elem_tol=parity.GRAD_ELEM_TOL_SMOOTH if smooth else None)

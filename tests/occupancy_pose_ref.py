"""Gradients to the rays with an occupancy grid: the reference, on the CPU under torch autograd, and the restatement of "a
ray's run in the ascending list" that csrc/ray_grad.hip's LIST instances search for on the device.

The rule (DESIGN.md 4.8 "Gradients to the rays"): an unlisted sample's raw is the constant 0 and sends the rays nothing through
the field; in the composite its sigma = 0 gives an exact 0 in dL/d|d|; a listed sample sends the rays what it sends without a
grid; the depths, occupancy and the clipped bounds carry no gradient.  Stated as autograd: R.points_on_rays -> field ->
where(mask, raw, 0) -> R.composite per pass at fixed depths, the two passes' gradients to the rays summed.

Shared by tests/test_occupancy_pose_host.py (the conditioning of the GPU cases and the planted mistakes) and
tests/test_gpu_occupancy_pose.py.
"""
import numpy as np
import torch

import occupancy_train_ref as tref
from oracle import fields as ofields, render_ref as R

PLANTS = ("mask_shifted", "z_at_entry", "no_composite_term")


# ---- a ray's run in the ascending list ---------------------------------------------------------------------------------------
def ray_runs(lst, count: int, n: int, S: int) -> np.ndarray:
    """int64 [n,2]: (e0, e1) of every ray - the entries e < count of the ascending list with r S <= list[e] < (r + 1) S are
    exactly e0 <= e < e1 (e0 = lower_bound(list[:count], r S), e1 = lower_bound(list[:count], (r + 1) S))."""
    head = np.asarray(lst, dtype=np.int64)[:count]
    edges = np.arange(n + 1, dtype=np.int64) * S
    e = np.searchsorted(head, edges, side="left")
    return np.stack([e[:-1], e[1:]], 1)


# ---- the reference gradient ----------------------------------------------------------------------------------------------------
def pass_ray_grad(kind: str, sd: dict, rays, z, mask, cot, dtype=torch.float64, plant=None) -> torch.Tensor:
    """dL/d(rays) [n,2,3] (dtype) of sum(rgb * cot[0]) + sum(depth * cot[1]) + sum(acc * cot[2]) for one pass over rays [n,2,3]
    at the fixed depths z [n,S] under the bool mask [n,S] (None: no grid).  plant: one of PLANTS, what a wrong kernel computes."""
    assert plant is None or plant in PLANTS, plant
    rays, z = rays.detach().cpu().to(dtype), z.detach().cpu().to(dtype)
    mask = None if mask is None else torch.as_tensor(mask).cpu()
    if plant == "mask_shifted":
        mask = tref.shifted(mask)
    rr = rays.clone().requires_grad_(True)
    ro, rd = rr[:, 0], rr[:, 1]
    pts = R.points_on_rays(ro, rd, z)
    pts.retain_grad()
    raw = R.query_field(pts, rd / torch.norm(rd, dim=-1, keepdim=True), ofields.make_field(kind, {k: v.to(dtype) for k, v in sd.items()}))
    if mask is not None:
        raw = torch.where(mask[..., None], raw, torch.zeros((), dtype=dtype))
    rgb, depth, acc, _ = R.composite(raw, z, rd.detach() if plant == "no_composite_term" else rd)
    loss = (rgb * cot[0].cpu().to(dtype)).sum() + (depth * cot[1].cpu().to(dtype)).sum() + (acc * cot[2].cpu().to(dtype)).sum()
    loss.backward()
    g = rr.grad.clone()
    if plant == "z_at_entry":
        # the depth read at the ENTRY index e of the compact rows in place of the point index list[e]: only the z_s g_pos
        # term of g_d moves
        n, S = z.shape
        listed = torch.ones(n * S, dtype=torch.bool) if mask is None else mask.reshape(-1)
        lst = torch.nonzero(listed).reshape(-1)
        g_pos = pts.grad.reshape(-1, 3)[lst]
        right = torch.zeros(n, 3, dtype=dtype).index_add_(0, lst // S, z.reshape(-1)[lst][:, None] * g_pos)
        wrong = torch.zeros(n, 3, dtype=dtype).index_add_(0, lst // S, z.reshape(-1)[:lst.numel()][:, None] * g_pos)
        g[:, 1] += wrong - right
    return g


def case_ray_grads(case: str, z_c, m_c, z_f, m_f, plant=None) -> dict:
    """{dtype: dL/d(rays) [n,2,3]} of occupancy_train_ref.GRAD_CASES[case] at the given depths and masks: the coarse pass from
    the first three cotangents of tref.case_cots, the fine pass from the last three, summed."""
    kind = tref.GRAD_CASES[case][0]
    sd_c, sd_f = tref.case_state_dicts(case)
    rays, cots = tref.case_rays(), tref.case_cots()
    out = {}
    for dt in (torch.float32, torch.float64):
        out[dt] = (pass_ray_grad(kind, sd_c, rays, z_c, m_c, cots[:3], dt, plant)
                   + pass_ray_grad(kind, sd_f, rays, z_f, m_f, cots[3:], dt, plant))
    return out

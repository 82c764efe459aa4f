"""Rendering with an occupancy grid: the rule "which samples are occupied" restated in torch fp32 on the CPU (IEEE, nothing
fused), shared by tests/test_occupancy_render_host.py (which counts cases by hand) and tests/test_gpu_occupancy_render.py
(which holds the mark kernel, the list-driven forward and the whole render against it, bit for bit).

The point is the one the fused forward evaluates, p = o + d * z (a multiply, then an add); it is placed by
t = (p - lo) * inv_cell (a subtract, then a multiply), is inside iff 0 <= t < G on every axis (so a NaN is not inside), its
cell is floor(t), and the cell's bit in the dense bool [Gx,Gy,Gz] says whether it is occupied.
"""
import numpy as np
import torch


def inv_cell_of(lo, hi, dims) -> np.ndarray:
    """OccupancyGrid's three inv_cell floats: np.float32(dims) / (np.float32(hi) - np.float32(lo))."""
    return np.float32(dims) / (np.asarray(hi, np.float32).reshape(3) - np.asarray(lo, np.float32).reshape(3))


def points(rays: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """[n,S,3] sample points of rays [n,2,3] at depths z [n,S]."""
    rays, z = rays.detach().cpu().to(torch.float32), z.detach().cpu().to(torch.float32)
    return rays[:, None, 0, :] + rays[:, None, 1, :] * z[:, :, None]


def occupied_points(p: torch.Tensor, lo, inv_cell, dense) -> torch.Tensor:
    """bool [...] for points p [...,3] (CPU fp32): inside the box and in a cell whose bit is set."""
    dense = torch.from_numpy(np.ascontiguousarray(np.asarray(dense, dtype=bool)))
    dims = torch.tensor(dense.shape)
    t = (p - torch.from_numpy(np.asarray(lo, np.float32).reshape(3))) * torch.from_numpy(np.asarray(inv_cell, np.float32).reshape(3))
    inside = ((t >= 0) & (t < dims.to(torch.float32))).all(-1)
    c = torch.minimum(torch.floor(torch.nan_to_num(t)).to(torch.int64).clamp(min=0), dims - 1)    # any valid cell where outside
    return inside & dense[c[..., 0], c[..., 1], c[..., 2]]


def occupied_mask(rays, z, lo, inv_cell, dense) -> torch.Tensor:
    """bool [n,S] on the CPU: True = the sample is evaluated."""
    return occupied_points(points(rays, z), lo, inv_cell, dense)


def cells_of(p: torch.Tensor, lo, inv_cell, dims) -> torch.Tensor:
    """int64 [m,3] cells of the points p [m,3] that lie inside the box (the others are dropped)."""
    dims = torch.tensor(tuple(int(d) for d in dims))
    t = (p - torch.from_numpy(np.asarray(lo, np.float32).reshape(3))) * torch.from_numpy(np.asarray(inv_cell, np.float32).reshape(3))
    inside = ((t >= 0) & (t < dims.to(torch.float32))).all(-1)
    return torch.floor(t[inside]).to(torch.int64)

"""Mesh export on the device: marching cubes (csrc/mesh_stages.hip), the binary PLY writer, and drop-ins for
create_mesh / convert_sdf_samples_to_ply (pi_GAN/utils.py:42-180).  The -sigma grid never leaves the device; only the
final vertex and face arrays are copied to the host, to be written out."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .grid import density_grid

RANGE_ERROR = "Surface level must be within volume data range."
_ERANGE = -3          # MI_ERANGE in include/mi_render.h


def marching_cubes(volume, level: float = 0.0, spacing=(1.0, 1.0, 1.0), gradient_direction: str = "descent"):
    """skimage.measure.marching_cubes_lewiner(volume, level, spacing, gradient_direction) on the device.

    volume: [X, Y, Z] fp32 (a device tensor, a CPU tensor or an ndarray; CPU data is copied to cuda:0).  Returns
    device tensors (verts [V,3] f32 in the volume's axis order times `spacing`, faces [F,3] int32, normals [V,3] f32,
    values [V] f32).  allow_degenerate=True semantics only (degenerate triangles of ties are kept), step_size 1.
    Vertex positions and each cube's boundary are those of skimage; cubes whose interior Lewiner tunnels through a
    centre vertex are triangulated without one.  normals: the interpolated central-difference gradient,
    normalised, pointing toward lower values; values: max - min of the first cube holding the vertex's edge.
    Raises ValueError when `level` is outside [min, max] of the volume, as skimage does."""
    if gradient_direction not in ("descent", "ascent"):
        raise ValueError("Incorrect input %s in `gradient_direction`, see docstring." % (gradient_direction,))
    if isinstance(volume, np.ndarray):
        volume = torch.from_numpy(np.ascontiguousarray(volume, dtype=np.float32))
    if volume.ndim != 3:
        raise ValueError("Input volume should be a 3D numpy array.")
    if volume.device.type != "cuda":
        volume = volume.to("cuda")
    volume = volume.to(torch.float32).contiguous()
    nx, ny, nz = (int(s) for s in volume.shape)
    if min(nx, ny, nz) < 2:
        raise ValueError("Input array must be at least 2x2x2.")
    sp = (ctypes.c_double * 3)(*(float(s) for s in spacing))
    lib = _lib.load()
    dev = volume.device
    ws = torch.empty(_lib.query("mi_mc_workspace_bytes", nx, ny, nz), dtype=torch.uint8, device=dev)
    nv, nf = ctypes.c_int64(), ctypes.c_int64()
    # not _lib.call: one of this entry point's return codes is not an error of the library but skimage's ValueError
    with torch.cuda.device(dev):
        rc = lib.mi_marching_cubes_count(_lib.ptr(volume), nx, ny, nz, float(level), _lib.ptr(ws), ctypes.byref(nv),
                                         ctypes.byref(nf), _lib.stream_ptr(dev))
    if rc == _ERANGE:
        raise ValueError(RANGE_ERROR)
    _lib.check(rc, "mi_marching_cubes_count")
    verts = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
    values = torch.empty((nv.value,), dtype=torch.float32, device=dev)
    faces = torch.empty((nf.value, 3), dtype=torch.int32, device=dev)
    if nv.value:
        _lib.call("mi_marching_cubes_emit", dev, _lib.ptr(volume), nx, ny, nz, float(level), sp,
                  int(gradient_direction == "descent"), _lib.ptr(ws), _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(normals),
                  _lib.ptr(values))
    return verts, faces, normals, values


marching_cubes_lewiner = marching_cubes


def ply_bytes(verts, faces) -> bytes:
    """The file plyfile writes for create_mesh's two elements: vertex (float x, y, z) and face (list uchar int)."""
    v = np.ascontiguousarray(np.asarray(verts, dtype="<f4").reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(faces, dtype="<i4").reshape(-1, 3))
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    rows = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rows["n"] = 3
    rows["i"] = f
    return header + v.tobytes() + rows.tobytes()


def write_ply(path, verts, faces) -> None:
    """Binary little-endian PLY of a triangle mesh, byte for byte what plyfile writes for utils.py's elements."""
    if isinstance(verts, torch.Tensor):
        verts = verts.detach().cpu().numpy()
    if isinstance(faces, torch.Tensor):
        faces = faces.detach().cpu().numpy()
    with open(path, "wb") as fh:
        fh.write(ply_bytes(verts, faces))


def convert_sdf_samples_to_ply(sdf, voxel_grid_origin, voxel_size, ply_filename_out, offset=None, scale=None,
                               level=-20.0):
    """utils.py:109-180 on the device: marching cubes at `level` with spacing voxel_size, then origin + verts (no axis
    flip, as the reference), / scale, - offset, written as PLY.  No surface (the level outside the grid's range) gives
    an empty mesh, as the reference's bare `except: pass`.  Returns the written (verts [V,3], faces [F,3]) arrays."""
    try:
        verts, faces, _, _ = marching_cubes(sdf, level=level, spacing=[float(voxel_size)] * 3)
    except ValueError:
        verts = torch.zeros((0, 3), dtype=torch.float32)
        faces = torch.zeros((0, 3), dtype=torch.int32)
    pts = verts.detach().cpu().numpy().astype(np.float64)      # the reference does this arithmetic in float64
    pts = np.asarray(voxel_grid_origin, dtype=np.float64).reshape(1, 3) + pts
    if scale is not None:
        pts = pts / scale
    if offset is not None:
        pts = pts - offset
    pts = pts.astype(np.float32)
    faces_np = faces.detach().cpu().numpy()
    write_ply(ply_filename_out, pts, faces_np)
    return pts, faces_np


def create_mesh(generator, filename, N=256, max_batch=64 ** 3, offset=None, scale=None, level=-20.0, z=None):
    """utils.py:42-106: z ~ randn(1, input_dim) (unless given) -> FiLM table -> -sigma on the N^3 grid (device) ->
    marching cubes (device) -> `filename`.ply.  Returns (verts, faces) as written (the reference returns None)."""
    dev = next(generator.parameters()).device
    if z is None:
        z = torch.randn(1, generator.input_dim, device=dev)
    with torch.no_grad():
        film = generator.get_mapping(z.to(dev))
        generator.set_film_params(film[0])
        voxel_origin = [-0.1, -0.1, -0.1]
        voxel_size = 0.2 / (N - 1)
        sdf = density_grid(generator.film_siren_nerf, N, max_batch, voxel_origin, voxel_size)
        return convert_sdf_samples_to_ply(sdf, voxel_origin, voxel_size, filename + ".ply", offset, scale, level)

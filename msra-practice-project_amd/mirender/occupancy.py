"""Per-scene occupancy grids: one bit per cell of a box, saying which cells can hold density.

    grid = OccupancyGrid.from_field(fine_model, lo=(-1.5,) * 3, hi=(1.5,) * 3, resolution=128)
    grid.occupied_fraction(); grid.to_dense()
    rgb, depth, acc = render_image(W, H, focal, pose, near, far, coarse_model, fine_model, 64, 128, grid=grid)

`from_field` builds the grid on the device from a field's sigma (mi_occupancy_cell_points, the fused field kernel,
mi_occupancy_pack; include/mi_render.h), `from_dense` / `to_dense` go through bool [Gx,Gy,Gz] arrays in numpy.
For the kinds without FiLM (NeRF, SirenNeRF, TinyNeRF).  This module builds and holds grids; the renderer reads them through the
keyword `grid=` of render_rays / render_image / render_image_tensor / render_video (inference only): a sample whose point
o + d * z lies in an unoccupied cell, or outside [lo, hi), counts as raw = 0 and is not evaluated (ops.render_rays_occupancy,
mi_render_rays_occupancy).  A grid that misses cells where the field has density therefore changes the picture: build it with
a threshold, supersampling and dilation that suit the field.  With `clip_probes=` next to `grid=` the grid also places the
samples: each ray's range is clipped to its first and last occupied probe and both passes sample inside it
(ops.occupancy_clip_rays, mi_render_rays_occupancy_clip).  Training with a grid is the opt-in module
mirender.occupancy_train (render_rays(..., grid=) with a graph to the fields' parameters).  LiveOccupancyGrid keeps a grid current
while its field trains: a per-cell density on the device, updated a part at a time and re-thresholded into the bits in place.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, fields


def _i3(v):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(3))
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _f3(v):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(3))
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def pack_dense(dense) -> np.ndarray:
    """bool [Gx,Gy,Gz] -> uint32 words: cell (ix, iy, iz) is bit (ix * Gy + iy) * Gz + iz, in word index >> 5, bit index & 31."""
    flat = np.asarray(dense, dtype=bool).reshape(-1)
    padded = np.zeros((flat.size + 31) // 32 * 32, dtype=np.uint8)
    padded[:flat.size] = flat
    return np.packbits(padded.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).copy()


def unpack_dense(words, dims) -> np.ndarray:
    """The inverse of pack_dense: bool [Gx,Gy,Gz]."""
    dims = tuple(int(d) for d in dims)
    cells = dims[0] * dims[1] * dims[2]
    w = np.ascontiguousarray(np.asarray(words).astype("<u4")).view(np.uint8).reshape(-1, 4)
    return np.unpackbits(w, axis=1, bitorder="little").reshape(-1)[:cells].astype(bool).reshape(dims)


class OccupancyGrid:
    """One bit per cell of a dims[0] x dims[1] x dims[2] grid over the box [lo, hi).  `bits`: an int32 device tensor of
    mi_occupancy_words(dims) words (the uint32 words' bits).  inv_cell, the cells per unit length that places a point in its cell
    (t = (p - lo) * inv_cell, cell = floor(t)), is computed once on the host as np.float32(dims) / (np.float32(hi) - np.float32(lo))."""

    def __init__(self, bits: torch.Tensor, lo, hi, dims):
        self.dims = tuple(int(d) for d in np.asarray(dims).reshape(3))
        self.lo = np.asarray(lo, dtype=np.float32).reshape(3).copy()
        self.hi = np.asarray(hi, dtype=np.float32).reshape(3).copy()
        if min(self.dims) < 1 or self.dims[0] * self.dims[1] * self.dims[2] >= 2 ** 31:
            raise _lib.MiRenderError(f"occupancy grid dims {self.dims}: each at least 1, fewer than 2^31 cells")
        if not bool(np.all(self.hi > self.lo)):
            raise _lib.MiRenderError("occupancy grid: hi must be above lo on every axis")
        self.inv_cell = np.float32(self.dims) / (self.hi - self.lo)
        if not (isinstance(bits, torch.Tensor) and bits.is_cuda and bits.dtype == torch.int32 and bits.is_contiguous()
                and bits.numel() == self.words):
            raise _lib.MiRenderError(f"occupancy grid bits: a contiguous int32 device tensor of {self.words} words")
        self.bits = bits
        self._c = None

    def c_args(self):
        """(dims, lo, inv_cell) as the three ctypes arrays every grid-reading call of the library takes.  Made on first use and
        kept on the grid, with the numpy arrays they point into."""
        if self._c is None:
            self._c = (_i3(self.dims), _f3(self.lo), _f3(self.inv_cell))
        return tuple(p for _, p in self._c)

    @property
    def cells(self) -> int:
        return self.dims[0] * self.dims[1] * self.dims[2]

    @property
    def words(self) -> int:
        return (self.cells + 31) // 32

    @property
    def device(self):
        return self.bits.device

    def to_dense(self) -> np.ndarray:
        return unpack_dense(self.bits.cpu().numpy().view(np.uint32), self.dims)

    @classmethod
    def from_dense(cls, dense, lo, hi, device=None) -> "OccupancyGrid":
        """From bool [Gx,Gy,Gz]; the packing is done in numpy."""
        dense = np.asarray(dense, dtype=bool)
        if dense.ndim != 3:
            raise _lib.MiRenderError("from_dense: expected bool [Gx,Gy,Gz]")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        bits = torch.from_numpy(pack_dense(dense).view(np.int32)).to(device)
        return cls(bits, lo, hi, dense.shape)

    def occupied_fraction(self) -> float:
        return float(self.to_dense().mean())

    @classmethod
    def from_field(cls, model, lo, hi, resolution=128, threshold=0.0, supersample=2, dilate=1,
                   max_batch=64 ** 3) -> "OccupancyGrid":
        """A cell is occupied iff sigma of `model` exceeds `threshold` at any of its supersample^3 regular sub-sample points
        (at (i + 0.5) / supersample of the cell); the bits are then dilated `dilate` times by the 6-neighbourhood.  Points are
        generated on the device (mi_occupancy_cell_points), evaluated by the fused kernel in batches of `max_batch` points
        with a zero direction (sigma does not depend on it, as in grid.py) and packed by mi_occupancy_pack."""
        pf = _grid_field(model, "OccupancyGrid.from_field")
        dev = pf.device
        dims = (int(resolution),) * 3 if np.ndim(resolution) == 0 else tuple(int(r) for r in resolution)
        k = int(supersample)
        lo32, hi32 = np.asarray(lo, dtype=np.float32).reshape(3), np.asarray(hi, dtype=np.float32).reshape(3)
        _, pdims = _i3(dims)
        _, plo = _f3(lo32)
        _, pcell = _f3((hi32 - lo32) / np.float32(dims))
        words = _lib.query("mi_occupancy_words", pdims)
        cells, k3 = dims[0] * dims[1] * dims[2], k ** 3
        per = max(1, int(max_batch) // k3)
        sigma = torch.empty(cells * k3, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for head in range(0, cells, per):
                count = min(per, cells - head)
                pts = torch.empty((count * k3, 6), dtype=torch.float32, device=dev)
                _lib.call("mi_occupancy_cell_points", dev, pdims, plo, pcell, k, head, count, _lib.ptr(pts))
                sigma[head * k3:(head + count) * k3] = fields.eval_points(pf, pts)[:, 3]
            bits = torch.empty(words, dtype=torch.int32, device=dev)
            ws_bytes = _lib.query("mi_occupancy_pack_workspace_bytes", pdims, int(dilate))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.call("mi_occupancy_pack", dev, _lib.ptr(sigma), pdims, k, float(threshold), int(dilate), _lib.ptr(bits),
                      _lib.ptr(ws), ws_bytes)
        return cls(bits, lo32, hi32, dims)


def _grid_field(model, who):
    """The PackedField of a model a per-scene grid can be built from, or MiRenderError under the caller's name."""
    pf = fields.as_packed_field(model)
    if pf is None or fields.is_film(pf.kind):
        raise _lib.MiRenderError(f"{who}: needs a NeRF, SirenNeRF or TinyNeRF field (a FiLM field's table is per image, a "
                                 "per-scene grid has no meaning there)")
    return pf


class LiveOccupancyGrid:
    """An occupancy grid that follows a field while it trains (include/mi_render.h "a live grid").

        live = LiveOccupancyGrid(lo, hi, 128)                    # every cell occupied until the first update
        live.update(fine_model)                                  # a sweep: every cell at one jittered point
        live.update(fine_model, cells=live.grid.cells // 4)      # a partial update: half uniform, half among the occupied
        occupancy_train.render_rays(..., grid=live.grid)

    `density` (float32 [cells] on the device, +0 at the start) is folded with max(density * decay, sigma) at the cells an
    update samples; the bits are then density > (min(threshold, mean density) if relative else threshold), dilated `dilate`
    times.  `grid` is an ordinary OccupancyGrid whose `bits` tensor is written IN PLACE by every update: whatever holds
    `live.grid` (a render call, a captured graph) sees the new bits, and the tensor's data_ptr never changes.  `updates`
    counts the updates and is the epoch of the next one's random words, with `seed` their key.  update() reads nothing back;
    when to sweep and how many rows to draw is the caller's policy (examples/train_nerf_live_grid.py shows one)."""

    def __init__(self, lo, hi, resolution, device=None, *, decay=0.95, threshold=0.01, relative=True, dilate=0, seed=0):
        dims = (int(resolution),) * 3 if np.ndim(resolution) == 0 else tuple(int(r) for r in resolution)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if min(dims) < 1:
            raise _lib.MiRenderError(f"occupancy grid dims {dims}: each at least 1")
        self.grid = OccupancyGrid.from_dense(np.ones(dims, dtype=bool), lo, hi, device)
        self.decay, self.threshold, self.relative, self.dilate = float(decay), float(threshold), bool(relative), int(dilate)
        self.seed = _lib.seed64(seed)
        self.updates = 0
        self.density = torch.zeros(self.grid.cells, dtype=torch.float32, device=device)
        self._dims = _i3(dims)
        self._lo = _f3(self.grid.lo)
        self._cell = _f3((self.grid.hi - self.grid.lo) / np.float32(dims))
        self._ws_bytes = _lib.query("mi_occupancy_density_workspace_bytes", self._dims[1], self.dilate)
        self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=device)

    def update(self, model, cells=None, occupied_share=0.5, max_batch=64 ** 3):
        """One update.  cells=None: a sweep, every cell at one jittered point.  Otherwise `cells` rows are drawn, the first
        cells - int(cells * occupied_share) uniformly over the grid and the others among the currently occupied cells.  The
        points are evaluated in batches of `max_batch` by the fused kernel, as from_field does, and all rows' sigma is folded
        in one call and packed into the grid's bits in one call.
        Not under stream capture (MiRenderError): `updates` is counted on the host and goes to the kernel by value."""
        _lib.refuse_capture("LiveOccupancyGrid.update", "the epoch of its random words (`updates`) is counted on the host and goes "
                            "to the kernel by value, so every replay would draw the captured update's points again; call "
                            "update() eagerly between replays (it rewrites grid.bits in place, which a graph that holds the "
                            "grid sees)")
        pf = _grid_field(model, "LiveOccupancyGrid.update")
        g, dev = self.grid, self.grid.device
        if pf.device != dev:
            raise _lib.MiRenderError(f"LiveOccupancyGrid.update: the field is on {pf.device}, the grid on {dev}")
        sweep = cells is None
        rows = g.cells if sweep else int(cells)
        if rows < 1 or not 0.0 <= float(occupied_share) <= 1.0 or int(max_batch) < 1:
            raise _lib.MiRenderError("LiveOccupancyGrid.update: needs cells >= 1, 0 <= occupied_share <= 1, max_batch >= 1")
        n_uniform = rows if sweep else rows - int(rows * float(occupied_share))
        pdims, plo, pcell = self._dims[1], self._lo[1], self._cell[1]
        ids = torch.empty(rows, dtype=torch.int32, device=dev)
        sigma = torch.empty(rows, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for head in range(0, rows, int(max_batch)):
                count = min(int(max_batch), rows - head)
                pts = torch.empty((count, 6), dtype=torch.float32, device=dev)
                _lib.call("mi_occupancy_draw_points", dev, _lib.ptr(g.bits), pdims, plo, pcell, self.seed,
                          self.updates & 0xFFFFFFFF, 0 if sweep else 1, head, count, n_uniform, _lib.ptr(ids[head:head + count]),
                          _lib.ptr(pts))
                sigma[head:head + count] = fields.eval_points(pf, pts)[:, 3]
            _lib.call("mi_occupancy_density_update", dev, _lib.ptr(sigma), _lib.ptr(ids), rows, pdims, self.decay,
                      _lib.ptr(self.density), _lib.ptr(self._ws), self._ws_bytes)
            _lib.call("mi_occupancy_density_pack", dev, _lib.ptr(self.density), pdims, self.threshold, int(self.relative),
                      self.dilate, _lib.ptr(g.bits), _lib.ptr(self._ws), self._ws_bytes)
        self.updates += 1

    def occupied_fraction(self) -> float:
        return self.grid.occupied_fraction()

    def to_dense(self) -> np.ndarray:
        return self.grid.to_dense()

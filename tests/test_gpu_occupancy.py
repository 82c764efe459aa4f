"""GPU: construction of per-scene occupancy grids (include/mi_render.h, mirender/occupancy.py).

    mi_occupancy_pack         against the numpy restatement tests/test_occupancy_host.py:dense_reference, bits equal
    mi_occupancy_cell_points  against a torch restatement, within 1 ulp
    OccupancyGrid.from_field  end to end against the dense restatement on the field's own sigma, and a consistency check on
                              the samples of a 257-ray call (rays of tests/test_gpu_deferred_colour.py, NEAR, FAR = 2, 6,
                              jitter synth.t_rand(257, 16, seed=9); 67.1 % of those samples lie inside the box [-1.5, 1.5]^3)
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import render_ref as R, synth  # noqa: E402
from test_occupancy_host import dense_reference  # noqa: E402

NEAR, FAR = 2.0, 6.0
NC = 16
LO, HI = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)


def dev():
    return torch.device("cuda", 0)


def _sd(kind, seed, sigma_bias=0.0):
    sd = synth.state_dict(kind, seed=seed, sharp=True, bias_jitter=0.05)
    if sigma_bias:
        sd["output_layer_sigma.bias"] = sd["output_layer_sigma.bias"] + sigma_bias
    return sd


def _rays(n):
    """n rays spread over a 40x40 view of the volume (n = 1: a ray through its middle)."""
    r = torch.from_numpy(R.rays_from_camera(40, 40, 1.3875 * 40, synth.pose_degrees(4.0, 20.0, -30.0)))
    idx = (torch.arange(n) * 1600 // n + 20) % 1600 if n > 1 else torch.tensor([820])
    return r[idx].contiguous().to(dev())


def _mask(grid, dense, rays, z):
    """The definition restated in torch fp32 on the CPU (IEEE, nothing fused): bool [n,S], True = the sample is live."""
    rays, z = rays.cpu(), z.cpu()
    p = rays[:, None, 0, :] + rays[:, None, 1, :] * z[:, :, None]             # a multiply, then an add
    t = (p - torch.from_numpy(grid.lo)) * torch.from_numpy(grid.inv_cell)       # a subtract, then a multiply
    dims = torch.tensor(grid.dims)
    inside = ((t >= 0) & (t < dims.to(torch.float32))).all(-1)
    c = torch.minimum(torch.floor(torch.nan_to_num(t)).to(torch.int64).clamp(min=0), dims - 1)
    occ = torch.from_numpy(np.ascontiguousarray(dense))[c[..., 0], c[..., 1], c[..., 2]]
    return (inside & occ).to(dev())


# ---- 1. construction -------------------------------------------------------------------------------------------------------
def _pack(sigma, dims, k, threshold, dilate):
    from mirender import _lib
    lib = _lib.load()
    d = (ctypes.c_int * 3)(*dims)
    words = lib.mi_occupancy_words(d)
    ws_bytes = lib.mi_occupancy_pack_workspace_bytes(d, dilate)
    bits = torch.full((words,), -1, dtype=torch.int32, device=dev())
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev())
    sig = torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.float32)).to(dev())
    rc = lib.mi_occupancy_pack(_lib.ptr(sig), d, k, float(threshold), dilate, _lib.ptr(bits), _lib.ptr(ws), ws_bytes,
                               _lib.stream_ptr(dev()))
    assert rc == 0, lib.mi_last_error()
    return bits.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("dims", [(3, 5, 7), (16, 16, 16), (33, 2, 2)])
@pytest.mark.parametrize("k", [1, 2])
def test_pack_equals_the_numpy_restatement(dims, k):
    from mirender import occupancy
    cells = dims[0] * dims[1] * dims[2]
    rng = np.random.Generator(np.random.PCG64(11))
    vol = rng.normal(size=(cells, k ** 3)).astype(np.float32) - np.float32(1.2 if k == 1 else 2.0)   # a minority above 0
    corner = np.zeros((cells, k ** 3), np.float32)
    corner[cells - 1, k ** 3 - 1] = 3.0                        # one hot sub-sample in the far corner cell
    present = float(vol.reshape(-1)[17])                       # a threshold equal to a value in the volume: strict >
    for sigma, thr in ((vol, 0.0), (corner, 0.0), (vol, present)):
        for dilate in (0, 1, 2):
            want = dense_reference(sigma, dims, k, thr, dilate)
            got = _pack(sigma, dims, k, thr, dilate)
            assert np.array_equal(got, occupancy.pack_dense(want)), (dims, k, thr, dilate)
        if thr == 0.0:
            assert 0 < dense_reference(sigma, dims, k, thr, 0).sum() < cells
    c1 = dense_reference(corner, dims, k, 0.0, 1)
    assert c1.sum() == 1 + sum(1 for g in dims if g > 1)      # clipped at the box: one neighbour per axis that has one


@pytest.mark.parametrize("dims,k", [((3, 5, 7), 2), ((16, 16, 16), 1), ((33, 2, 2), 3)])
def test_cell_points_against_torch(dims, k):
    from mirender import _lib
    lib = _lib.load()
    lo, hi = np.float32([-1.5, -1.0, 0.25]), np.float32([1.5, 1.0, 2.0])
    cell = (hi - lo) / np.float32(dims)
    cells, k3 = dims[0] * dims[1] * dims[2], k ** 3
    head, count = 3, cells - 5                                # a batch that starts and ends inside the grid
    pts = torch.full((count * k3, 6), float("nan"), device=dev())
    rc = lib.mi_occupancy_cell_points((ctypes.c_int * 3)(*dims), lo.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                      cell.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), k, head, count, _lib.ptr(pts),
                                      _lib.stream_ptr(dev()))
    assert rc == 0, lib.mi_last_error()
    c = torch.arange(head, head + count)
    ijk = torch.stack([c // (dims[1] * dims[2]), (c // dims[2]) % dims[1], c % dims[2]], -1).to(torch.float32)   # [count,3]
    s = torch.arange(k3)
    sub = torch.stack([s // (k * k), (s // k) % k, s % k], -1).to(torch.float32)                                  # [k3,3]
    f = (sub + 0.5) / float(k)
    want = torch.from_numpy(lo) + (ijk[:, None, :] + f[None]) * torch.from_numpy(cell)
    got = pts.cpu()
    assert torch.equal(got[:, 3:], torch.zeros(count * k3, 3))
    err = (got[:, :3].reshape(count, k3, 3) - want).abs()
    ulp = torch.from_numpy(np.spacing(np.abs(want.numpy()).astype(np.float32)))
    assert bool((err <= ulp).all()), float((err / ulp).max())


# ---- 2. from_field end to end ----------------------------------------------------------------------------------------------
SIGMA_SHIFT = -60.0       # CPU oracle, siren_nerf seed 5: 43.2 % of the 32^3 cells occupied after one dilation, centres 35 % live


def test_from_field_end_to_end():
    """A 32^3 grid over [-1.5, 1.5]^3 from the siren_nerf fine field (seed 5) with its sigma bias shifted by SIGMA_SHIFT,
    threshold 0, supersample 2, dilate 1.  A consistency check, not a conservativeness proof: the grid equals the dense
    restatement on the field's own sigma, and every sample of the 257-ray call that falls in a cell whose CENTRE has sigma > 0
    is marked.  The field is the SirenNeRF because the check presumes a field that varies slowly across a cell (3 / 32 wide):
    SirenNeRF reads raw xyz, and on the CPU oracle no cell at all has a live centre and no mark, at shifts -46, -60 and -72
    (57.7 / 43.2 / 27.9 % occupied).  The positionally encoded ReLU fields carry frequencies up to 2^9 and do not qualify: the
    oracle counts 13 to 115 such cells for nerf (medium head) and tiny_nerf at the same occupancies."""
    from mirender import _lib, fields, occupancy, ops
    lib = _lib.load()
    dims, k = (32, 32, 32), 2
    model = fields.field_from_state_dict(_sd("siren_nerf", 5, SIGMA_SHIFT), dev())
    pf = fields.as_packed_field(model)
    grid = occupancy.OccupancyGrid.from_field(model, LO, HI, resolution=32, threshold=0.0, supersample=k, dilate=1,
                                              max_batch=50000)       # several uneven batches
    lo, hi = np.float32(LO), np.float32(HI)
    cell = (hi - lo) / np.float32(dims)

    def sigma_at(kk):
        pts = torch.empty((32 ** 3 * kk ** 3, 6), device=dev())
        assert lib.mi_occupancy_cell_points((ctypes.c_int * 3)(*dims), lo.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                            cell.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), kk, 0, 32 ** 3, _lib.ptr(pts),
                                            _lib.stream_ptr(dev())) == 0
        return fields.eval_points(pf, pts)[:, 3].cpu().numpy()

    want = dense_reference(sigma_at(k), dims, k, 0.0, 1)
    dense = grid.to_dense()
    assert np.array_equal(dense, want)
    frac = grid.occupied_fraction()
    assert frac == float(want.mean()) and 0.02 < frac < 0.98, frac
    centre_live = (sigma_at(1) > 0).reshape(dims)
    n = 257
    rays = _rays(n)
    z = ops.sample_coarse(n, NEAR, FAR, NC, dev(), synth.t_rand(n, NC, seed=9).to(dev()), seed=0)
    ones = occupancy.OccupancyGrid.from_dense(np.ones(dims, bool), LO, HI, dev())
    in_centre_live = _mask(ones, centre_live, rays, z)
    marked = _mask(grid, dense, rays, z)
    assert int(in_centre_live.sum()) > 0
    assert bool((marked | ~in_centre_live).all()), int((in_centre_live & ~marked).sum())

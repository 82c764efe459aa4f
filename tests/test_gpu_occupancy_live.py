"""GPU: a live occupancy grid (include/mi_render.h "a live grid", mirender/occupancy.py LiveOccupancyGrid), bit for bit against
the numpy restatement tests/occupancy_live_ref.py on the inputs tests/test_occupancy_live_host.py checks.

    mi_occupancy_draw_points      cell ids and points of sweep, uniform and occupied-share rows; batches; the epoch
    mi_occupancy_density_update   the decayed-maximum fold over rows with many duplicates and every special value
    mi_occupancy_density_pack     mean, relative / absolute threshold, strict comparison, dilation, words
    LiveOccupancyGrid             a sweep and a partial update end to end on a SirenNeRF, in place, reproducibly
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import occupancy_live_ref as ref  # noqa: E402
import occupancy_render_ref as render_ref  # noqa: E402
from oracle import render_ref as R, synth  # noqa: E402

LO, HI = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)
BOX_LO, BOX_CELL = np.float32([-1.5, -1.0, 0.25]), np.float32([0.1, 0.2, 0.3])
SIGMA_SHIFT = -60.0       # tests/test_gpu_occupancy.py: the siren_nerf seed 5 field with a minority of the box above sigma 0


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


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# ---- 1. the draw -------------------------------------------------------------------------------------------------------------
def _draw(bits, dims, epoch, mode, row0, count, n_uniform, lo=BOX_LO, cell=BOX_CELL, seed=ref.SEED):
    from mirender import _lib
    lib = _lib.load()
    words = None if bits is None else _to_dev(bits.view(np.int32))
    ids = torch.full((count,), -7, dtype=torch.int32, device=dev())
    pts = torch.full((count, 6), float("nan"), device=dev())
    rc = lib.mi_occupancy_draw_points(_lib.ptr(words), (ctypes.c_int * 3)(*dims), _fp(lo), _fp(cell), seed, epoch, mode, row0,
                                      count, n_uniform, _lib.ptr(ids), _lib.ptr(pts), _lib.stream_ptr(dev()))
    assert rc == 0, lib.mi_last_error()
    return ids.cpu().numpy(), pts.cpu().numpy()


@pytest.mark.parametrize("dims", ref.DIMS)
def test_draw_equals_the_restatement(dims):
    cells = dims[0] * dims[1] * dims[2]
    for name in ("random", "zeros", "ones"):
        bits = ref.draw_bits(name, dims)
        for count in (1, 255, 1000):
            for n_uniform in (0, count // 2, count):
                want_ids, want_pts, tries = ref.draw(bits, dims, BOX_LO, BOX_CELL, ref.SEED, 0, 1, 0, count, n_uniform)
                ids, pts = _draw(bits, dims, 0, 1, 0, count, n_uniform)
                case = (dims, name, count, n_uniform)
                assert ref.same_bits(ids, want_ids), case
                assert ref.same_bits(pts, want_pts), case                # NaN-filled outputs fully overwritten, direction 0
                assert not np.isnan(pts).any() and not pts[:, 3:].any()
                if name == "zeros":
                    assert (tries[n_uniform:] == 8).all()                   # every occupied-share row gives c_7
                if name == "ones":
                    assert (tries[n_uniform:] == 0).all()
    bits = ref.draw_bits("random", dims)
    full_ids, full_pts = _draw(bits, dims, 0, 1, 0, 1000, 500)
    tail_ids, tail_pts = _draw(bits, dims, 0, 1, 77, 1000 - 77, 500)       # a later batch of the same update
    assert ref.same_bits(tail_ids, full_ids[77:]) and ref.same_bits(tail_pts, full_pts[77:])
    e3_ids, e3_pts = _draw(bits, dims, 3, 1, 0, 1000, 500)
    want_ids, want_pts, _ = ref.draw(bits, dims, BOX_LO, BOX_CELL, ref.SEED, 3, 1, 0, 1000, 500)
    assert ref.same_bits(e3_ids, want_ids) and ref.same_bits(e3_pts, want_pts)
    assert not ref.same_bits(e3_ids, full_ids) and not ref.same_bits(e3_pts, full_pts)
    # a sweep over [3, cells - 2): the cells in order, with no grid to read
    ids, pts = _draw(None, dims, 2, 0, 3, cells - 5, 0)
    want_ids, want_pts, _ = ref.draw(None, dims, BOX_LO, BOX_CELL, ref.SEED, 2, 0, 3, cells - 5, 0)
    assert np.array_equal(ids, np.arange(3, cells - 2)) and ref.same_bits(ids, want_ids) and ref.same_bits(pts, want_pts)


# ---- 2. the fold -------------------------------------------------------------------------------------------------------------
def _fold(density, sigma, ids, decay, dims=(3, 5, 7)):
    from mirender import _lib
    lib = _lib.load()
    d = (ctypes.c_int * 3)(*dims)
    ws_bytes = lib.mi_occupancy_density_workspace_bytes(d, 0)
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev())
    den, sig, cid = _to_dev(density), _to_dev(sigma), _to_dev(ids)
    rc = lib.mi_occupancy_density_update(_lib.ptr(sig), _lib.ptr(cid), sigma.size, d, decay, _lib.ptr(den), _lib.ptr(ws), ws_bytes,
                                         _lib.stream_ptr(dev()))
    assert rc == 0, lib.mi_last_error()
    return den.cpu().numpy()


@pytest.mark.parametrize("decay", [0.95, 1.0, 0.0])
def test_fold_equals_the_restatement(decay):
    density, sigma, ids = ref.fold_inputs()
    want = ref.fold(density, sigma, ids, decay)
    got = _fold(density, sigma, ids, decay)
    assert ref.same_bits(got, want), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    for c in ref.FOLD_UNSAMPLED:
        assert ref.same_bits(got[c], density[c])
    assert ref.same_bits(_fold(density, sigma, ids, decay), got)            # the same bits in a second run


# ---- 3. the pack -------------------------------------------------------------------------------------------------------------
def _pack(density, dims, threshold, relative, dilate):
    from mirender import _lib
    lib = _lib.load()
    d = (ctypes.c_int * 3)(*dims)
    ws_bytes = lib.mi_occupancy_density_workspace_bytes(d, dilate)
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev())
    bits = torch.full((lib.mi_occupancy_words(d),), -1, dtype=torch.int32, device=dev())
    den = _to_dev(density)
    rc = lib.mi_occupancy_density_pack(_lib.ptr(den), d, threshold, relative, dilate, _lib.ptr(bits), _lib.ptr(ws), ws_bytes,
                                       _lib.stream_ptr(dev()))
    assert rc == 0, lib.mi_last_error()
    assert ref.same_bits(den.cpu().numpy(), density)                        # the density is read, not written
    return bits.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("dims", ref.DIMS)
def test_pack_equals_the_restatement(dims):
    density = ref.pack_inputs(dims)
    for name, threshold, relative in ref.PACK_CASES:
        for dilate in (0, 1, 2):
            want = ref.pack(density, dims, threshold, relative, dilate)[1]
            assert ref.same_bits(_pack(density, dims, threshold, relative, dilate), want), (dims, name, dilate)
    for dilate in (0, 2):
        assert not _pack(np.zeros_like(density), dims, 0.01, 1, dilate).any()


# ---- 4. LiveOccupancyGrid end to end -------------------------------------------------------------------------------------------
G = 16


def _sigma_at(pf, pts):
    from mirender import fields
    return fields.eval_points(pf, _to_dev(pts))[:, 3].cpu().numpy()


@pytest.fixture(scope="module")
def field():
    from mirender import fields
    model = fields.field_from_state_dict(_sd("siren_nerf", 5, SIGMA_SHIFT), dev())
    return model, fields.as_packed_field(model)


@pytest.fixture(scope="module")
def restated(field):
    """The two updates of the end-to-end tests, restated once: a sweep, then a partial update of 2 000 rows."""
    _, pf = field
    dims, seed = (G, G, G), 11
    lo = np.float32(LO)
    cell = (np.float32(HI) - lo) / np.float32(dims)
    _, pts0, _ = ref.draw(None, dims, lo, cell, seed, 0, 0, 0, G ** 3, 0)
    sigma0 = _sigma_at(pf, pts0)
    density0 = ref.fold(np.zeros(G ** 3, np.float32), sigma0, np.arange(G ** 3, dtype=np.int32), 0.95)
    dense0, bits0 = ref.pack(density0, dims, 0.01, 1, 1)
    ids1, pts1, _ = ref.draw(bits0, dims, lo, cell, seed, 1, 1, 0, 2000, 1000)
    density1 = ref.fold(density0, _sigma_at(pf, pts1), ids1, 0.95)
    dense1, bits1 = ref.pack(density1, dims, 0.01, 1, 1)
    return dict(seed=seed, sigma0=sigma0, density0=density0, dense0=dense0, bits0=bits0, ids1=ids1, density1=density1,
                dense1=dense1, bits1=bits1)


def _live(seed, **kw):
    from mirender import occupancy
    return occupancy.LiveOccupancyGrid(LO, HI, G, dev(), decay=0.95, threshold=0.01, relative=True, dilate=1, seed=seed, **kw)


def _bits(live):
    return live.grid.bits.cpu().numpy().view(np.uint32)


def test_live_grid_sweep_and_partial_update(field, restated):
    from mirender import occupancy, ops
    model, pf = field
    r = restated
    live = _live(r["seed"])
    assert isinstance(live.grid, occupancy.OccupancyGrid) and live.updates == 0
    assert live.to_dense().all() and live.occupied_fraction() == 1.0 and ref.same_bits(_bits(live), occupancy.pack_dense(np.ones((G,) * 3, bool)))
    assert live.density.dtype == torch.float32 and tuple(live.density.shape) == (G ** 3,) and not live.density.any()
    grid, at = live.grid, live.grid.bits.data_ptr()

    live.update(model)                                                      # a sweep
    assert live.updates == 1
    assert ref.same_bits(r["density0"], np.where(r["sigma0"] > 0, r["sigma0"], np.float32(0.0)))   # max(sigma, 0), from +0
    assert ref.same_bits(live.density.cpu().numpy(), r["density0"])
    assert ref.same_bits(_bits(live), r["bits0"]) and np.array_equal(live.to_dense(), r["dense0"])
    assert 0.02 < live.occupied_fraction() < 0.98

    # the renderer reads the grid object it was given: the evaluated count is the restated mask's
    n, nc = 257, 16
    rays = _rays(n)
    tr = synth.t_rand(n, nc, seed=9).to(dev())
    z = ops.sample_coarse(n, 2.0, 6.0, nc, dev(), tr, seed=0)
    want = int(render_ref.occupied_mask(rays, z, grid.lo, grid.inv_cell, r["dense0"]).sum())
    _, counts = ops.render_rays_occupancy(pf, pf, rays, 2.0, 6.0, nc, 0, grid, tr)
    assert 0 < want < n * nc and counts.tolist()[0] == want

    live.update(model, cells=2000)                                          # 1 000 uniform rows, 1 000 among the occupied
    assert live.updates == 2 and live.grid is grid and grid.bits.data_ptr() == at
    got = live.density.cpu().numpy()
    untouched = np.setdiff1d(np.arange(G ** 3), r["ids1"])
    assert untouched.size > 0 and ref.same_bits(got[untouched], r["density0"][untouched])
    assert ref.same_bits(got, r["density1"]) and not ref.same_bits(got, r["density0"])
    assert ref.same_bits(_bits(live), r["bits1"])


def test_live_grid_is_reproducible_and_batches_do_not_matter(field, restated):
    model, _ = field
    r = restated
    a, b, c = _live(r["seed"]), _live(r["seed"]), _live(r["seed"] + 1)
    for live, batch in ((a, 64 ** 3), (b, 5000), (c, 64 ** 3)):             # 5 000: uneven batches of the 4 096 / 6 000 rows
        live.update(model, max_batch=batch)
        live.update(model, cells=6000, occupied_share=0.75, max_batch=batch)
    assert ref.same_bits(a.density.cpu().numpy(), b.density.cpu().numpy()) and ref.same_bits(_bits(a), _bits(b))
    assert not ref.same_bits(a.density.cpu().numpy(), c.density.cpu().numpy())        # another seed, other points


def test_live_grid_refuses_what_from_field_refuses():
    from mirender import _lib, fields
    live = _live(0)
    with pytest.raises(_lib.MiRenderError, match="LiveOccupancyGrid.update: needs a NeRF, SirenNeRF or TinyNeRF field"):
        live.update(fields.FilmSirenNeRF().to(dev()))
    with pytest.raises(_lib.MiRenderError, match="LiveOccupancyGrid.update"):
        live.update(lambda x: x)
    assert live.updates == 0 and live.to_dense().all()

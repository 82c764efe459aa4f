"""GPU: rendering with an occupancy grid (include/mi_render.h "rendering with a grid", mirender.ops.render_rays_occupancy,
render_rays(..., grid=)).  Every comparison is bit equality; the rule "which samples are occupied" is the torch restatement
tests/occupancy_render_ref.py, which tests/test_occupancy_render_host.py counts by hand.

    mi_occupancy_mark_rays      the sorted list equals the restatement's occupied indices; unoccupied raw rows are zeroed,
                                occupied rows keep their sentinel
    mi_field_eval_rays_list     listed rows have mi_field_eval_rays' bits, every other row keeps its sentinel
    mi_render_rays_occupancy    all six outputs equal the composition of the existing stage calls with where(mask, raw, 0)
                                between the field and the composite; `evaluated` equals the two mask sums
    a grid over every sample with sigma > 0 leaves every output bit of mi_render_rays as it is, while it culls
    render_rays / render_image (grid=)    equal the ops call; a frame in two ray ranges equals the frame in one; what is
                                not built raises MiRenderError
"""
import ctypes
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import occupancy_render_ref as ref  # noqa: E402
from oracle import parity, render_ref as R, synth  # noqa: E402

NEAR, FAR = 2.0, 6.0
SENTINEL = -7.25
BOX = ((-4.0,) * 3, (4.0,) * 3)              # holds every sample of the rays below (camera at radius 4, depths 2..6)
SMALL = ((-1.5,) * 3, (1.5,) * 3)            # a box the rays partly leave


def dev():
    return torch.device("cuda", 0)


def _rays(n):
    """n rays spread over a 40x40 view (focal 55) of the volume."""
    r = torch.from_numpy(R.rays_from_camera(40, 40, 55.0, synth.pose_degrees(4.0, 20.0, -30.0)))
    idx = (torch.arange(n) * 1600 // n + 20) % 1600
    return r[idx].contiguous().to(dev())


_FIELDS = {}


def _field(kind, seed):
    """(module, packed field) of a synthetic "medium" field, built once per (kind, seed)."""
    from mirender import fields
    if (kind, seed) not in _FIELDS:
        m = fields.field_from_state_dict(synth.state_dict(kind, seed=seed, sharp="medium", bias_jitter=0.05), dev())
        for p in m.parameters():
            p.requires_grad_(False)
        _FIELDS[(kind, seed)] = (m, fields.as_packed_field(m))
    return _FIELDS[(kind, seed)]


def _dense(name, dims):
    rng = np.random.Generator(np.random.PCG64(31))
    if name == "zeros":
        return np.zeros(dims, bool)
    if name == "ones":
        return np.ones(dims, bool)
    return rng.random(dims) < 0.3


def _grid(dense, box):
    from mirender import occupancy
    return occupancy.OccupancyGrid.from_dense(dense, box[0], box[1], dev())


def _grid_args(grid):
    d = (ctypes.c_int * 3)(*grid.dims)
    lo = (ctypes.c_float * 3)(*[float(v) for v in grid.lo])
    inv = (ctypes.c_float * 3)(*[float(v) for v in grid.inv_cell])
    return d, lo, inv


def _mask(grid, dense, rays, z):
    return ref.occupied_mask(rays, z, grid.lo, grid.inv_cell, dense)


# ---- 1. the mark kernel ----------------------------------------------------------------------------------------------------
MARK_GRIDS = [("random", (5, 7, 3), BOX), ("random", (16, 16, 16), BOX), ("zeros", (16, 16, 16), BOX), ("ones", (5, 7, 3), BOX),
              ("ones", (16, 16, 16), SMALL), ("random", (16, 16, 16), SMALL)]


@pytest.mark.parametrize("n,s", [(37, 5), (130, 192)])
def test_mark_equals_the_restatement(n, s):
    from mirender import _lib, ops
    lib = _lib.load()
    rays = _rays(n)
    z = ops.sample_coarse(n, NEAR, FAR, s, dev(), synth.t_rand(n, s, seed=9).to(dev()))
    seen = set()
    for name, dims, box in MARK_GRIDS:
        dense = _dense(name, dims)
        grid = _grid(dense, box)
        want = _mask(grid, dense, rays, z).reshape(-1)
        d, lo, inv = _grid_args(grid)
        for with_raw in (True, False):
            lst = torch.full((n * s,), -1, dtype=torch.int32, device=dev())
            count = torch.full((1,), 12345, dtype=torch.int32, device=dev())          # the call clears it
            raw = torch.full((n, s, 4), SENTINEL, device=dev()) if with_raw else None
            rc = lib.mi_occupancy_mark_rays(_lib.ptr(grid.bits), d, lo, inv, _lib.ptr(rays), _lib.ptr(z), n, s, _lib.ptr(lst),
                                            _lib.ptr(count), _lib.ptr(raw), _lib.stream_ptr(dev()))
            assert rc == 0, lib.mi_last_error()
            c = int(count.item())
            print(f"mark {n}x{s} {name} {dims} box {box[0][0]}: {c} of {n * s} occupied")
            assert c == int(want.sum()), (name, dims, box)
            got = lst.cpu()
            assert torch.equal(torch.sort(got[:c]).values.to(torch.int64), torch.nonzero(want).reshape(-1)), (name, dims, box)
            assert bool((got[c:] == -1).all())                                        # nothing behind the count is written
            if with_raw:
                rows = raw.cpu().reshape(-1, 4)
                assert torch.equal(rows[~want], torch.zeros(int((~want).sum()), 4)), (name, dims, box)
                assert torch.equal(rows[want], torch.full((c, 4), SENTINEL)), (name, dims, box)
        seen.add("none" if c == 0 else "all" if c == n * s else "some")
    assert seen == {"none", "all", "some"}                     # the grids really cover the empty, the full and the ragged case


# ---- 2. the list-driven forward --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nerf", "tiny_nerf", "siren_nerf"])
def test_list_forward_rows_equal_the_whole_forward(kind):
    from mirender import _lib, ops
    lib = _lib.load()
    n, s = 37, 7                                               # 259 points: two tiles and a partial one
    _, pf = _field(kind, 5)
    rays = _rays(n)
    z = ops.sample_coarse(n, NEAR, FAR, s, dev(), synth.t_rand(n, s, seed=9).to(dev()))
    full = ops.field_eval_rays(pf, rays, z).reshape(-1, 4)
    gen = torch.Generator().manual_seed(3)
    for c in (100, 0, 1, 128, 129, 259):
        # the buffer behind the count holds the other (valid) indices: their rows must stay untouched
        perm = torch.randperm(n * s, generator=gen).to(torch.int32)
        lst, count = perm.to(dev()), torch.tensor([c], dtype=torch.int32, device=dev())
        raw = torch.full((n * s, 4), SENTINEL, device=dev())
        rc = lib.mi_field_eval_rays_list(pf.kind, _lib.ptr(pf.refresh()), _lib.ptr(rays), _lib.ptr(z), n, s, _lib.ptr(lst),
                                         _lib.ptr(count), _lib.ptr(raw), _lib.stream_ptr(dev()))
        assert rc == 0, lib.mi_last_error()
        listed = torch.zeros(n * s, dtype=torch.bool)
        listed[perm[:c].to(torch.int64)] = True
        listed = listed.to(dev())
        assert torch.equal(raw[listed].view(torch.int32), full[listed].view(torch.int32)), (kind, c)
        assert bool((raw[~listed] == SENTINEL).all()), (kind, c)


# ---- 3. the render against the stage composition ---------------------------------------------------------------------------
def _stages(pf_c, pf_f, rays, nc, nf, grid, dense, t_rand=None, seed=0, ray0=0):
    """The reference: the existing stage calls, with where(mask, raw, 0) between the field and the composite."""
    from mirender import ops
    n = rays.shape[0]
    z_c = ops.sample_coarse(n, NEAR, FAR, nc, dev(), t_rand, seed, ray0=ray0)
    m_c = _mask(grid, dense, rays, z_c).to(dev())
    raw_c = torch.where(m_c[..., None], ops.field_eval_rays(pf_c, rays, z_c), torch.zeros((), device=dev()))
    rgb_c, depth_c, acc_c, w_c = ops.composite(raw_c, z_c, rays)
    z_f = ops.sample_fine(z_c, w_c, NEAR, FAR, nf)
    m_f = _mask(grid, dense, rays, z_f).to(dev())
    raw_f = torch.where(m_f[..., None], ops.field_eval_rays(pf_f, rays, z_f), torch.zeros((), device=dev()))
    rgb_f, depth_f, acc_f, _ = ops.composite(raw_f, z_f, rays, want_weights=False)
    return (rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f), [int(m_c.sum()), int(m_f.sum())]


def _assert_outs(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        if g is not None:
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), (what, k)


RENDER_CASES = {
    "nerf_pair": ("nerf", 5, "nerf", 6, 130, 64, 128, "t_rand"),
    "tiny_nerf": ("tiny_nerf", 5, "tiny_nerf", 6, 33, 5, 3, "t_rand"),
    "siren_nerf_nf0": ("siren_nerf", 5, "siren_nerf", 6, 101, 9, 0, "t_rand"),
    "nerf_shared": ("nerf", 5, "nerf", 5, 57, 12, 24, "t_rand"),
    "nerf_seeded": ("nerf", 5, "nerf", 6, 57, 12, 24, "seed"),
}


@pytest.mark.parametrize("case", sorted(RENDER_CASES))
def test_render_equals_the_stage_composition(case):
    from mirender import ops
    kc, sc, kf, sf, n, nc, nf, jitter = RENDER_CASES[case]
    pf_c, pf_f = _field(kc, sc)[1], _field(kf, sf)[1]
    rays = _rays(n)
    tr = synth.t_rand(n, nc, seed=9).to(dev()) if jitter == "t_rand" else None
    seed, ray0 = (0, 0) if jitter == "t_rand" else (77, 1000)
    dense = _dense("random", (16, 16, 16))
    grid = _grid(dense, BOX)
    want, sums = _stages(pf_c, pf_f, rays, nc, nf, grid, dense, tr, seed, ray0)
    got, counts = ops.render_rays_occupancy(pf_c, pf_f, rays, NEAR, FAR, nc, nf, grid, tr, seed, ray0=ray0)
    print(f"{case}: evaluated {counts.tolist()} of {[n * nc, n * (nc + nf)]}")
    _assert_outs(got, want, case)
    assert counts.tolist() == sums
    assert 0 < sums[0] < n * nc and 0 < sums[1] < n * (nc + nf)
    # rgb_c = NULL: the coarse pass's weights come from the sigma channel alone
    got2, counts2 = ops.render_rays_occupancy(pf_c, pf_f, rays, NEAR, FAR, nc, nf, grid, tr, seed, ray0=ray0, coarse_outputs=False)
    assert got2[0] is None and got2[1] is None and got2[2] is None
    _assert_outs(got2[3:], want[3:], case + " without coarse outputs")
    assert counts2.tolist() == sums


def test_all_zero_grid_renders_the_background():
    from mirender import ops
    n, nc, nf = 57, 12, 24
    pf_c, pf_f = _field("nerf", 5)[1], _field("nerf", 6)[1]
    grid = _grid(np.zeros((16, 16, 16), bool), BOX)
    outs, counts = ops.render_rays_occupancy(pf_c, pf_f, _rays(n), NEAR, FAR, nc, nf, grid, synth.t_rand(n, nc, seed=9).to(dev()))
    assert counts.tolist() == [0, 0]
    for k in (0, 3):
        assert bool((outs[k] == 1).all()) and bool((outs[k + 1] == 0).all()) and bool((outs[k + 2] == 0).all())


# ---- 4. a grid that covers every positive sample changes no bit ------------------------------------------------------------
COVER_CASES = {"nerf": ("nerf", 130, 64, 128), "tiny_nerf": ("tiny_nerf", 57, 7, 11), "siren_nerf": ("siren_nerf", 57, 9, 5)}


@pytest.mark.parametrize("case", sorted(COVER_CASES))
def test_covering_grid_changes_no_bit(case):
    """The plain stage composition says where sigma > 0; a 128^3 grid over (-4, 4)^3 with exactly those samples' cells set
    zeroes only samples whose weight is exactly 0 either way (0 * rgb is +0 for any sigmoid colour), so all six outputs keep
    mi_render_rays' bits - while the grid culls: for the nerf pair at most three quarters of n (2 Nc + Nf) are evaluated
    (on the CPU oracle 18 134 of 33 280 are, 54.5 %)."""
    from mirender import ops
    kind, n, nc, nf = COVER_CASES[case]
    pf_c, pf_f = _field(kind, 5)[1], _field(kind, 6)[1]
    rays = _rays(n)
    tr = synth.t_rand(n, nc, seed=9).to(dev())
    chain = parity.hip_stage_chain(ops, pf_c, pf_f, rays, NEAR, FAR, nc, nf, tr)
    dims = (128, 128, 128)
    inv = ref.inv_cell_of(BOX[0], BOX[1], dims)
    dense = np.zeros(dims, bool)
    for z, raw in ((chain["z_coarse"], chain["raw_c"]), (chain["z_fine"], chain["raw_f"])):
        pos = (raw[..., 3] > 0).cpu()
        cells = ref.cells_of(ref.points(rays, z)[pos], np.float32(BOX[0]), inv, dims)
        assert cells.shape[0] == int(pos.sum())                # every positive sample lies inside the box
        dense[cells[:, 0].numpy(), cells[:, 1].numpy(), cells[:, 2].numpy()] = True
    grid = _grid(dense, BOX)
    assert np.array_equal(grid.inv_cell, inv)
    plain = ops.render_rays_fused(pf_c, pf_f, rays, NEAR, FAR, nc, nf, None, tr)
    got, counts = ops.render_rays_occupancy(pf_c, pf_f, rays, NEAR, FAR, nc, nf, grid, tr)
    _assert_outs(got, plain, case)
    parity.assert_chain_equals_fused(chain, got)
    evaluated, total = int(counts.sum()), n * (2 * nc + nf)
    print(f"{case}: evaluated {counts.tolist()} = {evaluated} of {total} ({100.0 * evaluated / total:.1f} %)")
    assert evaluated < total
    if case == "nerf":
        assert 4 * evaluated <= 3 * total, (evaluated, total)


# ---- 5. the Python surface -------------------------------------------------------------------------------------------------
def test_render_rays_and_render_image_with_a_grid():
    from mirender import ops, render_core
    (mc, pf_c), (mf, pf_f) = _field("nerf", 5), _field("nerf", 6)
    nc, nf, w, h, focal = 12, 24, 16, 16, 22.0
    pose = synth.pose_degrees(4.0, 20.0, -30.0)
    dense = _dense("random", (16, 16, 16))
    grid = _grid(dense, BOX)
    n = 57
    rays, tr = _rays(n), synth.t_rand(n, nc, seed=9).to(dev())
    with torch.no_grad():
        a = render_core.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, t_rand=tr, grid=grid)
        b, _ = ops.render_rays_occupancy(pf_c, pf_f, rays, NEAR, FAR, nc, nf, grid, tr)
        _assert_outs(a, b, "render_rays(grid=)")
        plain = render_core.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, t_rand=tr)
        assert not torch.equal(a[3], plain[3])                  # the grid is really read
        # render_image: the fine outputs of render_rays over the frame's rays
        tri = synth.t_rand(w * h, nc, seed=4).to(dev())
        img = render_core.render_image(w, h, focal, pose, NEAR, FAR, mc, mf, nc, nf, t_rand=tri, grid=grid)
        frame = render_core.render_rays(ops.gen_rays(w, h, focal, pose, dev()), NEAR, FAR, mc, mf, nc, nf, t_rand=tri, grid=grid)[3:6]
        for x, y, shape in zip(img, frame, ((h, w, 3), (h, w, 1), (h, w, 1))):
            assert np.array_equal(x, y.cpu().numpy().reshape(shape))
        ten = render_core.render_image_tensor(w, h, focal, pose, NEAR, FAR, mc, mf, nc, nf, t_rand=tri, grid=grid)
        assert torch.equal(ten, frame[0].reshape(h, w, 3))
        # a frame in two ray ranges equals the frame in one call: the seeded jitter is keyed by ray0 + ray index
        args = (w, h, focal, pose, NEAR, FAR, mc, mf, nc, nf, None)
        whole = render_core._render_image_device(*args, seed=5, grid=grid)
        first = render_core._render_image_device(*args, seed=5, ray0=0, n_rays=100, grid=grid)
        second = render_core._render_image_device(*args, seed=5, ray0=100, n_rays=w * h - 100, grid=grid)
        for k in range(3):
            assert torch.equal(torch.cat([first[k], second[k]]), whole[k])
        vid = render_core.render_video(w, h, focal, [pose], NEAR, FAR, mc, mf, nc, nf, t_rand=tri[None], grid=grid)
        assert np.array_equal(vid[0][0], img[0])


def test_what_is_not_built_raises():
    from mirender import _lib, fields, render_core
    (mc, _), (mf, _) = _field("nerf", 5), _field("nerf", 6)
    grid = _grid(np.ones((4, 4, 4), bool), BOX)
    rays = _rays(8)
    kw = dict(t_rand=synth.t_rand(8, 8, seed=1).to(dev()), grid=grid)
    film = fields.FilmSirenNeRF().to(dev())
    film.set_film_params(synth.film_params(1)[0].to(dev()))
    with torch.no_grad():
        with pytest.raises(_lib.MiRenderError, match="FiLM"):
            render_core.render_rays(rays, NEAR, FAR, film, film, 8, 8, **kw)
        with pytest.raises(_lib.MiRenderError, match="callable"):
            render_core.render_rays(rays, NEAR, FAR, lambda x: torch.zeros(x.shape[0], 4, device=x.device), mf, 8, 8, **kw)
        with pytest.raises(_lib.MiRenderError, match="is on"):
            other = types.SimpleNamespace(device=torch.device("cuda", 1), bits=grid.bits, dims=grid.dims, lo=grid.lo, inv_cell=grid.inv_cell)
            render_core.render_rays(rays, NEAR, FAR, mc, mf, 8, 8, t_rand=kw["t_rand"], grid=other)
    trainable = fields.NeRF().to(dev())                         # parameters that require grad, grad mode on
    with pytest.raises(_lib.MiRenderError, match="gradients"):
        render_core.render_rays(rays, NEAR, FAR, trainable, trainable, 8, 8, **kw)

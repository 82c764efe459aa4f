"""GPU: clipping each ray's sampling range to an occupancy grid, layer by layer (include/mi_render.h "clipping",
DESIGN.md 4.8).  Bit equality unless said otherwise.

    1 mi_occupancy_clip_rays         against tests/occupancy_clip_ref.py: 1 .. 130 rays, 1 .. 192 probes (a partial round, an
                                     exact round, several rounds), pad 0 / 1 / 3, random / empty / full grids, a box the rays
                                     partly leave; bounds pre-filled with NaN so that an unwritten row shows
    2 mi_sample_coarse_bounds        constant bounds == mi_sample_coarse(z_lin = NULL); varied bounds ray by ray == the scalar call
                                     on that single ray with ray0 + r; injected and seeded jitter; the restated formula
    3 mi_sample_fine_bounds          the same two comparisons against mi_sample_fine_pos, z_samples and pos included; a ray whose
                                     weights are all zero; the restatement of tests/sampler_ref.py
    4 mi_render_rays_occupancy_clip  == clip, coarse bounds, mark, list forward, composite, fine bounds, mark, list forward,
                                     composite; with an all-ones grid over every probe == mi_render_rays_occupancy(z_lin = NULL)
    5 the training pair              outputs == the inference call's; all-ones grid: gradients == mi_render_rays_occupancy_train's
                                     (z_lin = NULL); partial grid: gradients against tests/occupancy_train_ref.py's masked
                                     reference at the clipped depths, through parity.gate_grad's hard gate
    6 the Python surface             render_rays(grid=, clip_probes=) == the ops composition; a split call == the unsplit one;
                                     clip_probes without a grid raises
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import occupancy_clip_ref as cref  # noqa: E402
import occupancy_render_ref as ref  # noqa: E402
import occupancy_train_ref as tref  # noqa: E402
import sampler_ref as sref  # noqa: E402
from oracle import parity, synth  # noqa: E402

NEAR, FAR = cref.NEAR, cref.FAR
NAN = float("nan")
F = np.float32


def dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _grid(dense, box):
    from mirender import occupancy
    return occupancy.OccupancyGrid.from_dense(dense, box[0], box[1], dev())


_FIELDS = {}


def _field(kind, seed, grad=False, sharp="medium"):
    from mirender import fields
    key = (kind, seed, grad, sharp)
    if key not in _FIELDS:
        m = fields.field_from_state_dict(synth.state_dict(kind, seed=seed, sharp=sharp, bias_jitter=0.05), dev())
        for p in m.parameters():
            p.requires_grad_(grad)
        _FIELDS[key] = (m, fields.as_packed_field(m))
    return _FIELDS[key]


# ---- 1. the clip kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cref.CLIP_N)
def test_clip_kernel_against_the_restatement(n):
    from mirender import _lib
    lib = _lib.load()
    rays_cpu = cref.case_rays(n)
    rays = rays_cpu.to(dev())
    seen = set()
    for _n, m, name, dims, box in cref.clip_cases((n,)):
        dense = cref.case_dense(name, dims)
        grid = _grid(dense, box)
        k0, k1, hit = cref.first_last(cref.probe_mask(rays_cpu, NEAR, FAR, grid.lo, grid.inv_cell, dense, m))
        for pad in cref.CLIP_PAD:
            want = cref.bounds_from(k0, k1, hit, NEAR, FAR, m, pad)
            bounds = torch.full((n, 2), NAN, device=dev())
            rc = lib.mi_occupancy_clip_rays(_lib.ptr(grid.bits), *grid.c_args(), _lib.ptr(rays), n, NEAR, FAR, m, pad, _lib.ptr(bounds),
                                            _lib.stream_ptr(dev()))
            assert rc == 0, lib.mi_last_error()
            got = bounds.cpu().numpy()
            assert not np.isnan(got).any(), (n, m, name, dims, pad)                     # every row written
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (n, m, name, dims, box, pad)
        seen.add("none" if not hit.any() else "all" if hit.all() else "some")
    assert "none" in seen and ("some" in seen or "all" in seen)


def test_clip_through_ops_and_a_large_ray_count():
    """ops.occupancy_clip_rays, at a ray count past one sweep of the kernel's grid (4 rays per workgroup, at most 4096
    workgroups): 16 389 rays, every ray's row equal to the row of the same ray in a short call."""
    from mirender import ops
    n_small = 130
    rays = cref.case_rays(n_small).to(dev())
    dense = cref.case_dense("ones", (16, 16, 16))
    grid = _grid(dense, cref.SMALL)
    few = ops.occupancy_clip_rays(grid, rays, NEAR, FAR, 65, 1)
    want = cref.clip_bounds(rays.cpu(), NEAR, FAR, grid.lo, grid.inv_cell, dense, 65, 1)
    assert np.array_equal(few.cpu().numpy().view(np.int32), want.view(np.int32))
    n = 4 * 4096 + 5
    idx = torch.arange(n, device=dev()) % n_small
    many = ops.occupancy_clip_rays(grid, rays[idx].contiguous(), NEAR, FAR, 65, 1)
    assert _same(many, few[idx])


# ---- 2. / 3. the samplers with bounds ---------------------------------------------------------------------------------------------
def _varied_bounds(n, seed=5):
    """[n,2] on the device: near <= near_r < far_r <= far, the first ray the whole range, the second a narrow one."""
    g = torch.Generator().manual_seed(seed)
    a = NEAR + (FAR - NEAR) * 0.5 * torch.rand(n, generator=g)
    b = a + 0.05 + (FAR - a - 0.05) * torch.rand(n, generator=g)
    out = torch.stack([a, b], 1).to(torch.float32)
    out[0] = torch.tensor([NEAR, FAR])
    if n > 1:
        out[1] = torch.tensor([3.0, 3.0 + 2.0 ** -10])
    assert bool((out[:, 0] < out[:, 1]).all())
    return out.to(dev())


@pytest.mark.parametrize("nc", [1, 5, 64])
def test_sample_coarse_bounds(nc):
    from mirender import ops
    n = 37
    tr = synth.t_rand(n, nc, seed=9).to(dev())
    const = torch.tensor([[NEAR, FAR]], device=dev()).repeat(n, 1)
    varied = _varied_bounds(n)
    for kw in (dict(t_rand=tr), dict(seed=77, ray0=1000)):
        # constant bounds: the scalar call with the in-kernel linspace
        want = ops.sample_coarse(n, NEAR, FAR, nc, dev(), exact_linspace=False, **kw)
        assert _same(ops.sample_coarse_bounds(const, nc, **kw), want), (nc, sorted(kw))
        # varied bounds, ray by ray: the scalar call on that single ray, its jitter keyed by ray0 + r
        got = ops.sample_coarse_bounds(varied, nc, **kw)
        for r in range(n):
            one = dict(t_rand=tr[r:r + 1]) if "t_rand" in kw else dict(seed=77, ray0=1000 + r)
            lo, hi = float(varied[r, 0]), float(varied[r, 1])
            assert _same(got[r:r + 1], ops.sample_coarse(1, lo, hi, nc, dev(), exact_linspace=False, **one)), (nc, r, sorted(kw))
    # the restated formula (injected jitter)
    want = cref.sample_coarse_bounds(varied.cpu().numpy(), nc, tr)
    assert np.array_equal(ops.sample_coarse_bounds(varied, nc, t_rand=tr).cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("nc,nf", [(5, 3), (64, 128), (9, 0)])
def test_sample_fine_bounds(nc, nf):
    from mirender import ops
    n = 37
    g = torch.Generator().manual_seed(6)
    w = torch.rand(n, nc, generator=g) ** 4
    w[3] = 0.0                                                                   # one ray whose weights are all zero
    w = w.to(dev())
    const = torch.tensor([[NEAR, FAR]], device=dev()).repeat(n, 1)
    varied = _varied_bounds(n)
    tr = synth.t_rand(n, nc, seed=9).to(dev())
    # constant bounds against mi_sample_fine_pos with the in-kernel linspace (u_lin: the same table in both)
    z_c = ops.sample_coarse(n, NEAR, FAR, nc, dev(), tr, exact_linspace=False)
    want = _sample_fine_pos_no_zlin(z_c, w, NEAR, FAR, nf)
    got = ops.sample_fine_bounds(const, z_c, w, nf)
    for a, b, what in zip(got, want, ("z_fine", "z_samples", "pos")):
        assert _same(a, b), (nc, nf, what)
    # without the optional outputs: the same z_fine
    assert _same(ops.sample_fine_bounds(const, z_c, w, nf, want_pos=False), want[0])
    # varied bounds, ray by ray
    z_v = ops.sample_coarse_bounds(varied, nc, t_rand=tr)
    got = ops.sample_fine_bounds(varied, z_v, w, nf)
    for r in range(n):
        one = _sample_fine_pos_no_zlin(z_v[r:r + 1], w[r:r + 1], float(varied[r, 0]), float(varied[r, 1]), nf)
        for a, b, what in zip(got, one, ("z_fine", "z_samples", "pos")):
            assert _same(a[r:r + 1], b), (nc, nf, r, what)
    assert bool((got[0][:, 1:] >= got[0][:, :-1]).all())
    # ... and against the restatement on the CPU (tests/sampler_ref.py), so that a mistake both instances share shows too
    ul = ops.linspace_table(0.0, 1.0, nf, "cpu")
    want = sref.sample_fine_bounds(varied.cpu().numpy(), z_v.cpu().numpy(), w.cpu().numpy(), nf, None if ul is None else ul.numpy())
    for a, b, what in zip(got, (want[1], want[0], want[2]), ("z_fine", "z_samples", "pos")):
        a = a.cpu().numpy()
        assert np.array_equal(a, b) if what == "pos" else np.array_equal(sref.bits(a), sref.bits(b)), (nc, nf, what)
    zs_ref, zf_ref = cref.sample_fine_bounds(varied.cpu().numpy(), z_v.cpu(), w.cpu(), nf)
    assert _same(got[0].cpu(), zf_ref) and _same(got[1].cpu(), zs_ref)
    if nf:
        assert bool((got[1] >= varied[:, :1]).all()) and bool((got[1] <= varied[:, 1:]).all())


def _sample_fine_pos_no_zlin(z_c, w, near, far, nf):
    """mi_sample_fine_pos with z_lin = NULL (the in-kernel linspace) and the u table ops.sample_fine_bounds passes."""
    from mirender import _lib, ops
    n, nc = z_c.shape
    z_fine = torch.empty((n, nc + nf), dtype=torch.float32, device=dev())
    zs = torch.empty((n, nf), dtype=torch.float32, device=dev())
    pos = torch.empty((n, nc + nf), dtype=torch.int32, device=dev())
    ul = ops.linspace_table(0.0, 1.0, nf, dev())
    _lib.call("mi_sample_fine_pos", dev(), n, float(near), float(far), nc, nf, None, _lib.ptr(ul), _lib.ptr(z_c.contiguous()),
              _lib.ptr(w.contiguous()), _lib.ptr(zs), _lib.ptr(z_fine), _lib.ptr(pos))
    return z_fine, zs, pos


# ---- 4. the inference call against the composition of the stage calls ----------------------------------------------------------
N_FRONT = cref.N_SPECIAL - 1


def _finite_rays(n):
    """cref.case_rays without the NaN ray (the clip kernel's test keeps it): a NaN direction makes every output of its ray a NaN,
    which says nothing about a render.  The N_FRONT rays in front are the other special ones."""
    r = cref.case_rays(n + 1)
    return torch.cat([r[:1], r[2:]]).contiguous().to(dev())


def _render_c(name, pf_c, pf_f, rays, nc, nf, grid, tr, coarse_outputs=True, probes=None, pad=1, train=False):
    """mi_render_rays_occupancy[_clip][_train] from C with z_lin = NULL: (outputs, counts, workspace, saved)."""
    from mirender import _lib, ops
    lib = _lib.load()
    n = rays.shape[0]
    outs = ops._render_outputs(n, dev(), coarse_outputs)
    for o in outs:
        if o is not None:
            o.fill_(NAN)
    counts = torch.full((2,), -1, dtype=torch.int32, device=dev())
    extra = lib.mi_render_occupancy_train_extra_bytes if train else lib.mi_render_occupancy_extra_bytes
    ws_bytes = lib.mi_render_workspace_bytes(n, nc, nf) + extra(n, nc, nf)
    if probes is not None:
        ws_bytes += lib.mi_render_occupancy_clip_extra_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
    ul = ops.linspace_table(0.0, 1.0, nf, dev())
    args = [pf_c.kind, _lib.ptr(pf_c.refresh()), pf_f.kind, _lib.ptr(pf_f.refresh()), _lib.ptr(rays), n, NEAR, FAR, nc, nf,
            *((None,) if probes is None else (probes, pad)), _lib.ptr(ul), _lib.ptr(tr), 0, 0, _lib.ptr(grid.bits), *grid.c_args(),
            *[_lib.ptr(o) for o in outs], _lib.ptr(counts), _lib.ptr(ws), ws_bytes]
    saved = None
    if train:
        sv = lib.mi_render_occupancy_train_saved_bytes(pf_c.kind, pf_f.kind, n, nc, nf)
        saved = torch.empty(sv, dtype=torch.uint8, device=dev())
        args += [_lib.ptr(saved), sv]
    _lib.call(name, dev(), *args)
    torch.cuda.synchronize()
    return outs, counts.tolist(), ws, saved


def _composition(pf_c, pf_f, rays, nc, nf, grid, dense, tr, probes, pad):
    """clip, coarse bounds, mark, list forward, composite, fine bounds, mark, list forward, composite - from the stage calls.
    The mark and the list forward of a pass are stated as `where(mask, field, 0)` with the restated mask: what
    tests/test_gpu_occupancy_render.py holds mi_occupancy_mark_rays + mi_field_eval_rays_list to, bit for bit."""
    from mirender import ops
    bounds = ops.occupancy_clip_rays(grid, rays, NEAR, FAR, probes, pad)
    z_c = ops.sample_coarse_bounds(bounds, nc, t_rand=tr)
    m_c = ref.occupied_mask(rays, z_c, grid.lo, grid.inv_cell, dense).to(dev())
    zero = torch.zeros((), device=dev())
    raw_c = torch.where(m_c[..., None], ops.field_eval_rays(pf_c, rays, z_c), zero)
    rgb_c, depth_c, acc_c, w_c = ops.composite(raw_c, z_c, rays)
    z_f = ops.sample_fine_bounds(bounds, z_c, w_c, nf, want_pos=False)
    m_f = ref.occupied_mask(rays, z_f, grid.lo, grid.inv_cell, dense).to(dev())
    raw_f = torch.where(m_f[..., None], ops.field_eval_rays(pf_f, rays, z_f), zero)
    rgb_f, depth_f, acc_f, _ = ops.composite(raw_f, z_f, rays, want_weights=False)
    return [rgb_c, depth_c, acc_c, rgb_f, depth_f, acc_f], [int(m_c.sum()), int(m_f.sum())], bounds


RENDER_CASES = {
    "nerf_pair": ("nerf", 5, "nerf", 6, 64, 128),
    "tiny_nerf": ("tiny_nerf", 5, "tiny_nerf", 6, 5, 3),
    "siren_nerf_nf0": ("siren_nerf", 5, "siren_nerf", 6, 9, 0),
    "nerf_shared": ("nerf", 5, "nerf", 5, 12, 24),
}


@pytest.mark.parametrize("case", sorted(RENDER_CASES))
def test_clipped_render_equals_the_composition(case):
    kc, sc, kf, sf, nc, nf = RENDER_CASES[case]
    pf_c, pf_f = _field(kc, sc)[1], _field(kf, sf)[1]
    n = 37
    rays = _finite_rays(n)
    tr = synth.t_rand(n, nc, seed=9).to(dev())
    probes, pad = 65, 1
    for name, dims, box in (("random", (16, 16, 16), cref.SMALL), ("ones", (16, 16, 16), cref.SMALL)):
        dense = cref.case_dense(name, dims)
        grid = _grid(dense, box)
        want, wc, bounds = _composition(pf_c, pf_f, rays, nc, nf, grid, dense, tr, probes, pad)
        assert int(((bounds[:, 0] > NEAR) & (bounds[:, 1] < FAR)).sum()) >= 4                # the clip really moves bounds
        for coarse_outputs in (True, False):
            got, gc, _, _ = _render_c("mi_render_rays_occupancy_clip", pf_c, pf_f, rays, nc, nf, grid, tr, coarse_outputs, probes, pad)
            assert gc == wc, (case, name, gc, wc)
            assert 0 < gc[0] < n * nc and 0 < gc[1] < n * (nc + nf), gc
            for k in range(6):
                if got[k] is None:
                    assert k < 3 and not coarse_outputs
                    continue
                assert _same(got[k], want[k]), (case, name, coarse_outputs, k)
    # an all-ones grid over every probe: every bound is (near, far), the call is mi_render_rays_occupancy(z_lin = NULL)
    ok = slice(N_FRONT, None)                                                         # the camera's rays: every probe inside the box
    rays_in = rays[ok].contiguous()
    tr_in = tr[ok].contiguous()
    grid = _grid(np.ones((4, 4, 4), bool), ((-8.0,) * 3, (8.0,) * 3))
    for coarse_outputs in (True, False):
        want, wc, _, _ = _render_c("mi_render_rays_occupancy", pf_c, pf_f, rays_in, nc, nf, grid, tr_in, coarse_outputs)
        got, gc, _, _ = _render_c("mi_render_rays_occupancy_clip", pf_c, pf_f, rays_in, nc, nf, grid, tr_in, coarse_outputs, probes, pad)
        assert gc == wc == [rays_in.shape[0] * nc, rays_in.shape[0] * (nc + nf)]
        for k in range(6):
            assert (got[k] is None and want[k] is None) or _same(got[k], want[k]), (case, "ones", coarse_outputs, k)


# ---- 5. the training pair ------------------------------------------------------------------------------------------------------------
def _cots(n, seed=4):
    return [c.to(dev()) for c in tref.case_cots(n, seed)]


def _grads_of(models, fn):
    for m in models:
        for p in m.parameters():
            p.grad = None
    outs = fn()
    sum((o * c).sum() for o, c in zip(outs, _cots(outs[0].shape[0]))).backward()
    return [o.detach() for o in outs], [[p.grad.clone() for p in m.parameters()] for m in models]


@pytest.mark.parametrize("kinds", [("nerf", "nerf"), ("tiny_nerf", "siren_nerf")])
def test_clipped_training_forward_is_the_inference_call(kinds):
    """200 rays at 8 + 16 samples on a partial grid: the six outputs and the two counts of mi_render_rays_occupancy_clip_train
    equal mi_render_rays_occupancy_clip's, and the bounds both left behind their lists are the clip kernel's."""
    from mirender import ops
    n, nc, nf, probes, pad = 200, 8, 16, 64, 1
    pf_c, pf_f = _field(kinds[0], 5)[1], _field(kinds[1], 6)[1]
    rays = _finite_rays(n)
    tr = synth.t_rand(n, nc, seed=9).to(dev())
    grid = _grid(cref.case_dense("random", (16, 16, 16)), cref.SMALL)
    want, wc, ws_i, _ = _render_c("mi_render_rays_occupancy_clip", pf_c, pf_f, rays, nc, nf, grid, tr, True, probes, pad)
    got, gc, ws_t, _ = _render_c("mi_render_rays_occupancy_clip_train", pf_c, pf_f, rays, nc, nf, grid, tr, True, probes, pad, train=True)
    assert gc == wc and 0 < wc[0] < n * nc and 0 < wc[1] < n * (nc + nf), (gc, wc)
    for k in range(6):
        assert _same(got[k], want[k]), (kinds, k)
    bounds = ops.occupancy_clip_rays(grid, rays, NEAR, FAR, probes, pad)
    tail = (2 * n + 63) // 64 * 64 * 4
    for ws in (ws_i, ws_t):                                                       # the bounds region is the workspace's last
        assert _same(ws[-tail:].view(torch.float32)[:2 * n].reshape(n, 2), bounds)


@pytest.mark.parametrize("case", ["nerf_pair", "tiny_nerf", "siren_nerf_nf0", "nerf_seeded"])
def test_clipped_pair_with_an_all_ones_grid_equals_the_unclipped_pair(case):
    """Every bound (near, far): outputs and every gradient have the bits of occupancy_train.render_rays without clipping, run
    with the in-kernel linspace (mi_render_rays_occupancy_train with z_lin = NULL), which is what the bounds samplers evaluate."""
    from mirender import occupancy_train, ops
    cases = {"nerf_pair": ("nerf", 5, "nerf", 6, 12, 24, "t_rand"), "tiny_nerf": ("tiny_nerf", 5, "tiny_nerf", 6, 5, 3, "t_rand"),
             "siren_nerf_nf0": ("siren_nerf", 5, "siren_nerf", 6, 9, 0, "t_rand"), "nerf_seeded": ("nerf", 5, "nerf", 6, 12, 24, "seed")}
    kc, sc, kf, sf, nc, nf, jitter = cases[case]
    (mc, _), (mf, _) = _field(kc, sc, True), _field(kf, sf, True)
    n = 24
    rays = tref.case_rays(n).to(dev())
    kw = dict(t_rand=synth.t_rand(n, nc, seed=9).to(dev())) if jitter == "t_rand" else dict(seed=77, ray0=1000)
    grid = _grid(np.ones((4, 4, 4), bool), tref.BIG)
    tables = ops._lin_tables
    ops._lin_tables = lambda near, far, n_coarse, n_fine, device, exact_linspace=True: (None, tables(near, far, n_coarse, n_fine, device)[1])
    try:                                                                          # z_lin = NULL, the same u table
        want, gw = _grads_of((mc, mf), lambda: occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, grid=grid, **kw))
    finally:
        ops._lin_tables = tables
    got, gg = _grads_of((mc, mf), lambda: occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, grid=grid, clip_probes=33,
                                                                      clip_pad=0, **kw))
    for k in range(6):
        assert _same(got[k], want[k]), (case, k)
    for f in range(2):
        for i, (a, b) in enumerate(zip(gg[f], gw[f])):
            assert _same(a, b), (case, "coarse" if f == 0 else "fine", i)
            assert float(b.abs().max()) > 0


@pytest.mark.parametrize("case", sorted(tref.GRAD_CASES))
def test_clipped_pair_gradients_against_the_masked_oracle(case):
    """occupancy_train_ref.GRAD_CASES with each ray's range clipped (cref.CLIP_TRAIN_PROBES probes, pad cref.CLIP_TRAIN_PAD):
    tests/test_occupancy_clip_host.py shows the fp32 oracle of these cases inside the HARD gate against its fp64 self, so the
    hard gate is demanded here.  The reference is evaluated at the restated bounds' depths: the coarse depths from the
    restated sampler (bit-equal to the device's, checked here), the fine depths from the device's stage call on them."""
    from mirender import occupancy_train, ops
    kind, sc, sf, sharp, nc, nf, gname, dims, box = tref.GRAD_CASES[case]
    shared, full = sc == sf, case.endswith("_ones")
    (mc, pf_c), (mf, pf_f) = _field(kind, sc, True, sharp), _field(kind, sf, True, sharp)
    n = tref.N_RAYS
    rays, tr = tref.case_rays().to(dev()), tref.case_t_rand(nc).to(dev())
    dense = tref.case_dense(gname, dims)
    grid = _grid(dense, box)
    models = (mc,) if shared else (mc, mf)
    probes, pad = cref.CLIP_TRAIN_PROBES, cref.CLIP_TRAIN_PAD
    counts = []

    def run():
        outs, c = occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, grid=grid, t_rand=tr, return_counts=True,
                                              clip_probes=probes, clip_pad=pad)
        counts.append(c)
        return outs
    got, gg = _grads_of(models, run)
    again, gg2 = _grads_of(models, run)
    with torch.no_grad():
        want, wc = ops.render_rays_occupancy(pf_c, pf_f, rays, NEAR, FAR, nc, nf, grid, tr, clip_probes=probes, clip_pad=pad)
    assert counts[0].tolist() == [wc.tolist()], (counts, wc)
    if full:
        assert wc.tolist() == [n * nc, n * (nc + nf)]
    else:
        assert 0 < wc[0] < n * nc and 0 < wc[1] < n * (nc + nf), wc
    for k in range(6):
        assert _same(got[k], want[k]) and _same(again[k], want[k]), (case, k)
    for f in range(len(models)):
        assert all(_same(a, b) for a, b in zip(gg[f], gg2[f])), (case, "two runs")
    # the depths and masks of both passes at the restated bounds
    b_ref = cref.train_case_bounds(case)
    assert np.array_equal(ops.occupancy_clip_rays(grid, rays, NEAR, FAR, probes, pad).cpu().numpy().view(np.int32), b_ref.view(np.int32))
    z_c = torch.from_numpy(cref.sample_coarse_bounds(b_ref, nc, tr))
    b_dev = torch.from_numpy(b_ref).to(dev())
    assert _same(ops.sample_coarse_bounds(b_dev, nc, t_rand=tr).cpu(), z_c)
    m_c = ref.occupied_mask(rays, z_c, grid.lo, grid.inv_cell, dense)
    raw_c = torch.where(m_c.to(dev())[..., None], ops.field_eval_rays(pf_c, rays, z_c.to(dev())), torch.zeros((), device=dev()))
    w_c = ops.composite(raw_c, z_c.to(dev()), rays)[3]
    z_f = ops.sample_fine_bounds(b_dev, z_c.to(dev()), w_c, nf, want_pos=False)
    m_f = ref.occupied_mask(rays, z_f, grid.lo, grid.inv_cell, dense)
    assert [int(m_c.sum()), int(m_f.sum())] == wc.tolist()
    refs = tref.case_refs(case, z_c, m_c, z_f, m_f)
    names = tref.param_names(kind, tref.case_state_dicts(case)[0])
    recs = []
    for f in range(len(models)):
        for name, t in zip(names, gg[f]):
            recs.append(parity.gate_grad(f"occupancy clip train {case}", ("coarse." if f == 0 else "fine.") + name, t.cpu(),
                                         refs[torch.float32][f][name], refs[torch.float64][f][name], check=False,
                                         **tref.case_gates(kind)))
    print(f"clipped {case}: evaluated {wc.tolist()}, worst rel l2 {max(r['rel_l2_err'] for r in recs):.3g}, "
          f"worst elem/rms {max(r['max_elem_err_over_rms'] for r in recs):.3g}")
    bad = [r for r in recs if not r["passed"] or r["active"] != "hard"]
    assert not bad, bad[0]


# ---- 6. the Python surface ---------------------------------------------------------------------------------------------------------
def test_python_surface():
    from mirender import _lib, occupancy_train, ops, render_core
    (mc, pf_c), (mf, pf_f) = _field("tiny_nerf", 5), _field("tiny_nerf", 6)
    n, nc, nf, probes, pad = 24, 5, 3, 40, 2
    rays = _finite_rays(n)
    dense = cref.case_dense("random", (16, 16, 16))
    grid = _grid(dense, cref.SMALL)
    tr = synth.t_rand(n, nc, seed=9).to(dev())
    want, wc, _ = _composition(pf_c, pf_f, rays, nc, nf, grid, dense, tr, probes, pad)
    with torch.no_grad():
        got = render_core.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, grid=grid, t_rand=tr, clip_probes=probes, clip_pad=pad)
        named, counts = ops.render_rays_occupancy_clip(pf_c, pf_f, rays, NEAR, FAR, nc, nf, grid, probes, pad, t_rand=tr)
    assert counts.tolist() == wc
    for k in range(6):
        assert _same(got[k], want[k]) and _same(named[k], want[k]), k
    # a split call: bounds are per ray and the seeded jitter is keyed by ray0 + ray, so no bit changes
    kw = dict(grid=grid, seed=77, ray0=1000, clip_probes=probes, clip_pad=pad)
    (gc, _), (gf, _) = _field("tiny_nerf", 5, True), _field("tiny_nerf", 6, True)
    whole = occupancy_train.render_rays(rays, NEAR, FAR, gc, gf, nc, nf, **kw)
    parts = occupancy_train.render_rays(rays, NEAR, FAR, gc, gf, nc, nf, max_points=8 * (2 * nc + nf), **kw)
    with torch.no_grad():
        plain = render_core.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, **kw)
        halves = [render_core.render_rays(rays[a:b], NEAR, FAR, mc, mf, nc, nf, **{**kw, "ray0": 1000 + a}) for a, b in ((0, 7), (7, n))]
    for k in range(6):
        assert _same(whole[k].detach(), parts[k].detach()) and _same(whole[k].detach(), plain[k]), k
        assert _same(torch.cat([h[k] for h in halves]), plain[k]), k
    # a frame rendered in chunks of rays: render_image with one chunk per call against the frame's rays in one call
    W = H = 150                                                                # 22 500 rays: two calls of at most 16 384
    pose, focal = synth.pose_degrees(4.0, 20.0, -30.0), 200.0
    with torch.no_grad():
        rgb, depth, acc = render_core.render_image(W, H, focal, pose, NEAR, FAR, mc, mf, nc, nf, seed=3, grid=grid,
                                                   clip_probes=probes, clip_pad=pad)
        one = render_core.render_rays(ops.gen_rays(W, H, focal, pose, dev()), NEAR, FAR, mc, mf, nc, nf, seed=3, grid=grid,
                                      clip_probes=probes, clip_pad=pad)
    assert np.array_equal(rgb.reshape(-1, 3).view(np.int32), one[3].cpu().numpy().view(np.int32))
    assert np.array_equal(depth.reshape(-1).view(np.int32), one[4].cpu().numpy().view(np.int32))
    # clip_probes=None is today's call
    with torch.no_grad():
        a = render_core.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, grid=grid, seed=77, clip_probes=None)
        b = render_core.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, grid=grid, seed=77)
    assert all(_same(x, y) for x, y in zip(a, b))
    # clip_probes without a grid raises; so do bad clip arguments, by name
    with torch.no_grad():
        with pytest.raises(_lib.MiRenderError, match="needs grid="):
            render_core.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, seed=77, clip_probes=probes)
        with pytest.raises(_lib.MiRenderError, match="needs grid="):
            render_core.render_image(8, 8, 10.0, pose, NEAR, FAR, mc, mf, nc, nf, seed=77, clip_probes=probes)
        with pytest.raises(_lib.MiRenderError, match="probes"):
            render_core.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, seed=77, grid=grid, clip_probes=5000)
    with pytest.raises(TypeError):
        occupancy_train.render_rays(rays, NEAR, FAR, gc, gf, nc, nf, seed=77, clip_probes=probes)   # grid= is required there

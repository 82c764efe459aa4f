"""GPU: gradients to the rays with an occupancy grid (include/mi_render.h "gradients to the rays with a grid", mirender.pose
with grid=), layer by layer against the rule of DESIGN.md 4.8: only the listed samples send the rays a gradient, and each sends
what it sends without a grid.

    1 mi_field_input_grad_rays_list   compact dA / E rows of the real list forward and counted chain at the counts of
                                      tests/test_gpu_occupancy_train.py: value-equal to mi_field_input_grad_rays on the same
                                      rows expanded to full [P] buffers with zeros at the unlisted rows, and held per element
                                      to input_grad_gates.check_rays on those; rows at and past the count are NaN, the list's
                                      tail holds valid indices that are not entries (an int list has no NaN, and a wrong but
                                      valid index shows a read past the count as a wrong value, not as a fault); accumulate 0
                                      and 1; two runs; more rays than one sweep of the launch
    2 the pair with an all-ones grid  two fields: outputs, parameter gradients and rays.grad == pose.render_rays without a grid;
                                      one shared field: outputs ==, gradients gated (its sums run over other rows)
    3 the pair with a partial grid    occupancy_train_ref.GRAD_CASES: outputs and parameter gradients == occupancy_train.render_rays;
                                      rays.grad against tests/occupancy_pose_ref.py through parity.gate_grad's hard gate at the
                                      launch's own depths; an all-zero grid gives rays.grad == 0
    4 clipping and the surface        one case with clip_probes at the clipped depths; max_points; no_grad and rays without
                                      requires_grad; render_image_tensor(grid=); what is not built
    5 a ten-step pose loop            with a grid that lists every sample, against the same loop without a grid
"""
import ctypes
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bwd_gates as G  # noqa: E402
import input_grad_gates as D  # noqa: E402
import occupancy_clip_ref as cref  # noqa: E402
import occupancy_pose_ref as pref  # noqa: E402
import occupancy_render_ref as ref  # noqa: E402
import occupancy_train_ref as tref  # noqa: E402
import test_gpu_occupancy_train as T  # noqa: E402
import test_gpu_pose_grad as PG  # noqa: E402
from oracle import parity, synth  # noqa: E402

NEAR, FAR = T.NEAR, T.FAR
NAN = float("nan")
KINDS = T.KINDS
N, S = T.N, T.S                                # 37 rays x 7 samples = 259 points
COUNTS = (0, 1, 31, 32, 33, 128, 129, 259)
BIG = ((-8.0,) * 3, (8.0,) * 3)
CLIP_CASE = "nerf_random"                      # tests/test_occupancy_pose_host.py conditions it at the clipped oracle depths


def dev():
    return T.dev()


def _par(params):
    return (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])


# ---- 1. the stage call ---------------------------------------------------------------------------------------------------------
def _list_state(kind, n, s, lst, c):
    """The list-driven training forward and the counted backward over list[:c] of n rays x s samples, acts / grads_ws / raw NaN
    beforehand: the compact rows mi_field_input_grad_rays_list reads, and the same rows expanded to full [P] buffers (zeros at
    the unlisted rows) for mi_field_input_grad_rays."""
    from mirender import _lib, ops
    lib = _lib.load()
    pf = T._field(kind, 5)[1]
    k, P = pf.kind, n * s
    stream = _lib.stream_ptr(dev())
    rays = T._rays(n)
    z = ops.sample_coarse(n, NEAR, FAR, s, dev(), synth.t_rand(n, s, seed=9).to(dev()))
    lst_d, count = lst.to(dev()), torch.tensor([c], dtype=torch.int32, device=dev())
    acts = torch.full((lib.mi_field_train_acts_floats(k) * P,), NAN, device=dev())
    raw = torch.full((P, 4), NAN, device=dev())
    rc = lib.mi_field_eval_rays_list_train(k, _lib.ptr(pf.refresh()), _lib.ptr(rays), _lib.ptr(z), n, s, _lib.ptr(lst_d), _lib.ptr(count),
                                           _lib.ptr(raw), _lib.ptr(acts), stream)
    assert rc == 0, lib.mi_last_error()
    idx = lst_d[:c].to(torch.int64)
    listed = torch.zeros(P, dtype=torch.bool, device=dev())
    listed[idx] = True
    g = torch.Generator(device=dev()).manual_seed(3)
    mag = 10.0 ** (4.0 * torch.rand(n, 1, 1, device=dev(), generator=g) - 3.0)
    g_raw = (torch.randn(n, s, 4, device=dev(), generator=g) * mag).reshape(P, 4)
    g_raw = torch.where(listed[:, None], g_raw, torch.full((), NAN, device=dev())).contiguous()
    gws = torch.full((lib.mi_field_train_grads_floats(k) * P,), NAN, device=dev())
    part = torch.full((lib.mi_field_bwd_partial_floats_kind(k, P),), NAN, device=dev())
    out = [torch.full_like(p, NAN) for p in pf.params]
    rc = lib.mi_field_backward_list(k, _lib.ptr(pf.refresh_bwd()), _lib.ptr(acts), _lib.ptr(gws), _lib.ptr(raw), _lib.ptr(g_raw),
                                    _lib.ptr(lst_d), _lib.ptr(count), P, _lib.ptr(part), _par(out), stream)
    assert rc == 0, lib.mi_last_error()
    acts_full, gws_full = torch.zeros_like(acts), torch.zeros_like(gws)
    for layout, compact, full in ((G.ACTS[kind], acts, acts_full), (G.GRADS[kind], gws, gws_full)):
        C, F = G.regions(layout, compact, P), G.regions(layout, full, P)
        for name, _w in layout:
            assert bool(torch.isnan(C[name][c:]).all()), (kind, c, name)       # rows at and past the count: NaN, as prefilled
            F[name][idx] = C[name][:c]
    torch.cuda.synchronize()
    return dict(pf=pf, k=k, n=n, s=s, P=P, rays=rays, z=z, lst=lst_d, count=count, acts=acts, gws=gws, acts_full=acts_full,
                gws_full=gws_full, A=G.regions(G.ACTS[kind], acts_full, P), D=G.regions(G.GRADS[kind], gws_full, P))


def _list_form(st, accumulate=0, into=None):
    from mirender import _lib
    lib = _lib.load()
    if into is None:
        into = torch.full((st["n"], 2, 3), NAN, device=dev())
    par = st["pf"].params
    _lib.check(lib.mi_field_input_grad_rays_list(st["k"], _par(par), len(par), _lib.ptr(st["acts"]), _lib.ptr(st["gws"]),
                                                 _lib.ptr(st["lst"]), _lib.ptr(st["count"]), st["P"], _lib.ptr(st["rays"]),
                                                 _lib.ptr(st["z"]), st["n"], st["s"], accumulate, _lib.ptr(into),
                                                 _lib.stream_ptr(dev())), "mi_field_input_grad_rays_list")
    return into


def _plain_form(st):
    from mirender import _lib
    lib = _lib.load()
    into = torch.full((st["n"], 2, 3), NAN, device=dev())
    par = st["pf"].params
    _lib.check(lib.mi_field_input_grad_rays(st["k"], _par(par), len(par), None, _lib.ptr(st["acts_full"]), _lib.ptr(st["gws_full"]),
                                            _lib.ptr(st["rays"]), _lib.ptr(st["z"]), 1, st["n"], st["s"], 0, _lib.ptr(into),
                                            _lib.stream_ptr(dev())), "mi_field_input_grad_rays")
    return into


def _check_stage(case, kind, st, c):
    got, want = _list_form(st), _plain_form(st)
    assert bool(torch.isfinite(got).all()), case                            # no NaN row, no entry past the count was read
    assert torch.equal(got, want), (case, float((got - want).abs().max()))
    assert D.check_rays(case, kind, got, st["A"], st["D"], st["pf"].params, None, st["n"], st["rays"], st["z"]), case
    assert torch.equal(_list_form(st), got), (case, "two runs")
    base = torch.randn(got.shape, device=dev(), generator=torch.Generator(device=dev()).manual_seed(c + 1))
    assert torch.equal(_list_form(st, accumulate=1, into=base.clone()), base + got), (case, "accumulate")
    if c == 0:
        assert bool((got == 0).all()), case
    # a ray without a listed sample gets exact zeros, and keeps what it holds under accumulate (checked above: base + 0)
    runs = pref.ray_runs(st["lst"].cpu().numpy(), c, st["n"], st["s"])
    empty = torch.from_numpy(runs[:, 0] == runs[:, 1]).to(dev())
    assert bool((got[empty] == 0).all()), case
    return int(empty.sum())


@pytest.mark.parametrize("kind", KINDS)
def test_list_form_equals_the_plain_form_on_expanded_rows(kind):
    seen_empty = 0
    for c in COUNTS:
        st = _list_state(kind, N, S, T._sorted_subset(c, seed=c), c)
        seen_empty += _check_stage(f"occupancy pose stage {kind} count {c} of {T.P}", kind, st, c)
    assert seen_empty > 0
    # the list a random grid gives: whole stretches of a ray listed or not, as the mark writes them
    from mirender import ops
    dense = T._dense("random", (16, 16, 16))
    grid = T._grid(dense, T.BOX)
    z = ops.sample_coarse(N, NEAR, FAR, S, dev(), synth.t_rand(N, S, seed=9).to(dev()))
    mask = ref.occupied_mask(T._rays(N), z, grid.lo, grid.inv_cell, dense).reshape(-1)
    head = torch.nonzero(mask).reshape(-1).to(torch.int32)
    c = head.numel()
    assert 0 < c < T.P
    lst = torch.cat([head, torch.randperm(T.P, generator=torch.Generator().manual_seed(2)).to(torch.int32)])[:T.P]
    _check_stage(f"occupancy pose stage {kind} random grid, {c} of {T.P}", kind, _list_state(kind, N, S, lst, c), c)


@pytest.mark.parametrize("kind", ["nerf", "siren_nerf"])
def test_list_form_past_one_sweep_of_the_launch(kind):
    """More rays than the largest grid takes at once: a wave's loop runs `u += stride` and searches a second run."""
    pe = kind in D.PE_KINDS
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, s = D.sweep_units(pe, cus) + 5, 3
    blocks, stride = D.launch_plan(pe, n, cus)
    assert stride < n
    P = n * s
    gen = torch.Generator().manual_seed(5)
    c = P // 3
    lst = torch.cat([torch.sort(torch.randperm(P, generator=gen)[:c]).values, torch.randperm(P, generator=gen)])[:P].to(torch.int32)
    st = _list_state(kind, n, s, lst, c)
    _check_stage(f"occupancy pose stage wrap {kind} {n}x{s}, {c} listed", kind, st, c)


# ---- 2. - 5. the pair, through the Python surface ---------------------------------------------------------------------------------
def _run(models, fn, rays):
    """fn(rays_req) -> outs under autograd with the fixed cotangents: (outs, [[grads] per model], rays.grad)."""
    for m in models:
        for p in m.parameters():
            p.grad = None
    rays_req = rays.clone().requires_grad_(True)
    outs = fn(rays_req)
    T._loss(outs, T._cots(outs[0].shape[0])).backward()
    return [o.detach() for o in outs], [[p.grad.clone() for p in m.parameters()] for m in models], rays_req.grad


@pytest.mark.parametrize("case", sorted(T.PAIR_CASES))
def test_pair_with_an_all_ones_grid_equals_pose_without_a_grid(case):
    from mirender import pose
    kc, sc, kf, sf, nc, nf, jitter = T.PAIR_CASES[case]
    (mc, _), (mf, _) = T._field(kc, sc, True), T._field(kf, sf, True)
    shared = mc is mf
    models = (mc,) if shared else (mc, mf)
    n = 24
    rays = T._rays(n)
    kw = dict(t_rand=synth.t_rand(n, nc, seed=9).to(dev())) if jitter == "t_rand" else dict(seed=77, ray0=1000)
    grid = T._grid(np.ones((4, 4, 4), bool), BIG)
    want, gw, rw = _run(models, lambda r: pose.render_rays(r, NEAR, FAR, mc, mf, nc, nf, **kw), rays)
    got, gg, rg = _run(models, lambda r: pose.render_rays(r, NEAR, FAR, mc, mf, nc, nf, grid=grid, **kw), rays)
    assert rg is not None and bool(torch.isfinite(rg).all()) and float(rg.abs().max()) > 0
    for k in range(6):
        assert T._same(got[k], want[k]), (case, k)
    if shared:
        # one field: without a grid the Nc coarse rows carry the sum of both composites' gradients and the Nf new rows follow;
        # with a grid both passes run over all their rows (no merge): the same gradient, other sums
        for i, (a, b) in enumerate(zip(gg[0], gw[0])):
            rec = parity.gate_grad(f"occupancy pose {case}: all-ones grid against pose without a grid", f"p{i}", a.cpu(), b.cpu(), None,
                                   tol=parity.GRAD_TOL_RELU, check=True)
            assert rec["rel_l2_err"] <= 1e-4, rec
        for j, part in enumerate(("rays origin", "rays direction")):
            rec = parity.gate_grad(f"occupancy pose {case}: all-ones grid against pose without a grid", part, rg[:, j].cpu(),
                                   rw[:, j].cpu(), None, tol=parity.GRAD_TOL_RELU, check=True)
            assert rec["rel_l2_err"] <= 1e-4, rec
        return
    for f in range(2):
        for i, (a, b) in enumerate(zip(gg[f], gw[f])):
            assert T._same(a, b), (case, "coarse" if f == 0 else "fine", i)
    assert torch.equal(rg, rw), (case, float((rg - rw).abs().max()))


def _gate_rays(case, label, rg, refs, kind):
    recs = [parity.gate_grad(label, part, rg[:, j].cpu(), refs[torch.float32][:, j], refs[torch.float64][:, j], check=False,
                             **tref.case_gates(kind)) for j, part in enumerate(("rays origin", "rays direction"))]
    print(f"{label}: rays.grad rel l2 {[float('%.3g' % r['rel_l2_err']) for r in recs]}, worst elem/rms "
          f"{max(r['max_elem_err_over_rms'] for r in recs):.3g}, fp32 oracle rel l2 "
          f"{[float('%.3g' % r['oracle32_rel_l2_from_fp64']) for r in recs]}")
    bad = [r for r in recs if not r["passed"] or r["active"] != "hard"]
    assert not bad, bad[0]


@pytest.mark.parametrize("case", sorted(tref.GRAD_CASES))
def test_pair_ray_gradient_against_the_masked_oracle(case):
    """The cases tests/test_occupancy_pose_host.py shows inside the HARD gate on the CPU: the hard gate is demanded here."""
    from mirender import occupancy_train, pose
    kind, sc, sf, sharp, nc, nf, gname, dims, box = tref.GRAD_CASES[case]
    shared = sc == sf
    (mc, pf_c), (mf, _) = T._field(kind, sc, True, sharp), T._field(kind, sf, True, sharp)
    rays, tr = tref.case_rays().to(dev()), tref.case_t_rand(nc).to(dev())
    dense = tref.case_dense(gname, dims)
    grid = T._grid(dense, box)
    models = (mc,) if shared else (mc, mf)
    want, gw = T._grads_of(models, lambda: occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, grid=grid, t_rand=tr))
    got, gg, rg = _run(models, lambda r: pose.render_rays(r, NEAR, FAR, mc, mf, nc, nf, grid=grid, t_rand=tr), rays)
    _, _, rg2 = _run(models, lambda r: pose.render_rays(r, NEAR, FAR, mc, mf, nc, nf, grid=grid, t_rand=tr), rays)
    for k in range(6):
        assert T._same(got[k], want[k]), (case, k)
    for f in range(len(models)):
        assert all(T._same(a, b) for a, b in zip(gg[f], gw[f])), (case, "parameter gradients")
    assert bool(torch.isfinite(rg).all()) and T._same(rg, rg2), (case, "two runs")
    z_c, m_c, z_f, m_f = T._stage_depths(pf_c, rays, nc, nf, grid, dense, tr)
    _gate_rays(case, f"occupancy pose {case}", rg, pref.case_ray_grads(case, z_c, m_c, z_f, m_f), kind)


def test_all_zero_grid_gives_a_zero_ray_gradient():
    from mirender import pose
    (mc, _), (mf, _) = T._field("nerf", 5, True), T._field("nerf", 6, True)
    n, nc, nf = 24, 12, 24
    grid = T._grid(np.zeros((16, 16, 16), bool), T.BOX)
    tr = synth.t_rand(n, nc, seed=9).to(dev())
    outs, grads, rg = _run((mc, mf), lambda r: pose.render_rays(r, NEAR, FAR, mc, mf, nc, nf, grid=grid, t_rand=tr), T._rays(n))
    assert bool((outs[3] == 1).all()) and all(bool((g == 0).all()) for f in grads for g in f)
    assert rg is not None and bool((rg == 0).all())


def test_clipped_pair_ray_gradient_against_the_masked_oracle():
    """CLIP_CASE with each ray's range clipped, at the depths tests/test_gpu_occupancy_clip.py takes: the restated bounds, the
    restated coarse sampler on them (bit-equal to the device's, checked here), the device's fine stage call."""
    from mirender import occupancy_train, ops, pose
    case = CLIP_CASE
    kind, sc, sf, sharp, nc, nf, gname, dims, box = tref.GRAD_CASES[case]
    (mc, pf_c), (mf, _) = T._field(kind, sc, True, sharp), T._field(kind, sf, True, sharp)
    rays, tr = tref.case_rays().to(dev()), tref.case_t_rand(nc).to(dev())
    dense = tref.case_dense(gname, dims)
    grid = T._grid(dense, box)
    probes, pad = cref.CLIP_TRAIN_PROBES, cref.CLIP_TRAIN_PAD
    kw = dict(grid=grid, t_rand=tr, clip_probes=probes, clip_pad=pad)
    want, gw = T._grads_of((mc, mf), lambda: occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, **kw))
    got, gg, rg = _run((mc, mf), lambda r: pose.render_rays(r, NEAR, FAR, mc, mf, nc, nf, **kw), rays)
    for k in range(6):
        assert T._same(got[k], want[k]), k
    assert all(T._same(a, b) for f in range(2) for a, b in zip(gg[f], gw[f]))
    b_ref = cref.train_case_bounds(case)
    assert np.array_equal(ops.occupancy_clip_rays(grid, rays, NEAR, FAR, probes, pad).cpu().numpy().view(np.int32), b_ref.view(np.int32))
    z_c = torch.from_numpy(cref.sample_coarse_bounds(b_ref, nc, tr))
    b_dev = torch.from_numpy(b_ref).to(dev())
    assert T._same(ops.sample_coarse_bounds(b_dev, nc, t_rand=tr).cpu(), z_c)
    m_c = ref.occupied_mask(rays, z_c, grid.lo, grid.inv_cell, dense)
    raw_c = torch.where(m_c.to(dev())[..., None], ops.field_eval_rays(pf_c, rays, z_c.to(dev())), torch.zeros((), device=dev()))
    w_c = ops.composite(raw_c, z_c.to(dev()), rays)[3]
    z_f = ops.sample_fine_bounds(b_dev, z_c.to(dev()), w_c, nf, want_pos=False)
    m_f = ref.occupied_mask(rays, z_f, grid.lo, grid.inv_cell, dense)
    assert 0 < int(m_c.sum()) < m_c.numel() and 0 < int(m_f.sum()) < m_f.numel()
    _gate_rays(case, f"occupancy pose clipped {case}", rg, pref.case_ray_grads(case, z_c, m_c, z_f, m_f), kind)


def test_python_surface_chunks_no_grad_image_and_refusals():
    from mirender import _lib, fields, occupancy_train, pose
    (mc, _), (mf, _) = T._field("tiny_nerf", 5, True), T._field("tiny_nerf", 6, True)
    n, nc, nf = 24, 5, 3
    rays = T._rays(n)
    grid = T._grid(T._dense("random", (16, 16, 16)), T.BOX)
    kw = dict(grid=grid, seed=77, ray0=1000)
    whole, _, rw = _run((mc, mf), lambda r: pose.render_rays(r, NEAR, FAR, mc, mf, nc, nf, **kw), rays)
    parts, _, rp = _run((mc, mf), lambda r: pose.render_rays(r, NEAR, FAR, mc, mf, nc, nf, max_points=8 * (2 * nc + nf), **kw), rays)
    assert float(rw.abs().max()) > 0
    for k in range(6):
        assert T._same(whole[k], parts[k]), k                               # three calls of 8 rays: the same samples
    assert T._same(rw, rp)                                                  # disjoint ray slices: the same bits
    clipped = dict(kw, clip_probes=64)
    _, _, rc1 = _run((mc, mf), lambda r: pose.render_rays(r, NEAR, FAR, mc, mf, nc, nf, **clipped), rays)
    _, _, rc3 = _run((mc, mf), lambda r: pose.render_rays(r, NEAR, FAR, mc, mf, nc, nf, max_points=8 * (2 * nc + nf), **clipped), rays)
    assert T._same(rc1, rc3)
    # no_grad, and rays that need no gradient: occupancy_train.render_rays' outputs (and its graph to the parameters)
    with torch.no_grad():
        a = pose.render_rays(rays.clone().requires_grad_(True), NEAR, FAR, mc, mf, nc, nf, **kw)
        b = occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, **kw)
    assert all(T._same(x, y) for x, y in zip(a, b)) and all(T._same(x, y) for x, y in zip(a, whole))
    want, gw = T._grads_of((mc, mf), lambda: occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, **kw))
    got, gg = T._grads_of((mc, mf), lambda: pose.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, **kw))
    assert all(T._same(x, y) for x, y in zip(got, want)) and all(T._same(x, y) for f in range(2) for x, y in zip(gg[f], gw[f]))
    # a frame: c2w.grad through get_rays
    c2w = torch.from_numpy(synth.pose_degrees(4.0, 20.0, -30.0)[:3].astype(np.float32).copy()).to(dev()).requires_grad_(True)
    img = pose.render_image_tensor(12, 10, 16.5, c2w, NEAR, FAR, mc, mf, nc, nf, chunk=50, seed=3, grid=grid, clip_probes=32)
    assert tuple(img.shape) == (10, 12, 3)
    (img * torch.linspace(0.5, 1.5, 360, device=dev()).reshape(10, 12, 3)).sum().backward()
    assert c2w.grad is not None and bool(torch.isfinite(c2w.grad).all()) and float(c2w.grad.abs().max()) > 0
    # what is not built, by name
    req = rays.clone().requires_grad_(True)
    film = fields.FilmSirenNeRF().to(dev())
    film.set_film_params(synth.film_params(1)[0].to(dev()))
    with pytest.raises(_lib.MiRenderError, match="FiLM kinds"):
        pose.render_rays(req, NEAR, FAR, film, film, 8, 8, **kw)
    with pytest.raises(_lib.MiRenderError, match="film="):
        pose.render_rays(req, NEAR, FAR, mc, mf, nc, nf, film=synth.film_params(1).to(dev()), **kw)
    with pytest.raises(_lib.MiRenderError, match="generic callables"):
        pose.render_rays(req, NEAR, FAR, lambda x: torch.zeros(x.shape[0], 4, device=x.device), mf, 8, 8, **kw)
    other = types.SimpleNamespace(device=torch.device("cuda", 1), bits=grid.bits, dims=grid.dims, lo=grid.lo, inv_cell=grid.inv_cell)
    with pytest.raises(_lib.MiRenderError, match="is on"):
        pose.render_rays(req, NEAR, FAR, mc, mf, nc, nf, grid=other, seed=77)
    with pytest.raises(_lib.MiRenderError, match="grid="):
        pose.render_rays(req, NEAR, FAR, mc, mf, nc, nf, clip_probes=8, seed=77)
    # occupancy_train keeps refusing, and says where the gradient is
    with pytest.raises(_lib.MiRenderError, match=r"gradients to the rays.*pose\.render_rays\(grid=\)"):
        occupancy_train.render_rays(req, NEAR, FAR, mc, mf, nc, nf, **kw)


def test_pose_loop_with_a_grid_follows_the_loop_without():
    """tests/test_gpu_pose_grad.py's refinement loop (a 24 x 24 view of a synthetic SirenNeRF, 12 + 12 samples, ten Adam steps on
    the six pose parameters) with a grid that lists every sample - all cells set, in a box that holds every ray's range - against
    the same loop without a grid, each step's loss within that test's 1 %."""
    from mirender import pose, render_core
    W = H = 24
    focal, near, far, nc, nf, steps, lr = 33.0, 2.0, 6.0, 12, 12, 10, 2e-3
    m = PG._module("siren_nerf", synth.state_dict("siren_nerf", 60, "medium", 0.05))
    for p in m.parameters():
        p.requires_grad_(False)                       # the field is fixed: only the pose is optimised
    true = torch.from_numpy(synth.pose_degrees(4.0, 15.0, -30.0)[:3].astype(np.float32).copy()).to(dev())
    tr = synth.t_rand(W * H, nc, seed=61).to(dev())
    grid = T._grid(np.ones((8, 8, 8), bool), BIG)
    with torch.no_grad():
        target = render_core.render_rays(pose.get_rays(W, H, focal, true), near, far, m, m, nc, nf, t_rand=tr)[3]

    def loop(**kw):
        w = torch.tensor([0.02, -0.02, 0.01], device=dev(), requires_grad=True)
        t = torch.tensor([0.03, -0.02, 0.03], device=dev(), requires_grad=True)
        opt = torch.optim.Adam([w, t], lr=lr)
        losses = []
        for _ in range(steps):
            opt.zero_grad()
            rgb = pose.render_rays(pose.get_rays(W, H, focal, PG._pose_of(true, w, t)), near, far, m, m, nc, nf, t_rand=tr, **kw)[3]
            loss = torch.mean((rgb - target) ** 2)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return losses

    plain, gridded = loop(), loop(grid=grid)
    rel = np.abs(np.array(gridded) - np.array(plain)) / np.array(plain)
    print("losses without a grid", plain, "with", gridded)
    assert np.isfinite(gridded).all() and gridded[-1] < gridded[0]
    assert rel.max() <= 0.01, (int(rel.argmax()), float(rel.max()))

"""GPU: training with an occupancy grid, stage by stage (include/mi_render.h "training with a grid",
mirender.occupancy_train).  Bit equality wherever rows are independent of each other.

    1 mi_occupancy_mark_rays_ordered   list == the ascending indices of the restatement's mask; the count; unlisted raw rows
                                       zeroed, listed rows untouched; two runs give the same list; against the atomic mark
                                       around the 4096-point workgroup: the same points, count and raw
    2 mi_field_eval_rays_list_train    raw[list[e]] and saved row e == mi_field_eval_rays_train's rows list[e], every region;
                                       rows at and past the count and unlisted raw rows keep a NaN sentinel
    3 the counted chain                every dA region, row e == the plain chain's row list[e]
    4 the counted weight gradients     dW, db against bwd_gates.stage_c_ref from the kernel's own compact dA / X rows, L from the
                                       restated device rule; NaN scratch and NaN rows past the count change nothing; the list of
                                       all points gives mi_field_backward's bits
    5 the pair with an all-ones grid   outputs and every gradient == the plain training path's; one shared field: outputs ==,
                                       gradients gated (its sums run over other rows)
    6 the pair with a partial grid     outputs == mi_render_rays_occupancy (also from C, across a mark workgroup); gradients
                                       against tests/occupancy_train_ref.py through parity.gate_grad's hard gate (sharp and plain heads; one shared field, also at full
                                       occupancy); two runs equal; an all-zero grid gives gradients exactly 0
    7 the Python surface               chunks by max_points, no_grad, what is not built, ten optimiser steps
"""
import ctypes
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bwd_gates as G  # noqa: E402
import occupancy_render_ref as ref  # noqa: E402
import occupancy_train_ref as tref  # noqa: E402
from oracle import parity, render_ref as R, synth  # noqa: E402

NEAR, FAR = 2.0, 6.0
BOX = ((-4.0,) * 3, (4.0,) * 3)              # holds every sample of the rays below (camera at radius 4, depths 2..6)
SMALL = ((-1.5,) * 3, (1.5,) * 3)            # a box the rays partly leave
NAN = float("nan")
KINDS = ["nerf", "tiny_nerf", "siren_nerf"]
N, S = 37, 7                                 # 259 points: two tiles and a partial one; two dW slabs
P = N * S
COUNTS = (100, 0, 1, 31, 32, 33, 128, 129, 259)


def dev():
    return torch.device("cuda", 0)


def _rays(n):
    r = torch.from_numpy(R.rays_from_camera(40, 40, 55.0, synth.pose_degrees(4.0, 20.0, -30.0)))
    idx = (torch.arange(n) * 1600 // n + 20) % 1600
    return r[idx].contiguous().to(dev())


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


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- 1. the ordered mark ------------------------------------------------------------------------------------------------------
MARK_GRIDS = [("random", (5, 7, 3), BOX), ("random", (16, 16, 16), BOX), ("zeros", (16, 16, 16), BOX), ("ones", (5, 7, 3), BOX),
              ("ones", (16, 16, 16), SMALL), ("random", (16, 16, 16), SMALL)]


@pytest.mark.parametrize("n,s", [(37, 5), (130, 192)])
def test_ordered_mark(n, s):
    from mirender import _lib, ops
    lib = _lib.load()
    rays = _rays(n)
    z = ops.sample_coarse(n, NEAR, FAR, s, dev(), synth.t_rand(n, s, seed=9).to(dev()))
    ints = lib.mi_occupancy_ordered_list_ints(n, s)
    assert ints == n * s + (n * s + 4095) // 4096
    seen = set()
    for name, dims, box in MARK_GRIDS:
        dense = _dense(name, dims)
        grid = _grid(dense, box)
        want = ref.occupied_mask(rays, z, grid.lo, grid.inv_cell, dense).reshape(-1)
        d, lo, inv = _grid_args(grid)
        lists = []
        for with_raw in (True, False):
            lst = torch.full((ints,), -1, dtype=torch.int32, device=dev())
            count = torch.full((1,), 12345, dtype=torch.int32, device=dev())
            raw = torch.full((n, s, 4), NAN, device=dev()) if with_raw else None
            rc = lib.mi_occupancy_mark_rays_ordered(_lib.ptr(grid.bits), d, lo, inv, _lib.ptr(rays), _lib.ptr(z), n, s,
                                                    _lib.ptr(lst), _lib.ptr(count), _lib.ptr(raw), _lib.stream_ptr(dev()))
            assert rc == 0, lib.mi_last_error()
            c = int(count.item())
            assert c == int(want.sum()), (name, dims, box)
            got = lst.cpu()
            assert torch.equal(got[:c].to(torch.int64), torch.nonzero(want).reshape(-1)), (name, dims, box)   # ascending
            assert bool((got[c:n * s] == -1).all())                      # nothing between the count and the scan slots
            if with_raw:
                rows = raw.cpu().reshape(-1, 4)
                assert torch.equal(rows[~want], torch.zeros(int((~want).sum()), 4)), (name, dims, box)
                assert bool(torch.isnan(rows[want]).all()), (name, dims, box)
            lists.append(got[:c])
        assert torch.equal(lists[0], lists[1])                            # two runs: the same list
        seen.add("none" if c == 0 else "all" if c == n * s else "some")
    assert seen == {"none", "all", "some"}


def _mark(ordered, grid, rays, z, sentinel):
    """One of the two marks over rays x z: (list[:count] on the host, count, raw after the call), raw prefilled with `sentinel`."""
    from mirender import _lib
    lib = _lib.load()
    n, s = z.shape
    ints = lib.mi_occupancy_ordered_list_ints(n, s) if ordered else n * s
    lst = torch.full((ints,), -1, dtype=torch.int32, device=dev())
    count = torch.full((1,), 12345, dtype=torch.int32, device=dev())
    raw = torch.full((n, s, 4), sentinel, device=dev())
    call = lib.mi_occupancy_mark_rays_ordered if ordered else lib.mi_occupancy_mark_rays
    d, lo, inv = _grid_args(grid)
    rc = call(_lib.ptr(grid.bits), d, lo, inv, _lib.ptr(rays), _lib.ptr(z), n, s, _lib.ptr(lst), _lib.ptr(count), _lib.ptr(raw),
              _lib.stream_ptr(dev()))
    assert rc == 0, lib.mi_last_error()
    c = int(count.item())
    return lst.cpu()[:c], c, raw


# 1, then either side of the mark kernels' 4096-point workgroup, then a third workgroup with a short tail
@pytest.mark.parametrize("n,s", [(1, 1), (819, 5), (1024, 4), (241, 17), (1171, 7)])
def test_the_two_marks_agree(n, s):
    """mi_occupancy_mark_rays (one atomic per workgroup, any order) and mi_occupancy_mark_rays_ordered (count, scan, scatter) on
    the same grid, rays and depths: the same set of points, the same count, the same raw afterwards."""
    assert n * s in (1, 4095, 4096, 4097, 2 * 4096 + 5)
    sentinel = -7.25
    rays = _rays(n)
    z = (NEAR + (FAR - NEAR) * torch.rand(n, s, generator=torch.Generator().manual_seed(11))).to(dev())
    # one point: a grid that lists it and one that does not; otherwise a grid that lists a part of the points
    names = ("ones", "zeros") if n * s == 1 else ("random",)
    for name in names:
        grid = _grid(_dense(name, (16, 16, 16)), BOX)
        got_a, c_a, raw_a = _mark(False, grid, rays, z, sentinel)
        got_o, c_o, raw_o = _mark(True, grid, rays, z, sentinel)
        print(f"marks {n}x{s} {name}: {c_a} / {c_o} of {n * s} listed")
        if n * s == 1:
            assert c_a == (1 if name == "ones" else 0)
        else:
            assert 0 < c_a < n * s
        assert c_a == c_o
        assert torch.equal(torch.sort(got_a).values, got_o), (n, s, name)
        assert _same(raw_a, raw_o), (n, s, name)
        listed = torch.zeros(n * s, dtype=torch.bool)
        listed[got_o.to(torch.int64)] = True
        rows = raw_o.cpu().reshape(-1, 4)
        assert bool((rows[~listed] == 0).all()) and bool((rows[listed] == sentinel).all()), (n, s, name)


# ---- 2. - 4. the list-driven training forward and the counted backward --------------------------------------------------------
def _sorted_subset(c, seed):
    gen = torch.Generator().manual_seed(seed)
    head = torch.sort(torch.randperm(P, generator=gen)[:c]).values
    rest = torch.randperm(P, generator=gen)                               # behind the count: valid indices that must not be used
    return torch.cat([head, rest])[:P].to(torch.int32)


_PLAIN = {}


def _plain(kind):
    """mi_field_eval_rays_train + mi_field_backward over all P points, once per kind: the rows the list-driven calls must
    reproduce.  Never modified afterwards."""
    if kind in _PLAIN:
        return _PLAIN[kind]
    from mirender import _lib, ops
    lib = _lib.load()
    _, pf = _field(kind, 5)
    k = pf.kind
    rays = _rays(N)
    z = ops.sample_coarse(N, NEAR, FAR, S, dev(), synth.t_rand(N, S, seed=9).to(dev()))
    acts = torch.empty(lib.mi_field_train_acts_floats(k) * P, device=dev())
    raw = torch.empty(P, 4, device=dev())
    stream = _lib.stream_ptr(dev())
    _lib.check(lib.mi_field_eval_rays_train(k, _lib.ptr(pf.refresh()), None, _lib.ptr(rays), _lib.ptr(z), 1, N, S, _lib.ptr(raw),
                                            _lib.ptr(acts), stream), "mi_field_eval_rays_train")
    g = torch.Generator(device=dev()).manual_seed(3)
    mag = 10.0 ** (4.0 * torch.rand(N, 1, 1, device=dev(), generator=g) - 3.0)
    g_raw = (torch.randn(N, S, 4, device=dev(), generator=g) * mag).reshape(P, 4).contiguous()
    gws = torch.empty(lib.mi_field_train_grads_floats(k) * P, device=dev())
    part = torch.empty(lib.mi_field_bwd_partial_floats_kind(k, P), device=dev())
    out = [torch.empty_like(p) for p in pf.params]
    arr = (ctypes.c_void_p * len(out))(*[t.data_ptr() for t in out])
    _lib.check(lib.mi_field_backward(k, _lib.ptr(pf.refresh_bwd()), None, _lib.ptr(acts), _lib.ptr(gws), _lib.ptr(raw),
                                     _lib.ptr(g_raw), 1, P, _lib.ptr(part), None, arr, None, len(out), None, stream),
               "mi_field_backward")
    torch.cuda.synchronize()
    _PLAIN[kind] = dict(pf=pf, rays=rays, z=z, raw=raw, g_raw=g_raw, A=G.regions(G.ACTS[kind], acts, P),
                        D=G.regions(G.GRADS[kind], gws, P), grads=out, keep=(acts, gws))
    return _PLAIN[kind]


def _list_run(kind, lst, c, nan_partial=True):
    """The list-driven training forward and the counted backward over list[:c], everything NaN beforehand."""
    from mirender import _lib
    lib = _lib.load()
    pl = _plain(kind)
    pf = pl["pf"]
    k = pf.kind
    stream = _lib.stream_ptr(dev())
    lst_d, count = lst.to(dev()), torch.tensor([c], dtype=torch.int32, device=dev())
    acts = torch.full((lib.mi_field_train_acts_floats(k) * P,), NAN, device=dev())
    raw = torch.full((P, 4), NAN, device=dev())
    rc = lib.mi_field_eval_rays_list_train(k, _lib.ptr(pf.refresh()), _lib.ptr(pl["rays"]), _lib.ptr(pl["z"]), N, S, _lib.ptr(lst_d),
                                           _lib.ptr(count), _lib.ptr(raw), _lib.ptr(acts), stream)
    assert rc == 0, lib.mi_last_error()
    raw_fwd = raw.clone()
    # the backward reads raw / g_raw at rows list[e] only: the unlisted rows of both stay NaN
    listed = torch.zeros(P, dtype=torch.bool, device=dev())
    listed[lst_d[:c].to(torch.int64)] = True
    g_raw = torch.where(listed[:, None], pl["g_raw"], torch.full((), NAN, device=dev())).contiguous()
    gws = torch.full((lib.mi_field_train_grads_floats(k) * P,), NAN, device=dev())
    part = torch.empty(lib.mi_field_bwd_partial_floats_kind(k, P), device=dev())
    part.fill_(NAN if nan_partial else 0.0)
    out = [torch.full_like(p, NAN) for p in pf.params]
    arr = (ctypes.c_void_p * len(out))(*[t.data_ptr() for t in out])
    rc = lib.mi_field_backward_list(k, _lib.ptr(pf.refresh_bwd()), _lib.ptr(acts), _lib.ptr(gws), _lib.ptr(raw), _lib.ptr(g_raw),
                                    _lib.ptr(lst_d), _lib.ptr(count), P, _lib.ptr(part), arr, stream)
    assert rc == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    return dict(raw=raw_fwd, listed=listed, A=G.regions(G.ACTS[kind], acts, P), D=G.regions(G.GRADS[kind], gws, P), grads=out,
                idx=lst_d[:c].to(torch.int64))


@pytest.mark.parametrize("kind", KINDS)
def test_list_train_forward_chain_and_weight_grads(kind):
    pl = _plain(kind)
    for c in COUNTS:
        lst = _sorted_subset(c, seed=c)
        st = _list_run(kind, lst, c)
        idx, listed = st["idx"], st["listed"]
        what = (kind, c)
        # 2. the saving forward
        assert _same(st["raw"][listed], pl["raw"][listed]), what
        assert bool(torch.isnan(st["raw"][~listed]).all()), what
        for name, _w in G.ACTS[kind]:
            assert _same(st["A"][name][:c], pl["A"][name][idx]), (what, name)
            assert bool(torch.isnan(st["A"][name][c:]).all()), (what, name)      # rows at and past the count: not written
        # 3. the counted chain
        for name, _w in G.GRADS[kind]:
            assert _same(st["D"][name][:c], pl["D"][name][idx]), (what, name)
            assert bool(torch.isnan(st["D"][name][c:]).all()), (what, name)
        # 4. the counted weight gradients, from the kernel's own compact rows
        for lay in G.network(kind):
            dA = (st["D"]["heads"][:, lay.grad[1]:lay.grad[2]] if lay.head else st["D"][lay.grad])[:c]
            gw, gb = st["grads"][2 * lay.p], st["grads"][2 * lay.p + 1]
            for r in lay.ins:
                n_slabs = G.group_plan(kind, r.group, P)[1]
                L = tref.counted_slab_len(c, n_slabs) + n_slabs
                ref_w, b_w, ref_b, b_b = G.stage_c_ref(dA, st["A"][r.region][:c, r.c0:r.c1], L)
                case = f"occupancy train {kind} count {c} of {P}"
                G.gate(case, "C weight grads (counted)", f"dW p{lay.p} ({r.group})", lay.weight_cols(gw, r), ref_w, b_w, G.active_c(L), check=True)
                if r.bias:
                    G.gate(case, "C weight grads (counted)", f"db p{lay.p} ({r.group})", gb, ref_b, b_b, G.active_c(L), check=True)
        if c == 0:
            assert all(bool((g == 0).all()) for g in st["grads"]), what
        # a zeroed scratch gives the same bits as the NaN-filled one
        if c in (33, 100):
            again = _list_run(kind, lst, c, nan_partial=False)
            assert all(_same(a, b) for a, b in zip(st["grads"], again["grads"])), what
    # the list of all points, in order: mi_field_backward's bits
    st = _list_run(kind, torch.arange(P, dtype=torch.int32), P)
    assert all(_same(a, b) for a, b in zip(st["grads"], pl["grads"])), kind


def test_counted_slabs_with_the_count_inside_the_first_slab():
    """A capacity of 2 600 points plans eleven 256-point slabs for TinyNeRF's 256 x 256 jobs; 150 listed rows make eleven slabs
    of 32: five hold rows, the last six are empty and write zero records."""
    from mirender import _lib, ops
    lib = _lib.load()
    kind, n, s, c = "tiny_nerf", 100, 26, 150
    cap = n * s
    assert G.group_plan(kind, "g422", cap)[1] >= 2 and tref.counted_slab_len(c, G.group_plan(kind, "g422", cap)[1]) * 2 <= 256
    _, pf = _field(kind, 5)
    k = pf.kind
    rays = _rays(n)
    z = ops.sample_coarse(n, NEAR, FAR, s, dev(), synth.t_rand(n, s, seed=9).to(dev()))
    gen = torch.Generator().manual_seed(1)
    lst = torch.sort(torch.randperm(cap, generator=gen)[:c]).values.to(torch.int32).to(dev())
    lst = torch.cat([lst, torch.zeros(cap - c, dtype=torch.int32, device=dev())])
    count = torch.tensor([c], dtype=torch.int32, device=dev())
    stream = _lib.stream_ptr(dev())
    acts = torch.full((lib.mi_field_train_acts_floats(k) * cap,), NAN, device=dev())
    raw = torch.full((cap, 4), NAN, device=dev())
    assert lib.mi_field_eval_rays_list_train(k, _lib.ptr(pf.refresh()), _lib.ptr(rays), _lib.ptr(z), n, s, _lib.ptr(lst), _lib.ptr(count),
                                             _lib.ptr(raw), _lib.ptr(acts), stream) == 0, lib.mi_last_error()
    g_raw = torch.randn(cap, 4, device=dev(), generator=torch.Generator(device=dev()).manual_seed(2))
    gws = torch.full((lib.mi_field_train_grads_floats(k) * cap,), NAN, device=dev())
    part = torch.full((lib.mi_field_bwd_partial_floats_kind(k, cap),), NAN, device=dev())
    out = [torch.full_like(p, NAN) for p in pf.params]
    arr = (ctypes.c_void_p * len(out))(*[t.data_ptr() for t in out])
    assert lib.mi_field_backward_list(k, _lib.ptr(pf.refresh_bwd()), _lib.ptr(acts), _lib.ptr(gws), _lib.ptr(raw), _lib.ptr(g_raw),
                                      _lib.ptr(lst), _lib.ptr(count), cap, _lib.ptr(part), arr, stream) == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    A, D = G.regions(G.ACTS[kind], acts, cap), G.regions(G.GRADS[kind], gws, cap)
    for lay in G.network(kind):
        dA = (D["heads"][:, lay.grad[1]:lay.grad[2]] if lay.head else D[lay.grad])[:c]
        for r in lay.ins:
            n_slabs = G.group_plan(kind, r.group, cap)[1]
            L = tref.counted_slab_len(c, n_slabs) + n_slabs
            ref_w, b_w, ref_b, b_b = G.stage_c_ref(dA, A[r.region][:c, r.c0:r.c1], L)
            G.gate("occupancy train: count in the first slab", "C weight grads (counted)", f"dW p{lay.p} ({r.group})",
                   lay.weight_cols(out[2 * lay.p], r), ref_w, b_w, G.active_c(L), check=True)
            if r.bias:
                G.gate("occupancy train: count in the first slab", "C weight grads (counted)", f"db p{lay.p} ({r.group})",
                       out[2 * lay.p + 1], ref_b, b_b, G.active_c(L), check=True)


# ---- 5. - 7. the pair, through the Python surface -------------------------------------------------------------------------------
def _cots(n, seed=4):
    return [c.to(dev()) for c in tref.case_cots(n, seed)]


def _loss(outs, cots):
    return sum((o * c).sum() for o, c in zip(outs, cots))


def _grads_of(models, fn):
    """Run fn() -> outs under autograd, backpropagate the fixed cotangents, return (outs, {id(model): [grads]})."""
    for m in models:
        for p in m.parameters():
            p.grad = None
    outs = fn()
    _loss(outs, _cots(outs[0].shape[0])).backward()
    return [o.detach() for o in outs], [[p.grad.clone() for p in m.parameters()] for m in models]


PAIR_CASES = {
    "nerf_pair": ("nerf", 5, "nerf", 6, 12, 24, "t_rand"),
    "tiny_nerf": ("tiny_nerf", 5, "tiny_nerf", 6, 5, 3, "t_rand"),
    "siren_nerf_nf0": ("siren_nerf", 5, "siren_nerf", 6, 9, 0, "t_rand"),
    "nerf_seeded": ("nerf", 5, "nerf", 6, 12, 24, "seed"),
    "nerf_shared": ("nerf", 5, "nerf", 5, 12, 24, "t_rand"),
}


@pytest.mark.parametrize("case", sorted(PAIR_CASES))
def test_pair_with_an_all_ones_grid_equals_plain_training(case):
    """Every sample listed, in ascending order: the list-driven passes are the plain passes row for row, so outputs and
    gradients have the plain training path's bits (render_core.render_rays under autograd = mi_render_rays_train /
    mi_render_rays_backward, tests/test_gpu_cabi_train.py)."""
    from mirender import occupancy_train, render_core
    kc, sc, kf, sf, nc, nf, jitter = PAIR_CASES[case]
    (mc, _), (mf, _) = _field(kc, sc, True), _field(kf, sf, True)
    shared = mc is mf
    models = (mc,) if shared else (mc, mf)
    n = 24
    rays = _rays(n)
    kw = dict(t_rand=synth.t_rand(n, nc, seed=9).to(dev())) if jitter == "t_rand" else dict(seed=77, ray0=1000)
    grid = _grid(np.ones((4, 4, 4), bool), ((-8.0,) * 3, (8.0,) * 3))
    want, gw = _grads_of(models, lambda: render_core.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, **kw))
    counts = []

    def run():
        outs, c = occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, grid=grid, return_counts=True, **kw)
        counts.append(c)
        return outs
    got, gg = _grads_of(models, run)
    assert counts[0].tolist() == [[n * nc, n * (nc + nf)]]
    for k in range(6):
        assert _same(got[k], want[k]), (case, k)                          # rows are independent: the plain path's bits
    if shared:
        # One field: the plain path sums the Nc coarse rows and the Nf new rows, the pair with a grid sums the Nc coarse rows
        # and all Nc + Nf fine rows (no merge): the same gradient, other sums, so not the same bits.  Gated against the plain
        # shared training path with the project's tolerance for this kind; the oracle gates the same case in
        # test_pair_gradients_against_the_masked_oracle[nerf_shared_ones].
        for i, (a, b) in enumerate(zip(gg[0], gw[0])):
            rec = parity.gate_grad(f"occupancy train {case}: all-ones grid against the plain shared path", f"p{i}", a.cpu(), b.cpu(),
                                   None, tol=parity.GRAD_TOL_RELU, check=True)
            assert rec["rel_l2_err"] <= 1e-4, rec                         # a reordered fp32 sum, far inside the gate
        return
    for f in range(2):
        for i, (a, b) in enumerate(zip(gg[f], gw[f])):
            assert _same(a, b), (case, "coarse" if f == 0 else "fine", i)


@pytest.mark.parametrize("kinds", [("nerf", "nerf"), ("tiny_nerf", "siren_nerf")])
def test_training_forward_is_the_inference_call(kinds):
    """mi_render_rays_occupancy_train against mi_render_rays_occupancy on the same inputs and a partial grid: the six outputs
    and the two counts bit for bit (every listed row of both list-driven forwards has mi_field_eval_rays' bits, and the
    composite is the same kernel on the same raw).  200 rays at 8 + 16 samples: the coarse pass's 1 600 points lie inside one
    workgroup of the mark kernels, the fine pass's 4 800 cross into a second."""
    from mirender import _lib, ops
    lib = _lib.load()
    n, nc, nf = 200, 8, 16
    pf_c, pf_f = _field(kinds[0], 5)[1], _field(kinds[1], 6)[1]
    rays = _rays(n)
    tr = synth.t_rand(n, nc, seed=9).to(dev())
    grid = _grid(_dense("random", (16, 16, 16)), BOX)
    d, lo, inv = _grid_args(grid)
    zl, ul = ops.linspace_table(NEAR, FAR, nc, dev()), ops.linspace_table(0.0, 1.0, nf, dev())
    base = lib.mi_render_workspace_bytes(n, nc, nf)
    results = []
    for train in (False, True):
        outs = [torch.full(s, NAN, device=dev()) for s in ((n, 3), (n,), (n,), (n, 3), (n,), (n,))]
        counts = torch.full((2,), -1, dtype=torch.int32, device=dev())
        extra = lib.mi_render_occupancy_train_extra_bytes(n, nc, nf) if train else lib.mi_render_occupancy_extra_bytes(n, nc, nf)
        ws = torch.empty(base + extra, dtype=torch.uint8, device=dev())
        head = (pf_c.kind, _lib.ptr(pf_c.refresh()), pf_f.kind, _lib.ptr(pf_f.refresh()), _lib.ptr(rays), n, NEAR, FAR, nc, nf,
                _lib.ptr(zl), _lib.ptr(ul), _lib.ptr(tr), 0, 0, _lib.ptr(grid.bits), d, lo, inv, *[_lib.ptr(o) for o in outs],
                _lib.ptr(counts), _lib.ptr(ws), base + extra)
        if train:
            sv = lib.mi_render_occupancy_train_saved_bytes(pf_c.kind, pf_f.kind, n, nc, nf)
            saved = torch.empty(sv, dtype=torch.uint8, device=dev())
            rc = lib.mi_render_rays_occupancy_train(*head, _lib.ptr(saved), sv, _lib.stream_ptr(dev()))
        else:
            rc = lib.mi_render_rays_occupancy(*head, _lib.stream_ptr(dev()))
        assert rc == 0, lib.mi_last_error()
        torch.cuda.synchronize()
        results.append((outs, counts.tolist()))
    (want, wc), (got, gc) = results
    print(f"{kinds}: evaluated {wc} of {[n * nc, n * (nc + nf)]}")
    assert 0 < wc[0] < n * nc and 0 < wc[1] < n * (nc + nf), wc
    assert gc == wc
    for k in range(6):
        assert _same(got[k], want[k]), (kinds, k)


def _stage_depths(pf_c, rays, nc, nf, grid, dense, tr):
    """The depths and masks of both passes, from the existing stage calls (the pair's outputs are held to this composition)."""
    from mirender import ops
    n = rays.shape[0]
    z_c = ops.sample_coarse(n, NEAR, FAR, nc, dev(), tr, 0)
    m_c = ref.occupied_mask(rays, z_c, grid.lo, grid.inv_cell, dense)
    raw_c = torch.where(m_c.to(dev())[..., None], ops.field_eval_rays(pf_c, rays, z_c), torch.zeros((), device=dev()))
    w_c = ops.composite(raw_c, z_c, rays)[3]
    z_f = ops.sample_fine(z_c, w_c, NEAR, FAR, nf)
    m_f = ref.occupied_mask(rays, z_f, grid.lo, grid.inv_cell, dense)
    return z_c, m_c, z_f, m_f


@pytest.mark.parametrize("case", sorted(tref.GRAD_CASES))
def test_pair_gradients_against_the_masked_oracle(case):
    """The cases of occupancy_train_ref.GRAD_CASES, which tests/test_occupancy_train_host.py puts through the same gates on the
    CPU: there the fp32 oracle is inside the HARD gate in every tensor, so here the hard gate is demanded too (the 3x
    fp64-bound fallback of parity.gate_grad never decides)."""
    from mirender import occupancy_train, ops
    kind, sc, sf, sharp, nc, nf, gname, dims, box = tref.GRAD_CASES[case]
    shared, full = sc == sf, case.endswith("_ones")
    (mc, pf_c), (mf, pf_f) = _field(kind, sc, True, sharp), _field(kind, sf, True, sharp)
    assert (mc is mf) == shared
    n = tref.N_RAYS
    rays, tr = tref.case_rays().to(dev()), tref.case_t_rand(nc).to(dev())
    dense = tref.case_dense(gname, dims)
    grid = _grid(dense, box)
    models = (mc,) if shared else (mc, mf)
    counts = []

    def run():
        outs, c = occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, grid=grid, t_rand=tr, return_counts=True)
        counts.append(c)
        return outs
    got, gg = _grads_of(models, run)
    again, gg2 = _grads_of(models, run)
    with torch.no_grad():
        want, wc = ops.render_rays_occupancy(pf_c, pf_f, rays, NEAR, FAR, nc, nf, grid, tr)
    assert counts[0].tolist() == [wc.tolist()], (counts, wc)
    if full:
        assert wc.tolist() == [n * nc, n * (nc + nf)]
    else:
        assert 0 < wc[0] < n * nc and 0 < wc[1] < n * (nc + nf), wc
    for k in range(6):
        assert _same(got[k], want[k]) and _same(again[k], want[k]), (case, k)
    for f in range(len(models)):
        assert all(_same(a, b) for a, b in zip(gg[f], gg2[f])), (case, "two runs")
    # gradients against the masked oracle, pass by pass, at the device's own depths
    z_c, m_c, z_f, m_f = _stage_depths(pf_c, rays, nc, nf, grid, dense, tr)
    refs = tref.case_refs(case, z_c, m_c, z_f, m_f)
    names = tref.param_names(kind, tref.case_state_dicts(case)[0])
    recs = []
    for f in range(len(models)):
        for name, t in zip(names, gg[f]):
            recs.append(parity.gate_grad(f"occupancy train {case}", ("coarse." if f == 0 else "fine.") + name, t.cpu(),
                                         refs[torch.float32][f][name], refs[torch.float64][f][name], check=False,
                                         **tref.case_gates(kind)))
    print(f"{case}: evaluated {wc.tolist()}, worst rel l2 {max(r['rel_l2_err'] for r in recs):.3g}, "
          f"worst elem/rms {max(r['max_elem_err_over_rms'] for r in recs):.3g}")
    bad = [r for r in recs if not r["passed"] or r["active"] != "hard"]
    assert not bad, bad[0]


def test_all_zero_grid_gives_the_background_and_zero_gradients():
    from mirender import occupancy_train
    (mc, _), (mf, _) = _field("nerf", 5, True), _field("nerf", 6, True)
    n, nc, nf = 24, 12, 24
    grid = _grid(np.zeros((16, 16, 16), bool), BOX)
    outs, grads = _grads_of((mc, mf), lambda: occupancy_train.render_rays(_rays(n), NEAR, FAR, mc, mf, nc, nf, grid=grid,
                                                                         t_rand=synth.t_rand(n, nc, seed=9).to(dev())))
    for k in (0, 3):
        assert bool((outs[k] == 1).all()) and bool((outs[k + 1] == 0).all()) and bool((outs[k + 2] == 0).all())
    assert all(bool((g == 0).all()) for f in grads for g in f)


def test_python_surface_chunks_no_grad_and_refusals():
    from mirender import _lib, fields, occupancy_train, render_core
    (mc, _), (mf, _) = _field("tiny_nerf", 5, True), _field("tiny_nerf", 6, True)
    n, nc, nf = 24, 5, 3
    rays = _rays(n)
    grid = _grid(_dense("random", (16, 16, 16)), BOX)
    kw = dict(grid=grid, seed=77, ray0=1000)
    whole, gw = _grads_of((mc, mf), lambda: occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, **kw))
    parts, gp = _grads_of((mc, mf), lambda: occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, max_points=8 * (2 * nc + nf), **kw))
    for k in range(6):
        assert _same(whole[k], parts[k]), k                               # three chunks of 8 rays: the same samples
    # Three chunk sums added against one sum over all rows: the rows have the same bits, only the order of the additions
    # differs.  Each result is within the stage-C bound C_C u sqrt(L) sum|dA||X| of the exact sum (L = the rows of the fine
    # pass), so the two differ by at most twice that.  sum|dA||X| is not at hand here; for L terms of mixed sign it is taken
    # as sqrt(L) times the tensor's largest entry.
    L = n * (nc + nf)
    for f in range(2):
        for a, b in zip(gw[f], gp[f]):
            tol = 2 * G.C_C * G.U * np.sqrt(L) * max(float(a.abs().max()), 1e-30) * np.sqrt(L)
            assert float((a - b).abs().max()) <= tol
    with torch.no_grad():
        a = occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, **kw)
        b = render_core.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, **kw)
        a2, c2 = occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, return_counts=True, **kw)
    assert all(_same(x, y) for x, y in zip(a, b)) and all(_same(x, y) for x, y in zip(a, whole))
    assert all(_same(x, y) for x, y in zip(a, a2)) and tuple(c2.shape) == (1, 2) and 0 < int(c2.sum()) < n * (2 * nc + nf)
    other = types.SimpleNamespace(device=torch.device("cuda", 1), bits=grid.bits, dims=grid.dims, lo=grid.lo, inv_cell=grid.inv_cell)
    with pytest.raises(_lib.MiRenderError, match="is on"):
        occupancy_train.render_rays(rays, NEAR, FAR, mc, mf, nc, nf, grid=other, seed=77)
    film = fields.FilmSirenNeRF().to(dev())
    film.set_film_params(synth.film_params(1)[0].to(dev()))
    with pytest.raises(_lib.MiRenderError, match="FiLM kinds"):
        occupancy_train.render_rays(rays, NEAR, FAR, film, film, 8, 8, **kw)
    with pytest.raises(_lib.MiRenderError, match="generic callables"):
        occupancy_train.render_rays(rays, NEAR, FAR, lambda x: torch.zeros(x.shape[0], 4, device=x.device), mf, 8, 8, **kw)
    with pytest.raises(_lib.MiRenderError, match="gradients to the rays"):
        occupancy_train.render_rays(rays.clone().requires_grad_(True), NEAR, FAR, mc, mf, 8, 8, **kw)
    # render_core keeps refusing gradients with a grid
    with pytest.raises(_lib.MiRenderError, match="gradients"):
        render_core.render_rays(rays, NEAR, FAR, mc, mf, 8, 8, **kw)


def test_ten_optimiser_steps_lower_the_loss():
    """The loop of examples/train_nerf_occupancy.py behind its warm-up: render_rays(grid=), nerf_loss, FusedAdam."""
    from mirender import fields, occupancy_train, train
    torch.manual_seed(0)
    coarse, fine = fields.NeRF().to(dev()), fields.NeRF().to(dev())
    n, nc, nf = 256, 12, 24
    rays = _rays(n)
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).to(dev())
    alpha = torch.ones(n, device=dev())
    grid = _grid(np.ones((16, 16, 16), bool), SMALL)                     # a box the rays partly leave
    opt = train.FusedAdam([coarse, fine], lr=5e-4, betas=(0.9, 0.999))
    losses = []
    for step in range(10):
        out = occupancy_train.render_rays(rays, NEAR, FAR, coarse, fine, nc, nf, grid=grid, seed=step)
        loss, _psnr = train.nerf_loss(out, target, alpha, use_alpha=False, use_fine_model=True)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", [f"{v:.4f}" for v in losses])
    assert np.isfinite(losses).all() and losses[-1] < losses[0]

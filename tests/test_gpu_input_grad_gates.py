"""GPU: mi_field_input_grad and mi_field_input_grad_rays (csrc/ray_grad.hip) per element against float64, at every size
where the two kernels change behaviour.

One training forward and one mi_field_backward per size (test_gpu_bwd_stages.run), then the input gradient from the acts /
grads_ws they left behind, gated by stage D (tests/input_grad_gates.py): the float64 contraction of the kernel's OWN dA
rows, weights, saved encoding rows and FiLM rows, under a bound whose constant is the counted number of fp32 roundings.
No ReLU switch can flip between the two, so the ReLU kinds are judged per element like the sin kinds.

  point form   1, 2, 3, 4, 5, 7, 31, 32, 33, 63, 65, 333 points per group: a 4-point step of the PE kernel that is ragged
               from the start, full, ragged at the end; a 32-point chunk short, full, one over; FiLM kinds in 3 groups, the
               others in one group (the ABI refuses n_groups > 1 for them - asserted - so their 3 x 33 points run as one
               group of 99)
  ray form     n in {1, 3, 4, 5, 17} x S in {1, 2, 3, 4, 5, 8, 9}, and (5, 64), (5, 192); FiLM kinds 2, 4, 6, 10, 34 rays in
               2 groups; `accumulate` onto a known tensor bit for bit at every size
  wraps        past one sweep of the largest grid (input_grad_gates.launch_plan with the device's CU count) a wave's loop
               takes `u += stride`: 2 sweeps + 5 rays (S = 3 PE, S = 2 lin; FiLM in 3 groups), and sweep x 32 + 45 points
               (FiLM in 2 groups); every case asserts that it wrapped
  isolation    the call reads the weights from the pointers it is given: copies with every encoding column zeroed but one
               frequency, every position column (or every direction column) zeroed, the skip layer's or the first layer's
               input columns zeroed, a FiLM table with gamma_0 / gamma_rgb set to a ramp - each term on its own scale
  unwritten    acts, grads_ws and the outputs filled with a NaN bit pattern before the forward: finite results, the bits
               of the run on zero-filled buffers

Every check leaves one parity record per gated tensor with the achieved err / bound, the worst element and, beside the
kernel's RMS error against float64, that of torch's fp32 evaluation of the same contraction (err_vs_fp32_reference).

Measured on one MI355X: the 37 cases take 5 s (the slowest, the NeRF point sizes with the first library load, 1.4 s) and
leave 1 302 records; the largest point-form wrap case holds 5.1 GB of acts + grads_ws."""
import ctypes

import pytest
import torch

import bwd_gates as G
import film_depth_util as FU
import input_grad_gates as D
import test_gpu_bwd_stages as S
import test_gpu_bwd_stages_depth as SD
from oracle import parity, synth

pytestmark = pytest.mark.gpu

KINDS = ["nerf", "tiny_nerf", "siren_nerf", "film_siren_nerf", "film_siren_nerf_nodir", G.depth_name(4, False),
         G.depth_name(12, True)]
WRAP_KINDS = ["nerf", "tiny_nerf", "siren_nerf", "film_siren_nerf"]
PPG = [1, 2, 3, 4, 5, 7, 31, 32, 33, 63, 65, 333]
RAYS = [(n, s) for n in (1, 3, 4, 5, 17) for s in (1, 2, 3, 4, 5, 8, 9)] + [(5, 64), (5, 192)]
NAN_BITS = 0x7FC00000


def is_film(kind):
    return G.depth_of(kind) is not None


def field(kind):
    if kind in G.KIND_IDS:                                 # iterating the table gives the fixed kinds
        return S.packed(kind, False)[1]
    return SD.field(*G.depth_of(kind), False)[1]


def film_table(kind, n_img, seed):
    if not is_film(kind):
        return None
    if kind in G.KIND_IDS:
        return synth.film_params(n_img, seed=seed).to(S.dev()).contiguous()
    return FU.film_rows(n_img, G.depth_of(kind)[0], seed=seed).to(S.dev()).contiguous()


def fwd_bwd(kind, ppg, n_img, seed, samples=1, fill=None):
    """S.run on the kind's synthetic field; FiLM kinds: n_img groups of ppg points, the others one group of n_img * ppg."""
    pf = field(kind)
    st = S.run(kind, ppg, n_img, False, seed, pf=pf, film=film_table(kind, n_img, seed), kind_queries=True, samples=samples,
               fill=fill, zero_from=1)
    st["k"] = pf.kind
    return st


def _par(params):
    return (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])


def point_form(st, n_groups, ppg, params=None, film=None, expect=0):
    from mirender import _lib
    lib = _lib.load()
    params, film = params or st["params"], st["film"] if film is None else film
    g_x = torch.full((st["P"], 6), float("nan"), device=S.dev())
    rc = lib.mi_field_input_grad(st["k"], _par(params), len(params), _lib.ptr(film), _lib.ptr(st["acts"]), _lib.ptr(st["gws"]),
                                 n_groups, ppg, _lib.ptr(g_x), _lib.stream_ptr(S.dev()))
    assert rc == expect, (rc, lib.mi_last_error())
    return g_x


def ray_form(st, n_groups, rpg, params=None, film=None, accumulate=0, into=None):
    from mirender import _lib
    lib = _lib.load()
    params, film = params or st["params"], st["film"] if film is None else film
    n, n_s = st["z"].shape
    assert n == n_groups * rpg
    if into is None:
        into = torch.full((n, 2, 3), float("nan"), device=S.dev())
    _lib.check(lib.mi_field_input_grad_rays(st["k"], _par(params), len(params), _lib.ptr(film), _lib.ptr(st["acts"]),
                                            _lib.ptr(st["gws"]), _lib.ptr(st["rays"]), _lib.ptr(st["z"]), n_groups, rpg, n_s,
                                            accumulate, _lib.ptr(into), _lib.stream_ptr(S.dev())), "mi_field_input_grad_rays")
    return into


def check_points(case, kind, st, g_x, ppg, params=None, film=None):
    return D.check_points(case, kind, g_x, st["A"], st["D"], params or st["params"], st["film"] if film is None else film, ppg)


def check_rays(case, kind, st, g_rays, rpg, params=None, film=None):
    return D.check_rays(case, kind, g_rays, st["A"], st["D"], params or st["params"], st["film"] if film is None else film,
                        rpg, st["rays"], st["z"])


def failed(prefix):
    return [r for r in parity.RECORDS if str(r.get("case", "")).startswith(prefix) and not r["passed"]]


def ray_groups(kind, n):
    """(groups, rays per group): FiLM kinds take 2, 4, 6, 10, 34 rays in 2 groups in place of 1, 3, 4, 5, 17."""
    return (2, {1: 1, 3: 2, 4: 3, 5: 5, 17: 17}[n]) if is_film(kind) else (1, n)


# ---- every size --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_point_form_sizes(kind):
    groups = 3 if is_film(kind) else 1
    prefix = f"input grad gates points {kind} "
    for ppg in PPG:
        st = fwd_bwd(kind, ppg, groups, seed=ppg)
        check_points(f"{prefix}{groups}x{ppg}", kind, st, point_form(st, groups, ppg), ppg)
    if not is_film(kind):
        # n_groups > 1 is refused for a kind without FiLM rows (check_input_grad): the 3 x 33 points run as one group
        st = fwd_bwd(kind, 33, 3, seed=99)
        point_form(st, 3, 33, expect=-1)
        check_points(f"{prefix}1x99", kind, st, point_form(st, 1, 99), 99)
    assert not failed(prefix), failed(prefix)[:3]


@pytest.mark.parametrize("kind", KINDS)
def test_ray_form_sizes_and_accumulate(kind):
    prefix = f"input grad gates rays {kind} "
    for n, n_s in RAYS:
        groups, rpg = ray_groups(kind, n)
        st = fwd_bwd(kind, rpg * n_s, groups, seed=17 * n + n_s, samples=n_s)
        g = ray_form(st, groups, rpg)
        check_rays(f"{prefix}{groups}x{rpg}x{n_s}", kind, st, g, rpg)
        base = torch.randn(g.shape, device=S.dev())
        assert torch.equal(ray_form(st, groups, rpg, accumulate=1, into=base.clone()), base + g), (n, n_s)
        assert torch.equal(ray_form(st, groups, rpg), g), (n, n_s)
    assert not failed(prefix), failed(prefix)[:3]


# ---- past one sweep of the grid ------------------------------------------------------------------------------------
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("kind", WRAP_KINDS)
def test_ray_form_wraps(kind):
    """2 sweeps + 5 rays: every wave of the largest grid takes the stride twice, some a third time; a FiLM kind's 3 groups
    end inside the first and the second sweep."""
    pe = kind in D.PE_KINDS
    sweep = D.sweep_units(pe, cus())
    groups = 3 if is_film(kind) else 1
    n = -(-(2 * sweep + 5) // groups) * groups
    n_s = 3 if pe else 2
    blocks, stride = D.launch_plan(pe, D.units_for(True, groups, n // groups), cus())
    assert stride == sweep and n > 2 * stride and n % stride != 0
    st = fwd_bwd(kind, n // groups * n_s, groups, seed=3, samples=n_s)
    prefix = f"input grad gates wrap rays {kind} "
    g = ray_form(st, groups, n // groups)
    check_rays(f"{prefix}{groups}x{n // groups}x{n_s}", kind, st, g, n // groups)
    base = torch.randn(g.shape, device=S.dev())
    ok = torch.equal(ray_form(st, groups, n // groups, accumulate=1, into=base.clone()), base + g)
    del st, g, base
    torch.cuda.empty_cache()
    assert ok and not failed(prefix), failed(prefix)[:3]


def filled_regions(kind, ppg, groups, seed):
    """The regions the kernels read, filled directly (no forward, no backward) - everything else in acts and grads_ws holds
    a NaN bit pattern: the consuming layers' dA rows are normal with one magnitude per point over four decades and every
    29th point zero; the E rows are sin and cos of random angles with zero pads; a synthetic FiLM table."""
    from mirender import _lib
    lib = _lib.load()
    pf = field(kind)
    P = ppg * groups
    dev = S.dev()
    acts = torch.empty(lib.mi_field_train_acts_floats(pf.kind) * P, device=dev)
    gws = torch.empty(lib.mi_field_train_grads_floats(pf.kind) * P, device=dev)
    acts.view(torch.int32).fill_(NAN_BITS)
    gws.view(torch.int32).fill_(NAN_BITS)
    A, Dg = G.regions(G.ACTS[kind], acts, P), G.regions(G.GRADS[kind], gws, P)
    g = torch.Generator(device=dev).manual_seed(seed)
    mag = 10.0 ** (4.0 * torch.rand(P, 1, device=dev, generator=g) - 3.0)
    mag[1::29] = 0.0
    pos, dr = D.consumers(kind)
    for lay, _ in pos + ([dr] if dr else []):
        Dg[lay.grad].copy_(torch.randn(Dg[lay.grad].shape, device=dev, generator=g) * mag)
    if kind in D.PE_KINDS:
        for name, freqs in (("E_pos", 10), ("E_dir", 4)):
            ang = 6.3 * torch.rand(P, freqs, 3, device=dev, generator=g)
            A[name].zero_()
            A[name][:, :6 * freqs] = torch.cat([torch.sin(ang), torch.cos(ang)], -1).reshape(P, -1)
    return dict(P=P, k=pf.kind, acts=acts, gws=gws, A=A, D=Dg, params=[p.detach() for p in pf.params],
                film=film_table(kind, groups, seed))


@pytest.mark.parametrize("kind", WRAP_KINDS)
def test_point_form_wraps(kind):
    """One sweep of 32-point chunks and 45 points more (a full chunk and one of 13; the FiLM kind in 2 groups, each ending in a
    chunk of 23) on directly filled regions (filled_regions)."""
    pe = kind in D.PE_KINDS
    sweep = D.sweep_units(pe, cus())
    groups = 2 if is_film(kind) else 1
    ppg = (sweep * D.CHUNK + 45 + groups - 1) // groups
    units = D.units_for(False, groups, ppg)
    blocks, stride = D.launch_plan(pe, units, cus())
    assert stride == sweep and units > stride
    st = filled_regions(kind, ppg, groups, seed=11)
    prefix = f"input grad gates wrap points {kind} "
    check_points(f"{prefix}{groups}x{ppg}", kind, st, point_form(st, groups, ppg), ppg)
    del st
    torch.cuda.empty_cache()
    assert not failed(prefix), failed(prefix)[:3]


# ---- one term at a time ------------------------------------------------------------------------------------------------
def edited(params, edits):
    """A copy of the parameter list with columns zeroed: edits = [(layer, In, (first, last) kept of the In's columns or None)]."""
    out = list(params)
    for lay, r, keep in edits:
        if out[2 * lay.p] is params[2 * lay.p]:
            out[2 * lay.p] = params[2 * lay.p].clone()
        cols = lay.weight_cols(out[2 * lay.p], r)
        kept = None if keep is None else cols[:, keep[0]:keep[1]].clone()
        cols.zero_()
        if keep is not None:
            cols[:, keep[0]:keep[1]] = kept
    return out


def both_forms(kind, seed):
    """The two launches every isolation case runs on: 65 points, and 5 rays of 9 samples (FiLM: 2 groups of 5)."""
    g_p = 3 if is_film(kind) else 1
    g_r, rpg = ray_groups(kind, 5)
    return (fwd_bwd(kind, 65, g_p, seed=seed), g_p), (fwd_bwd(kind, rpg * 9, g_r, seed=seed + 1, samples=9), g_r, rpg)


def run_both(prefix, name, kind, forms, params=None, film=None):
    (sp, g_p), (sr, g_r, rpg) = forms
    check_points(f"{prefix}{name} points", kind, sp, point_form(sp, g_p, 65, params and params[0], film and film[0]), 65,
                 params and params[0], film and film[0])
    check_rays(f"{prefix}{name} rays", kind, sr, ray_form(sr, g_r, rpg, params and params[1], film and film[1]), rpg,
               params and params[1], film and film[1])


@pytest.mark.parametrize("kind", ["nerf", "tiny_nerf"])
def test_one_encoding_frequency_at_a_time(kind):
    """Position frequency i alone (direction columns zero) for i in 0..9, direction frequency i alone (position columns zero)
    for i in 0..3: sin and cos together.  2^0 is judged on its own scale, not next to 2^9."""
    forms = both_forms(kind, seed=41)
    pos, dr = D.consumers(kind)
    prefix = f"input grad gates isolation {kind} "
    for i in range(10):
        ed = [(lay, r, (6 * i, 6 * i + 6)) for lay, r in pos] + [(*dr, None)]
        run_both(prefix, f"position frequency {i}", kind, forms, [edited(f[0]["params"], ed) for f in forms])
    for i in range(4):
        ed = [(lay, r, None) for lay, r in pos] + [(*dr, (6 * i, 6 * i + 6))]
        run_both(prefix, f"direction frequency {i}", kind, forms, [edited(f[0]["params"], ed) for f in forms])
    assert not failed(prefix), failed(prefix)[:3]


@pytest.mark.parametrize("kind", ["nerf", "siren_nerf"])
def test_one_position_layer_at_a_time(kind):
    """The skip layer's input columns zeroed, then the first layer's, then both (the direction term alone)."""
    forms = both_forms(kind, seed=43)
    pos, _ = D.consumers(kind)
    prefix = f"input grad gates isolation {kind} "
    for name, drop in (("first layer only", pos[1:]), ("skip layer only", pos[:1]), ("direction only", pos)):
        ed = [(lay, r, None) for lay, r in drop]
        run_both(prefix, name, kind, forms, [edited(f[0]["params"], ed) for f in forms])
    assert not failed(prefix), failed(prefix)[:3]


@pytest.mark.parametrize("kind", ["film_siren_nerf", "film_siren_nerf_nodir", G.depth_name(4, False), G.depth_name(12, True)])
def test_film_gamma_ramps(kind):
    """gamma_0, then gamma_rgb, set to a ramp over the 256 features (another one per group); the reference reads the same table."""
    forms = both_forms(kind, seed=47)
    pos, dr = D.consumers(kind)
    prefix = f"input grad gates isolation {kind} "
    for name, row in [("gamma_0 ramp", pos[0][0].film)] + ([("gamma_rgb ramp", dr[0].film)] if dr else []):
        tables = []
        for f in forms:
            t = f[0]["film"].clone()
            ramp = torch.linspace(0.25, 4.0, 256, device=t.device)
            for g in range(t.shape[0]):
                t[g, row, :256] = ramp.roll(37 * g) * (-1.0) ** g
            tables.append(t)
        run_both(prefix, name, kind, forms, film=tables)
    assert not failed(prefix), failed(prefix)[:3]


# ---- nothing but what the library wrote ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_unwritten_memory_is_not_read(kind):
    """acts, grads_ws and the outputs hold a NaN bit pattern before the forward and the backward: the input gradients are
    finite and have the bits of the run on zero-filled buffers."""
    g_p = 3 if is_film(kind) else 1
    g_r, rpg = ray_groups(kind, 5)
    got = {}
    for fill in (0, NAN_BITS):
        sp = fwd_bwd(kind, 33, g_p, seed=51, fill=fill)
        sr = fwd_bwd(kind, rpg * 9, g_r, seed=52, samples=9, fill=fill)
        got[fill] = (point_form(sp, g_p, 33 if is_film(kind) else sp["P"]), ray_form(sr, g_r, rpg))
    for zero, nan, form in zip(got[0], got[NAN_BITS], ("point form", "ray form")):
        assert bool(torch.isfinite(nan).all()), f"{kind} {form}: {int((~torch.isfinite(nan)).sum())} values not finite"
        assert torch.equal(zero, nan), f"{kind} {form}: {int((zero != nan).sum())} values differ"

"""The field backward stage by stage against float64, at the sizes training uses, with a dense cotangent.

One training forward (mi_field_eval_rays_train) and one backward (mi_field_backward) per case, called through the C ABI
as mirender.autograd does, keeping what the library writes between the stages: the saved rows `acts`, the per-layer dA
`grads_ws` and, for FiLM kinds, the last image's per-layer sums in the FiLM scratch.  Each stage is then rebuilt in
float64 from the kernels' own inputs to it (tests/bwd_gates.py) and gated per element:

  A  every saved row against act(W X + b) of its layer's saved input; every ReLU switch bit against the saved row, bit
     for bit; every sin / FiLM cosine-sign bit against cos(w0 u) outside the 1e-3 band
  B  every dA region (and the head gradients) against the chain rebuilt from the kernel's dA of the next layers
  C  every weight and bias gradient (GEMM and thin jobs, the split writes into one weight included), the FiLM per-image
     sums, dW / db / d gamma / d beta against the kernel's dA and X

The point counts come from the planner's own formulas (bwd_gates.slabs_for / slab_pts_for): a partial stage, slabs
shorter than the ring, both sides of every slab-count cap of the kind, fewer slabs than the plan asked for, and the
production sizes (65 536 / 196 608 points of a 1024-ray NeRF step, one 128 x 128 x 36 C4 image per FiLM group).

The FiLM depth kinds (hidden_layers 4..12 other than 8) run the same `run` and the same stage checks from
test_gpu_bwd_stages_depth.py, which holds their depth x size matrix.

Measured on one MI355X: the 66 cases take 20 s, with a device-memory peak of 34 GiB allocated (40 GiB held by torch's
cache) - the two 589 824-point FiLM images, 22 GiB of acts + grads; stage B works on blocks of ROWS points to keep its
float64 temporaries small."""
import ctypes

import pytest
import torch

import bwd_gates as G
from oracle import synth

pytestmark = pytest.mark.gpu

KINDS = ["nerf", "siren_nerf", "film_siren_nerf", "film_siren_nerf_nodir", "tiny_nerf"]


def dev():
    return torch.device("cuda", 0)


def point_counts(kind):
    """Points per image (FiLM) or per pass: small and ragged, both sides of every cap, production."""
    ps = {1, 31, 33, 257, 8193}
    film = kind.startswith("film")
    for grp in G.group_jobs(kind):
        t = 256 * G.group_plan(kind, grp, 1)[2]
        if film and not grp.endswith("_img"):
            t //= 2                                    # the heads run over both images at once
        ps |= {t - 5, t + 37}
    if film:
        ps.add(128 * 128 * 36)                         # one C4 image (128 x 128 rays, 12 + 24 samples)
    else:
        ps |= {1024 * 64, 1024 * 192}                  # the 1024-ray NeRF step: coarse 64, fine 64 + 128
    if kind == "nerf":
        ps.add(500_009)
    return sorted(ps)


CASES = [(k, p, i % 2 == 1) for k in KINDS for i, p in enumerate(point_counts(k))]


_MODELS = {}


def packed(kind, sharp):
    from mirender import fields
    key = (kind, sharp)
    if key not in _MODELS:
        m = fields.FilmSirenNeRF(use_dir=False) if kind == "film_siren_nerf_nodir" else {
            "nerf": fields.NeRF, "tiny_nerf": fields.TinyNeRF, "siren_nerf": fields.SirenNeRF,
            "film_siren_nerf": fields.FilmSirenNeRF}[kind]()
        m.load_state_dict(synth.state_dict(kind, 11, True if sharp else "medium", 0.05))
        m = m.to(dev())
        _MODELS[key] = (m, fields.as_packed_field(m))
    return _MODELS[key]


def samples_for(ppg):
    for s in (36, 32):
        if ppg % s == 0:
            return s
    return 1


CANARY = 0x5CA1AB1E            # the bit pattern of every float of a workspace's tail (run(..., tail=n))


def run(kind, ppg, n_img, sharp, seed, pf=None, film=None, kind_queries=False, tail=0, samples=None, fill=None,
        zero_from=0):
    """Training forward + backward through the C ABI; returns everything the stages read and wrote.

    pf / film: another packed field of the kind's network (a FiLM depth kind, a kind id of the same network, a w_0) and
    its FiLM table, instead of the synthetic fixed-kind field.  kind_queries: size the two scratch buffers with the _kind
    queries (the only ones that know a depth kind).  tail: floats of CANARY behind the queried size of acts, grads and both
    scratch buffers; st["tails"] names the buffers whose tail the two calls changed.  samples: the samples per ray (a divisor
    of ppg) instead of samples_for's.  fill: a bit pattern every float of acts and grads holds before
    the two calls (default: whatever the allocator returns).  zero_from: the first of the every-29th rays whose cotangent
    is zero."""
    from mirender import _lib
    lib = _lib.load()
    if pf is None:
        _m, pf = packed(kind, sharp)
    k = pf.kind
    S = samples_for(ppg) if samples is None else samples
    assert ppg % S == 0, (ppg, S)
    rpg = ppg // S
    n, P = n_img * rpg, n_img * ppg
    g = torch.Generator(device=dev()).manual_seed(seed)
    o = torch.randn(n, 3, device=dev(), generator=g)
    o = 4.0 * o / o.norm(dim=1, keepdim=True)
    d = -o / 4.0 + 0.3 * torch.randn(n, 3, device=dev(), generator=g)
    rays = torch.stack([o, d], 1).contiguous()
    z = torch.sort(2.0 + 4.0 * torch.rand(n, S, device=dev(), generator=g), 1).values.contiguous()
    if film is None and kind.startswith("film"):
        film = synth.film_params(n_img, seed=seed).to(dev()).contiguous()
    tails = {}

    def buffer(name, floats):
        assert floats > 0, (name, floats, lib.mi_last_error())
        t = torch.empty(floats + tail, device=dev())
        if fill is not None and name in ("acts", "grads"):
            t.view(torch.int32).fill_(fill)
        if tail:
            tails[name] = t[floats:].view(torch.int32).fill_(CANARY)
        return t[:floats]

    acts = buffer("acts", lib.mi_field_train_acts_floats(k) * P)
    raw = torch.empty(n, S, 4, device=dev())
    stream = _lib.stream_ptr(dev())
    _lib.check(lib.mi_field_eval_rays_train(k, _lib.ptr(pf.refresh()), _lib.ptr(film), _lib.ptr(rays), _lib.ptr(z),
                                            n_img if film is not None else 1, rpg if film is not None else n, S,
                                            _lib.ptr(raw), _lib.ptr(acts), stream), "mi_field_eval_rays_train")
    # dense cotangent: per-ray magnitudes over four decades, every 29th ray exactly zero
    mag = 10.0 ** (4.0 * torch.rand(n, 1, 1, device=dev(), generator=g) - 3.0)
    mag[zero_from::29] = 0.0
    g_raw = (torch.randn(n, S, 4, device=dev(), generator=g) * mag).reshape(P, 4).contiguous()
    gws = buffer("grads", lib.mi_field_train_grads_floats(k) * P)
    part = buffer("partial", lib.mi_field_bwd_partial_floats_kind(k, P) if kind_queries else lib.mi_field_bwd_partial_floats(P))
    out = [torch.empty_like(p) for p in pf.params]
    arr = (ctypes.c_void_p * len(out))(*[t.data_ptr() for t in out])
    fp = gfilm = par = None
    if film is not None:
        fp = buffer("film partial", lib.mi_field_film_partial_floats_kind(k, n_img, ppg) if kind_queries
                    else lib.mi_field_film_partial_floats(n_img, ppg))
        gfilm = torch.empty_like(film)
        par = (ctypes.c_void_p * len(out))(*[p.data_ptr() for p in pf.params])
    _lib.check(lib.mi_field_backward(k, _lib.ptr(pf.refresh_bwd()), _lib.ptr(film), _lib.ptr(acts), _lib.ptr(gws),
                                     _lib.ptr(raw), _lib.ptr(g_raw), n_img if film is not None else 1,
                                     ppg if film is not None else P, _lib.ptr(part), _lib.ptr(fp), arr, par, len(out),
                                     _lib.ptr(gfilm), stream), "mi_field_backward")
    torch.cuda.synchronize()
    touched = [name for name, t in tails.items() if not bool((t == CANARY).all())]
    del part, tails
    return dict(P=P, ppg=ppg, n_img=n_img, w0=pf.w_0, params=[p.detach() for p in pf.params], film=film,
                A=G.regions(G.ACTS[kind], acts, P), D=G.regions(G.GRADS[kind], gws, P), raw=raw.reshape(P, 4),
                g_raw=g_raw, grads=out, film_partial=fp, grad_film=gfilm, rays=rays, z=z, acts=acts, gws=gws, tails=touched)


def _images(st, lay):
    """Row ranges and FiLM rows (gamma, beta) the layer is evaluated over: one range, or one per image for FiLM."""
    if lay.film is None:
        return [(slice(0, st["P"]), None)]
    f, ppg = st["film"], st["ppg"]
    return [(slice(g * ppg, (g + 1) * ppg), (f[g, lay.film, :256], f[g, lay.film, 256:])) for g in range(st["n_img"])]


def stage_a(case, kind, st):
    ok, A, prm, w0 = True, st["A"], st["params"], st["w0"]
    for lay in G.network(kind):
        W, b = prm[2 * lay.p], prm[2 * lay.p + 1]
        got_all = st["raw"][:, lay.out[0]:lay.out[1]] if lay.head else A[lay.out]
        name = f"p{lay.p}" if lay.head else lay.out
        for rows, fr in _images(st, lay):
            ins = [(A[r.region][rows, r.c0:r.c1], lay.weight_cols(W, r)) for r in lay.ins]
            pre, mag = G.pre_activation(ins, b)
            ref, bound = G.stage_a_ref(lay.act, pre, mag, fr, w0)
            got = got_all[rows]
            tag = "" if fr is None else f" image {rows.start // st['ppg']}"
            ok &= G.gate(case, "A forward", name + tag, got, ref, bound, f"{G.C_A:g} u (|W||X|+|b|) through {lay.act}")
            if lay.act == "relu" and not lay.head:
                sw = "S" + lay.out[1:]
                ok &= G.gate(case, "A forward", sw + " switch bits", G.decode_switches(A[sw][rows]).double(),
                             (got > 0).double(), torch.zeros((), dtype=torch.float64, device=got.device), "bit for bit")
            if lay.act in ("sin", "film"):
                u = pre if fr is None else fr[0].double() * pre + fr[1].double()
                ref_b, bound_b = G.sign_bit_ref(u, w0)
                ok &= G.gate(case, "A forward", name + " cos sign bits" + tag, G.cos_negative(got).double(), ref_b, bound_b,
                             f"exact where |cos| > {G.COS_BAND:g}")
            del pre, mag, ref, bound
    return ok


ROWS = 1 << 16                 # stage B works on blocks of this many points: the fp64 temporaries stay ~1 GiB


def stage_b(case, kind, st):
    ok, A, D, prm, w0, P = True, st["A"], st["D"], st["params"], st["w0"], st["P"]
    net = G.network(kind)
    ref, bound = G.heads_ref(st["raw"], st["g_raw"])
    ok &= G.gate(case, "B chain", "heads", D["heads"], ref, bound, "4 u |ref|")
    for lay in net:
        if lay.head:
            continue
        worst, where = 0.0, -1
        for r0 in range(0, P, ROWS):
            rows = slice(r0, min(P, r0 + ROWS))
            cons, starts = [], []
            for m in net:
                for r in m.ins:
                    if r.region != lay.out:
                        continue
                    dA = (D["heads"][:, m.grad[1]:m.grad[2]] if m.head else D[m.grad])[rows]
                    if m.act == "film":                  # the FiLM layer's dA is gamma (.) dL/du, gamma of each point's image
                        img = torch.arange(rows.start, rows.stop, device=dA.device) // st["ppg"]
                        dA = dA.double() * st["film"][img, m.film, :256].double()
                    (starts if m.head else cons).append((dA, m.weight_cols(prm[2 * m.p], r)))
            # a head feeding a layer that also feeds the MFMAs is the accumulators' start (SCALED in bwd_layer); alone (the
            # rgb head into the dir layer) it is the whole VALU sum
            dx, mag = G.chain_dx(cons, starts) if cons else G.chain_dx(starts)
            del cons, starts
            saved = G.decode_switches(A["S" + lay.out[1:]][rows]) if lay.act == "relu" else A[lay.out][rows]
            ref, bound = G.stage_b_ref("sin" if lay.act == "film" else lay.act, dx, mag,
                                       None if lay.act == "linear" else saved, w0)
            w, i = G.worst_ratio(D[lay.grad][rows], ref, bound)
            if w > worst or where < 0:
                worst, where = w, i + rows.start * ref.shape[1]
            del dx, mag, ref, bound
        ok &= G.record(case, "B chain", lay.grad, worst, where, D[lay.grad].numel(),
                       f"{G.C_B:g} u |act'| |W|^T|dA| ({lay.act})")
    return ok


def stage_c(case, kind, st):
    ok, A, D, prm, P = True, st["A"], st["D"], st["params"], st["P"]
    for lay in G.network(kind):
        if lay.act == "film":
            ok &= _stage_c_film(case, kind, st, lay)
            continue
        dA = D["heads"][:, lay.grad[1]:lay.grad[2]] if lay.head else D[lay.grad]
        gw, gb = st["grads"][2 * lay.p], st["grads"][2 * lay.p + 1]
        for r in lay.ins:
            L = G.sum_length(kind, r.group, P)
            ref_w, b_w, ref_b, b_b = G.stage_c_ref(dA, A[r.region][:, r.c0:r.c1], L)
            cols = f"{r.wcol}:{r.wcol + r.c1 - r.c0}"
            ok &= G.gate(case, "C weight grads", f"dW p{lay.p} cols {cols} ({r.group})", lay.weight_cols(gw, r), ref_w, b_w,
                         G.active_c(L))
            if r.bias:
                ok &= G.gate(case, "C weight grads", f"db p{lay.p} ({r.group})", gb, ref_b, b_b, G.active_c(L))
    return ok


def _stage_c_film(case, kind, st, lay):
    """FiLM layer: per image T_g = dU^T X, s_g = sum dU; dW = sum_g gamma_g T_g, db = sum_g gamma_g s_g,
    d gamma_g = <W, T_g> + b s_g, d beta_g = s_g; the last image's T / s also straight from the FiLM scratch."""
    ok, A, D, ppg, n_img = True, st["A"], st["D"], st["ppg"], st["n_img"]
    W, b = st["params"][2 * lay.p].double(), st["params"][2 * lay.p + 1].double()
    l = lay.film
    dW = dWb = db = dbb = None
    for g in range(n_img):
        rows = slice(g * ppg, (g + 1) * ppg)
        gam = st["film"][g, l, :256].double()
        dU = D[lay.grad][rows]
        dg_ref = dg_b = s = s_b = None
        T_parts = []
        for r in lay.ins:
            L = G.sum_length(kind, r.group, ppg)
            T, Tb, s_r, s_rb = G.stage_c_ref(dU, A[r.region][rows, r.c0:r.c1], L)
            if r.bias:
                s, s_b = s_r, s_rb
            Wc = lay.weight_cols(W, r)
            t1 = (Wc * T).sum(1)
            part_b = (Wc.abs() * Tb).sum(1) + 16 * G.U * (Wc * T).abs().sum(1)
            dg_ref = t1 if dg_ref is None else dg_ref + t1
            dg_b = part_b if dg_b is None else dg_b + part_b
            full = torch.zeros_like(W)
            full_b = torch.zeros_like(W)
            lay.weight_cols(full, r)[:], lay.weight_cols(full_b, r)[:] = T, Tb
            T_parts.append((r, T, Tb, L))
            dW = gam[:, None] * full if dW is None else dW + gam[:, None] * full
            add_b = gam.abs()[:, None] * full_b + n_img * G.U * (gam[:, None] * full).abs()
            dWb = add_b if dWb is None else dWb + add_b
        dg_ref = dg_ref + b * s
        dg_b = dg_b + b.abs() * s_b + 16 * G.U * (b * s).abs()
        db = gam * s if db is None else db + gam * s
        add = gam.abs() * s_b + n_img * G.U * (gam * s).abs()
        dbb = add if dbb is None else dbb + add
        ok &= G.gate(case, "C FiLM finish", f"d gamma layer {l} image {g}", st["grad_film"][g, l, :256], dg_ref, dg_b,
                     f"{G.C_C:g} u sqrt(L) |W||dU|^T|X| + 16 u |W T|")
        ok &= G.gate(case, "C FiLM finish", f"d beta layer {l} image {g}", st["grad_film"][g, l, 256:], s, s_b,
                     f"{G.C_C:g} u sqrt(L) sum |dU|")
        if g == n_img - 1:
            ok &= _film_scratch(case, st, l, T_parts, s, s_b)
    ok &= G.gate(case, "C FiLM finish", f"dW p{lay.p}", st["grads"][2 * lay.p], dW, dWb,
                 f"sum over images of |gamma| {G.C_C:g} u sqrt(L) |dU|^T|X|")
    ok &= G.gate(case, "C FiLM finish", f"db p{lay.p}", st["grads"][2 * lay.p + 1], db, dbb,
                 f"sum over images of |gamma| {G.C_C:g} u sqrt(L) sum |dU|")
    return ok


KFS = 256 * 256 + 256          # one 256-wide FiLM layer's T_l and s_l in the FiLM scratch (field_bwd_dw.hip)


def _film_scratch(case, st, l, T_parts, s, s_b):
    """The last image's T_l / s_l as reduce_jobs_kernel left them: T_l [256][256] + s_l [256] for l = 1..L (L = 8 for the
    fixed kinds: one row of the FiLM table less), then the K = 3 blocks of layer 0 (xyz) and layer L (dir) as [256][3],
    then s_0."""
    fp, ok = st["film_partial"], True
    base3 = (st["film"].shape[1] - 1) * KFS
    for r, T, Tb, L in T_parts:
        if r.c1 - r.c0 == 256:
            got = fp[(l - 1) * KFS:(l - 1) * KFS + 65536].view(256, 256)
        else:
            o = base3 if l == 0 else base3 + 1024
            got = fp[o:o + 768].view(256, 3)
        ok &= G.gate(case, "C FiLM sums", f"T layer {l} {r.region} (last image)", got, T, Tb, G.active_c(L))
    got_s = fp[base3 + 2048:base3 + 2048 + 256] if l == 0 else fp[(l - 1) * KFS + 65536:(l - 1) * KFS + 65536 + 256]
    ok &= G.gate(case, "C FiLM sums", f"s layer {l} (last image)", got_s, s, s_b, "sum |dU| bound")
    return ok


@pytest.mark.parametrize("kind,pts,sharp", CASES, ids=[f"{k}-{p}-{'sharp' if s else 'medium'}" for k, p, s in CASES])
def test_backward_stages_vs_fp64(kind, pts, sharp):
    film = kind.startswith("film")
    n_img = (3 if pts <= 8192 + 64 else 2) if film else 1
    st = run(kind, pts, n_img, sharp, seed=pts % 1000 + 7)
    assert all(torch.isfinite(t).all() for t in st["grads"])
    case = f"bwd stages {kind} {'x'.join(map(str, (n_img, pts))) if film else pts} pts sharp={sharp}"
    res = {"A": stage_a(case, kind, st), "B": stage_b(case, kind, st), "C": stage_c(case, kind, st)}
    from oracle import parity
    bad = [r for r in parity.RECORDS if r.get("case") == case and not r["passed"]]
    del st
    torch.cuda.empty_cache()                         # the next case's buffers are allocated afresh, not beside this one's
    assert all(res.values()) and not bad, bad[:3]

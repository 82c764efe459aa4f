"""The stage gates of test_gpu_bwd_stages.py on the FiLM depth kinds: FilmSirenNeRF(hidden_layers = L) for every L the
fused kernels run (4 to 12), through the run-time-depth chain (film_bwd_kernel<USE_DIR, RT_DEPTH = true>), the per-image
planner with L GEMM jobs and the FiLM finish with L + 2 jobs.

The same `run` and the same stage checks as the fixed kinds (imported from test_gpu_bwd_stages.py), on the networks
bwd_gates.film_depth_network describes, with the committed C_A, C_B, C_C, SIN_EPS and COS_BAND: a depth kind runs the same
layer arithmetic and no stage compounds through the network, so a ratio above 1 here is a finding, not a reason to raise a
constant.

  depths    every L in 4..12 except 8, with and without the view direction (16 kinds); depth 8 once: the macro kind against
            kinds 2 / 3, every acts, grads and gradient bit, just past the 32-slab cap
  points    per image: 1, 33, 257; 256 x cap - 5 and 256 x cap + 37 for every launch group of the depth - the L GEMM jobs of
            an image (cap = ceil(256 / L): 5 632 points at L = 12, 13 312 at L = 5), its thin jobs (131 072 with the dir
            columns, 262 144 without) and the head jobs over all images (65 536 per image of two); one production image
            (128 x 128 x 36 points) for L = 12 with dir and L = 5 without
  images    three up to 8 256 points per image, two above (the head jobs always run over more than one image)
  heads     the medium (x8) and the sharp (x50) sigma head alternate over the sizes of a kind
  w_0       30 everywhere but one case (L = 6, w_0 = 25): the references take the packed field's w_0
  scratch   sized with mi_field_bwd_partial_floats_kind / mi_field_film_partial_floats_kind; behind the queried size of
            acts, grads and both scratch buffers lie TAIL floats of a fixed bit pattern that both calls must leave alone
  forward   mi_field_eval_rays (the inference kernel) must return the bits of the training forward's raw

Measured on one MI355X: the 148 cases take 51 s (the fixed kinds' 66 cases: 20 s); the slowest are the two production
cases with 4.9 s (L = 12) and 2.3 s (L = 5), every other case stays below 1.5 s.  The device-memory peak is 43 GiB allocated
(49 GiB held by torch's cache; fixed kinds: 34 GiB / 40 GiB) in the L = 12 production case: 1 179 648 points x 6 668 floats
of acts + grads are 29 GiB, the rest are the float64 temporaries of the stage checks."""
import pytest
import torch

import bwd_gates as G
import film_depth_util as U
import test_gpu_bwd_stages as S
from oracle import parity

pytestmark = pytest.mark.gpu

DEPTHS = [L for L in range(G.DEPTH_MIN, G.DEPTH_MAX + 1) if L != 8]
PRODUCTION = 128 * 128 * 36                          # one C4 image (128 x 128 rays, 12 + 24 samples)
PRODUCTION_KINDS = (G.depth_name(12, True), G.depth_name(5, False))
TAIL = 2 * (256 * 256 + 256)                         # two records of the largest job: a misplaced slab lands inside it


def point_counts(kind):
    """Points per image: small and ragged, both sides of every cap of the depth's planner, production for two kinds."""
    ps = {1, 33, 257}
    for grp in G.group_jobs(kind):
        t = 256 * G.group_plan(kind, grp, 1)[2]
        if not grp.endswith("_img"):
            t //= 2                                  # the heads run over both images at once
        ps |= {t - 5, t + 37}
    if kind in PRODUCTION_KINDS:
        ps.add(PRODUCTION)
    return sorted(ps)


# (L, use_dir, points per image, sharp, w_0)
CASES = [(L, d, p, i % 2 == 1, 30.0) for L in DEPTHS for d in (True, False)
         for i, p in enumerate(point_counts(G.depth_name(L, d)))]
CASES.append((6, True, 256 * 43 + 37, False, 25.0))   # past the cap of six GEMM jobs, with another frequency


def case_id(L, d, p, sharp, w_0):
    return f"L{L}-{'dir' if d else 'nodir'}-{p}-{'sharp' if sharp else 'medium'}" + ("" if w_0 == 30.0 else f"-w0_{w_0:g}")


_FIELDS = {}


def field(L, use_dir, sharp, w_0=30.0):
    """(module, packed field) of a synthetic depth-L network, cached."""
    from mirender import fields
    key = (L, use_dir, sharp, w_0)
    if key not in _FIELDS:
        sd = U.state_dict(L, use_dir, seed=11 + L, head="sharp" if sharp else "medium")
        m = fields.field_from_state_dict(sd, S.dev(), w_0=w_0)
        pf = fields.as_packed_field(m)
        assert pf is not None and pf.w_0 == w_0
        _FIELDS[key] = (m, pf)
    return _FIELDS[key]


def n_images(pts):
    return 3 if pts <= 8192 + 64 else 2


@pytest.mark.parametrize("L,use_dir,pts,sharp,w_0", CASES, ids=[case_id(*c) for c in CASES])
def test_depth_backward_stages_vs_fp64(L, use_dir, pts, sharp, w_0):
    from mirender import ops
    kind = G.depth_name(L, use_dir)
    _m, pf = field(L, use_dir, sharp, w_0)
    assert pf.kind == G.KIND_IDS[kind] == U.kind_of(L, use_dir)
    n_img, seed = n_images(pts), pts % 1000 + 7
    film = U.film_rows(n_img, L, seed=seed).to(S.dev()).contiguous()
    st = S.run(kind, pts, n_img, sharp, seed, pf=pf, film=film, kind_queries=True, tail=TAIL)   # both calls returned 0
    assert st["tails"] == [], f"written behind the queried size: {st['tails']}"
    assert st["w0"] == w_0
    assert all(torch.isfinite(t).all() for t in st["grads"]) and bool(torch.isfinite(st["grad_film"]).all())
    # the inference kernel on the same rays: the bits of the training forward
    raw = ops.field_eval_rays(pf, st["rays"], st["z"], film).reshape(-1, 4)
    assert torch.equal(raw, st["raw"]), f"{int((raw != st['raw']).sum())} of {raw.numel()} raw values differ"
    case = f"bwd stages {kind} {n_img}x{pts} pts sharp={sharp}" + ("" if w_0 == 30.0 else f" w_0={w_0:g}")
    res = {"A": S.stage_a(case, kind, st), "B": S.stage_b(case, kind, st), "C": S.stage_c(case, kind, st)}
    bad = [r for r in parity.RECORDS if r.get("case") == case and not r["passed"]]
    del st, raw
    torch.cuda.empty_cache()
    assert all(res.values()) and not bad, bad[:3]


def test_depth_8_macro_gives_every_bit_of_kinds_2_and_3():
    """MI_FIELD_FILM_DEPTH(8, use_dir) is the network of kinds 2 / 3: the same saved rows, per-layer gradients, parameter
    and FiLM gradients, bit for bit, just past the cap of the eight GEMM jobs (29 slabs of 288 points where 32 were planned)."""
    from mirender import fields
    pts = 8192 + 37
    for kind, use_dir in (("film_siren_nerf", True), ("film_siren_nerf_nodir", False)):
        _m, pf = S.packed(kind, False)
        macro = fields.PackedField(U.kind_of(8, use_dir), pf.params, pf.w_0)
        assert macro.kind == G.KIND_IDS[G.depth_name(8, use_dir)] and macro.kind != pf.kind
        a = S.run(kind, pts, 3, False, seed=5)
        b = S.run(kind, pts, 3, False, seed=5, pf=macro, kind_queries=True, tail=TAIL)
        assert b["tails"] == []
        for name in ("raw", "acts", "gws", "grad_film"):
            assert torch.equal(a[name], b[name]), f"{kind} {name}: {int((a[name] != b[name]).sum())} values differ"
        for i, (x, y) in enumerate(zip(a["grads"], b["grads"])):
            assert torch.equal(x, y), f"{kind} gradient {i}: {int((x != y).sum())} of {x.numel()} values differ"
        assert max(float(t.abs().max()) for t in a["grads"]) > 0
        del a, b
        torch.cuda.empty_cache()

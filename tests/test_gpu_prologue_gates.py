"""The prologue of the field forward per element against float64: what mi_field_eval_rays_train and
mi_field_eval_points_train save as the first layers' inputs - E_pos and E_dir of the NeRF kinds, xin of the sin and FiLM
kinds - against the definition of those rows (tests/prologue_gates.py, stage "P prologue").

One saving forward per case and input regime through the C ABI, acts filled with a NaN bit pattern before the call and a
canary tail behind its queried size; only the prologue's regions are read back and gated on the host:

  kinds     nerf, tiny_nerf, siren_nerf, film_siren_nerf, film_siren_nerf_nodir, the FiLM depth kinds 4 and 12 with and
            without the view
  shapes    ray form (n, S) = (1, 1), (127, 1), (129, 1), (26, 5), (37, 36), (3, 192): the smallest at which the 128-point
            tile and the row indexing change behaviour; FiLM kinds also 2 and 3 groups of 65 rays x 5 samples (325 points:
            two tiles and a tail of 69) and 2 groups of one point; point form 1, 31, 129 and 333 points per group
  regimes   scene (test_gpu_bwd_stages.run's own inputs and call), wide (+-64), small (1e-30 .. 1e-2, signed zeros, rays
            along an axis), |d| over six decades, turn boundaries - prologue_gates.REGIMES, shared with the host test
  forward   in the scene and wide regimes mi_field_eval_rays' raw equals the saving forward's bit for bit, which carries the
            gate over to the inference kernels, which save nothing

The bounds are derived (prologue_gates.py); a ratio above 1 is a finding about load_point / pe_feature, not a reason to
raise a constant.  No element is masked or skipped.  Every gate leaves a record with the worst ratio, its position and the
fp32 oracle's ratio on the same inputs."""
import pytest
import torch

import bwd_gates as G
import film_depth_util as U
import prologue_gates as P
import test_gpu_bwd_stages as S
import test_gpu_bwd_stages_depth as D
from oracle import parity, synth

pytestmark = pytest.mark.gpu

TAIL = 4096                                        # canary floats behind acts: 16 rows of the widest region


def field_of(kind):
    """The packed synthetic field of a kind (medium sigma head), cached by the stage tests' own caches."""
    d = G.depth_of(kind)
    if kind in S.KINDS:
        return S.packed(kind, False)[1]
    return D.field(d[0], d[1], False)[1]


def film_of(kind, n_groups, seed):
    if not P.is_film(kind):
        return None
    if kind in S.KINDS:
        return synth.film_params(n_groups, seed=seed).to(S.dev()).contiguous()
    return U.film_rows(n_groups, G.depth_of(kind)[0], seed=seed).to(S.dev()).contiguous()


def saving_forward(kind, pf, film, inp, n_groups):
    """One mi_field_eval_rays_train (inp: rays, z) or mi_field_eval_points_train (inp: x) call over n_groups groups.
    Returns (raw [P, 4], acts of the queried size, its canary tail)."""
    from mirender import _lib
    lib = _lib.load()
    k = pf.kind
    dev = S.dev()
    Pn = inp["x"].shape[0] if "x" in inp else inp["z"].numel()
    floats = lib.mi_field_train_acts_floats(k) * Pn
    assert floats == G.floats_per_point(G.ACTS[kind]) * Pn, (floats, lib.mi_last_error())
    buf = torch.empty(floats + TAIL, device=dev)
    buf.view(torch.int32)[:floats] = P.FILL
    buf.view(torch.int32)[floats:] = S.CANARY
    raw = torch.empty(Pn, 4, device=dev)
    stream = _lib.stream_ptr(dev)
    t = {name: v.to(dev).contiguous() for name, v in inp.items()}
    if "x" in inp:
        assert Pn % n_groups == 0 and t["x"].shape == (Pn, 6)
        _lib.check(lib.mi_field_eval_points_train(k, _lib.ptr(pf.refresh()), _lib.ptr(film), _lib.ptr(t["x"]), n_groups,
                                                  Pn // n_groups, _lib.ptr(raw), _lib.ptr(buf), stream),
                   "mi_field_eval_points_train")
    else:
        n, Sm = t["z"].shape
        assert n % n_groups == 0 and t["rays"].shape == (n, 2, 3)
        _lib.check(lib.mi_field_eval_rays_train(k, _lib.ptr(pf.refresh()), _lib.ptr(film), _lib.ptr(t["rays"]), _lib.ptr(t["z"]),
                                                n_groups, n // n_groups, Sm, _lib.ptr(raw), _lib.ptr(buf), stream),
                   "mi_field_eval_rays_train")
    torch.cuda.synchronize()
    return raw, buf[:floats], buf[floats:]


def gate_call(case, kind, inp, acts, Pn, tail=None):
    """Stage P on one call's acts: the written extent on the device, the prologue's regions on the host."""
    res = P.extent(case, kind, acts, Pn, tail=tail, canary=S.CANARY)
    A = G.regions(G.ACTS[kind], acts, Pn)
    first = {name: A[name].cpu() for name in (("E_pos", "E_dir") if kind in P.PE_KINDS else ("xin",))}
    res.update(P.check(case, kind, {name: v.cpu() for name, v in inp.items()}, first))
    return res


def assert_stage_p(case, res):
    recs = [r for r in parity.RECORDS if r.get("case") == case and r["stage"] == P.STAGE]
    assert len(recs) == len(res) and all("oracle32_ratio" in r and "worst_index" in r and r["elements"] > 0 for r in recs)
    print(f"{case}: " + ", ".join(f"{r['qty']} {r['err_over_bound']:.3g} (fp32 oracle {r['oracle32_ratio']:.3g})" for r in recs))
    assert all(r["oracle32_ratio"] <= 1.0 for r in recs), [r for r in recs if not r["oracle32_ratio"] <= 1.0][:3]
    assert not P.failed(res), [r for r in recs if not r["passed"]][:4]


RAY_CASES = [(k, 1, n, s) for k in P.KINDS for n, s in P.RAY_SHAPES] + \
            [(k, g, rpg, s) for k in P.KINDS if P.is_film(k) for g, rpg, s in P.GROUP_SHAPES]


@pytest.mark.parametrize("kind,groups,rpg,samples", RAY_CASES, ids=[f"{k}-{g}x{r}x{s}" for k, g, r, s in RAY_CASES])
def test_ray_form_prologue_vs_fp64(kind, groups, rpg, samples):
    from mirender import ops
    pf = field_of(kind)
    assert pf.kind == G.KIND_IDS[kind]
    n, ppg = groups * rpg, rpg * samples
    Pn, seed = n * samples, 100 + n + samples
    film = film_of(kind, groups, seed)
    for regime, gen in P.REGIMES.items():
        case = f"prologue {regime} {kind} rays {groups}x{rpg}x{samples}"
        if regime == "scene":                       # the stage tests' own call and inputs; the backward runs behind it
            st = S.run(kind, ppg if P.is_film(kind) else Pn, groups if P.is_film(kind) else 1, False, seed, pf=pf, film=film,
                       kind_queries=True, tail=TAIL, samples=samples, fill=P.FILL)
            assert st["tails"] == [], f"written behind the queried size: {st['tails']}"
            assert st["P"] == Pn and st["z"].shape == (n, samples)
            inp, raw, acts, tail = dict(rays=st["rays"], z=st["z"]), st["raw"], st["acts"], None
        else:
            inp = gen(n, samples, seed)
            raw, acts, tail = saving_forward(kind, pf, film, inp, groups if film is not None else 1)
        assert_stage_p(case, gate_call(case, kind, inp, acts, Pn, tail))
        if regime in ("scene", "wide"):
            inf = ops.field_eval_rays(pf, inp["rays"].to(S.dev()), inp["z"].to(S.dev()), film).reshape(-1, 4)
            assert torch.equal(inf, raw), f"{case}: {int((inf != raw).sum())} of {raw.numel()} raw values differ"


POINT_CASES = [(k, ppg) for k in P.KINDS for ppg in P.POINTS_PER_GROUP]


@pytest.mark.parametrize("kind,ppg", POINT_CASES, ids=[f"{k}-{p}" for k, p in POINT_CASES])
def test_point_form_prologue_vs_fp64(kind, ppg):
    """mi_field_eval_points_train: xin[:, 0:6] is the caller's x bit for bit (no normalisation), the NeRF kinds encode the
    caller's columns.  FiLM kinds run two groups."""
    pf = field_of(kind)
    groups = 2 if P.is_film(kind) else 1
    Pn, seed = groups * ppg, 200 + ppg
    film = film_of(kind, groups, seed)
    for regime, gen in P.REGIMES.items():
        case = f"prologue {regime} {kind} points {groups}x{ppg}"
        inp = P.as_points(gen(Pn, 1, seed))
        raw, acts, tail = saving_forward(kind, pf, film, inp, groups)
        assert_stage_p(case, gate_call(case, kind, inp, acts, Pn, tail))

"""CPU: stage P (tests/prologue_gates.py), the per-element gate of the field forward's prologue, is the oracle's definition,
is honest, and has teeth.

  the definition   the restatement equals the oracle's own code in float64 - oracle.render_ref.points_on_rays, the view
                   expression of test_gpu_stages.test_field_eval_rays_golden, the oracle field's positional encoding - and its
                   column order is the one the oracle's NeRF applies
  honest bounds    the reference's fp32 torch evaluation of the prologue passes every gate, nothing masked, in all five
                   input regimes, both forms and every shape of the GPU test; fp32 torch.sin / cos stay within 3.6e-8 of
                   float64 up to 2^9 x 1024 rad; the fp32 view (torch's and the kernel's stated shape) stays within 4 u
  teeth            `simulate` restates load_point / posenc_blocks / store_xin in numpy float32 with their index arithmetic;
                   as it stands it passes, and each mistake a prologue could make fails the gate that names it

The failing gates below are self-checks, not findings: each test leaves parity.RECORDS as it found it (`_no_records`)."""
import math

import numpy as np
import pytest
import torch

import bwd_gates as G
import prologue_gates as P
from oracle import fields as ofields, parity, render_ref as R

f32, f64 = np.float32, np.float64


@pytest.fixture(autouse=True)
def _no_records():
    n = len(parity.RECORDS)
    yield
    del parity.RECORDS[n:]


# ---- the definition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", list(P.REGIMES))
def test_restatement_is_the_oracle_in_float64(regime):
    inp = P.REGIMES[regime](37, 9, seed=3)
    o, d, z = inp["rays"][:, 0].double(), inp["rays"][:, 1].double(), inp["z"].double()
    assert torch.equal(P.points(o, d, z), R.points_on_rays(o, d, z))
    pts32 = P.restate(inp)["pts"]
    assert pts32.dtype == torch.float32
    assert torch.equal(pts32, R.points_on_rays(inp["rays"][:, 0], inp["rays"][:, 1], inp["z"]).reshape(-1, 3))
    pts = R.points_on_rays(o, d, z)
    view = (d / torch.norm(d, dim=-1, keepdim=True))[:, None].expand_as(pts)        # test_field_eval_rays_golden's expression
    assert torch.equal(P.restate(inp)["view"], view.reshape(-1, 3))
    for v, n in ((pts32.double(), P.N_POS), (view.reshape(-1, 3), P.N_DIR)):
        assert torch.equal(P.encoding(v, n), ofields.posenc(v, n))


def test_column_order_is_the_oracle_nerfs():
    """Column 6 i + c: sin (c < 3) or cos of 2^i x_(c mod 3), 60 columns of the position and 24 of the direction - the
    widths the oracle NeRF's first and direction layers take (oracle.fields.SPECS)."""
    x = torch.tensor([[0.3, -1.1, 2.5], [4.0, 0.01, -0.7]], dtype=torch.float64)
    for n in (P.N_POS, P.N_DIR):
        e = ofields.posenc(x, n)
        assert e.shape == (2, 6 * n)
        for i in range(n):
            for c in range(6):
                want = (torch.sin if c < 3 else torch.cos)(2.0 ** i * x[:, c % 3])
                assert torch.equal(e[:, 6 * i + c], want), (i, c)
                assert bool(P.is_cos(n)[6 * i + c]) == (c >= 3)
    spec = dict(ofields.SPECS["nerf"])
    assert spec["layers_pos.0"][1] == 6 * P.N_POS and spec["layers_dir.1"][1] == 256 + 6 * P.N_DIR
    assert dict(G.ACTS["nerf"])["E_pos"] == 64 and dict(G.ACTS["nerf"])["E_dir"] == 32 and dict(G.ACTS["siren_nerf"])["xin"] == 8


def test_turn_values_sit_on_quarter_turns():
    v = P.turn_values()
    assert v.shape == (P.N_POS * 17 * 3,) and v.dtype == f32
    v = v.reshape(P.N_POS, 17, 3)
    for i in range(P.N_POS):
        q = v[i].astype(f64) * 2.0 ** i / (math.pi / 2)          # quarter turns of the angle at frequency i
        k = np.arange(-8, 9)[:, None]
        assert np.all(np.abs(q - k) < 1e-6)
        assert np.all(v[i, :, 0] < v[i, :, 1]) and np.all(v[i, :, 1] < v[i, :, 2])
    inp = P.turns(170, 3, seed=0)                              # 170 rays x 3 components: every value, bit for bit, as a point
    got = P.restate(inp)["pts"].reshape(170, 3, 3)[:, 0].reshape(-1).numpy()
    assert np.array_equal(got.view(np.int32), P.turn_values().view(np.int32))


# ---- honest bounds -------------------------------------------------------------------------------------------------------
def test_fp32_sin_cos_within_3p6e8_of_fp64():
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(400_000, generator=g) * 2 - 1) * (2.0 ** 9 * 1024)
    x = torch.cat([x, x * 1e-3, torch.from_numpy(P.turn_values()) * 2.0 ** 9])
    assert float((torch.sin(x).double() - torch.sin(x.double())).abs().max()) <= 3.6e-8
    assert float((torch.cos(x).double() - torch.cos(x.double())).abs().max()) <= 3.6e-8


def test_fp32_view_within_its_bound():
    """torch's fp32 expression and the kernel's stated shape sqrt((d0^2 + d1^2) + d2^2), on 200 000 directions at three
    scales: both below the 4 u of the gate (derived: 3.5 u)."""
    g = torch.Generator().manual_seed(2)
    worst = 0.0
    for scale in (1e-3, 1.0, 1e3):
        d = torch.randn(200_000, 3, generator=g) * scale
        ref = P.view_dirs(d.double())
        nrm = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        for got in (d / torch.norm(d, dim=-1, keepdim=True), d / nrm[:, None]):
            worst = max(worst, float(((got.double() - ref).abs() / (P.U * ref.abs())).max()))
    assert worst <= 3.5, worst


def ray_cases():
    out = [(k, 1, n, S) for k in P.KINDS for n, S in P.RAY_SHAPES]
    return out + [(k, g, g * rpg, S) for k in P.KINDS if P.is_film(k) for g, rpg, S in P.GROUP_SHAPES]


def _oracle_first(kind, inp):
    return P.assemble(kind, *P.oracle32(inp))


@pytest.mark.parametrize("regime", list(P.REGIMES))
def test_fp32_oracle_passes_every_gate(regime):
    """Ray form at every shape, point form at every count, one representative of each first-region layout per network
    family (the gates do not depend on the kind beyond it) - and every kind at one shape."""
    done = 0
    for kind in ("nerf", "siren_nerf"):
        for n, S in P.RAY_SHAPES + [(g * rpg, S) for g, rpg, S in P.GROUP_SHAPES]:
            inp = P.REGIMES[regime](n, S, seed=n + S)
            res = P.check(f"host {regime} {kind} {n}x{S}", kind, inp, _oracle_first(kind, inp))
            assert not P.failed(res), (kind, n, S, res)
            done += 1
        for ppg in P.POINTS_PER_GROUP:
            inp = P.as_points(P.REGIMES[regime](2 * ppg, 1, seed=ppg))
            res = P.check(f"host {regime} {kind} points {ppg}", kind, inp, _oracle_first(kind, inp))
            assert not P.failed(res), (kind, ppg, res)
            done += 1
    for kind in P.KINDS:
        inp = P.REGIMES[regime](26, 5, seed=9)
        assert not P.failed(P.check(f"host {regime} {kind}", kind, inp, _oracle_first(kind, inp)))
    recs = [r for r in parity.RECORDS if r["stage"] == P.STAGE and r["case"].startswith(f"host {regime} ")]
    assert len(recs) >= 4 * done
    for r in recs:                                    # what every stage-P record holds
        assert r["passed"] and r["elements"] > 0 and "worst_index" in r and r["err_over_bound"] <= 1.0
        assert r["oracle32_ratio"] == r["err_over_bound"]          # here the gated rows are the oracle's own


def test_regimes_are_what_they_say():
    n, S = 200, 8
    sc, wd, sm, dc = (P.REGIMES[k](n, S, seed=4) for k in ("scene", "wide", "small", "decades"))
    assert np.allclose(sc["rays"][:, 0].norm(dim=1).numpy(), 4.0, rtol=1e-6) and 2 <= float(sc["z"].min()) and float(sc["z"].max()) <= 6
    pw = P.restate(wd)["pts"].abs()
    assert 48 < float(pw.max()) <= 64 and float(pw.max()) * 2 ** 9 <= 32768
    ps, ds = P.restate(sm)["pts"], sm["rays"][:, 1]
    nz = ps[ps != 0].abs()
    assert float(nz.max()) <= 2.1e-2 and float(nz.min()) < 1e-25
    for t in (sm["rays"][:, 0], ds):                  # components exactly +0 and exactly -0
        b = t.contiguous().view(torch.int32)
        assert bool((b == 0).any()) and bool((b == -2 ** 31).any())
    assert bool(((ds != 0).sum(1) == 1).any()) and bool(((ds != 0).sum(1) >= 1).all())   # along one axis; never the zero vector
    assert bool((sm["z"] == 0).any())
    nd = dc["rays"][:, 1].norm(dim=1)
    assert float(nd.min()) < 1e-2 and float(nd.max()) > 1e2 and float(P.restate(dc)["pts"].abs().max()) <= 10.5


# ---- teeth ---------------------------------------------------------------------------------------------------------------
def posenc_np(v, nfreq, mut=None):
    """numpy restatement of posenc_blocks: feature 6 i + c of fp32 v; the angle 2^i v_c is exact, its sine is rounded once."""
    cols = []
    for i in range(nfreq):
        ang = (v * f32(2.0 ** (i + (mut == "frequency")))).astype(f64)
        s, c = np.sin(ang), np.cos(ang + (1e-6 if mut == "cos phase" else 0.0))
        cols += [c, s] if mut == "halves" else [s, c]
    return np.concatenate(cols, -1).astype(f32)


def simulate(kind, inp, n_groups=1, mut=None):
    """load_point + posenc_blocks / store_xin of a ray-form call in numpy float32, row by row as the kernels index them:
    point p = group * ppg + local, ray = group * rpg + local / S.  Returns the saved rows ({"E_pos", "E_dir"} or {"xin"})."""
    rays, z = inp["rays"].numpy(), inp["z"].numpy()
    n, S = z.shape
    rpg = n // n_groups
    ppg, Pn = rpg * S, n * S
    p = np.arange(Pn)
    group, local = p // ppg, p % ppg
    ray = np.minimum(group * (ppg if mut == "ray offset" else rpg) + local // S, n - 1)
    zz = z.reshape(-1)[np.minimum(p + (1 if mut == "z shift" else 0), Pn - 1)][:, None]
    o, d = rays[ray, 0], rays[ray, 1]
    if mut == "fma":
        pts = (o.astype(f64) + d.astype(f64) * zz.astype(f64)).astype(f32)
    else:
        pts = o + d * zz
    nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    view = d if mut == "view" else d / nrm
    assert pts.dtype == f32 and view.dtype == f32
    pad = f32(1e-30) if mut == "pad" else f32(0)
    if kind in P.PE_KINDS:
        out = {"E_pos": np.concatenate([posenc_np(pts, P.N_POS, mut), np.full((Pn, 4), pad)], 1),
               "E_dir": np.concatenate([posenc_np(view, P.N_DIR, mut), np.full((Pn, 8), pad)], 1)}
    else:
        out = {"xin": np.concatenate([pts, view, np.full((Pn, 2), pad)], 1)}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


SIM_KINDS = ["nerf", "tiny_nerf", "siren_nerf", "film_siren_nerf", G.depth_name(12, False)]


@pytest.mark.parametrize("regime", list(P.REGIMES))
@pytest.mark.parametrize("kind", SIM_KINDS)
def test_simulated_prologue_passes(kind, regime):
    for groups, rpg, S in [(1, n, S) for n, S in P.RAY_SHAPES] + (P.GROUP_SHAPES if P.is_film(kind) else []):
        inp = P.REGIMES[regime](groups * rpg, S, seed=11)
        res = P.check(f"sim {kind}", kind, inp, simulate(kind, inp, groups))
        assert not P.failed(res), (groups, rpg, S, res)


# mutation -> the gates that must fail, for the kinds that save encodings and for the kinds that save xin (None: the kind
# has no such step)
MUTATIONS = {
    "fma": (["E_pos cos", "E_pos sin"], ["xin pts"]),
    "halves": (["E_dir cos", "E_dir sin", "E_pos cos", "E_pos sin"], None),
    "frequency": (["E_dir cos", "E_dir sin", "E_pos cos", "E_pos sin"], None),
    "view": (["E_dir cos", "E_dir sin"], ["xin view"]),
    "z shift": (["E_pos cos", "E_pos sin"], ["xin pts"]),
    "ray offset": (["E_dir cos", "E_dir sin", "E_pos cos", "E_pos sin"], ["xin pts", "xin view"]),
    "pad": (["E_dir pads", "E_pos pads"], ["xin pads"]),
    "cos phase": (["E_dir cos", "E_pos cos"], None),
}


@pytest.mark.parametrize("kind", ["nerf", "film_siren_nerf"])
@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_fails_the_gate_that_names_it(mut, kind):
    """Two groups of 65 rays x 5 samples (a group's first ray is not a multiple of its first point) of the scene regime:
    exactly the gates of the mistaken step fail, every other gate still passes."""
    want = MUTATIONS[mut][0 if kind in P.PE_KINDS else 1]
    if want is None:
        assert kind not in P.PE_KINDS
        return
    inp = P.scene(130, 5, seed=5)
    res = P.check(f"mutation {mut} {kind}", kind, inp, simulate(kind, inp, 2, mut))
    assert P.failed(res) == want, res
    rec = [r for r in parity.RECORDS if r["case"] == f"mutation {mut} {kind}" and not r["passed"]]
    assert sorted(r["qty"] for r in rec) == want and all(r["oracle32_ratio"] <= 1.0 for r in rec)


def test_a_row_written_past_p_fails_the_extent_gate():
    """The last region's row P lands in the canary tail; a row that is never written keeps the fill; a clean buffer passes."""
    kind, Pn = "siren_nerf", 5
    floats = G.floats_per_point(G.ACTS[kind]) * Pn
    canary = 0x5CA1AB1E

    def buffers():
        a = torch.zeros(floats + 256)
        a.view(torch.int32)[floats:] = canary
        return a
    a = buffers()
    assert not P.failed(P.extent("extent clean", kind, a[:floats], Pn, tail=a[floats:], canary=canary))
    a = buffers()
    a[floats:floats + 128] = 0.5                      # X_d is 128 wide: its row P
    assert P.failed(P.extent("extent past P", kind, a[:floats], Pn, tail=a[floats:], canary=canary)) == ["acts extent"]
    a = buffers()
    a.view(torch.int32)[8 * (Pn - 1):8 * Pn] = P.FILL   # xin's last row never written
    assert P.failed(P.extent("extent short", kind, a[:floats], Pn, tail=a[floats:], canary=canary)) == ["acts extent"]
    assert [r["passed"] for r in parity.RECORDS[-3:]] == [True, False, False]

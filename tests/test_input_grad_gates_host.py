"""CPU: stage D (tests/input_grad_gates.py), the per-element gate of the input-gradient kernels, has teeth.

`simulate` restates csrc/ray_grad.hip in numpy float32, operation by operation in the kernels' summation order: the lane
partition (lin kernel: lane l owns features 4l..4l+3; PE kernel: lane = encoding column, one sequential fmaf chain per
column), the 4-point steps with the clamped and masked tail, the butterfly reduction, units handed out to waves by the
grid-stride loop of launch_plan's grid, the per-ray sums and store_ray.  On synthetic fp32 data it passes stage D at every
size class of the GPU test (with one "CU", so a sweep is 16 or 32 units and the wraps happen at a few dozen units), and each
mistake a kernel could make fails it.

The failing gates below are self-checks, not findings: each test leaves parity.RECORDS as it found it (`_no_records`)."""
import numpy as np
import pytest
import torch

import bwd_gates as G
import film_depth_util as FU
import input_grad_gates as D
from oracle import parity

KINDS = ["nerf", "tiny_nerf", "siren_nerf", "film_siren_nerf", "film_siren_nerf_nodir", G.depth_name(4, False),
         G.depth_name(12, True)]
PPG = [1, 2, 3, 4, 5, 7, 31, 32, 33, 63, 65, 333]
RAYS = [(n, S) for n in (1, 3, 4, 5, 17) for S in (1, 2, 3, 4, 5, 8, 9)] + [(5, 64), (5, 192)]
f32 = np.float32


@pytest.fixture(autouse=True)
def _no_records():
    n = len(parity.RECORDS)
    yield
    del parity.RECORDS[n:]


def is_film(kind):
    return G.depth_of(kind) is not None


# ---- synthetic inputs ----------------------------------------------------------------------------------------------
def synthetic(kind, n_groups, per_group, S, seed):
    """What the kernels read, in the buffers and the layout the GPU test reads: dA rows of the consuming layers with one
    magnitude per unit of S points over four decades (every 29th unit zero, from unit 1), saved encoding rows (sin and cos
    of 2^i x, zero pads), full-size weights, a FiLM table with gamma in 1 +- 0.25, non-unit ray directions, sorted depths."""
    rng = np.random.Generator(np.random.PCG64(seed))
    P = n_groups * per_group * S
    n = P // S
    acts = torch.zeros(G.floats_per_point(G.ACTS[kind]) * P)
    gws = torch.zeros(G.floats_per_point(G.GRADS[kind]) * P)
    A, Dg = G.regions(G.ACTS[kind], acts, P), G.regions(G.GRADS[kind], gws, P)
    scale = 10.0 ** rng.uniform(-3, 1, size=(n, 1))
    scale[1::29] = 0.0
    scale = np.repeat(scale, S, 0)
    widths = dict(G.GRADS[kind])
    pos, dr = D.consumers(kind)
    params = [None] * (2 * len(G.network(kind)))
    for lay, _ in pos + ([dr] if dr else []):
        rows, cols = widths[lay.grad], sum(r.c1 - r.c0 for r in lay.ins)
        Dg[lay.grad][:] = torch.from_numpy((rng.normal(size=(P, rows)) * scale).astype(f32))
        params[2 * lay.p] = torch.from_numpy((rng.normal(size=(rows, cols)) / 16).astype(f32))
    if kind in D.PE_KINDS:
        x = rng.uniform(-1.5, 1.5, size=(P, 6))
        for name, xs, freqs in (("E_pos", x[:, :3], 10), ("E_dir", x[:, 3:], 4)):
            ang = (2.0 ** np.arange(freqs))[None, :, None] * xs[:, None, :]
            A[name][:, :6 * freqs] = torch.from_numpy(np.concatenate([np.sin(ang), np.cos(ang)], -1).reshape(P, -1).astype(f32))
    film = FU.film_rows(n_groups, G.depth_of(kind)[0], seed + 1) if is_film(kind) else None
    o = rng.normal(size=(n, 3)).astype(f32)
    d = (rng.normal(size=(n, 3)) * rng.uniform(0.5, 2.0, size=(n, 1))).astype(f32)
    z = np.sort(rng.uniform(2.0, 6.0, size=(n, S)).astype(f32), -1)
    return dict(P=P, A=A, D=Dg, params=params, film=film, rays=torch.from_numpy(np.stack([o, d], 1)), z=torch.from_numpy(z))


# ---- the kernels in numpy float32 ------------------------------------------------------------------------------------
LANE = np.arange(64)


def wave_sum(v):
    """v += shfl_xor(v, o) for o = 32 .. 1, over the last axis; every lane ends with the same float."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., LANE ^ o]
    return v[..., 0]


def fma_chain(dE, dA, cols):
    """pe_contract: dE = fmaf(dA[:, k], cols[k], dE) for k in order (the product is exact in float64)."""
    for k in range(dA.shape[1]):
        dE = (dA[:, k:k + 1].astype(np.float64) * cols[k].astype(np.float64) + dE).astype(f32)
    return dE


def visited_units(pe, units, cus, stride_off=0):
    """The units in the order the grid hands them to its waves: wave w of block b takes b * per_block + w, then += stride."""
    blocks, stride = D.launch_plan(pe, units, cus)
    per_block = D.PE_WAVES if pe else D.LIN_WAVES
    out = []
    for b in range(blocks):
        for w in range(per_block):
            u = b * per_block + w
            while u < units:
                out.append(u)
                u += stride + stride_off
    return out


def store_ray(out, ray, rays, so, sz, sv, accumulate, bug):
    d = rays[ray, 1]
    nrm = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    v = d / nrm
    vg = v[0] * sv[0] + v[1] * sv[1] + v[2] * sv[2]
    if bug == "no projection":
        vg = f32(0)
    tail = (sv - v * vg) if bug == "no norm" else (sv - v * vg) / nrm
    g = np.concatenate([so, sz + tail]).astype(f32)
    out[ray] = out[ray] + g if accumulate and bug != "accumulate overwrites" else g


def simulate(kind, st, n_groups, per_group, S, ray_form, cus=1, accumulate=0, out=None, bug=None, stride_off=0):
    """g_x [P,6] (point form) or g_rays [n,6] (ray form) as the kernels sum them; `bug` plants one mistake."""
    P, Dg, A, params = st["P"], st["D"], st["A"], st["params"]
    pe = kind in D.PE_KINDS
    pos, dr = D.consumers(kind)
    if bug == "no skip":
        assert len(pos) == 2
        pos = pos[:1]
    units = D.units_for(ray_form, n_groups, per_group)
    upg = units // n_groups
    ppg = per_group * S if ray_form else per_group
    z, rays = st["z"].numpy().reshape(-1), st["rays"].numpy()
    if out is None:
        out = np.full((units if ray_form else P, 6), np.nan, f32)
    film = None if st["film"] is None else st["film"].numpy()
    cols = lambda lay, r: lay.weight_cols(params[2 * lay.p], r).numpy()     # noqa: E731

    def unit_points(u):
        group = u // upg
        if ray_form:
            return u * S, S, group
        if bug == "chunks straddle groups":                 # chunks cut over all points; the group of the chunk's first point
            p0 = u * D.CHUNK
            return (p0, min(D.CHUNK, P - p0), p0 // ppg) if p0 < P else (0, 0, 0)
        c = u % upg
        return group * ppg + c * D.CHUNK, min(D.CHUNK, ppg - c * D.CHUNK), group

    def z_at(p):
        return z[min(p + 1, P - 1)] if bug == "z shifted" else z[p]

    if pe:
        # per point and lane, independent of how the points are cut into units: the two chains
        dEp = np.zeros((P, 64), f32)
        for lay, r in pos:
            w = np.zeros((256, 64), f32)
            w[:, :60] = cols(lay, r)
            dEp = fma_chain(dEp, Dg[lay.grad].numpy(), w)
        wd = np.zeros((128, 32), f32)
        wd[:, :24] = cols(*dr)
        dEd = fma_chain(np.zeros((P, 32), f32), Dg[dr[0].grad].numpy(), wd)[:, LANE & 31]
        fi, fc = LANE // 6, LANE % 6
        is_cos, comp = fc >= 3, fc % 3
        mate = np.where(is_cos, LANE - 3, LANE + 3)
        sign = np.where(is_cos & (bug != "cos sign lost"), -1.0, 1.0) * 2.0 ** fi
        if bug in ("frequency 0 dropped", "frequencies 0 and 1 dropped"):
            sign = np.where(fi < (1 if bug == "frequency 0 dropped" else 2), 0.0, sign)
        if bug == "mate swapped":
            mate = LANE.copy()
        mate_p, coef_p = np.where(LANE < 60, mate, LANE), np.where(LANE < 60, sign, 0.0).astype(f32)
        mate_d, coef_d = np.where(LANE < 24, mate, LANE & 31), np.where(LANE < 24, sign, 0.0).astype(f32)
        e_pos, e_dir = A["E_pos"].numpy(), A["E_dir"].numpy()
        pick = [(comp == j) for j in range(3)]
        for u in visited_units(True, units, cus, stride_off):
            p0, cnt, _ = unit_points(u)
            tp, tz, tv = (np.zeros(64, f32) for _ in range(3))
            for s0 in range(0, cnt, 4):
                for q in range(4):
                    inside = s0 + q < cnt or (bug == "tail counted" and ray_form)
                    p = p0 + min(s0 + q, cnt - 1)
                    t = (dEp[p] * e_pos[p, mate_p]) * coef_p if inside else np.zeros(64, f32)
                    v = (dEd[p] * e_dir[p, mate_d]) * coef_d if inside else np.zeros(64, f32)
                    if ray_form:
                        tp, tz, tv = tp + t, tz + z_at(p) * t, tv + v
                    elif inside:
                        out[p] = [wave_sum(np.where(pick[j], t, f32(0))) for j in range(3)] + \
                                 [wave_sum(np.where(pick[j], v, f32(0))) for j in range(3)]
            if ray_form:
                so, sz, sv = (np.array([wave_sum(np.where(pick[j], x, f32(0))) for j in range(3)], f32) for x in (tp, tz, tv))
                store_ray(out, u, rays, so, sz, sv, accumulate, bug)
        return out

    w_pos = [cols(lay, r).reshape(64, 4, 3) for lay, r in pos]
    rows_d = 0
    if dr:
        rows_d = dict(G.GRADS[kind])[dr[0].grad]
        w_dir = np.zeros((64, 4, 3), f32)
        w_dir[:rows_d // 4] = cols(*dr).reshape(rows_d // 4, 4, 3)

    def lane_dot(r, w):                                     # [cnt,64,4] x [64,4,3] -> [cnt,64,3], left to right
        acc = r[:, :, 0, None] * w[None, :, 0]
        for q in (1, 2, 3):
            acc = acc + r[:, :, q, None] * w[None, :, q]
        return acc

    for u in visited_units(False, units, cus, stride_off):
        p0, cnt, group = unit_points(u)
        sl = slice(p0, p0 + cnt)
        gp = None
        for (lay, _), w in zip(pos, w_pos):
            r = Dg[lay.grad].numpy()[sl].reshape(cnt, 64, 4)
            if film is not None and bug != "no gamma":
                r = r * film[group, lay.film, :256].reshape(1, 64, 4)
            gp = lane_dot(r, w) if gp is None else gp + lane_dot(r, w)
        gv = np.zeros((cnt, 64, 3), f32)
        if dr:
            t = np.zeros((cnt, 64, 4), f32)
            t[:, :rows_d // 4] = Dg[dr[0].grad].numpy()[sl].reshape(cnt, rows_d // 4, 4)
            if film is not None and bug != "no gamma":
                t = t * film[group, dr[0].film, :256].reshape(1, 64, 4)
            gv = lane_dot(t, w_dir)
        if not ray_form:
            out[sl, :3] = wave_sum(np.moveaxis(gp, 1, -1))
            out[sl, 3:] = wave_sum(np.moveaxis(gv, 1, -1))
            continue
        so, sz, sv = (np.zeros((64, 3), f32) for _ in range(3))
        for s in range(cnt):
            so, sz, sv = so + gp[s], sz + z_at(p0 + s) * gp[s], sv + gv[s]
        store_ray(out, u, rays, *(wave_sum(x.T) for x in (so, sz, sv)), accumulate, bug)
    return out


def check(case, kind, st, got, n_groups, per_group, S, ray_form):
    got = torch.from_numpy(got)
    if ray_form:
        return D.check_rays(case, kind, got.reshape(-1, 2, 3), st["A"], st["D"], st["params"], st["film"], per_group,
                            st["rays"], st["z"])
    return D.check_points(case, kind, got, st["A"], st["D"], st["params"], st["film"], per_group)


def faithful(kind, n_groups, per_group, S, ray_form, seed=3, cus=1):
    st = synthetic(kind, n_groups, per_group, S, seed)
    got = simulate(kind, st, n_groups, per_group, S, ray_form, cus)
    case = f"host D {kind} {'rays' if ray_form else 'points'} {n_groups}x{per_group}x{S}"
    assert check(case, kind, st, got, n_groups, per_group, S, ray_form), \
        [r for r in parity.RECORDS if r.get("case") == case and not r["passed"]]
    return st, got


# ---- the faithful kernels pass at every size class -----------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_faithful_point_form_passes_at_every_size(kind):
    groups = 3 if is_film(kind) else 1
    for ppg in PPG:
        faithful(kind, groups, ppg, 1, False, seed=ppg)
    pe = kind in D.PE_KINDS
    ppg = D.sweep_units(pe, 1) * D.CHUNK + 45                # one sweep and a ragged second one
    if is_film(kind):
        ppg = (ppg + 1) // 2
    units = D.units_for(False, 2 if is_film(kind) else 1, ppg)
    assert units > D.launch_plan(pe, units, 1)[1]
    faithful(kind, 2 if is_film(kind) else 1, ppg, 1, False)


@pytest.mark.parametrize("kind", KINDS)
def test_faithful_ray_form_passes_at_every_size(kind):
    for n, S in RAYS:
        g = 2 if is_film(kind) else 1
        faithful(kind, g, n if g == 1 else {1: 1, 3: 2, 4: 3, 5: 5, 17: 17}[n], S, True, seed=n + S)
    pe = kind in D.PE_KINDS
    n = 2 * D.sweep_units(pe, 1) + 5                        # two wraps and a ragged third
    groups = 3 if is_film(kind) else 1
    n = -(-n // groups) * groups
    assert n > 2 * D.launch_plan(pe, n, 1)[1]
    faithful(kind, groups, n // groups, 3 if pe else 2, True)


def test_launch_mirror():
    """launch_input_grad's grid: cus blocks of 16 waves (PE), 8 cus blocks of 4 waves (lin); 256 CUs as the issue states."""
    assert D.sweep_units(True, 256) == 4096 and D.sweep_units(False, 256) == 8192
    assert D.launch_plan(True, 5, 256) == (1, 16) and D.launch_plan(True, 4097, 256) == (256, 4096)
    assert D.launch_plan(False, 5, 256) == (2, 8) and D.launch_plan(False, 8193, 256) == (2048, 8192)
    assert D.units_for(False, 3, 33) == 6 and D.units_for(True, 3, 33) == 99
    assert sorted(visited_units(True, 37, 1)) == list(range(37)) and visited_units(True, 37, 1)[:3] == [0, 16, 32]
    # the counted constants (module docstring of input_grad_gates)
    assert D.roundings("nerf") == {"pos": 519, "dir": 135} and D.roundings("tiny_nerf") == {"pos": 263, "dir": 135}
    assert D.roundings("siren_nerf") == {"pos": 12, "dir": 11} and D.roundings("film_siren_nerf") == {"pos": 11, "dir": 11}
    assert D.roundings("nerf", 9) == {"o": 513 + 15, "d_z": 513 + 17, "d_sv": 129 + 33}
    assert D.roundings("siren_nerf", 2) == {"o": 14, "d_z": 16, "d_sv": 31}


# ---- each planted mistake fails ----------------------------------------------------------------------------------------
def planted(kind, n_groups, per_group, S, ray_form, bug, seed=5, stride_off=0, direction_only=False):
    st = synthetic(kind, n_groups, per_group, S, seed)
    if direction_only:                                      # the position columns zeroed, as the GPU test's isolation cases do
        for lay, r in D.consumers(kind)[0]:
            lay.weight_cols(st["params"][2 * lay.p], r).zero_()
    case = f"host D planted {bug} {kind} {'rays' if ray_form else 'points'} {n_groups}x{per_group}x{S}"
    good = simulate(kind, st, n_groups, per_group, S, ray_form)
    assert check(case + " (faithful)", kind, st, good, n_groups, per_group, S, ray_form)
    bad = simulate(kind, st, n_groups, per_group, S, ray_form, bug=bug, stride_off=stride_off)
    ok = check(case, kind, st, bad, n_groups, per_group, S, ray_form)
    failed = {r["qty"] for r in parity.RECORDS if r.get("case") == case and not r["passed"]}
    return ok, failed, st, good, bad


PE_BUGS = ["frequency 0 dropped", "frequencies 0 and 1 dropped", "mate swapped", "cos sign lost"]


@pytest.mark.parametrize("bug", PE_BUGS)
@pytest.mark.parametrize("kind", ["nerf", "tiny_nerf"])
def test_encoding_mistakes_fail(kind, bug):
    for ray_form, per_group, S in ((False, 65, 1), (True, 5, 9)):
        ok, failed, *_ = planted(kind, 1, per_group, S, ray_form, bug)
        assert not ok, (bug, ray_form)
        if ray_form:
            assert failed == {"g_rays origin", "g_rays direction"}
        else:
            assert failed == {"g_x position", "g_x direction"}


def test_two_dropped_frequencies_stay_under_the_tensor_wide_tolerance():
    """Why this gate exists: without the i = 0 and i = 1 terms of dx_c the position gradient of a NeRF moves by less than
    GRAD_TOL_RELU in relative L2 - the only gate the ReLU kinds had - while stage D rejects it."""
    for kind in ("nerf", "tiny_nerf"):
        ok, failed, st, good, bad = planted(kind, 1, 333, 1, False, "frequencies 0 and 1 dropped")
        ref = D.stage_d_points(kind, st["A"], st["D"], st["params"], None, 333)[0].numpy()
        rel = np.linalg.norm(bad[:, :3] - ref) / np.linalg.norm(ref)
        assert 1e-3 < rel < parity.GRAD_TOL_RELU, rel
        assert not ok and "g_x position" in failed


@pytest.mark.parametrize("kind", ["nerf", "siren_nerf"])
def test_missing_skip_layer_fails(kind):
    for ray_form, per_group, S in ((False, 65, 1), (True, 5, 9)):
        ok, failed, *_ = planted(kind, 1, per_group, S, ray_form, "no skip")
        assert not ok and failed == ({"g_rays origin", "g_rays direction"} if ray_form else {"g_x position"})


@pytest.mark.parametrize("kind", ["film_siren_nerf", "film_siren_nerf_nodir", G.depth_name(12, True)])
def test_missing_gamma_fails(kind):
    nodir = kind.endswith("nodir")
    ok, failed, *_ = planted(kind, 3, 33, 1, False, "no gamma")
    assert not ok and failed == ({"g_x position"} if nodir else {"g_x position", "g_x direction"})
    ok, failed, *_ = planted(kind, 2, 5, 9, True, "no gamma")
    assert not ok and failed == {"g_rays origin", "g_rays direction"}


def test_chunk_straddling_a_group_fails():
    """33 points per group in chunks of 32 cut over all points: the second chunk holds points of groups 0 and 1."""
    ok, failed, *_ = planted("film_siren_nerf", 3, 33, 1, False, "chunks straddle groups")
    assert not ok and "g_x position" in failed


@pytest.mark.parametrize("kind", ["nerf", "tiny_nerf"])
def test_counted_tail_point_fails(kind):
    for S in (1, 3, 5, 9):                                  # every ragged last step; S = 4, 8 have none
        ok, failed, *_ = planted(kind, 1, 5, S, True, "tail counted")
        assert not ok and failed >= {"g_rays origin"}, S
    ok, *_ = planted(kind, 1, 5, 8, True, "tail counted")
    assert ok


@pytest.mark.parametrize("kind", ["nerf", "siren_nerf", "film_siren_nerf"])
@pytest.mark.parametrize("bug", ["z shifted", "no projection", "no norm"])
def test_ray_reduction_mistakes_fail(kind, bug):
    """NeRF's g_d is dominated by sum_s z_s g_pos,s - 512 products per encoding column, frequencies up to 2^9 - whose
    worst-case bound (gamma(530) of its magnitude) is as large as the whole 4-frequency direction term: a mistake in
    (I - v v^T) / |d| is judged on its own scale only with the position columns zeroed, which is why the GPU test runs
    the direction frequencies in calls of their own."""
    g = 2 if is_film(kind) else 1
    ok, failed, *_ = planted(kind, g, 6 // g + 2, 9, True, bug, direction_only=kind in D.PE_KINDS and bug != "z shifted")
    assert not ok and failed == {"g_rays direction"}


@pytest.mark.parametrize("kind", ["nerf", "siren_nerf"])
def test_wrong_stride_fails(kind):
    """A stride one unit too long skips units (their outputs keep the NaN fill); one too short does units twice, which
    only `accumulate` can show: base + g twice is not base + g."""
    pe = kind in D.PE_KINDS
    n = 2 * D.sweep_units(pe, 1) + 5
    S = 3 if pe else 2
    for ray_form, per_group, s in ((True, n, S), (False, D.sweep_units(pe, 1) * D.CHUNK + 45, 1)):
        ok, failed, *_ = planted(kind, 1, per_group, s, ray_form, "stride", stride_off=1)
        assert not ok and len(failed) >= 2
    st = synthetic(kind, 1, n, S, 7)
    g = simulate(kind, st, 1, n, S, True)
    base = np.random.Generator(np.random.PCG64(8)).normal(size=g.shape).astype(f32)
    assert np.array_equal(simulate(kind, st, 1, n, S, True, accumulate=1, out=base.copy()), base + g)
    twice = simulate(kind, st, 1, n, S, True, accumulate=1, out=base.copy(), stride_off=-1)
    assert not np.array_equal(twice, base + g)
    over = simulate(kind, st, 1, n, S, True, accumulate=1, out=base.copy(), bug="accumulate overwrites")
    assert not np.array_equal(over, base + g) and np.array_equal(over, g)

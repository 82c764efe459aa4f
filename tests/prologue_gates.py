"""Stage P, the prologue of the field forward (test_gpu_prologue_gates.py, test_prologue_gates_host.py): torch / numpy only.

The prologue turns the caller's inputs into the rows the first layers read (csrc/field_mlp_device.h: load_point,
posenc_blocks / pe_feature, store_xin): the points `pts = fl(o + fl(d z))`, the view `d / |d|`, and for the NeRF kinds their
positional encodings E_pos (10 frequencies, 60 columns + 4 pads) and E_dir (4 frequencies, 24 + 8 pads); the sin and FiLM
kinds save `xin = (pts, view, 0, 0)`.  Here that step is restated from its definition and every saved element is gated
against it (u = 2^-24):

  pts      bit for bit against the fp32 expression `o + d * z` with two roundings (the reference's rays_o + rays_d * z);
           observable as xin[:, 0:3].  In point form xin[:, 0:6] is the caller's x, bit for bit.
  view     |view - d / |d|_fp64| <= 4 u |view| per element: the sum of squares carries at most 3 u relative, the square root
           halves that and adds its own u, the division adds u - 3.5 u, rounded up.  Observable as xin[:, 3:6].  Every sample
           of one ray carries bit-identical view columns (NeRF kinds: bit-identical E_dir rows).
  E_pos    column 6 i + c against sin (c < 3) or cos of 2^i p_c in fp64, p the fp32 pts above (the product is exact).
           Sine columns: SIN_EPS (bwd_gates.SIN_EPS, csrc/mi_math.h's measurement of the six-instruction reduction).  Cosine
           columns: SIN_EPS + 2 pi 2^-25 - pe_feature forms r = turns + 1/4 in fp32, and for r in [1/2, 3/4] that addition
           rounds at half an ulp of [1/2, 1), 2^-25 turn.  No term grows with |2^i p|: the reduction's split constant is good to
           about 2^-49 relative and hi - rndne(hi) is exact.
  E_dir    the same rule over four frequencies of the fp64 view, plus the propagated 2^i 3.5 u |v_c| (a NeRF kind does not
           save the view itself).  In point form the direction is the caller's and nothing propagates.
  pads     columns 60..63 of E_pos, 24..31 of E_dir, 6..7 of xin: +0, bit for bit.
  extent   with the buffer filled with a NaN bit pattern before the call, no float of any region keeps it (every region has
           exactly P rows' worth of written floats) and the canary tail behind the queried size is untouched.

The bounds are derived or taken from bwd_gates.SIN_EPS, never calibrated on the kernels.  Every gate leaves one parity record
of stage "P prologue": the worst ratio, its position, the element count, and beside it (`oracle32_ratio`) the ratio of the
reference's own fp32 torch evaluation of the same inputs (`oracle32` / `assemble`), which has to stay below 1 as well for the
bound to be an honest one.  Nothing is masked.

The five input regimes (`REGIMES`) are shared by the host and the GPU test."""
from __future__ import annotations

import math

import numpy as np
import torch

import bwd_gates as G
from oracle import fields as ofields, parity, render_ref as R

U = G.U
STAGE = "P prologue"
N_POS, N_DIR = 10, 4                               # frequencies of E_pos / E_dir (nerf/nerf.py:44-49)
COS_SHIFT = 2.0 * math.pi * 2.0 ** -25             # the quarter-turn addition's rounding, in radians
SIN_BOUND = G.SIN_EPS
COS_BOUND = G.SIN_EPS + COS_SHIFT
C_VIEW = 4.0                                       # view: c u |view|
C_VIEW_PROP = 3.5                                  # what E_dir's angle inherits from the view, before the rounding up
PE_KINDS = ("nerf", "tiny_nerf")                   # the kinds that save encodings; every other kind saves xin
FILL = 0x7FC0BEEF                                  # a quiet NaN no kernel produces: the buffer's floats before the call
f32 = np.float32

# ---- the cases (shared by the host and the GPU test) --------------------------------------------------------------------
KINDS = (["nerf", "tiny_nerf", "siren_nerf", "film_siren_nerf", "film_siren_nerf_nodir"]
         + [G.depth_name(L, use_dir) for L in (4, 12) for use_dir in (True, False)])
# (rays, samples): one point; either side of the 128-point tile; 130 points, a tile ending inside a ray; 1 332 points, ten
# full tiles and 52 tail lanes; three long rays
RAY_SHAPES = [(1, 1), (127, 1), (129, 1), (26, 5), (37, 36), (3, 192)]
# FiLM kinds, (groups, rays per group, samples): 325 points per group are two tiles and a tail of 69; one-point groups
GROUP_SHAPES = [(2, 65, 5), (3, 65, 5), (2, 1, 1)]
POINTS_PER_GROUP = [1, 31, 129, 333]               # point form


def is_film(kind: str) -> bool:
    return G.depth_of(kind) is not None


# ---- the restatement ---------------------------------------------------------------------------------------------------
def points(o, d, z):
    """[n, S, 3] = o + d * z in the dtype of its inputs: a multiply and an add, each rounded (nerf/render.py:134)."""
    return o[..., None, :] + d[..., None, :] * z[..., :, None]


def view_dirs(d):
    """[n, 3] = d / |d| in the dtype of its input (nerf/render.py:122)."""
    return d / torch.norm(d, dim=-1, keepdim=True)


def encoding(v, nfreq: int):
    """[P, 6 nfreq]: column 6 i + c is sin (c < 3) or cos (c >= 3) of 2^i v_(c mod 3), in v's dtype."""
    s = 2.0 ** torch.arange(nfreq, dtype=v.dtype)
    ang = s[None, :, None] * v[:, None, :]
    return torch.cat([torch.sin(ang), torch.cos(ang)], -1).reshape(v.shape[0], 6 * nfreq)


def encoding_bound(v64, nfreq: int, prop: float = 0.0):
    """Per-element bound of an encoding: SIN_BOUND on sine, COS_BOUND on cosine columns, + 2^i prop u |v_c|."""
    s = 2.0 ** torch.arange(nfreq, dtype=torch.float64)
    carried = prop * U * s[None, :, None] * v64.abs()[:, None, :]
    return torch.cat([SIN_BOUND + carried, COS_BOUND + carried], -1).reshape(v64.shape[0], 6 * nfreq)


def is_cos(nfreq: int):
    return (torch.arange(6 * nfreq) % 6) >= 3


def restate(inp: dict) -> dict:
    """The definition of the prologue on one call's inputs (CPU or device fp32 tensors): form "rays" = rays [n, 2, 3] and
    z [n, S]; form "points" = x [P, 6].  pts [P, 3] fp32 (bits); view [P, 3] fp64; prop: the view's relative error in u that
    an encoding of it inherits; S: samples per ray (rows of one ray are consecutive), None in point form."""
    if "x" in inp:
        x = inp["x"]
        return dict(pts=x[:, :3].contiguous(), view=x[:, 3:6].double(), view_bits=x[:, 3:6].contiguous(), prop=0.0, S=None)
    rays, z = inp["rays"], inp["z"]
    n, S = z.shape
    pts = points(rays[:, 0], rays[:, 1], z).reshape(-1, 3)
    v = view_dirs(rays[:, 1].double())
    return dict(pts=pts, view=v[:, None].expand(n, S, 3).reshape(-1, 3), view_bits=None, prop=C_VIEW_PROP, S=S)


def oracle32(inp: dict):
    """(pts, view) [P, 3] as the reference computes them in fp32 torch: oracle.render_ref.points_on_rays and the view
    expression of its render_rays; in point form the caller's columns."""
    if "x" in inp:
        return inp["x"][:, :3], inp["x"][:, 3:6]
    rays, z = inp["rays"], inp["z"]
    o, d = rays[:, 0], rays[:, 1]
    pts = R.points_on_rays(o, d, z)
    view = (d / torch.norm(d, dim=-1, keepdim=True))[:, None].expand_as(pts)
    return pts.reshape(-1, 3), view.reshape(-1, 3)


def assemble(kind: str, pts, view) -> dict:
    """The rows a prologue saves, from its points and view: {"E_pos": [P, 64], "E_dir": [P, 32]} with the oracle field's
    positional encoding, or {"xin": [P, 8]}."""
    P = pts.shape[0]
    zeros = lambda w: torch.zeros(P, w, dtype=pts.dtype, device=pts.device)  # noqa: E731
    if kind in PE_KINDS:
        return {"E_pos": torch.cat([ofields.posenc(pts, N_POS), zeros(4)], 1),
                "E_dir": torch.cat([ofields.posenc(view, N_DIR), zeros(8)], 1)}
    return {"xin": torch.cat([pts, view, zeros(2)], 1)}


# ---- the gates ---------------------------------------------------------------------------------------------------------
def bits(t):
    """The bit patterns of fp32 values as exact float64 numbers (+0 and -0 differ)."""
    return torch.as_tensor(t).contiguous().view(torch.int32).double()


def _gate(res: dict, case: str, name: str, got, ora, ref, bound, active: str):
    worst, where = G.worst_ratio(got, ref, bound)
    G.record(case, STAGE, name, worst, where, torch.as_tensor(got).numel(), active)
    parity.RECORDS[-1]["oracle32_ratio"] = G.worst_ratio(ora, ref, bound)[0]
    res[name] = worst


def _exact(res, case, name, got_bits, ora_bits, ref_bits, active="bit for bit"):
    _gate(res, case, name, got_bits, ora_bits, ref_bits, torch.zeros((), dtype=torch.float64), active)


def _same_per_ray(res, case, name, rows, ora_rows, S):
    """Every sample's row of one ray against the ray's first sample, bit for bit."""
    def spread(t):
        b = bits(t).reshape(-1, S, t.shape[-1])
        return b, b[:, :1].expand_as(b)
    (got, ref), (ora, ora_ref) = spread(rows), spread(ora_rows)
    # the oracle's rows are held to the oracle's own first sample: shifted onto `ref`, its differences are what is gated
    _exact(res, case, name, got, ora - ora_ref + ref, ref, "bit-identical over the samples of a ray")


def check(case: str, kind: str, inp: dict, first: dict) -> dict:
    """Gate the saved rows `first` ({"E_pos", "E_dir"} or {"xin"}, [P, width] fp32) of one call against the restatement of
    `inp`.  One record per gate; returns {gate: worst ratio} (passed: every ratio <= 1)."""
    dev = next(iter(first.values())).device
    inp = {k: torch.as_tensor(v).to(dev) for k, v in inp.items()}
    ref = restate(inp)
    o_pts, o_view = oracle32(inp)
    ora = assemble(kind, o_pts, o_view)
    pts, view, S = ref["pts"], ref["view"], ref["S"]
    res = {}
    if kind in PE_KINDS:
        for name, v64, nfreq, prop in (("E_pos", pts.double(), N_POS, 0.0), ("E_dir", view, N_DIR, ref["prop"])):
            got, o, w = first[name], ora[name], 6 * nfreq
            e_ref, e_bound = encoding(v64, nfreq), encoding_bound(v64, nfreq, prop)
            carried = f" + 2^i {prop:g} u |v|" if prop else ""
            for part, cols, active in (("sin", ~is_cos(nfreq), f"SIN_EPS{carried}"),
                                       ("cos", is_cos(nfreq), f"SIN_EPS + 2 pi 2^-25{carried}")):
                cols = cols.to(dev)
                _gate(res, case, f"{name} {part}", got[:, :w][:, cols], o[:, :w][:, cols], e_ref[:, cols], e_bound[:, cols],
                      active)
            _exact(res, case, f"{name} pads", bits(got[:, w:]), bits(o[:, w:]), torch.zeros_like(got[:, w:]).double(),
                   "+0 bit for bit")
        if S is not None:
            _same_per_ray(res, case, "E_dir rows of one ray", first["E_dir"], ora["E_dir"], S)
        return res
    got, o = first["xin"], ora["xin"]
    _exact(res, case, "xin pts", bits(got[:, :3]), bits(o[:, :3]), bits(pts))
    if ref["view_bits"] is not None:                 # point form: the caller's columns
        _exact(res, case, "xin view", bits(got[:, 3:6]), bits(o[:, 3:6]), bits(ref["view_bits"]))
    else:
        _gate(res, case, "xin view", got[:, 3:6], o[:, 3:6], view, C_VIEW * U * view.abs(), f"{C_VIEW:g} u |view|")
        _same_per_ray(res, case, "xin view of one ray", got[:, 3:6], o[:, 3:6], S)
    _exact(res, case, "xin pads", bits(got[:, 6:]), bits(o[:, 6:]), torch.zeros_like(got[:, 6:]).double(), "+0 bit for bit")
    return res


def extent(case: str, kind: str, acts, P: int, tail=None, canary: int = 0, fill: int = FILL) -> dict:
    """The written extent of a training forward's acts: `acts` (the queried size, FILL in every float before the call) keeps
    no FILL in any region - each has exactly P rows' worth of written floats - and `tail` (floats behind the queried size,
    `canary` in each before the call) is untouched.  One record; the ratio is inf for any float out of place."""
    a = torch.as_tensor(acts).contiguous().view(torch.int32)
    layout = G.ACTS[kind]
    assert a.numel() == G.floats_per_point(layout) * P, (a.numel(), G.floats_per_point(layout), P)
    kept = a == fill
    bad, where = int(kept.sum()), int(kept.int().argmax()) if bool(kept.any()) else -1
    if tail is not None:
        t = torch.as_tensor(tail).contiguous().view(torch.int32) != canary
        if bool(t.any()):
            bad, where = bad + int(t.sum()), (a.numel() + int(t.int().argmax()) if where < 0 else where)
    G.record(case, STAGE, "acts extent", math.inf if bad else 0.0, where, a.numel() + (0 if tail is None else len(tail)),
             f"every region P rows written, tail untouched ({bad} floats out of place)")
    parity.RECORDS[-1]["oracle32_ratio"] = 0.0
    return {"acts extent": math.inf if bad else 0.0}


def failed(res: dict) -> list:
    return sorted(k for k, v in res.items() if not v <= 1.0)


# ---- input regimes -----------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _pack(o, d, z):
    return dict(rays=torch.from_numpy(np.stack([o, d], 1).astype(f32)), z=torch.from_numpy(np.ascontiguousarray(z, dtype=f32)))


def scene(n, S, seed):
    """|o| = 4, d = -o / 4 + 0.3 N(0, 1), z sorted in [2, 6]: the inputs of test_gpu_bwd_stages.run."""
    rng = _rng(seed)
    o = 4.0 * _unit(rng, n)
    return _pack(o, -o / 4.0 + 0.3 * rng.normal(size=(n, 3)), np.sort(2.0 + 4.0 * rng.random((n, S)), -1))


def wide(n, S, seed):
    """Coordinates up to +-64 (|o| <= 40, |d| <= 4, z <= 6): 2^9 x reaches 32 768 rad."""
    rng = _rng(seed)
    return _pack(rng.uniform(-40, 40, (n, 3)), rng.uniform(-4, 4, (n, 3)), np.sort(rng.uniform(0, 6, (n, S)), -1))


def small(n, S, seed):
    """Point magnitudes 1e-30 .. 1e-2 (o log-uniform there, d z too), components exactly +0 and -0, rays along one axis.
    The direction's components stay in 1e-12 .. 1e-2, where their squares and the view's components are normal fp32
    numbers: below that the fp32 reference itself loses the relative accuracy the view gate asks for."""
    rng = _rng(seed)
    sign = lambda shape: rng.choice([-1.0, 1.0], shape)  # noqa: E731
    o = sign((n, 3)) * 10.0 ** rng.uniform(-30, -2, (n, 3))
    d = sign((n, 3)) * 10.0 ** rng.uniform(-12, -2, (n, 3))
    z = np.sort(10.0 ** rng.uniform(-18, 0, (n, S)), -1)
    r = np.arange(n)
    o[r[0::3], r[0::3] % 3] = 0.0
    o[r[1::6], (r[1::6] + 1) % 3] = -0.0
    d[r[2::4], r[2::4] % 3] = -0.0                    # one component -0, the ray still has two others
    axis = r[1::5]                                    # along one axis: the other two +0 and -0
    d[axis, (axis + 1) % 3], d[axis, (axis + 2) % 3] = 0.0, -0.0
    d[axis, axis % 3] = sign(len(axis)) * 10.0 ** rng.uniform(-12, -2, len(axis))
    z[r[3::4], 0] = 0.0
    return _pack(o, d, z)


def decades(n, S, seed):
    """|d| over six decades (1e-3 .. 1e3), z scaled by 1 / |d| so the points stay in the scene's box."""
    rng = _rng(seed)
    o, u = 4.0 * _unit(rng, n), _unit(rng, n)
    d = (u * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(f32)
    z = np.sort(2.0 + 4.0 * rng.random((n, S)), -1) / np.linalg.norm(d.astype(np.float64), axis=-1, keepdims=True)
    return _pack(o, d, z)


def turn_values():
    """[10 * 17 * 3] fp32: for each frequency i the nearest float to k pi / 2^(i+1), k = -8 .. 8, and its two neighbours -
    2^i x is a whole number of quarter turns, where rndne ties and the quarter-turn shift crosses 1/2."""
    out = []
    for i in range(N_POS):
        for k in range(-8, 9):
            t = f32(k * math.pi / 2.0 ** (i + 1))
            out += [np.nextafter(t, f32(-np.inf)), t, np.nextafter(t, f32(np.inf))]
    return np.asarray(out, dtype=f32)


def turns(n, S, seed):
    """Turn boundaries: ray r starts (z = +0 on its first sample, so pts = o bit for bit) at three consecutive values of
    turn_values(), from value 3 (r + seed) on, cyclically; its later samples are ordinary points (d ~ 0.3 N, z in (0, 1))."""
    rng = _rng(seed)
    vals = turn_values()
    o = vals[(3 * (np.arange(n)[:, None] + seed) + np.arange(3)[None, :]) % len(vals)]
    z = np.sort(rng.random((n, S)), -1)
    z[:, 0] = 0.0
    return _pack(o, 0.3 * rng.normal(size=(n, 3)), z)


REGIMES = {"scene": scene, "wide": wide, "small": small, "decades": decades, "turns": turns}


def as_points(inp: dict):
    """Point-form inputs of a regime: x [P, 6] = (the regime's points, its directions as they are - not normalised)."""
    rays, z = inp["rays"], inp["z"]
    pts = points(rays[:, 0], rays[:, 1], z)
    return dict(x=torch.cat([pts, rays[:, 1][:, None].expand_as(pts)], -1).reshape(-1, 6).contiguous())

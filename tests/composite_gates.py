"""Stage gates of compositing (test_gpu_composite_stages.py, test_composite_gates_host.py): torch only.

composite_kernel, composite_weights_kernel and composite_bwd_kernel (csrc/render_stages.hip) are rebuilt in float64 from
the kernels' OWN fp32 inputs (raw [n,S,4], z [n,S], ray directions [n,3], the cotangents g_rgb, g_depth, g_acc, g_w), and
beside every exact value runs a first-order bound of what fp32 arithmetic of the same formula may lose, built from
absolute values as bwd_gates.py does for the MLP.  With u = 2^-24 and tiny = 2^-126 (fp32's underflow floor):

  delta_k = (z_{k+1} - z_k) |d|  (last: 1e10 |d|)    x = sigma delta    e = exp(-x)    alpha = 1 - e    f = 1 - alpha + 1e-10
  T_0 = 1, T_{k+1} = T_k f_k      w = alpha T      acc = sum w      depth = sum w z      rgb = sum w c + (1 - acc)
  G_k = sum_c g_rgb[c] (c_k[c] - 1) + g_depth z_k + g_acc + g_w[k]          |G|_k: the same, absolute values term by term
  R_k = G_k alpha_k + f_k R_{k+1}, R_S = 0                                   |R|_k = |G|_k alpha_k + f_k |R|_{k+1}
  d/dsigma_k = T_k (G_k - R_{k+1}) delta_k e_k                               d/dc_k = g_rgb w_k

  e_alpha = u (e + 6 x e) + min(u alpha, e) + tiny          e_f = e_alpha + u f
  e_T[k+1] = e_T[k] (f_k + e_f[k]) + T_k e_f[k] + u T_{k+1} + tiny
  e_w     = e_alpha T + (alpha + e_alpha) e_T + u w + tiny
  e_acc   = sum e_w + 2 u sqrt(S) sum w
  e_depth = sum e_w |z| + u (2 sqrt(S) + 1) sum w |z|        (+ 1: the product w z)
  e_rgb   = sum e_w |c| + u (2 sqrt(S) + 1) sum w |c| + e_acc + u (1 + |rgb|)
  e_R[k]  = 4 u |G|_k alpha_k + |G|_k e_alpha[k] + e_f[k] |R|_{k+1} + (f_k + e_f[k]) e_R[k+1] + u |R|_k
  e_dsig  = (e_T (|G| + |R|_{k+1}) + (T + e_T) (4 u |G| + e_R[k+1])) delta e + u (6 + 6 x) T (|G| + |R|_{k+1}) delta e
            + tiny delta T (|G| + |R|_{k+1}) + tiny (1 + delta)
  e_dc    = |g_rgb| (e_w + u w) + tiny

Where the terms come from.  x is three fp32 products and a difference of the inputs (6 u x covers them and |d|'s square
root), and an error dx of x moves e by e dx.  alpha = fl(1 - e): rounding to nearest is no further from 1 - e than ANY
fp32 number is, and 1 is one, so that rounding loses at most min(u alpha, e) - behind an opaque sample (e = 1e-87) alpha
is exact, and f = 1e-10 is known to u f.  (With u alpha alone the bound of T behind a wall is u T_k, six hundred times the
1e-10 T_k that the floor itself contributes: a kernel without the + 1e-10 passed.  test_composite_gates_host.py holds
that mutation.)  The products keep their second-order terms (|T' f' - T f| <= e_T (f + e_f) + T e_f, not e_T f + T e_f): behind a
saturated sample f is 1e-10 + e with e near u, its fp32 value is off by as much as f itself, and two such samples in a row
put the fp32 oracle 1.4 first-order bounds away (seen on the x50 NeRF field's own raw, oracle and kernel alike).  The sums
allow 2 u sqrt(S) of the sum of magnitudes: S sequential additions in the oracle, ceil(S / G)
sequential and log2 G tree additions per lane in the kernels (9 for S = 192).  G_k is seven products and additions (4 u).
The tiny terms are fp32's underflow floor: where T or e leaves the fp32 range the fp32 oracle itself sits 1e3 .. 1e308
bounds away without them.

Gate: |got - ref64| <= C e for EVERY element: every ray, every sample, the last sample included, nothing masked.

The constants C come from the reference, never from the HIP result.  With C = 1 the bound is a worst case of the
formula's own fp32 roundings, so a result inside it is within rounding by derivation; a margin times the fp32 oracle's own
worst err / e takes over only if the oracle itself needs more than 1 anywhere on the case matrix (S_MATRIX x REGIMES,
n = 257, seed = S; `matrix_cases`, `constant_for`): C = 1 while that ratio is <= 1, else margin x ratio.  The oracle is
oracle.render_ref.composite and its autograd on the CPU, g_w included.  The margins are the project's (oracle/parity.py):
FP64_FACTOR 1.5 for rgb / depth / acc, FP64_FACTOR_INTERMEDIATE 2.0 for the weights, gate_grad's cpu_factor 3.0 for the
two gradients; they would pay for the device's expf and tree-ordered sums against the host's exp and sequential sums.
test_composite_gates_host.py re-measures the ratios on every run and fails when the rule's constant leaves the committed
one by more than 10 %.  This is the stricter reading of max(1, margin x ratio): the min(u alpha, e) term is ATTAINED
(a sample with e just below u / 2 has alpha = 1 in every fp32 pipeline, the sample behind it T = 1e-10 T_k instead of
(e + 1e-10) T_k: an error of exactly e T_k), so the oracle's worst ratio of the three quantities that see T per sample is
1.000 by arithmetic, not by noise, and a margin on it would triple the gradient bounds everywhere - the host test's
1e-3 change of the median sharp-regime element then passes.

  quantity     oracle's worst err / e over the 126 cases    margin    C
  rgb          0.238                                        1.5       1
  depth        0.236                                        1.5       1
  acc          0.247                                        1.5       1
  weights      1.000 (attained, see above)                  2.0       1
  d/dsigma     1.000 (attained)                             3.0       1
  d/dcolour    1.000 (attained)                             3.0       1

For information only (the constants do not depend on it): the HIP kernels' worst err / (C e) over the 986 records of
test_gpu_composite_stages.py on one MI355X (profiles/composite_stage_parity.json), the oracle's on the same cases in
brackets: rgb 0.223 (0.238), depth 0.264 (0.280), acc 0.288 (0.247), weights, d/dsigma and d/dcolour 1.000 (1.000; the
attained corner, on the same elements as the oracle); away from it, e.g. 1024 x 192 of the x50 field: weights 0.62 (0.62),
d/dsigma 0.24 (0.24).  A scratch build whose backward wrote zeros on every sample but the last of a ray missed the
d/dsigma gate by 4e5 and the d/dcolour gate by 5e6.

What the gate cannot resolve: the bound of an element deep behind dense samples is set by the magnitudes upstream of
it, as fp32's own error is, so a 1e-5 relative change of such an element is below it.  The host test records, per regime,
the share of nonzero elements with |ref| >= 100 e (`SHARE_100`) and fails when a later loosening of a term lowers it.

Every gate call leaves one parity record per quantity: err_over_bound (in units of C e), oracle32_err_over_bound for
the same case, active (the bound in words and C), elements, worst_index ([ray, sample(, channel)])."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import parity, render_ref as R

U = 2.0 ** -24                 # unit roundoff of fp32
TINY = 2.0 ** -126             # smallest normal fp32: the absolute floor of anything that underflows

QUANTITIES = ("rgb", "depth", "acc", "weights", "dsigma", "dcolour")
MARGIN = {"rgb": parity.FP64_FACTOR, "depth": parity.FP64_FACTOR, "acc": parity.FP64_FACTOR,
          "weights": parity.FP64_FACTOR_INTERMEDIATE, "dsigma": 3.0, "dcolour": 3.0}
# 1 while the fp32 oracle's worst ratio over matrix_cases() is at most 1, else MARGIN x that ratio (`constant_for`)
C = {"rgb": 1.0, "depth": 1.0, "acc": 1.0, "weights": 1.0, "dsigma": 1.0, "dcolour": 1.0}

S_MATRIX = (1, 2, 15, 16, 17, 31, 32, 33, 36, 63, 64, 65, 72, 127, 128, 129, 192, 256)
REGIMES = ("plain", "sharp", "wall", "empty", "thin", "ties", "last")
N_MATRIX = 257


# ---- cases -------------------------------------------------------------------------------------------------------------
def make_case(S: int, n: int, regime: str, seed: int) -> dict:
    """fp32 CPU tensors raw, z, rd and the four cotangents.  Colours uniform, sigma exponential(2) on half the samples
    (plain), x50 (sharp), 0 or 1e4 (wall), 0 (empty), x1e-3 (thin), repeated depths (ties), the last sample's sigma 0 on
    even rays and positive on odd ones (last); |d| over two decades."""
    rng = np.random.Generator(np.random.PCG64(seed))
    raw = rng.uniform(0, 1, size=(n, S, 4)).astype(np.float32)
    sg = rng.exponential(2.0, size=(n, S)).astype(np.float32) * (rng.random((n, S)) < 0.5)
    if regime == "sharp":
        sg *= 50
    if regime == "wall":
        sg = np.where(rng.random((n, S)) < 0.1, 1e4, 0).astype(np.float32)
    if regime == "empty":
        sg *= 0
    if regime == "thin":
        sg *= 1e-3
    if regime == "last":
        sg[0::2, -1] = 0.0
        sg[1::2, -1] = 0.25 + sg[1::2, -1]
    raw[..., 3] = sg
    z = np.sort(rng.uniform(2, 6, size=(n, S)).astype(np.float32), -1)
    if regime == "ties" and S > 2:
        m = z[:, 1::3].shape[1]
        z[:, 1::3] = z[:, 0:-1:3][:, :m]
    rd = (rng.normal(size=(n, 3)) * 10 ** rng.uniform(-1, 1, size=(n, 1))).astype(np.float32)
    cot = [rng.normal(size=s).astype(np.float32) for s in ((n, 3), (n,), (n,), (n, S))]
    names = ("raw", "z", "rd", "g_rgb", "g_depth", "g_acc", "g_w")
    return {k: torch.from_numpy(a) for k, a in zip(names, [raw, z, rd] + cot)}


def constant_for(q: str, oracle_worst: float) -> float:
    """The constant that the rule gives quantity q when the fp32 oracle's worst err / e over the matrix is oracle_worst."""
    return 1.0 if oracle_worst <= 1.0 else MARGIN[q] * oracle_worst


def matrix_cases():
    """(name, S, regime) of the constants' case matrix; the case itself is make_case(S, N_MATRIX, regime, seed=S)."""
    return [(f"S={S} {regime}", S, regime) for S in S_MATRIX for regime in REGIMES]


# ---- the fp64 reference and its bound --------------------------------------------------------------------------------
def reference(raw, z, rd, g_rgb=None, g_depth=None, g_acc=None, g_w=None) -> dict:
    """{quantity: (exact value, bound e)} in float64 on the inputs' device; a cotangent that is None counts as zeros."""
    raw, z, rd = raw.double(), z.double(), rd.double()
    n, S, _ = raw.shape
    kw = dict(dtype=torch.float64, device=raw.device)
    zero = lambda *s: torch.zeros(*s, **kw)                                                    # noqa: E731
    g_rgb = zero(n, 3) if g_rgb is None else g_rgb.double()
    g_depth = zero(n) if g_depth is None else g_depth.double()
    g_acc = zero(n) if g_acc is None else g_acc.double()
    g_w = zero(n, S) if g_w is None else g_w.double()
    sig, col = raw[..., 3], raw[..., :3]
    assert bool((sig >= 0).all()), "sigma is a ReLU's output"
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full((n, 1), 1e10, **kw)], 1) * rd.norm(dim=-1, keepdim=True)
    x = sig * delta
    e = torch.exp(-x)
    al = -torch.expm1(-x)                     # 1 - e without float64's own rounding of it: the bound goes down to e itself
    f = e + 1e-10                             # 1 - alpha + 1e-10
    xe = torch.where(e == 0, torch.zeros_like(x), x * e)
    eal = U * (e + 6 * xe) + torch.minimum(U * al, e) + TINY
    ef = eal + U * f
    T, eT = torch.ones(n, S, **kw), zero(n, S)
    for k in range(1, S):
        T[:, k] = T[:, k - 1] * f[:, k - 1]
        eT[:, k] = eT[:, k - 1] * (f[:, k - 1] + ef[:, k - 1]) + T[:, k - 1] * ef[:, k - 1] + U * T[:, k] + TINY
    w = al * T
    ew = eal * T + (al + eal) * eT + U * w + TINY
    rs = 2 * math.sqrt(S)
    acc, eacc = w.sum(1), ew.sum(1) + U * rs * w.sum(1)
    wz, wc = w * z.abs(), w[..., None] * col.abs()
    depth, edepth = (w * z).sum(1), (ew * z.abs()).sum(1) + U * (rs + 1) * wz.sum(1)
    rgb = (w[..., None] * col).sum(1) + (1 - acc)[:, None]
    ergb = (ew[..., None] * col.abs()).sum(1) + U * (rs + 1) * wc.sum(1) + eacc[:, None] + U * (1 + rgb.abs())
    # backward
    Gk = (g_rgb[:, None, :] * (col - 1)).sum(-1) + g_depth[:, None] * z + g_acc[:, None] + g_w
    Gm = (g_rgb.abs()[:, None, :] * (col - 1).abs()).sum(-1) + g_depth.abs()[:, None] * z.abs() + g_acc.abs()[:, None] \
        + g_w.abs()
    Rn, Rm, eR = zero(n, S + 1), zero(n, S + 1), zero(n, S + 1)
    for k in range(S - 1, -1, -1):
        Rn[:, k] = Gk[:, k] * al[:, k] + f[:, k] * Rn[:, k + 1]
        Rm[:, k] = Gm[:, k] * al[:, k] + f[:, k] * Rm[:, k + 1]
        eR[:, k] = 4 * U * Gm[:, k] * al[:, k] + Gm[:, k] * eal[:, k] + ef[:, k] * Rm[:, k + 1] + (f[:, k] + ef[:, k]) * eR[:, k + 1] \
            + U * Rm[:, k]
    de = torch.where(e == 0, torch.zeros_like(e), delta * e)
    xde = torch.where(e == 0, torch.zeros_like(e), x * de)
    GR = Gm + Rm[:, 1:]
    dsig = T * (Gk - Rn[:, 1:]) * de
    edsig = (eT * GR + (T + eT) * (4 * U * Gm + eR[:, 1:])) * de + U * T * GR * (6 * de + 6 * xde) + TINY * delta * T * GR \
        + TINY * (1 + delta)
    dcol = g_rgb[:, None, :] * w[..., None]
    edcol = g_rgb.abs()[:, None, :] * (ew + U * w)[..., None] + TINY
    return dict(rgb=(rgb, ergb), depth=(depth, edepth), acc=(acc, eacc), weights=(w, ew), dsigma=(dsig, edsig),
                dcolour=(dcol, edcol))


def oracle32(raw, z, rd, g_rgb=None, g_depth=None, g_acc=None, g_w=None) -> dict:
    """The fp32 oracle (oracle.render_ref.composite and its autograd) on the CPU: {quantity: tensor}."""
    raw, z, rd = (t.detach().cpu().float() for t in (raw, z, rd))
    rt = raw.clone().requires_grad_(True)
    rgb, depth, acc, w = R.composite(rt, z, rd)
    loss = rgb.sum() * 0
    for out, g in ((rgb, g_rgb), (depth, g_depth), (acc, g_acc), (w, g_w)):
        if g is not None:
            loss = loss + (out * g.detach().cpu().float()).sum()
    loss.backward()
    return dict(rgb=rgb.detach(), depth=depth.detach(), acc=acc.detach(), weights=w.detach(), dsigma=rt.grad[..., 3],
                dcolour=rt.grad[..., :3])


def split_g_raw(g_raw) -> dict:
    """dL/d(raw) [n,S,4] as the two gated quantities."""
    return dict(dsigma=g_raw[..., 3], dcolour=g_raw[..., :3])


# ---- the gate --------------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, bound):
    """(max |got - ref| / bound over the elements, its index as a list): 0 where the error is 0, inf for a NaN."""
    got = torch.as_tensor(got)
    ref = torch.as_tensor(ref).to(got.device)
    bound = torch.as_tensor(bound).to(device=got.device, dtype=torch.float64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = (got.double() - ref.double()).abs()
    ratio = torch.nan_to_num(torch.where(err == 0, torch.zeros_like(err), err / bound), nan=math.inf)
    if not ratio.numel():
        return 0.0, []
    i = int(ratio.argmax())
    return float(ratio.reshape(-1)[i]), [int(v) for v in np.unravel_index(i, tuple(ratio.shape))]


def gate(case: str, stage: str, got: dict, ref: dict, oracle: dict, check: bool = False) -> dict:
    """Every quantity of `got` against (value, bound) of `ref`, per element, C e; the fp32 oracle's own ratio on the same
    case beside it.  One parity record per quantity; returns {quantity: record}."""
    res = {}
    for q, t in got.items():
        val, bound = ref[q]
        worst, where = worst_ratio(t, val, C[q] * bound)
        o32, _ = worst_ratio(oracle[q], val.cpu(), C[q] * bound.cpu())
        rec = parity.record(case=case, stage=stage, qty=q, err_over_bound=float(f"{worst:.6g}"),
                            oracle32_err_over_bound=float(f"{o32:.6g}"), active=f"{C[q]:g} x fp32 bound, per element",
                            elements=int(torch.as_tensor(t).numel()), worst_index=where, passed=bool(worst <= 1.0))
        res[q] = rec
        if check:
            assert rec["passed"], rec
    return res

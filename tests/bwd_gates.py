"""Stage gates of the field backward (test_gpu_bwd_stages.py, test_gpu_bwd_stages_depth.py, test_bwd_gates_host.py):
torch only.

The training buffers are mirrored from csrc/field_layout.h (`ACTS`, `GRADS`, the switch-bit decoder), every network is
written down once as a list of linear layers (`network`; the FiLM depth kinds from their depth, `film_depth_network`), and
each stage of the backward is rebuilt in float64 from the kernels' OWN inputs to that stage:

  A  saving forward   every saved row from the saved input of its layer (no compounding through the network)
  B  chain            every dA region from the kernel's dA of the layers it feeds and the saved rows
  C  weight grads     dW = dA^T X, db = sum dA from the kernel's dA and X, slab by slab as the planner cuts the points

There is no ReLU flip noise between two pipelines here, so the gates are per element against a bound built alongside the
reference from absolute values (|W| |X|, |W|^T |dA|, |dA|^T |X|).  Every gate leaves one parity record."""
from __future__ import annotations

import math
import re
from collections import namedtuple

import numpy as np
import torch

from mirender.fields import KIND_NAMES
from oracle import parity


# ---- FiLM depth kinds ------------------------------------------------------------------------------------------------
# FilmSirenNeRF(hidden_layers = L) for L = 4..12 is named film_depth_L{L}_dir / film_depth_L{L}_nodir here and is
# MI_FIELD_FILM_DEPTH(L, use_dir) of include/mi_render.h at the C ABI.  L = 8 under these names is the same network as the
# fixed kinds film_siren_nerf / film_siren_nerf_nodir, described a second time (test_bwd_gates_host.py holds the two equal).
_DEPTH_NAME = re.compile(r"film_depth_L(\d+)_(dir|nodir)$")
DEPTH_MIN, DEPTH_MAX = 4, 12


def depth_name(L: int, use_dir: bool) -> str:
    return f"film_depth_L{L}_{'dir' if use_dir else 'nodir'}"


def depth_of(kind: str):
    """(hidden_layers, use_dir) of a FiLM kind name, fixed (8) or depth; None for the kinds without FiLM."""
    if kind in ("film_siren_nerf", "film_siren_nerf_nodir"):
        return 8, kind == "film_siren_nerf"
    m = _DEPTH_NAME.match(kind)
    if not m or not DEPTH_MIN <= int(m.group(1)) <= DEPTH_MAX:
        return None
    return int(m.group(1)), m.group(2) == "dir"


class _PerKind(dict):
    """A table over the fixed kinds that computes a depth kind's entry from its name (and does not keep it: iterating the
    table always gives the fixed kinds only)."""

    def __init__(self, fixed, depth_entry):
        super().__init__(fixed)
        self._depth_entry = depth_entry

    def __missing__(self, kind):
        d = depth_of(kind)
        if d is None:
            raise KeyError(kind)
        return self._depth_entry(*d)


# kind name -> the C ABI's kind number
KIND_IDS = _PerKind({name: k for k, name in KIND_NAMES.items()}, lambda L, use_dir: 0x100 + 2 * L + (1 if use_dir else 0))

U = 2.0 ** -24                 # unit roundoff of fp32
W0 = 30.0                      # sin layers' frequency: the default of the reference functions below; the GPU tests hand them
#                                the packed field's own w_0 (a FiLM module's constructor argument)

# Stage constants, in units of U, calibrated on an MI355X over every case of test_gpu_bwd_stages.py: the worst achieved
# error was 7.5 u (|W||X| + |b|) in stage A, 7.5 u |act'| |W|^T|dA| in stage B and 1.4 u sqrt(L) |dA|^T|X| in stage C
# (31-point FiLM sums; past 60 000 points it stays below 0.2 u sqrt(L)), so each constant is 3x that, rounded up.
C_A = 24.0                     # forward layer: c u (|W| |X| + |b|)
C_B = 24.0                     # chain layer:   c u |act'| (|W|^T |dA| + sqrt(K / 2) |start|)
C_C = 4.5                      # weight grads:  c u sqrt(L) (|dA|^T |X|),  L = slab_pts + n_slabs
SIN_EPS = 2e-7                 # |X - sin| of the hardware sine on a reduced angle (csrc/mi_math.h, next to cos_sign_into)
COS_BAND = 1e-3                # the saved cosine sign is only claimed where |cos| exceeds this (mi_math.h, same place)

# ---- training buffers (csrc/field_layout.h) -------------------------------------------------------------------------
# Per-point row-major regions [points][width]; region r starts at (sum of the widths before it) * points.
_NERF_GRADS = [(f"dA{l}", 256) for l in range(9)] + [("dA9", 128), ("heads", 4)]
ACTS = _PerKind({
    # E_pos(60 + pad) | H1..H8 post-ReLU | G = layers_dir.0 out | E_dir(24 + pad) | H_d | switches of H1..H8 | of H_d
    "nerf": ([("E_pos", 64)] + [(f"H{l}", 256) for l in range(1, 9)] + [("G", 256), ("E_dir", 32), ("H_d", 128)]
             + [(f"S{l}", 8) for l in range(1, 9)] + [("S_d", 4)]),
    "tiny_nerf": ([("E_pos", 64)] + [(f"H{l}", 256) for l in range(1, 5)] + [("E_dir", 32), ("H_d", 128)]
                  + [(f"S{l}", 8) for l in range(1, 5)] + [("S_d", 4)]),
    # xin = (xyz, dir, 0, 0) | X_l = sin(30 A_{l-1}) with the cosine's sign in the lowest mantissa bit | G | X_d
    "siren_nerf": [("xin", 8)] + [(f"X{l}", 256) for l in range(1, 9)] + [("G", 256), ("X_d", 128)],
    # xin | X_l of FiLM layer l = 0..8, encoded like SirenNeRF's
    "film_siren_nerf": [("xin", 8)] + [(f"X{l}", 256) for l in range(9)],
    # field_layout.h:film_acts_depth(L): xin | X_0 .. X_L
}, lambda L, use_dir: [("xin", 8)] + [(f"X{l}", 256) for l in range(L + 1)])
ACTS["film_siren_nerf_nodir"] = ACTS["film_siren_nerf"]
GRADS = _PerKind({
    "nerf": _NERF_GRADS,
    "tiny_nerf": [(f"dA{l}", 256) for l in range(4)] + [("dA4", 128), ("heads", 4)],
    "siren_nerf": _NERF_GRADS,
    "film_siren_nerf": [(f"dU{l}", 256) for l in range(9)] + [("heads", 4)],   # dL/du of FiLM layer l
    # field_layout.h:film_grads_depth(L): dU_0 .. dU_L | heads
}, lambda L, use_dir: [(f"dU{l}", 256) for l in range(L + 1)] + [("heads", 4)])
GRADS["film_siren_nerf_nodir"] = GRADS["film_siren_nerf"]


def floats_per_point(layout) -> int:
    return sum(w for _, w in layout)


def regions(layout, buf: torch.Tensor, P: int) -> dict:
    """{name: [P, width] view} of a training buffer."""
    out, o = {}, 0
    for name, w in layout:
        out[name] = buf[o * P:(o + w) * P].view(P, w)
        o += w
    return out


# ---- ReLU switches ---------------------------------------------------------------------------------------------------
def switch_units(width: int) -> np.ndarray:
    """[width, 32]: the unit that bit b of dword d of a switch region `width` dwords wide stands for.  Lane (point, half h)
    owns dwords [h w/2, (h+1) w/2); block m, quarter rg, element q is bit 31 - (16 (m & 1) + 4 rg + q) of its dword m >> 1;
    that accumulator element carries feature 32 m + 8 rg + 4 h + q (field_layout.h: the epilogue's row mapping)."""
    half = width // 2
    feat = np.empty((width, 32), np.int64)
    for d in range(width):
        h, mm = divmod(d, half)
        for b in range(32):
            t = 31 - b
            m, rg, q = 2 * mm + t // 16, (t % 16) // 4, t % 4
            feat[d, b] = 32 * m + 8 * rg + 4 * h + q
    return feat


def decode_switches(words: torch.Tensor) -> torch.Tensor:
    """Switch region [P, width] (fp32 storage) -> bool [P, 32 width] indexed by unit."""
    w = words.contiguous().view(torch.int32)
    P, W = w.shape
    bits = (w.unsqueeze(-1) >> torch.arange(32, device=w.device, dtype=torch.int32)) & 1
    out = torch.empty((P, 32 * W), dtype=torch.bool, device=w.device)
    out[:, torch.as_tensor(switch_units(W).reshape(-1), device=w.device)] = bits.reshape(P, -1).bool()
    return out


def cos_negative(x_saved: torch.Tensor) -> torch.Tensor:
    """The saved sign of cos(w0 u): the lowest mantissa bit of the saved X (set = negative)."""
    return (x_saved.contiguous().view(torch.int32) & 1).bool()


def dsin_from_saved(x_saved: torch.Tensor, w0: float = W0) -> torch.Tensor:
    """fp64 of the derivative factor the chain rebuilds: +-w0 sqrt(1 - X^2), sign from the saved bit."""
    x = x_saved.double()
    c = w0 * torch.sqrt(torch.clamp(1.0 - x * x, min=0.0))
    return torch.where(cos_negative(x_saved), -c, c)


# ---- the networks as lists of linear layers ---------------------------------------------------------------------------
# One input of a linear layer: columns [c0, c1) of an acts region, multiplied by the weight columns starting at wcol; the
# launch group of its weight-gradient job (BwdBatcher: g422, g221, g412, g111, thin; FiLM kinds per image: g422_img,
# thin_img) and whether that job also sums the bias.
In = namedtuple("In", "region c0 c1 wcol group bias")


class Layer:
    """One linear layer: parameter pair p (weight gp[2p], bias gp[2p + 1]); its inputs (`In`); activation; output (acts
    region, or raw columns for a head); its dA region in grads (or head columns); FiLM row."""

    def __init__(self, p, ins, act, out, grad, film=None):
        self.p, self.ins, self.act, self.out, self.grad, self.film = p, [In(*r) for r in ins], act, out, grad, film

    def weight_cols(self, W, r: In):
        """The columns of W (this layer's weight) that input r multiplies."""
        return W[:, r.wcol:r.wcol + (r.c1 - r.c0)]

    @property
    def head(self) -> bool:
        return isinstance(self.out, tuple)


def network(kind: str) -> list:
    L = Layer
    if kind in ("nerf", "tiny_nerf"):
        n = 8 if kind == "nerf" else 4
        net = [L(0, [("E_pos", 0, 60, 0, "g221", True)], "relu", "H1", "dA0")]
        for l in range(1, n):
            ins = [(f"H{l}", 0, 256, 60 if l == 5 else 0, "g422", True)]
            if l == 5:
                ins = [("E_pos", 0, 60, 0, "g221", False)] + ins
            net.append(L(l, ins, "relu", f"H{l + 1}", f"dA{l}"))
        if kind == "nerf":
            net += [L(8, [("H8", 0, 256, 0, "g422", True)], "linear", "G", "dA8"),
                    L(9, [("G", 0, 256, 0, "g412", True), ("E_dir", 0, 24, 256, "g111", False)], "relu", "H_d", "dA9"),
                    L(10, [("H8", 0, 256, 0, "thin", True)], "relu", (3, 4), ("heads", 3, 4)),
                    L(11, [("H_d", 0, 128, 0, "thin", True)], "sigmoid", (0, 3), ("heads", 0, 3))]
        else:
            net += [L(4, [("H4", 0, 256, 0, "g412", True), ("E_dir", 0, 24, 256, "g111", False)], "relu", "H_d", "dA4"),
                    L(5, [("H4", 0, 256, 0, "thin", True)], "relu", (3, 4), ("heads", 3, 4)),
                    L(6, [("H_d", 0, 128, 0, "thin", True)], "sigmoid", (0, 3), ("heads", 0, 3))]
        return net
    if kind == "siren_nerf":
        net = [L(0, [("xin", 0, 3, 0, "thin", True)], "sin", "X1", "dA0")]
        for l in range(1, 8):
            ins = [(f"X{l}", 0, 256, 3 if l == 5 else 0, "g422", True)]
            if l == 5:
                ins = [("xin", 0, 3, 0, "thin", False)] + ins
            net.append(L(l, ins, "sin", f"X{l + 1}", f"dA{l}"))
        return net + [L(8, [("X8", 0, 256, 0, "g422", True)], "linear", "G", "dA8"),
                      L(9, [("G", 0, 256, 0, "g412", True), ("xin", 3, 6, 256, "thin", False)], "sin", "X_d", "dA9"),
                      L(10, [("X8", 0, 256, 0, "thin", True)], "relu", (3, 4), ("heads", 3, 4)),
                      L(11, [("X_d", 0, 128, 0, "thin", True)], "sigmoid", (0, 3), ("heads", 0, 3))]
    if kind.startswith("film_siren_nerf"):
        # per image: the eight 256-wide FiLM layers are one GEMM launch, the K = 3 blocks one thin launch; heads: all images
        net = [L(0, [("xin", 0, 3, 0, "thin_img", True)], "film", "X0", "dU0", film=0)]
        for l in range(1, 8):
            net.append(L(l, [(f"X{l - 1}", 0, 256, 0, "g422_img", True)], "film", f"X{l}", f"dU{l}", film=l))
        ins = [("X7", 0, 256, 0, "g422_img", True)]
        if kind == "film_siren_nerf":
            ins.append(("xin", 3, 6, 256, "thin_img", False))
        return net + [L(9, ins, "film", "X8", "dU8", film=8),
                      L(8, [("X7", 0, 256, 0, "thin", True)], "relu", (3, 4), ("heads", 3, 4)),
                      L(10, [("X8", 0, 256, 0, "thin", True)], "sigmoid", (0, 3), ("heads", 0, 3))]
    if depth_of(kind) is not None:
        return film_depth_network(*depth_of(kind))
    raise KeyError(kind)


def film_depth_network(n: int, use_dir: bool) -> list:
    """FilmSirenNeRF(hidden_layers = n): parameter pairs in the order of include/mi_render.h - 0 input_layer, 1..n-1
    hidden_layers.0..n-2, n output_layer_sigma.0, n + 1 hidden_layer_rgb, n + 2 output_layer_rgb.0.  FiLM layer l (row l of
    the image's table) saves X_l and writes dU_l: l = 0 the input layer, 1..n-1 the hidden layers, n the rgb hidden layer.
    Per image the n 256-wide layers are one GEMM launch and the K = 3 blocks one thin launch; the two heads (sigma on
    X_{n-1}, rgb on X_n) run over all images."""
    L = Layer
    net = [L(0, [("xin", 0, 3, 0, "thin_img", True)], "film", "X0", "dU0", film=0)]
    for l in range(1, n):
        net.append(L(l, [(f"X{l - 1}", 0, 256, 0, "g422_img", True)], "film", f"X{l}", f"dU{l}", film=l))
    ins = [(f"X{n - 1}", 0, 256, 0, "g422_img", True)]
    if use_dir:
        ins.append(("xin", 3, 6, 256, "thin_img", False))
    return net + [L(n + 1, ins, "film", f"X{n}", f"dU{n}", film=n),
                  L(n, [(f"X{n - 1}", 0, 256, 0, "thin", True)], "relu", (3, 4), ("heads", 3, 4)),
                  L(n + 2, [(f"X{n}", 0, 256, 0, "thin", True)], "sigmoid", (0, 3), ("heads", 0, 3))]


# ---- the planner (BwdBatcher::slabs_for / slab_pts_for, csrc/field_bwd_dw.hip) ----------------------------------------
def slabs_for(P: int, njobs: int, per_cu: int = 1) -> int:
    s = min((256 * per_cu + njobs - 1) // njobs, 256 * per_cu)
    return max(1, min(s, (P + 255) // 256))


def slab_pts_for(P: int, slabs: int) -> int:
    return ((P + slabs - 1) // slabs + 31) // 32 * 32


def group_jobs(kind: str) -> dict:
    """{launch group: jobs in that launch}, counted from the network."""
    n = {}
    for lay in network(kind):
        for r in lay.ins:
            n[r.group] = n.get(r.group, 0) + 1
    return n


def group_plan(kind: str, group: str, P: int):
    """(slab_pts, n_slabs, cap) of a launch group over P points (per image for the *_img groups)."""
    jobs = group_jobs(kind)[group]
    per_cu = 4 if group.startswith("thin") else 1
    slabs = slabs_for(P, jobs, per_cu)
    pts = slab_pts_for(P, slabs)
    cap = min((256 * per_cu + jobs - 1) // jobs, 256 * per_cu)
    return pts, -(-P // pts), cap


def sum_length(kind: str, group: str, P: int) -> int:
    pts, n, _ = group_plan(kind, group, P)
    return pts + n


def film_scratch_plan(kind: str, ppg: int, n_img: int) -> int:
    """Floats of dW scratch the backward of a FiLM kind hands out (launch_field_backward; BwdBatcher::take rounds every
    request up to 256 floats): the larger of an image's pass - one [256][256] + [256] record per slab and 256-wide layer,
    one [4][256] record and 4 bias sums per slab and thin job - and the head pass over all images."""
    jobs, up = group_jobs(kind), lambda n: -(-n // 256) * 256

    def thin(group, P):
        n = group_plan(kind, group, P)[1]
        return jobs[group] * (up(1024 * n) + up(4 * n))

    image = jobs["g422_img"] * up(group_plan(kind, "g422_img", ppg)[1] * (256 * 256 + 256)) + thin("thin_img", ppg)
    return max(image, thin("thin", n_img * ppg))


def cap_thresholds(kind: str) -> list:
    """256 x cap of every launch group of the kind: past it, slabs grow beyond 256 points."""
    return sorted({256 * group_plan(kind, g, 1)[2] for g in group_jobs(kind)})


# ---- the gate ----------------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, bound):
    """(max |got - ref| / bound over the elements, flat index of that element): 0 where both are 0, inf where only the
    bound is, inf for a NaN."""
    got = torch.as_tensor(got)
    ref = torch.as_tensor(ref, device=got.device)
    bound = torch.as_tensor(bound, device=got.device, dtype=torch.float64)
    err = (got.double() - ref.double()).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    if not ratio.numel():
        return 0.0, -1
    return float(ratio.max()), int(ratio.argmax())


def record(case: str, stage: str, tensor: str, worst: float, where: int, elements: int, active: str,
           check: bool = False) -> bool:
    """One parity record: case, stage, tensor, the achieved ratio and the active bound.  Returns pass / fail."""
    rec = parity.record(case=case, stage=stage, qty=tensor, err_over_bound=worst, active=active, elements=int(elements),
                        worst_index=where, passed=bool(worst <= 1.0))
    if check:
        assert rec["passed"], rec
    return rec["passed"]


def gate(case: str, stage: str, tensor: str, got, ref, bound, active: str, check: bool = False) -> bool:
    """worst_ratio + record: one parity record per call, pass / fail."""
    worst, where = worst_ratio(got, ref, bound)
    return record(case, stage, tensor, worst, where, torch.as_tensor(got).numel(), active, check)


# ---- stage A: one forward layer from its saved input ------------------------------------------------------------------
def pre_activation(ins, b):
    """fp64 A = sum_i X_i W_i^T + b and its magnitude |X| |W|^T + |b|.  ins: [(X [P, k], weight columns [n, k])]."""
    acc = b.double().unsqueeze(0).expand(ins[0][0].shape[0], -1).clone()
    mag = b.double().abs().unsqueeze(0).expand_as(acc).clone()
    for X, Wc in ins:
        X, Wc = X.double(), Wc.double()
        acc += X @ Wc.T
        mag += X.abs() @ Wc.abs().T
    return acc, mag


def stage_a_ref(act: str, pre, mag, film=None, w0: float = W0):
    """(reference, bound) of a layer's saved output.  film = (gamma [n], beta [n]) of the FiLM layer's image."""
    if act == "relu":
        return torch.clamp(pre, min=0.0), C_A * U * mag
    if act == "linear":
        return pre, C_A * U * mag
    if act == "sigmoid":
        return torch.sigmoid(pre), 0.25 * C_A * U * mag + 2 * U
    u = pre
    if act == "film":
        g, be = film[0].double(), film[1].double()
        u = g * pre + be
        mag = g.abs() * mag + be.abs()
    # the pre-activation's own error and the rounding of w0 u, both through a slope <= w0; then the sine on the reduced angle
    return torch.sin(w0 * u), w0 * C_A * U * mag + 2 * U * (w0 * u).abs() + SIN_EPS + U


def sign_bit_ref(u, w0: float = W0):
    """(expected bit as float, bound): cos(w0 u) < 0, claimed only where |cos| > COS_BAND (bound inf elsewhere)."""
    c = torch.cos(w0 * u)
    return (c < 0).double(), torch.where(c.abs() > COS_BAND, 0.0, math.inf).to(c.dtype)


# ---- stage B: one chain layer from the kernel's dA of the layers it feeds -------------------------------------------
def chain_dx(consumers, starts=()):
    """fp64 dX = sum_c dA_c W_c and its magnitude.  consumers: [(dA_c [P, n_c], weight columns [n_c, k])] contracted on
    the MFMAs; starts: head terms the layer's accumulators START from (the sigma head's row times its gradient).  A start
    value rides through every one of the K / 2 MFMA steps of the layer and each step rounds relative to it, so its
    magnitude counts sqrt(K / 2) times (measured: 42 u |start| with a x50 sigma head, where |W|^T |dA| allowed 8 u)."""
    dx = mag = None
    K = sum(dA.shape[1] for dA, _ in consumers)
    for i, (dA, Wc) in enumerate(list(consumers) + list(starts)):
        dA, Wc = dA.double(), Wc.double()
        t, m = dA @ Wc, dA.abs() @ Wc.abs()
        if i >= len(consumers):
            m = m * math.sqrt(K / 2)
        dx, mag = (t, m) if dx is None else (dx + t, mag + m)
    return dx, mag


def stage_b_ref(act: str, dx, mag, saved=None, w0: float = W0):
    """(reference, bound) of a layer's dA given dX of its output.  saved: the switch units (bool, ReLU) or the saved X
    rows (sin / FiLM: the derivative factor is rebuilt from them, as the chain does)."""
    if act == "linear":
        return dx, C_B * U * mag
    if act == "relu":
        on = saved.double()
        return on * dx, C_B * U * on * mag
    c = dsin_from_saved(saved, w0)
    x = saved.double()
    # the fp32 factor sqrt(fl(w0^2 - w0^2 X^2)) loses w0^2 X^2 u to cancellation where |cos| is small
    dc = w0 * w0 * x * x / torch.clamp(c.abs(), min=w0 * math.sqrt(U)) + 3 * c.abs()
    return c * dx, C_B * U * (c.abs() * mag + dx.abs() * dc)


def heads_ref(raw, g_raw):
    """(reference, bound) of the head pre-activation gradients: g o (1 - o) for rgb (sigmoid), g [o > 0] for sigma.  The
    kernel rounds three times (g o, 1 - o, the product), so 4 u |ref| is a bound, not a calibrated constant; sigma's is
    exact."""
    o, g = raw.double(), g_raw.double()
    ref = torch.cat([g[:, :3] * o[:, :3] * (1 - o[:, :3]), torch.where(o[:, 3:] > 0, g[:, 3:], 0.0)], 1)
    return ref, 4 * U * ref.abs()


# ---- stage C: a weight-gradient job from the kernel's own dA and X -----------------------------------------------------
def stage_c_ref(dA, X, L: int):
    """(dW = dA^T X, its bound, db = sum dA, its bound) in fp64; L = the longest chain of fp32 additions per element."""
    dA, X = dA.double(), X.double()
    s = C_C * U * math.sqrt(L)
    return dA.T @ X, s * (dA.abs().T @ X.abs()), dA.sum(0), s * dA.abs().sum(0)


def active_c(L: int) -> str:
    return f"{C_C:g} u sqrt(L) |dA|^T|X|, L={L}"

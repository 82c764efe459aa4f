"""CPU: the compositing gates of test_gpu_composite_stages.py (tests/composite_gates.py) have teeth.

Over the whole case matrix the fp32 oracle passes every gate with the committed constants, its worst ratios are
re-measured and must reproduce those constants, and a numpy fp32 model of the kernels' own order passes too
(`kernel_model`: G-lane inclusive product scan in fp64 with T rounded to fp32 per sample and carried across the passes,
per-lane sums and the butterfly, the reverse scan of the affine maps (f_k, G_k alpha_k) in fp32 with its carry,
dalpha * delta * e).  Each mistake a kernel could make, as a mutation of that model, fails at least one gate.

What the gate cannot resolve is measured, not hidden: `SHARE_100` is, per regime at S = 192, the share of the nonzero
elements whose exact value is at least 100 bounds large - the elements on which a 1 % error is certain to be seen.

The failing gates below are self-checks, not findings: each test leaves parity.RECORDS as it found it (`_no_records`)."""
import functools

import numpy as np
import pytest
import torch

import composite_gates as CG
from oracle import parity

F = np.float32


@pytest.fixture(autouse=True)
def _no_records():
    n = len(parity.RECORDS)
    yield
    del parity.RECORDS[n:]


# ---- the kernels' own order in numpy fp32 ------------------------------------------------------------------------------
def kernel_model(case, mut=""):
    """composite_kernel + composite_bwd_kernel (csrc/render_stages.hip) on a make_case dict, with one mistake `mut`."""
    raw, z, rd = (case[k].numpy() for k in ("raw", "z", "rd"))
    g_rgb, g_d, g_a, g_w = (case[k].numpy() for k in ("g_rgb", "g_depth", "g_acc", "g_w"))
    n, S, _ = raw.shape
    G = 16 if S <= 16 else 32 if S <= 32 else 64
    passes = -(-S // G)
    nrm = np.sqrt((rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2])
    if mut == "|d| = 1":
        nrm = np.ones_like(nrm)
    delta = np.full((n, S), 1e10, F)
    delta[:, :-1] = z[:, 1:] - z[:, :-1]
    if mut == "last delta = z spacing" and S > 1:
        delta[:, -1] = delta[:, -2]
    delta = delta * nrm[:, None]
    e = torch.exp(torch.from_numpy(-raw[..., 3] * delta)).numpy()     # numpy's own fp32 exp is up to 2.5 ulp off
    alpha = F(1) - e
    f = F(1) - alpha if mut == "no 1e-10" else (F(1) - alpha) + F(1e-10)
    pad = passes * G - S
    lanes = lambda a, fill: np.concatenate([a, np.full((n, pad), fill, a.dtype)], 1).reshape(n, passes, G)  # noqa: E731
    # sweep 1: T_k = fp32(T * exclusive fp64 product inside the pass), T carried in fp64
    fl = lanes(f, F(1)).astype(np.float64)
    Tk = np.empty((n, passes, G), F)
    T = np.ones(n)
    for p in range(passes):
        incl = np.cumprod(fl[:, p], 1)
        excl = np.concatenate([np.ones((n, 1)), incl[:, :-1]], 1)
        Tk[:, p] = (T[:, None] * excl).astype(F)
        if not (mut == "no T carry" and p == 0):
            T = T * incl[:, -1]
    Tk = Tk.reshape(n, -1)[:, :S]
    w = alpha * Tk

    def ray_sum(term):                                   # per lane over the passes, then the xor butterfly; lane 0
        t = lanes(term, F(0))
        s = np.zeros((n, G), F)
        for p in range(passes):
            s = s + t[:, p]
        o = G // 2
        while o:
            s = s + s[:, np.arange(G) ^ o]
            o //= 2
        return s[:, 0]

    sa = ray_sum(w)
    rgb = np.stack([ray_sum(w * raw[..., c]) + (F(1) - sa) for c in range(3)], 1)
    depth = ray_sum(w * z)
    # sweep 2: R by the reverse scan of the affine maps, carried between the passes
    Gk = g_rgb[:, None, 0] * (raw[..., 0] - F(1)) + g_rgb[:, None, 1] * (raw[..., 1] - F(1)) \
        + g_rgb[:, None, 2] * (raw[..., 2] - F(1)) + g_d[:, None] * z + g_a[:, None]
    if mut != "g_w ignored":
        Gk = Gk + g_w
    Ml, Al = lanes(f, F(1)), lanes(Gk * alpha, F(0))
    Snext = np.empty((n, passes, G), F)
    carry = np.zeros(n, F)
    for p in range(passes - 1, -1, -1):
        M, A = Ml[:, p].copy(), Al[:, p].copy()
        o = 1
        while o < G:
            A[:, :G - o], M[:, :G - o] = A[:, :G - o] + M[:, :G - o] * A[:, o:], M[:, :G - o] * M[:, o:]
            o *= 2
        Rk = A + M * carry[:, None]
        Snext[:, p] = Rk if mut == "S_k = R_k" else np.concatenate([Rk[:, 1:], carry[:, None]], 1)
        if mut != "no R carry":
            carry = Rk[:, 0]
    dalpha = Tk * (Gk - Snext.reshape(n, -1)[:, :S])
    dsig = dalpha * delta if mut == "no (1 - alpha)" else dalpha * delta * e
    dcol = g_rgb[:, None, :] * w[..., None]
    out = dict(rgb=rgb, depth=depth, acc=sa, weights=w, dsigma=dsig, dcolour=dcol)
    if mut == "row n-1 in n-2":
        for q in ("weights", "dsigma", "dcolour"):
            out[q][n - 2] = out[q][n - 1]
    return {q: torch.from_numpy(np.ascontiguousarray(a)) for q, a in out.items()}


@functools.lru_cache(maxsize=None)
def _case(S, regime):
    c = CG.make_case(S, CG.N_MATRIX, regime, seed=S)
    args = [c[k] for k in ("raw", "z", "rd", "g_rgb", "g_depth", "g_acc", "g_w")]
    return c, CG.reference(*args), CG.oracle32(*args)


def _gate(name, got, ref, oracle):
    """(quantities that failed, {quantity: err / e})."""
    recs = CG.gate(name, "host", got, ref, oracle)
    return sorted(q for q, r in recs.items() if not r["passed"]), {q: r["err_over_bound"] * CG.C[q] for q, r in recs.items()}


def _failed(name, got, ref, oracle):
    return _gate(name, got, ref, oracle)[0]


# ---- the oracle and the model pass; the constants are the oracle's ---------------------------------------------------
def test_oracle_and_kernel_model_pass_the_matrix_and_the_constants_are_the_oracles():
    worst = dict.fromkeys(CG.QUANTITIES, 0.0)
    worst_model = dict.fromkeys(CG.QUANTITIES, 0.0)
    for name, S, regime in CG.matrix_cases():
        c, ref, oracle = _case(S, regime)
        for who, got, into in (("oracle", oracle, worst), ("kernel model", kernel_model(c), worst_model)):
            bad, ratios = _gate(f"host {who} {name}", got, ref, oracle)
            assert bad == [], (who, name, bad, ratios)
            for q, v in ratios.items():
                into[q] = max(into[q], v)
    print("fp32 oracle, worst err / e over the matrix:", {q: round(v, 3) for q, v in worst.items()})
    print("kernel model, worst err / e over the matrix:", {q: round(v, 3) for q, v in worst_model.items()})
    for q in CG.QUANTITIES:
        assert abs(CG.constant_for(q, worst[q]) - CG.C[q]) <= 0.1 * CG.C[q], (q, worst[q], CG.C[q])


def test_tail_sizes_pass_for_oracle_and_model():
    """The ray-count tails and the sample counts of the GPU file's tail test (one S per G)."""
    for S in (13, 24, 100):
        for n in (1, 3, 4, 5, 7, 8, 9, 15, 16, 17):
            c = CG.make_case(S, n, "plain", seed=1000 * S + n)
            args = [c[k] for k in ("raw", "z", "rd", "g_rgb", "g_depth", "g_acc", "g_w")]
            ref, oracle = CG.reference(*args), CG.oracle32(*args)
            assert _failed(f"host tail {n}x{S}", oracle, ref, oracle) == []
            assert _failed(f"host tail {n}x{S} model", kernel_model(c), ref, oracle) == []


# ---- every mistake fails a gate ----------------------------------------------------------------------------------------
MODEL_MUTATIONS = ["no T carry", "no R carry", "S_k = R_k", "g_w ignored", "|d| = 1", "last delta = z spacing",
                   "no (1 - alpha)", "row n-1 in n-2"]


@pytest.mark.parametrize("regime", ["plain", "sharp"])
@pytest.mark.parametrize("mut", MODEL_MUTATIONS)
def test_model_mutation_fails_a_gate(mut, regime):
    c, ref, oracle = _case(192, regime)
    assert _failed("host faithful", kernel_model(c), ref, oracle) == []
    bad = _failed(f"host {mut} {regime}", kernel_model(c, mut), ref, oracle)
    print(mut, regime, "fails", bad)
    assert bad, (mut, regime)


@pytest.mark.parametrize("S", [64, 192])
def test_missing_floor_fails_a_gate_behind_a_wall(S):
    """f without + 1e-10: behind an opaque sample T is 1e-10 T_k, not 0."""
    c, ref, oracle = _case(S, "wall")
    bad = _failed("host no 1e-10 wall", kernel_model(c, "no 1e-10"), ref, oracle)
    print("no 1e-10, wall, S =", S, "fails", bad)
    assert bad


def _interior_conditioning(ref):
    """|ref| / (C e) of d/dsigma over the interior samples (k < S - 1); 0 where the value is zero as an fp32 number (below
    2^-126: half the sharp regime's interior, which no fp32 pipeline resolves and the tiny terms allow to be 0)."""
    val, bound = ref["dsigma"]
    r = (val.abs() / (CG.C["dsigma"] * bound))[:, :-1]
    return torch.where(val[:, :-1].abs() < CG.TINY, torch.zeros_like(r), r)


@pytest.mark.parametrize("regime", ["plain", "sharp"])
def test_scaled_and_zeroed_interior_elements_fail_the_gate(regime):
    c, ref, oracle = _case(192, regime)
    good = kernel_model(c)
    cond = _interior_conditioning(ref)
    nz = cond[cond > 0]
    median = float(nz.median())
    # one element at the median conditioning of the nonzero interior, 1e-3 relative
    i = int((torch.where(cond > 0, (cond - median).abs(), torch.full_like(cond, float("inf")))).argmin())
    ray, k = divmod(i, cond.shape[1])
    got = {q: t.clone() for q, t in good.items()}
    got["dsigma"][ray, k] *= F(1 + 1e-3)
    print(regime, "median |ref| / bound of the nonzero interior d/dsigma:", median, "max:", float(cond.max()))
    assert _failed(f"host median element x (1 + 1e-3) {regime}", got, ref, oracle) == ["dsigma"]
    # the best-conditioned interior element, 1e-5 relative
    ray, k = divmod(int(cond.argmax()), cond.shape[1])
    got = {q: t.clone() for q, t in good.items()}
    got["dsigma"][ray, k] *= F(1 + 1e-5)
    assert _failed(f"host best element x (1 + 1e-5) {regime}", got, ref, oracle) == ["dsigma"]
    # right on each ray's last sample, zero everywhere else
    got = {q: t.clone() for q, t in good.items()}
    got["dsigma"][:, :-1] = 0
    got["dcolour"][:, :-1] = 0
    assert _failed(f"host interior zeroed {regime}", got, ref, oracle) == ["dcolour", "dsigma"]


# ---- what the gate resolves ------------------------------------------------------------------------------------------
# Share of the nonzero elements with |ref| >= 100 e at S = 192, n = 257, measured with the committed bound.
SHARE_100 = {
    ("plain", "rgb"): 1.0000, ("plain", "depth"): 1.0000, ("plain", "acc"): 1.0000,
    ("plain", "weights"): 0.9912, ("plain", "dsigma"): 0.9734, ("plain", "dcolour"): 0.9911,
    ("sharp", "rgb"): 1.0000, ("sharp", "depth"): 1.0000, ("sharp", "acc"): 1.0000,
    ("sharp", "weights"): 0.4121, ("sharp", "dsigma"): 0.3678, ("sharp", "dcolour"): 0.4114,
    ("wall", "rgb"): 1.0000, ("wall", "depth"): 1.0000, ("wall", "acc"): 1.0000,
    ("wall", "weights"): 0.1928, ("wall", "dsigma"): 0.1769, ("wall", "dcolour"): 0.1924,
    ("empty", "rgb"): 1.0000, ("empty", "depth"): 0.0000, ("empty", "acc"): 0.0000,
    ("empty", "weights"): 0.0000, ("empty", "dsigma"): 0.9984, ("empty", "dcolour"): 0.0000,
    ("thin", "rgb"): 1.0000, ("thin", "depth"): 0.9183, ("thin", "acc"): 0.9261,
    ("thin", "weights"): 0.7084, ("thin", "dsigma"): 0.9927, ("thin", "dcolour"): 0.7084,
    ("ties", "rgb"): 1.0000, ("ties", "depth"): 1.0000, ("ties", "acc"): 1.0000,
    ("ties", "weights"): 0.9868, ("ties", "dsigma"): 0.9652, ("ties", "dcolour"): 0.9868,
    ("last", "rgb"): 1.0000, ("last", "depth"): 1.0000, ("last", "acc"): 1.0000,
    ("last", "weights"): 0.9911, ("last", "dsigma"): 0.9735, ("last", "dcolour"): 0.9910,
}


@pytest.mark.parametrize("regime", CG.REGIMES)
def test_share_of_well_resolved_elements_does_not_drop(regime):
    _c, ref, _oracle = _case(192, regime)
    for q in CG.QUANTITIES:
        val, bound = ref[q]
        nz = val != 0
        share = float((val.abs() >= 100 * CG.C[q] * bound)[nz].double().mean()) if bool(nz.any()) else 0.0
        print(f'    ("{regime}", "{q}"): {share:.4f},')
        assert share >= 0.9 * SHARE_100[(regime, q)], (regime, q, share)

"""GPU: mi_composite_bwd_rays per element against float64.

What mi_composite_bwd leaves out of raw_to_outputs' backward (nerf/render.py:91-93): dists = delta_z |d|, so
g_d = dL/d|d| d / |d| with dL/d|d| = sum_k dL/dalpha_k sigma_k delta_z_k exp(-sigma_k delta_z_k |d|).

Reference: oracle.render_ref.composite's autograd with respect to rays_d in float64.  Bound, per element, from the terms of
composite_gates.reference (the first-order fp32 bound e_dsig of d/dsigma_k = dL/dalpha_k delta_k e_k, delta_k = delta_z_k |d|):
since dL/d|d| = sum_k d/dsigma_k sigma_k / |d| exactly,

    e_n  = sum_k (e_dsig_k + 6 u |dsig_k|) sigma_k / |d|  +  2 u sqrt(S) sum_k |dsig_k| sigma_k / |d|
    e_gd = (e_n + 4 u |dL/d|d||) |d_j| / |d| + tiny

6 u: the kernel forms ((dL/dalpha e) sigma) delta_z, three products where d/dsigma has (delta_z |d|) e, and |d| once more;
2 u sqrt(S): the sum over the samples, as for acc in composite_gates; 4 u: the product with d_j, the division and |d|'s own
rounding.  C = 1: nothing is fitted to the kernel's result; the fp32 oracle's ratio to the same bound is recorded beside it."""
import math

import pytest
import torch

import composite_gates as CG
from oracle import parity, render_ref as R

pytestmark = pytest.mark.gpu

N = 70


def dev():
    return torch.device("cuda", 0)


def oracle_g_rd(c, dtype):
    rd = c["rd"].to(dtype).clone().requires_grad_(True)
    outs = R.composite(c["raw"].to(dtype), c["z"].to(dtype), rd)
    loss = sum((o * c[k].to(dtype)).sum() for o, k in zip(outs, ("g_rgb", "g_depth", "g_acc", "g_w")))
    loss.backward()
    return rd.grad


def bound(c):
    ref = CG.reference(*[c[k] for k in ("raw", "z", "rd", "g_rgb", "g_depth", "g_acc", "g_w")])
    dsig, edsig = ref["dsigma"]
    S = dsig.shape[1]
    sig, rd = c["raw"][..., 3].double(), c["rd"].double()
    nrm = rd.norm(dim=-1, keepdim=True)
    mag = (dsig.abs() * sig / nrm).sum(1)
    e_n = ((edsig + 6 * CG.U * dsig.abs()) * sig / nrm).sum(1) + 2 * CG.U * math.sqrt(S) * mag
    g_n = (dsig * sig / nrm).sum(1)
    return (e_n + 4 * CG.U * g_n.abs())[:, None] * rd.abs() / nrm + CG.TINY


def hip(c, accumulate=0, into=None):
    from mirender import _lib
    lib = _lib.load()
    d = {k: v.to(dev()).contiguous() for k, v in c.items()}
    rays = torch.stack([torch.zeros_like(d["rd"]), d["rd"]], 1).contiguous()
    n, S = d["z"].shape
    out = torch.full((n, 2, 3), float("nan"), device=dev()) if into is None else into
    _lib.check(lib.mi_composite_bwd_rays(n, S, _lib.ptr(d["raw"]), _lib.ptr(d["z"]), _lib.ptr(rays), _lib.ptr(d["g_rgb"]),
                                         _lib.ptr(d["g_depth"]), _lib.ptr(d["g_acc"]), _lib.ptr(d["g_w"]), accumulate,
                                         _lib.ptr(out), _lib.stream_ptr(dev())), "mi_composite_bwd_rays")
    return out


def special_case(S, regime, seed):
    """70 rays of composite_gates' generator (|d| over two decades: non-unit), plus: ray 0 with sigma = 0 everywhere, ray 1
    whose transmittance saturates at its first sample."""
    c = CG.make_case(S, N, regime, seed)
    c["raw"][0, :, 3] = 0.0
    c["raw"][1, 0, 3] = 1e4
    return c


@pytest.mark.parametrize("regime", ["plain", "sharp", "last"])
@pytest.mark.parametrize("S", [2, 36, 192])
def test_g_rays_vs_fp64(S, regime):
    c = special_case(S, regime, seed=31 * S)
    got = hip(c).cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(got[:, 0], torch.zeros(N, 3)), "compositing sends nothing to the origins"
    assert torch.equal(got[0, 1], torch.zeros(3)), "sigma = 0 on the whole ray: exactly zero"
    ref64, ref32 = oracle_g_rd(c, torch.float64), oracle_g_rd(c, torch.float32)
    assert torch.isfinite(ref32).all() and torch.equal(ref32[0], torch.zeros(3))
    b = bound(c)
    worst, where = CG.worst_ratio(got[:, 1], ref64, b)
    o32, _ = CG.worst_ratio(ref32, ref64, b)
    rec = parity.record(case=f"composite_bwd_rays {N}x{S} {regime}", stage="composite stage", qty="g_rays_d",
                        err_over_bound=float(f"{worst:.6g}"), oracle32_err_over_bound=float(f"{o32:.6g}"),
                        active="1 x fp32 bound, per element", elements=int(ref64.numel()), worst_index=where,
                        passed=bool(worst <= 1.0))
    print(rec)
    assert rec["passed"], rec


@pytest.mark.parametrize("S", [2, 36, 192])
def test_accumulate_and_partial_cotangents(S):
    c = special_case(S, "plain", seed=17 * S)
    plain = hip(c)
    base = torch.randn(N, 2, 3, device=dev())
    added = hip(c, accumulate=1, into=base.clone())
    assert torch.equal(added[:, 0], base[:, 0])
    assert torch.equal(added[:, 1], base[:, 1] + plain[:, 1])
    # absent cotangents are zeros
    c0 = dict(c, g_depth=torch.zeros_like(c["g_depth"]), g_w=torch.zeros_like(c["g_w"]))
    from mirender import autograd as A
    d = {k: v.to(dev()) for k, v in c.items()}
    rays = torch.stack([torch.zeros_like(d["rd"]), d["rd"]], 1).contiguous()
    g = torch.zeros(N, 2, 3, device=dev())
    A._composite_bwd_rays(d["raw"], d["z"], rays, d["g_rgb"], None, d["g_acc"], g)
    assert torch.equal(g, hip(c0))

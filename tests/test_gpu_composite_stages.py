"""GPU: compositing forward and backward per element against float64 (tests/composite_gates.py).

mi_composite (mirender.ops.composite) and mi_composite_bwd (autograd._composite_bwd) through the C ABI; every output
element - rgb, depth, acc, every weight, every d/dsigma and d/dcolour, the last sample included, nothing masked - within
the first-order fp32 bound of the formula around its float64 value, with the fp32 oracle's own ratio recorded beside it:

  matrix          every G dispatch edge and pass-count edge and the production sample counts, by seven regimes (saturated
                  alpha, opaque walls, empty and thin volumes, repeated depths, the last sample on / off), |d| over two decades
  tails           ray counts that do not fill a block, one S per G: a lane that read its clamped neighbour's row is seen
  training sizes  raw from a real field evaluation (the x50 NeRF on camera rays, coarse depths and the merged fine depths
                  of sample_fine), reference evaluated in float64 on the device
  cotangents      each of g_rgb, g_depth, g_acc, g_w alone and all together; None equals explicit zeros bit for bit
  autograd        autograd.composite (behind render_core.raw_to_outputs) hands out the gated g_raw bit for bit

composite_weights_kernel has no stage entry of its own; test_gpu_sigma_only.py pins it bit for bit to composite_kernel."""
import numpy as np
import pytest
import torch

import composite_gates as CG
from oracle import render_ref as R, synth

pytestmark = pytest.mark.gpu

ARGS = ("raw", "z", "rd", "g_rgb", "g_depth", "g_acc", "g_w")
COTS = ARGS[3:]


def dev():
    return torch.device("cuda", 0)


def _rays(rd):
    return torch.stack([torch.zeros_like(rd), rd], 1).contiguous()


def hip(c, cots=COTS):
    """Forward and backward through the C ABI on the case's tensors (moved to the device); the cotangents not in `cots`
    are passed as None."""
    from mirender import autograd as A, ops
    d = {k: v.to(dev()) for k, v in c.items()}
    rays = _rays(d["rd"])
    rgb, depth, acc, w = ops.composite(d["raw"], d["z"], rays)
    g_raw = A._composite_bwd(d["raw"], d["z"], rays, *[d[k] if k in cots else None for k in COTS])
    return dict(rgb=rgb, depth=depth, acc=acc, weights=w, **CG.split_g_raw(g_raw)), g_raw


def check(name, c, cots=COTS, on_device=False, quantities=CG.QUANTITIES):
    """Gate the HIP results of case c; the reference on the CPU, or in float64 on the device."""
    got, g_raw = hip(c, cots)
    used = {k: (c[k] if k in ARGS[:3] or k in cots else None) for k in ARGS}
    oracle = CG.oracle32(*[used[k] for k in ARGS])
    if on_device:
        ref = CG.reference(*[None if used[k] is None else used[k].to(dev()) for k in ARGS])
    else:
        ref = CG.reference(*[used[k] for k in ARGS])
        got = {q: t.cpu() for q, t in got.items()}
    recs = CG.gate(name, "composite stage", {q: got[q] for q in quantities}, ref, oracle)
    for q, r in recs.items():
        print(f"{name} {q}: err/bound {r['err_over_bound']:.3g} (fp32 oracle {r['oracle32_err_over_bound']:.3g}) at "
              f"{r['worst_index']}")
    bad = [r for r in recs.values() if not r["passed"]]
    assert not bad, bad
    return g_raw


@pytest.mark.parametrize("name,S,regime", CG.matrix_cases(), ids=[c[0].replace(" ", "-") for c in CG.matrix_cases()])
def test_matrix_vs_fp64(name, S, regime):
    check(f"composite matrix {name}", CG.make_case(S, CG.N_MATRIX, regime, seed=S))


@pytest.mark.parametrize("S", [13, 24, 100])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 7, 8, 9, 15, 16, 17])
def test_ray_count_tails_vs_fp64(n, S):
    check(f"composite tail {n}x{S}", CG.make_case(S, n, "plain", seed=1000 * S + n))


_FIELD = []


def _field():
    from mirender import fields
    if not _FIELD:
        _FIELD.append(fields.as_packed_field(fields.field_from_state_dict(synth.state_dict("nerf", sharp=True), dev())))
    return _FIELD[0]


# rays x (coarse + fine): the nerf step's fine and coarse composites, a pi_GAN slice at 12 + 24 and 24 + 48, a 256 x 256 frame
@pytest.mark.parametrize("n,nc,nf", [(1024, 64, 128), (1024, 64, 0), (4096, 12, 24), (4096, 24, 48), (65536, 64, 128)])
def test_training_and_frame_sizes_vs_fp64(n, nc, nf):
    from mirender import ops
    pf = _field()
    rays = torch.from_numpy(R.rays_from_camera(256, 256, 355.0, synth.pose_degrees(4.0, 30.0, -30.0))[:n]).to(dev())
    with torch.no_grad():
        z = ops.sample_coarse(n, 2.0, 6.0, nc, dev(), seed=nc + nf)
        raw = ops.field_eval_rays(pf, rays, z)
        if nf:
            w = ops.composite(raw, z, rays)[3]
            z = ops.sample_fine(z, w, 2.0, 6.0, nf)
            raw = ops.field_eval_rays(pf, rays, z)
    g = torch.Generator().manual_seed(n + nc)
    c = dict(raw=raw.cpu(), z=z.cpu(), rd=rays[:, 1].cpu())
    c.update({k: torch.randn(s, generator=g) for k, s in zip(COTS, ((n, 3), (n,), (n,), (n, nc + nf)))})
    sig = c["raw"][..., 3]
    print(f"{n} x {nc}+{nf}: sigma max {float(sig.max()):.3g}, zero on {float((sig == 0).double().mean()):.3f}, "
          f"repeated depths {int((c['z'][:, 1:] == c['z'][:, :-1]).sum())}")
    check(f"composite field raw {n} x {nc}+{nf}", c, on_device=True)


@pytest.mark.parametrize("S", [36, 192])
@pytest.mark.parametrize("cots", [("g_rgb",), ("g_depth",), ("g_acc",), ("g_w",), COTS], ids=lambda c: "+".join(c))
def test_cotangent_subsets_vs_fp64(cots, S):
    from mirender import autograd as A
    c = CG.make_case(S, CG.N_MATRIX, "plain", seed=7 * S)
    g_none = check(f"composite bwd S={S} cotangents {'+'.join(cots)}", c, cots, quantities=("dsigma", "dcolour"))
    d = {k: v.to(dev()) for k, v in c.items()}
    zeros = [d[k] if k in cots else torch.zeros_like(d[k]) for k in COTS]
    assert torch.equal(A._composite_bwd(d["raw"], d["z"], _rays(d["rd"]), *zeros), g_none)


@pytest.mark.parametrize("S", [13, 36, 192])
def test_autograd_wrapper_hands_out_the_gated_g_raw(S):
    from mirender import autograd as A
    c = CG.make_case(S, CG.N_MATRIX, "plain", seed=11 * S)
    d = {k: v.to(dev()) for k, v in c.items()}
    rays = _rays(d["rd"])
    raw = d["raw"].clone().requires_grad_(True)
    outs = A.composite(raw, d["z"], rays)
    torch.autograd.backward(outs, [d[k] for k in COTS])
    assert torch.equal(raw.grad, A._composite_bwd(d["raw"], d["z"], rays, *[d[k] for k in COTS]))
    assert np.isfinite(raw.grad.cpu().numpy()).all()

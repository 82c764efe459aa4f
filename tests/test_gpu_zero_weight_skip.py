"""GPU: mi_render_rays skips field evaluations whose compositing weight is exactly zero - and no output bit moves.

With rgb_c = NULL and two different fields the coarse pass runs front to back in windows of WINDOW samples
(kCoarseWindow, csrc/render_path.hip): after each window the resumable weights composite drops every ray whose running
transmittance has reached zero, and the field is not evaluated behind that point.  Those samples' weights are exactly 0
whatever the field says there, so rgb_f / depth_f / acc_f and depth_c / acc_c must be the SAME BITS as the unskipped
computation.  The yardstick is that computation assembled from the staged calls, which take no such shortcut:

    mi_sample_coarse -> mi_field_eval_rays -> mi_composite -> mi_sample_fine -> mi_field_eval_rays -> mi_composite

No case passes vacuously: each one first counts, in the staged reference alone, what it claims to exercise - the rays
whose transmittance (the reference's float32 exclusive product, from its own sigma) is 0.0 at a window boundary, i.e. the
rays the windowed pass terminates - and asserts that count before it compares anything.

Seeds were picked with the CPU oracle (oracle/render_ref.py) on the rays below, 257 rays, Nc = 64, t_rand seed 9,
`sharp` sigma head; rays terminated at a window boundary / first dead sample (5th, 50th, 95th percentile):
    nerf       seed 34: 209 of 257, 39 / 50 / 60      seed 12:  47 of 257      seed 7: 257 of 257, 13 / 16 / 18
    tiny_nerf  seed 25: 176 of 257, 41 / 51 / 64      seed 7: 257 of 257, 19 / 24 / 31
    siren_nerf seed 16: 100 of 257, 29 / 64 / 64
and every plain head (sharp=False) terminates none.  nerf seed 7 has 66 rays whose first dead sample is the last of a
window of 8 and 60 whose first dead sample is the first of the next.

The fine pass is not windowed and its colour branch is not deferred (DESIGN.md 4.3 says why): the fine-field case below
pins that a fine field with many empty (sigma == 0) points still gives the staged bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import render_ref as R, synth  # noqa: E402

WINDOW = 8          # kCoarseWindow of csrc/render_path.hip
NEAR, FAR = 2.0, 6.0


def dev():
    return torch.device("cuda", 0)


def _packed(kind, seed, sharp, sigma_bias=0.0):
    from mirender import fields
    sd = synth.state_dict(kind, seed=seed, sharp=sharp, bias_jitter=0.05)
    if sigma_bias:
        sd["output_layer_sigma.bias"] = sd["output_layer_sigma.bias"] + sigma_bias
    return fields.as_packed_field(fields.field_from_state_dict(sd, dev()))


def _rays(n):
    """n rays spread over a 40x40 view of the volume (n = 1: a ray through its middle)."""
    r = torch.from_numpy(R.rays_from_camera(40, 40, 1.3875 * 40, synth.pose_degrees(4.0, 20.0, -30.0)))
    idx = (torch.arange(n) * 1600 // n + 20) % 1600 if n > 1 else torch.tensor([820])
    return r[idx].contiguous().to(dev())


_REF = {}


def _staged(key, pf_c, pf_f, rays, nc, nf, tr, seed):
    """The unskipped computation, stage by stage; computed once per key and shared."""
    if key not in _REF:
        from mirender import ops
        n = rays.shape[0]
        with torch.no_grad():
            z_c = ops.sample_coarse(n, NEAR, FAR, nc, dev(), tr, seed=seed)
            raw_c = ops.field_eval_rays(pf_c, rays, z_c)
            _, depth_c, acc_c, w_c = ops.composite(raw_c, z_c, rays)
            z_f = ops.sample_fine(z_c, w_c, NEAR, FAR, nf)
            raw_f = ops.field_eval_rays(pf_f, rays, z_f)
            rgb_f, depth_f, acc_f, _ = ops.composite(raw_f, z_f, rays, want_weights=False)
        _REF[key] = dict(z_c=z_c, raw_c=raw_c, w_c=w_c, raw_f=raw_f, outs=(depth_c, acc_c, rgb_f, depth_f, acc_f))
    return _REF[key]


def _first_dead(ref, rays):
    """Per ray: the first sample whose transmittance - raw_to_outputs' exclusive cumprod of 1 - alpha + 1e-10, running
    product in float64 and rounded to float32 per sample as ATen's CPU cumprod does - is 0.0 (Nc if there is none).  From
    the staged reference's sigma, on the CPU."""
    z, sigma, rd = ref["z_c"].cpu(), ref["raw_c"][..., 3].cpu(), rays[:, 1].cpu()
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1) * torch.norm(rd, dim=-1, keepdim=True)
    f = (1.0 - (1.0 - torch.exp(-sigma * delta))) + 1e-10
    t = torch.cumprod(f.double(), -1).float()
    dead = torch.cat([torch.ones_like(t[:, :1]), t[:, :-1]], -1) == 0
    nc = z.shape[1]
    return torch.where(dead.any(-1), dead.float().argmax(-1), torch.full((z.shape[0],), nc))


def _terminated(first_dead, nc):
    """Rays the windowed pass drops: dead at some window boundary b (a multiple of WINDOW below Nc)."""
    last_boundary = (nc - 1) // WINDOW * WINDOW
    return int(((first_dead <= last_boundary) & (last_boundary > 0)).sum())


def _render(pf_c, pf_f, rays, nc, nf, tr, seed):
    """mi_render_rays with rgb_c = NULL, depth_c and acc_c asked for."""
    from mirender import _lib, ops
    lib = _lib.load()
    n = rays.shape[0]
    ws_bytes = lib.mi_render_workspace_bytes(n, nc, nf)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
    outs = [torch.full(s, float("nan"), device=dev()) for s in ((n,), (n,), (n, 3), (n,), (n,))]
    zl, ul = ops.linspace_table(NEAR, FAR, nc, dev()), ops.linspace_table(0.0, 1.0, nf, dev())
    rc = lib.mi_render_rays(pf_c.kind, _lib.ptr(pf_c.refresh()), pf_f.kind, _lib.ptr(pf_f.refresh()), None, _lib.ptr(rays),
                            1, n, NEAR, FAR, nc, nf, _lib.ptr(zl), _lib.ptr(ul), _lib.ptr(tr), seed, 0, None,
                            *[_lib.ptr(o) for o in outs], _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dev()))
    assert rc == 0, lib.mi_last_error()
    return outs


def _assert_same_bits(got, ref):
    for name, a, b in zip(("depth_c", "acc_c", "rgb_f", "depth_f", "acc_f"), got, ref["outs"]):
        assert torch.equal(a, b), name


def _jitter(jitter, n, nc):
    return synth.t_rand(n, nc, seed=9).to(dev()) if jitter == "t_rand" else None


# (a) mixed: between 10 % and 90 % of the rays terminate, in the reference alone
@pytest.mark.parametrize("kind,seed", [("nerf", 34), ("nerf", 12), ("tiny_nerf", 25), ("siren_nerf", 16)])
def test_mixed_terminated_and_live_rays(kind, seed):
    n, nc, nf = 257, 64, 128
    pf_c, pf_f = _packed(kind, seed, True), _packed(kind, 6, "medium")
    rays, tr = _rays(n), _jitter("t_rand", n, nc)
    ref = _staged(("mixed", kind, seed), pf_c, pf_f, rays, nc, nf, tr, 0)
    term = _terminated(_first_dead(ref, rays), nc)
    assert 0.1 * n <= term <= 0.9 * n, term
    _assert_same_bits(_render(pf_c, pf_f, rays, nc, nf, tr, 0), ref)


# sizes: partial tiles, partial ray groups of a windowed tile, Nc below / at / behind a window boundary, both jitters.
# Nearly every ray of these fields dies between samples 13 and 32 (CPU oracle: all 33 / the one ray of the nerf and tiny_nerf
# cases, 32 of 33 and 247 of 257 of the siren_nerf ones), so windows behind the first see a shrinking live list.
@pytest.mark.parametrize("kind,seed,n,nc,nf,jitter", [
    ("nerf", 7, 1, 64, 128, "seed"), ("nerf", 7, 33, 65, 3, "t_rand"), ("nerf", 7, 257, 64, 3, "seed"),
    ("tiny_nerf", 7, 33, 64, 128, "t_rand"), ("tiny_nerf", 7, 257, 65, 128, "seed"), ("tiny_nerf", 7, 1, 65, 3, "t_rand"),
    ("siren_nerf", 5, 33, 64, 3, "seed"), ("siren_nerf", 5, 257, 65, 128, "t_rand")])
def test_sizes_with_terminated_rays(kind, seed, n, nc, nf, jitter):
    pf_c, pf_f = _packed(kind, seed, True), _packed(kind, 6, "medium")
    rays, tr = _rays(n), _jitter(jitter, n, nc)
    ref = _staged(("sizes", kind, n, nc, nf, jitter), pf_c, pf_f, rays, nc, nf, tr, 1234)
    assert _terminated(_first_dead(ref, rays), nc) >= 1
    _assert_same_bits(_render(pf_c, pf_f, rays, nc, nf, tr, 1234), ref)


# (b) rays whose transmittance first rounds to zero at the last sample of a window, and at the first sample of the next
def test_rays_that_die_on_either_side_of_a_window_boundary():
    n0, nc, nf = 257, 64, 3
    pf_c, pf_f = _packed("nerf", 7, True), _packed("nerf", 6, "medium")
    rays0, tr0 = _rays(n0), _jitter("t_rand", n0, nc)
    first = _first_dead(_staged(("boundary pool",), pf_c, pf_f, rays0, nc, nf, tr0, 0), rays0)
    last_of_window = ((first < nc) & (first % WINDOW == WINDOW - 1)).nonzero().flatten()
    first_of_next = ((first < nc) & (first % WINDOW == 0)).nonzero().flatten()
    assert len(last_of_window) >= 1 and len(first_of_next) >= 1, (len(last_of_window), len(first_of_next))
    pick = torch.cat([last_of_window, first_of_next]).to(dev())
    rays, tr = rays0[pick].contiguous(), tr0[pick].contiguous()
    ref = _staged(("boundary picked",), pf_c, pf_f, rays, nc, nf, tr, 0)
    again = _first_dead(ref, rays)                      # t_rand travels with the ray: the same ray dies at the same sample
    assert torch.equal(again, first[pick.cpu()])
    _assert_same_bits(_render(pf_c, pf_f, rays, nc, nf, tr, 0), ref)


# (c) the plain head: no ray dies, every window is full (Nc = 9 and 17: a last window of one sample, the delta = 1e10 one)
@pytest.mark.parametrize("kind,n,nc,nf,jitter", [("nerf", 257, 64, 128, "seed"), ("tiny_nerf", 33, 9, 3, "t_rand"),
                                                 ("siren_nerf", 33, 17, 3, "seed"), ("nerf", 1, 5, 3, "t_rand")])
def test_no_ray_dies(kind, n, nc, nf, jitter):
    pf_c, pf_f = _packed(kind, 5, False), _packed(kind, 6, "medium")
    rays, tr = _rays(n), _jitter(jitter, n, nc)
    ref = _staged(("plain", kind, n, nc, nf, jitter), pf_c, pf_f, rays, nc, nf, tr, 77)
    first = _first_dead(ref, rays)
    assert int((first < nc).sum()) == 0
    _assert_same_bits(_render(pf_c, pf_f, rays, nc, nf, tr, 77), ref)


# (d) a density so high that every ray is dead behind the first window: every later window is empty
@pytest.mark.parametrize("kind,n,nc,nf", [("nerf", 257, 64, 128), ("tiny_nerf", 33, 9, 3), ("siren_nerf", 33, 65, 3)])
def test_every_ray_dies_in_the_first_window(kind, n, nc, nf):
    pf_c, pf_f = _packed(kind, 5, True, sigma_bias=3000.0), _packed(kind, 6, "medium")
    rays, tr = _rays(n), _jitter("t_rand", n, nc)
    ref = _staged(("dense", kind, n, nc, nf), pf_c, pf_f, rays, nc, nf, tr, 0)
    first = _first_dead(ref, rays)
    assert int((first <= WINDOW).sum()) == n                 # dead at the first boundary
    _assert_same_bits(_render(pf_c, pf_f, rays, nc, nf, tr, 0), ref)


# (e) a fine field with many empty points behind a coarse pass that terminates rays
def test_fine_field_with_empty_points():
    n, nc, nf = 257, 64, 128
    pf_c, pf_f = _packed("nerf", 34, True), _packed("nerf", 3, True)
    rays, tr = _rays(n), _jitter("t_rand", n, nc)
    ref = _staged(("empty fine",), pf_c, pf_f, rays, nc, nf, tr, 0)
    empty = int((ref["raw_f"][..., 3] == 0).sum())
    assert 0.1 * n * (nc + nf) <= empty <= 0.9 * n * (nc + nf), empty
    assert _terminated(_first_dead(ref, rays), nc) >= 0.1 * n
    _assert_same_bits(_render(pf_c, pf_f, rays, nc, nf, tr, 0), ref)

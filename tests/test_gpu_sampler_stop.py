"""GPU: with no coarse output asked for, mi_render_rays stops a coarse ray as soon as the fine sampler cannot see its
later weights - and no fine output bit moves.

With rgb_c = depth_c = acc_c = NULL and two different fields, the windowed coarse pass (csrc/render_path.hip) produces w_c alone,
and sample_fine reads a weight only as w + 1e-5f.  The resumable weights composite then drops a ray at the first window
boundary whose fp64 running product is <= 2^-42 (kStopBelowPdfEps, csrc/launchers.h carries the proof; the float32 side
of it is tests/test_sampler_stop_host.py): every later weight is below 2^-41 and vanishes in that sum.  The weights
behind the stop are written as zeros, which are NOT the unskipped weights - but z_fine, and with it rgb_f / depth_f /
acc_f, must be the SAME BITS as the unskipped computation.  A call that asks for depth_c or acc_c keeps the exact
2^-151 rule (tests/test_gpu_zero_weight_skip.py), since those sums add every weight.

The yardstick is the staged computation of tests/test_gpu_zero_weight_skip.py, which takes no shortcut:

    mi_sample_coarse -> mi_field_eval_rays -> mi_composite -> mi_sample_fine -> mi_field_eval_rays -> mi_composite

No case passes vacuously: each first asserts, on the staged reference alone (its sigma, on the CPU, the running product
in fp64), what it claims to exercise.

Seeds were picked with the CPU oracle (oracle/render_ref.py) on the rays below, 257 rays, Nc = 64, t_rand seed 9, `sharp`
sigma head, windows of 8.  Rays that cross 2^-42 at a boundary in front of a window / two or more windows from the end /
of those, rays that never cross 2^-151 / rays the 2^-151 rule drops:
    nerf seed 36: 183 / 140 / 183 / 0        nerf seed 15: 129 / 72 / 129 / 0        (most sharp seeds: all 257, or none)
and seed 36 has 32 rays whose product first falls to <= 2^-42 at the last sample of a window and 32 at the first of the
next.  The plain heads (sharp=False, seed 5) keep every product above 9e-4; sigma_bias = 3000 leaves at most 1.3e-74 in
front of sample 8."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import render_ref as R, synth  # noqa: E402

WINDOW = 8          # kCoarseWindow of csrc/render_path.hip
STOP = 2.0 ** -42   # kStopBelowPdfEps of csrc/launchers.h
ZERO = 2.0 ** -151  # kStopZeroWeight
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


def _jitter(jitter, n, nc):
    return synth.t_rand(n, nc, seed=9).to(dev()) if jitter == "t_rand" else None


_REF = {}


def _staged(key, pf_c, pf_f, rays, nc, nf, tr, seed):
    """The unskipped computation, stage by stage; computed once per key, shared and left unchanged."""
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
        _REF[key] = dict(z_c=z_c, raw_c=raw_c, w_c=w_c, depth_c=depth_c, acc_c=acc_c, fine=(rgb_f, depth_f, acc_f))
    return _REF[key]


def _first_below(ref, rays, threshold):
    """Per ray: the first sample k whose product in front of it - raw_to_outputs' factors 1 - alpha + 1e-10 in float32,
    their running product in float64 - is <= threshold (Nc if there is none).  From the staged reference's sigma, on the
    CPU."""
    z, sigma, rd = ref["z_c"].cpu(), ref["raw_c"][..., 3].cpu(), rays[:, 1].cpu()
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1) * torch.norm(rd, dim=-1, keepdim=True)
    f = (1.0 - (1.0 - torch.exp(-sigma * delta))) + 1e-10
    t = torch.cumprod(f.double(), -1)
    below = torch.cat([torch.ones_like(t[:, :1]), t[:, :-1]], -1) <= threshold
    nc = z.shape[1]
    return torch.where(below.any(-1), below.float().argmax(-1), torch.full((z.shape[0],), nc))


def _last_boundary(nc):
    return (nc - 1) // WINDOW * WINDOW          # the boundary in front of the last window (0: one window, nothing to stop)


def _stopped(first, nc):
    """Rays the windowed pass drops under a threshold: at or below it at some window boundary with a window behind it."""
    return (first <= _last_boundary(nc)) & (_last_boundary(nc) > 0)


class _Call:
    """mi_render_rays with rgb_c = NULL into fixed buffers (so that a graph can replay it); `want`: which of depth_c / acc_c
    the call asks for.  extra: the workspace also holds the deferred colour branch's buffer, as render_image's does."""

    def __init__(self, pf_c, pf_f, rays, nc, nf, tr, seed, want=(), extra=False):
        from mirender import _lib, ops
        self.lib, self.n, self.nc, self.nf, self.seed = _lib.load(), rays.shape[0], nc, nf, seed
        self.pf_c, self.pf_f, self.rays, self.tr = pf_c, pf_f, rays, tr
        n = self.n
        self.bytes = self.lib.mi_render_workspace_bytes(n, nc, nf)
        if extra:
            self.bytes += self.lib.mi_render_deferred_colour_extra_bytes(n, nc, nf)
        self.ws = torch.empty(self.bytes, dtype=torch.uint8, device=dev())
        self.coarse = {k: torch.full((n,), float("nan"), device=dev()) for k in want}
        self.outs = [torch.full(s, float("nan"), device=dev()) for s in ((n, 3), (n,), (n,))]
        self.zl, self.ul = ops.linspace_table(NEAR, FAR, nc, dev()), ops.linspace_table(0.0, 1.0, nf, dev())
        self.pc, self.pf = _lib.ptr(pf_c.refresh()), _lib.ptr(pf_f.refresh())

    def __call__(self):
        from mirender import _lib
        c = [_lib.ptr(self.coarse[k]) if k in self.coarse else None for k in ("depth_c", "acc_c")]
        rc = self.lib.mi_render_rays(self.pf_c.kind, self.pc, self.pf_f.kind, self.pf, None, _lib.ptr(self.rays), 1, self.n,
                                     NEAR, FAR, self.nc, self.nf, _lib.ptr(self.zl), _lib.ptr(self.ul),
                                     None if self.tr is None else _lib.ptr(self.tr), self.seed, 0, None, *c,
                                     *[_lib.ptr(o) for o in self.outs], _lib.ptr(self.ws), self.bytes, _lib.stream_ptr(dev()))
        assert rc == 0, self.lib.mi_last_error()
        return self.outs


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_fine_bits(got, ref):
    for name, a, b in zip(("rgb_f", "depth_f", "acc_f"), got, ref["fine"]):
        assert torch.equal(_bits(a), _bits(b)), name


def _mixed_case(seed):
    n, nc, nf = 257, 64, 128
    pf_c, pf_f = _packed("nerf", seed, True), _packed("nerf", 6, "medium")
    rays, tr = _rays(n), _jitter("t_rand", n, nc)
    return pf_c, pf_f, rays, nc, nf, tr, _staged(("mixed", seed), pf_c, pf_f, rays, nc, nf, tr, 0)


def _assert_mixed(ref, rays, nc):
    """10 - 90 % of the rays stop at a boundary in front of a window - and as many two or more windows from the end - and
    one of them at least is a ray the 2^-151 rule would have carried to the end."""
    n = rays.shape[0]
    first, first_zero = _first_below(ref, rays, STOP), _first_below(ref, rays, ZERO)
    stopped = _stopped(first, nc)
    early = first <= _last_boundary(nc) - WINDOW
    assert 0.1 * n <= int(stopped.sum()) <= 0.9 * n, int(stopped.sum())
    assert 0.1 * n <= int(early.sum()) <= 0.9 * n, int(early.sum())
    assert int((stopped & (first_zero == nc)).sum()) >= 1
    return stopped, first


# (a) mixed: between 10 % and 90 % of the rays stop early, in the reference alone; with and without the deferred colour buffer
@pytest.mark.parametrize("seed,extra", [(36, False), (15, True)])
def test_mixed_stopped_and_live_rays(seed, extra):
    pf_c, pf_f, rays, nc, nf, tr, ref = _mixed_case(seed)
    _assert_mixed(ref, rays, nc)
    _assert_fine_bits(_Call(pf_c, pf_f, rays, nc, nf, tr, 0, extra=extra)(), ref)


# (b) rays whose product first falls to <= 2^-42 at the last sample of a window, and at the first sample of the next
def test_rays_that_stop_on_either_side_of_a_window_boundary():
    pf_c, pf_f, rays0, nc, nf, tr0, pool = _mixed_case(36)
    first = _first_below(pool, rays0, STOP)
    last_of_window = ((first < nc) & (first % WINDOW == WINDOW - 1)).nonzero().flatten()
    first_of_next = ((first < nc) & (first % WINDOW == 0)).nonzero().flatten()
    assert len(last_of_window) >= 1 and len(first_of_next) >= 1, (len(last_of_window), len(first_of_next))
    pick = torch.cat([last_of_window, first_of_next]).to(dev())
    rays, tr = rays0[pick].contiguous(), tr0[pick].contiguous()
    ref = _staged(("boundary picked",), pf_c, pf_f, rays, nc, nf, tr, 0)
    again = _first_below(ref, rays, STOP)               # t_rand travels with the ray: the same ray stops at the same sample
    assert torch.equal(again, first[pick.cpu()])
    _assert_fine_bits(_Call(pf_c, pf_f, rays, nc, nf, tr, 0)(), ref)


# (c) the plain head: no ray reaches 2^-42, every window is full (Nc = 9 and 17: a last window of one sample; Nc = 5: one pass)
@pytest.mark.parametrize("kind,n,nc,nf,jitter", [("nerf", 257, 64, 128, "seed"), ("tiny_nerf", 33, 9, 3, "t_rand"),
                                                 ("siren_nerf", 33, 17, 3, "seed"), ("nerf", 1, 5, 3, "t_rand")])
def test_no_ray_stops(kind, n, nc, nf, jitter):
    pf_c, pf_f = _packed(kind, 5, False), _packed(kind, 6, "medium")
    rays, tr = _rays(n), _jitter(jitter, n, nc)
    ref = _staged(("plain", kind, n, nc, nf, jitter), pf_c, pf_f, rays, nc, nf, tr, 77)
    assert int((_first_below(ref, rays, STOP) < nc).sum()) == 0
    _assert_fine_bits(_Call(pf_c, pf_f, rays, nc, nf, tr, 77)(), ref)


# (d) a density so high that every ray stops at the first boundary: every later window is empty
@pytest.mark.parametrize("kind,n,nc,nf", [("nerf", 257, 64, 128), ("tiny_nerf", 33, 9, 3), ("siren_nerf", 33, 65, 3)])
def test_every_ray_stops_at_the_first_boundary(kind, n, nc, nf):
    pf_c, pf_f = _packed(kind, 5, True, sigma_bias=3000.0), _packed(kind, 6, "medium")
    rays, tr = _rays(n), _jitter("t_rand", n, nc)
    ref = _staged(("dense", kind, n, nc, nf), pf_c, pf_f, rays, nc, nf, tr, 0)
    assert int((_first_below(ref, rays, STOP) <= WINDOW).sum()) == n
    _assert_fine_bits(_Call(pf_c, pf_f, rays, nc, nf, tr, 0)(), ref)


# (e) a call that asks for one coarse sum keeps the 2^-151 rule: that sum has the staged bits, although the rays that the
# 2^-42 rule would stop carry weight behind their stop
@pytest.mark.parametrize("want", ["acc_c", "depth_c"])
def test_a_coarse_sum_keeps_the_exact_rule(want):
    pf_c, pf_f, rays, nc, nf, tr, ref = _mixed_case(36)
    stopped, first = _assert_mixed(ref, rays, nc)
    boundary = (first + WINDOW - 1) // WINDOW * WINDOW                               # where the 2^-42 rule would stop the ray
    behind = torch.arange(nc)[None, :] >= boundary[:, None]
    tail = (ref["w_c"].cpu() * behind).sum(-1)[stopped]
    assert int((tail > 0).sum()) >= 0.1 * rays.shape[0]                              # weight that the sum must not lose
    call = _Call(pf_c, pf_f, rays, nc, nf, tr, 0, want=(want,))
    _assert_fine_bits(call(), ref)
    assert torch.equal(_bits(call.coarse[want]), _bits(ref[want])), want


# (f) the call captured into a graph and replayed twice
def test_graph_replay():
    pf_c, pf_f, rays, nc, nf, tr, ref = _mixed_case(36)
    _assert_mixed(ref, rays, nc)
    call = _Call(pf_c, pf_f, rays, nc, nf, tr, 0, extra=True)
    call()                                                    # warm-up outside the capture (kernel attributes)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        for o in call.outs:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _assert_fine_bits(call.outs, ref)

"""GPU: corners of the drop-in boundary: DataParallel replicas, stale-weight detection, models that
move between devices, per-device kernel attributes."""
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import render_ref as R, synth  # noqa: E402


def dev(i=0):
    return torch.device("cuda", i)


def _rays(n=256, d=None):
    return torch.from_numpy(R.rays_from_camera(24, 24, 33.3, synth.pose_degrees(4.0, 25.0, -30.0))[100:100 + n]).to(d or dev())


def test_data_parallel_replica_is_recognised_and_trains():
    """torch.nn.DataParallel (pi_GAN/train.py:50) calls forward on replicas whose parameters are plain broadcast
    tensors: named_parameters() is empty there.  The replica must take the fused path (not fall through to the
    generic one) and gradients must flow back to the original module's parameters."""
    from mirender import fields, pigan, render_core
    m = fields.FilmSirenNeRF().to(dev())
    m.load_state_dict(synth.state_dict("film_siren_nerf", seed=40, sharp="medium"))
    (rep,) = torch.nn.parallel.replicate(m, [0])
    assert getattr(rep, "_is_replica", False) and not dict(rep.named_parameters())
    pf = fields.as_packed_field(rep)
    assert pf is not None and pf.kind == fields.FILM_SIREN_NERF
    film = synth.film_params(1, seed=3).to(dev())
    rays = torch.from_numpy(R.rays_from_camera(12, 12, 57.0, pigan.camera_pos_to_transform_matrix(1, 0.1, -0.1))).to(dev())
    tr = synth.t_rand(144, 6, seed=1).to(dev())
    out_r = render_core.render_rays(rays, 0.5, 1.5, rep, rep, 6, 12, t_rand=tr, film=film)
    out_m = render_core.render_rays(rays, 0.5, 1.5, m, m, 6, 12, t_rand=tr, film=film)
    assert out_r[3].requires_grad and torch.equal(out_r[3].detach(), out_m[3].detach())
    out_r[3].square().mean().backward()
    g_rep = [p.grad.clone() for p in m.parameters()]          # through Broadcast.backward onto the originals
    for p in m.parameters():
        p.grad = None
    out_m[3].square().mean().backward()
    for a, p in zip(g_rep, m.parameters()):
        assert a is not None and torch.equal(a, p.grad)
    # a whole Generator under DataParallel on this one device (device_ids=[0] calls the module itself)
    torch.manual_seed(0)
    gen = pigan.Generator(16, 12, near=0.5, far=1.5, fov=12, coarse_samples=6, fine_samples=12).to(dev())
    dp = torch.nn.DataParallel(gen, device_ids=[0])
    z = torch.randn(2, 16, device=dev())
    img = dp(z, [0.1, 0.2], [0.0, 0.1], tr.repeat(2, 1))
    assert tuple(img.shape) == (2, 3, 12, 12) and img.requires_grad


def test_weights_changed_between_forward_and_backward_raise():
    from mirender import fields, render_core
    m = fields.TinyNeRF().to(dev())
    m.load_state_dict(synth.state_dict("tiny_nerf", 3, "medium", 0.05))
    rays, tr = _rays(), synth.t_rand(256, 8, 1).to(dev())
    out = render_core.render_rays(rays, 2.0, 6.0, m, m, 8, 8, t_rand=tr)
    with torch.no_grad():
        m.layers_pos[1].weight.mul_(1.01)                       # e.g. an optimiser step before backward
    with pytest.raises(RuntimeError, match="modified in place"):
        out[3].sum().backward()
    # writes through .data are invisible to version counters: invalidate() is the documented way to repack
    with torch.no_grad():
        before = m(torch.rand(64, 6, device=dev()) * 0 + 0.3)
    m.output_layer_rgb.bias.data[:] = 2.0                        # the reference's own idiom, pi_GAN/modules.py:57-58
    fields.as_packed_field(m).invalidate()
    with torch.no_grad():
        after = m(torch.rand(64, 6, device=dev()) * 0 + 0.3)
    assert float((after[:, :3] - before[:, :3]).abs().min()) > 1e-3


def test_model_moved_to_cpu_and_back_repacks():
    from mirender import _lib, fields
    m = fields.NeRF().to(dev())
    m.load_state_dict(synth.state_dict("nerf", 5, "medium", 0.05))
    x = torch.rand(100, 6, device=dev()) * 2 - 1
    with torch.no_grad():
        a = m(x)
    m.cpu()
    with pytest.raises(_lib.MiRenderError):
        m(x)                                                     # no CPU path: a clear error, not a stale render
    m.to(dev())
    with torch.no_grad():
        b = m(x)
    assert torch.equal(a, b)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs in one process (DataParallel's layout)")
def test_two_devices_two_threads_one_process():
    """One process driving two GPUs from two threads (pi_GAN/train.py:50): the 148 KiB dynamic-LDS attribute of the
    MLP kernels is per device (csrc/mi_host.h:PerDeviceOnce); both devices must render, train and agree."""
    from mirender import fields, render_core
    sd = synth.state_dict("nerf", 5, "medium", 0.05)
    outs, errs = [None, None], []

    def work(i):
        try:
            with torch.cuda.device(i):
                m = fields.NeRF().to(dev(i))
                m.load_state_dict(sd)
                rays, tr = _rays(256, dev(i)), synth.t_rand(256, 8, 1).to(dev(i))
                o = render_core.render_rays(rays, 2.0, 6.0, m, m, 8, 16, t_rand=tr)
                (o[3].square().mean() + o[0].square().mean()).backward()
                torch.cuda.synchronize(i)
                outs[i] = [t.detach().cpu() for t in o] + [p.grad.cpu() for p in m.parameters()]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for a, b in zip(*outs):
        assert np.array_equal(a.numpy(), b.numpy())


def test_w0_is_the_modules_own_whichever_path_renders_it(monkeypatch):
    """pi_GAN/modules.py:11,73: `FilmSirenNeRF(w_0=...)` is a constructor argument.  An object with the FiLM layout whose
    layers name their w_0 like the reference's runs the fused kernels WITH that w_0 (round 4: it travels in the packed
    stream; round 3 refused anything but 30); one whose layers do not say (the same number under another attribute name) is
    driven through the generic path - its own forward between the sampling / compositing kernels.  Either way the image
    must match the oracle evaluated with that w_0."""
    from mirender import fields, render_core
    from oracle import fields as ofields, parity

    class FilmSiren(torch.nn.Module):                       # the reference layer's arithmetic (modules.py:22-25)
        def __init__(self, i, o, w_0, named):
            super().__init__()
            setattr(self, "w_0" if named else "omega", w_0)
            self.weight = torch.nn.Parameter(torch.zeros(o, i))
            self.bias = torch.nn.Parameter(torch.zeros(o))

        def forward(self, x, gamma, beta):
            w = self.w_0 if hasattr(self, "w_0") else self.omega
            return torch.sin(w * (gamma * torch.nn.functional.linear(x, self.weight, self.bias) + beta))

    class LookAlike(torch.nn.Module):                       # modules.py:70-118
        def __init__(self, w_0, named):
            super().__init__()
            self.film_params = None
            self.input_layer = FilmSiren(3, 256, w_0, named)
            self.hidden_layers = torch.nn.ModuleList([FilmSiren(256, 256, w_0, named) for _ in range(7)])
            self.output_layer_sigma = torch.nn.Sequential(torch.nn.Linear(256, 1), torch.nn.ReLU())
            self.hidden_layer_rgb = FilmSiren(259, 256, w_0, named)
            self.output_layer_rgb = torch.nn.Sequential(torch.nn.Linear(256, 3), torch.nn.Sigmoid())

        def forward(self, x):
            fp = self.film_params
            pos, d = x[:, :3], x[:, 3:]
            h = self.input_layer(pos, *fp[0])
            for i, lay in enumerate(self.hidden_layers):
                h = lay(h, *fp[i + 1])
            sigma = self.output_layer_sigma(h)
            h = self.hidden_layer_rgb(torch.cat([h, d], -1), *fp[8])
            return torch.cat([self.output_layer_rgb(h), sigma], -1)

    sd = synth.state_dict("film_siren_nerf", seed=44, sharp="medium")
    film = synth.film_params(1, seed=6)[0]
    rays = torch.from_numpy(R.rays_from_camera(16, 16, 76.0, synth.pose_radians(1.0, 0.15, -0.1)))
    tr = synth.t_rand(256, 8, seed=2)
    for w_0, named in ((25.0, False), (25.0, True), (30.0, True), (17.0, True)):
        m = LookAlike(w_0, named).to(dev())
        m.load_state_dict(sd)
        m.film_params = [torch.chunk(film[i].to(dev()), 2) for i in range(9)]
        assert fields.detect_kind(dict(m.named_parameters())) == fields.FILM_SIREN_NERF
        pf = fields.as_packed_field(m)
        assert (pf is None) == (not named) and (pf is None or pf.w_0 == w_0)   # named: the fused kernels, with its w_0
        monkeypatch.setattr(ofields, "W0", w_0)
        fo = ofields.make_field("film_siren_nerf", sd, film)
        with torch.no_grad():
            ref = R.render_rays(rays, 0.5, 1.5, fo, fo, 8, 16, tr)
            got = render_core.render_rays(rays.to(dev()), 0.5, 1.5, m, m, 8, 16, t_rand=tr.to(dev()))
        case = f"FiLM look-alike w_0={w_0:g} 8+16 ({'generic path' if pf is None else 'fused kernel'})"
        parity.gate(case, "coarse", "rgb", got[0], ref.rgb_c)
        parity.gate(case, "coarse", "acc", got[2], ref.acc_c)
        parity.gate(case, "coarse", "depth", got[1], ref.depth_c, tol=parity.DEPTH_TOL)
        d = (got[3].cpu() - ref.rgb_f).abs().max(-1).values
        frac = float((d > 1e-4).float().mean())
        ref25 = ref if w_0 == 25.0 else ref25
        parity.record(case=case, stage="end-to-end fine", qty="rgb", err_vs_oracle32=float(d.max()), tol=1e-4,
                      frac_rays_over=frac, active="distribution", passed=frac <= 0.03)
        assert frac <= 0.03, (w_0, float(d.max()), frac)
    # and the frequencies really differ: a kernel that ignored the module's w_0 (round 3's hard-coded 30) would have painted
    # the w_0 = 30 image for the w_0 = 25 module
    monkeypatch.setattr(ofields, "W0", 30.0)
    fo30 = ofields.make_field("film_siren_nerf", sd, film)
    with torch.no_grad():
        ref30 = R.render_rays(rays, 0.5, 1.5, fo30, fo30, 8, 16, tr)
    assert float((ref30.rgb_c - ref25.rgb_c).abs().max()) > 1e-2


@pytest.mark.parametrize("w_0", [1.0, 7.5, 30.0, 60.0, 120.0])
def test_fused_film_field_follows_w0_over_two_decades(w_0):
    """The FiLM kernels read w_0 from the packed stream (pi_GAN/modules.py:11,73): free-standing points through
    `fields.FilmSirenNeRF(w_0=w)` against the oracle evaluated with that w_0, weights as the reference initialises them FOR
    that w_0 (modules.py:27-31 divides the hidden layers' range by w_0).  A larger w_0 amplifies every fp32 pipeline's rounding
    (t = fl(w_0 u) grows), so the gate is the one the x50 heads use: no further from the fp64 evaluation than 2x the fp32
    oracle's own distance, or the flat 1e-4 where that holds."""
    from mirender import fields
    from oracle import fields as ofields, parity
    torch.manual_seed(int(w_0 * 10))
    m = fields.FilmSirenNeRF(w_0=w_0).to(dev())
    assert fields.as_packed_field(m).w_0 == w_0
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    rng = np.random.Generator(np.random.PCG64(3))
    M = 2048
    x = torch.from_numpy(np.concatenate([rng.uniform(-1, 1, size=(M, 3)), rng.normal(size=(M, 3))], -1).astype(np.float32))
    x[:, 3:] /= x[:, 3:].norm(dim=-1, keepdim=True)
    film = synth.film_params(1, seed=21)
    m.set_film_params(film[0].to(dev()))
    with torch.no_grad():
        got = m(x.to(dev())).cpu()
    old = ofields.W0
    try:
        ofields.W0 = w_0
        ref32 = ofields.make_field("film_siren_nerf", sd, film[0])(x)
        ref64 = ofields.make_field("film_siren_nerf", {k: v.double() for k, v in sd.items()}, film[0].double())(x.double())
    finally:
        ofields.W0 = old
    case = f"fused FilmSirenNeRF(w_0={w_0:g}), {M} free-standing points, reference initialisation for that w_0"
    parity.gate(case, "field", "rgb", got[:, :3], ref32[:, :3], ref64[:, :3], factor=parity.FP64_FACTOR_INTERMEDIATE)
    parity.gate(case, "field", "sigma", got[:, 3], ref32[:, 3], ref64[:, 3], factor=parity.FP64_FACTOR_INTERMEDIATE)
    assert float(got[:, :3].std()) > 1e-3                                  # the field is not constant: w_0 really acts

"""GPU: the fused FiLM kernels at hidden_layers other than 8 (the MI_FIELD_FILM_DEPTH kinds) - forward and training against
the reference-pinned fixtures (tests/golden/make_golden_film_depth.py) and the fp64 restatement of the depth-L network
(tests/film_depth_util.py), depth 8 through the macro against kinds 2 / 3 bit for bit, the C-ABI training pair, an image cut
into parts, FusedAdam's scatter refresh, the Generator and a reference-shaped look-alike.  Gates: oracle/parity.py's own."""
import ctypes

import numpy as np
import pytest
import torch

import film_depth_util as U
from oracle import parity

pytestmark = pytest.mark.gpu

OUT_SHAPES = lambda n: ((n, 3), (n,), (n,), (n, 3), (n,), (n,))  # noqa: E731


def dev():
    return torch.device("cuda", 0)


def module(L, use_dir, sd):
    from mirender import fields
    m = fields.FilmSirenNeRF(hidden_layers=L, use_dir=use_dir)
    m.load_state_dict(sd)
    return m.to(dev())


def tag(L, use_dir):
    return f"film_depth_L{L}_{'dir' if use_dir else 'nodir'}"


# ---- forward -------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("L", U.DEPTHS)
@pytest.mark.parametrize("use_dir", [True, False])
def test_forward_against_reference_and_fp64(golden, L, use_dir):
    from mirender import fields, ops
    g = golden(tag(L, use_dir))
    film2 = U.film_rows(2, L, seed=100 + L)
    x = torch.from_numpy(g["x"])
    for head in ("plain", "medium"):
        sd = U.state_dict(L, use_dir, seed=200 + L, head=head)
        assert U.digest(sd, film2) == str(g[f"digest.{head}"])
        pf = fields.as_packed_field(module(L, use_dir, sd))
        assert pf is not None and pf.kind == U.kind_of(L, use_dir)
        # the fixture's 257 points under FiLM row set 1: one group, not a multiple of the 128-point tile
        out = fields.eval_points(pf, x.to(dev()), film2[1:2].to(dev())).cpu()
        with torch.no_grad():
            o64 = U.forward(U.to64(sd), film2[1].double(), x.double())
        parity.gate(f"{tag(L, use_dir)}.{head}", "eval_points (fixture)", "rgb", out[:, :3], g[f"out.{head}"][:, :3], o64[:, :3])
        parity.gate(f"{tag(L, use_dir)}.{head}", "eval_points (fixture)", "sigma", out[:, 3], g[f"out.{head}"][:, 3], o64[:, 3],
                    factor=parity.FP64_FACTOR_INTERMEDIATE)
        # 3 groups with different FiLM rows, 171 points each (513 = 3 x 171: partial tiles in every group)
        film3 = U.film_rows(3, L, seed=600 + L)
        x3 = U.sample_points(513, seed=700 + L)
        out3 = fields.eval_points(pf, x3.to(dev()), film3.to(dev())).cpu()
        with torch.no_grad():
            r32 = torch.cat([U.forward(sd, film3[k], x3[171 * k:171 * (k + 1)]) for k in range(3)])
            r64 = torch.cat([U.forward(U.to64(sd), film3[k].double(), x3[171 * k:171 * (k + 1)].double()) for k in range(3)])
        parity.gate(f"{tag(L, use_dir)}.{head}", "eval_points (3 groups)", "rgb", out3[:, :3], r32[:, :3], r64[:, :3])
        parity.gate(f"{tag(L, use_dir)}.{head}", "eval_points (3 groups)", "sigma", out3[:, 3], r32[:, 3], r64[:, 3],
                    factor=parity.FP64_FACTOR_INTERMEDIATE)
        # eval_rays: 3 groups of 19 rays x 9 samples = 171 points per group; the same points through eval_points
        rng = np.random.Generator(np.random.PCG64(800 + L))
        rays = torch.from_numpy(rng.normal(size=(57, 2, 3)).astype(np.float32)).to(dev())
        z = torch.from_numpy(np.sort(rng.uniform(0.5, 1.5, size=(57, 9)).astype(np.float32), -1)).to(dev())
        raw = ops.field_eval_rays(pf, rays, z, film3.to(dev()))
        pts = rays[:, None, 0] + rays[:, None, 1] * z[..., None]
        view = (rays[:, 1] / torch.norm(rays[:, 1], dim=-1, keepdim=True))[:, None].expand_as(pts)
        xr = torch.cat([pts, view], -1).reshape(-1, 6).cpu()
        with torch.no_grad():
            r32 = torch.cat([U.forward(sd, film3[k], xr[171 * k:171 * (k + 1)]) for k in range(3)])
            r64 = torch.cat([U.forward(U.to64(sd), film3[k].double(), xr[171 * k:171 * (k + 1)].double()) for k in range(3)])
        parity.gate(f"{tag(L, use_dir)}.{head}", "eval_rays (3 groups)", "rgb", raw.reshape(-1, 4)[:, :3].cpu(), r32[:, :3], r64[:, :3])
        parity.gate(f"{tag(L, use_dir)}.{head}", "eval_rays (3 groups)", "sigma", raw.reshape(-1, 4)[:, 3].cpu(), r32[:, 3], r64[:, 3],
                    factor=parity.FP64_FACTOR_INTERMEDIATE)


# ---- the training call of the fixtures -----------------------------------------------------------------------------
class Call:
    """The gradient fixture's render_rays call on the device: one shared depth-L field, 64 rays in 2 groups, 8+16."""

    def __init__(self, L, use_dir, kind=None):
        from mirender import fields, ops
        self.L, self.use_dir = L, use_dir
        self.sd = U.state_dict(L, use_dir, seed=400 + L, head="medium")
        self.model = module(L, use_dir, self.sd)
        self.pf = fields.as_packed_field(self.model)
        if kind is not None:                       # the same parameters under another id of the same network
            self.pf = fields.PackedField(kind, self.pf.params, self.pf.w_0)
        self.kind = self.pf.kind
        self.film = U.film_rows(U.N_GROUPS, L, seed=500 + L).to(dev())
        self.rays, self.t_rand = U.grad_rays().to(dev()), U.t_rand().to(dev())
        self.cots = [c.to(dev()) for c in U.cotangents()]
        self.n, self.nc, self.nf, self.groups = U.N_RAYS, U.NC, U.NF, U.N_GROUPS
        self.z_lin = ops.linspace_table(U.NEAR, U.FAR, self.nc, dev())
        self.u_lin = ops.linspace_table(0.0, 1.0, self.nf, dev())

    def autograd(self):
        from mirender import autograd as A
        for p in self.pf.params:
            p.grad = None
        film = self.film.clone().requires_grad_(True)
        outs = A.render_rays_train(self.pf, self.pf, self.rays, U.NEAR, U.FAR, self.nc, self.nf, film, self.t_rand, 0)
        sum((o * c).sum() for o, c in zip(outs, self.cots)).backward()
        torch.cuda.synchronize()
        return [o.detach() for o in outs], [p.grad.detach().clone() for p in self.pf.params], film.grad.detach()

    def c_pair(self, saved="all", range_points=None):
        """mi_render_rays_train + mi_render_rays_backward through ctypes."""
        from mirender import _lib, autograd as A
        lib, pf, n, nc, nf = _lib.load(), self.pf, self.n, self.nc, self.nf
        rp = A._max_points_per_chunk(pf) if range_points is None else range_points
        ws_bytes = lib.mi_render_workspace_bytes(n, nc, nf) + lib.mi_render_shared_field_extra_bytes(n, nc, nf)
        full = lib.mi_render_train_saved_bytes(self.kind, self.kind, 1, n, nc, nf)
        sv_bytes = {"all": full, "none": 0}[saved]
        bw_bytes = lib.mi_render_backward_workspace_bytes(self.kind, self.kind, 1, self.groups, n // self.groups, nc, nf, rp, rp)
        assert min(ws_bytes, full, bw_bytes) > 0, lib.mi_last_error()
        ws, sv, bw = (torch.empty(int(b) + 16, dtype=torch.uint8, device=dev()) for b in (ws_bytes, sv_bytes, bw_bytes))
        outs = [torch.empty(s, dtype=torch.float32, device=dev()) for s in OUT_SHAPES(n)]
        packed, stream = pf.refresh(), _lib.stream_ptr(dev())
        _lib.check(lib.mi_render_rays_train(self.kind, _lib.ptr(packed), self.kind, _lib.ptr(packed), _lib.ptr(self.film),
                                            _lib.ptr(self.rays), self.groups, n // self.groups, U.NEAR, U.FAR, nc, nf,
                                            _lib.ptr(self.z_lin), _lib.ptr(self.u_lin), _lib.ptr(self.t_rand), 0, 0,
                                            *[_lib.ptr(o) for o in outs], _lib.ptr(ws), ws_bytes, rp, rp, _lib.ptr(sv), sv_bytes,
                                            stream), "mi_render_rays_train")
        arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
        grads = [torch.full_like(p, -7.25) for p in pf.params]
        g_film = torch.full_like(self.film, -7.25)
        written = ctypes.c_int(-1)
        par = arr([p.detach() for p in pf.params])
        _lib.check(lib.mi_render_rays_backward(
            self.kind, _lib.ptr(packed), _lib.ptr(pf.refresh_bwd()), par, self.kind, _lib.ptr(packed), _lib.ptr(pf.refresh_bwd()),
            par, _lib.ptr(self.film), _lib.ptr(self.rays), self.groups, n // self.groups, nc, nf, rp, rp, _lib.ptr(ws), ws_bytes,
            _lib.ptr(sv), sv_bytes, *[_lib.ptr(c) for c in self.cots], arr(grads), None, _lib.ptr(g_film), _lib.ptr(bw),
            bw_bytes, ctypes.byref(written), stream), "mi_render_rays_backward")
        torch.cuda.synchronize()
        return outs, grads, g_film


def equal_all(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what} {i}: {int((x != y).sum())} of {x.numel()} values differ"


def gate_call(case, g, outs, grads, g_film, sd, film):
    """Outputs and every gradient tensor against the fixture (the reference's autograd) and the fp32 / fp64 restatement."""
    o32, g32, f32 = U.oracle_render_grads(sd, film)
    o64, g64, f64 = U.oracle_render_grads(sd, film, torch.float64)
    for k, name in enumerate(U.OUT_NAMES):
        tol = parity.DEPTH_TOL if name.startswith("depth") else parity.TOL
        parity.gate(case, "render_rays", name, outs[k].cpu(), g[name], o64[k], tol=tol)
    named = list(zip(sd.keys(), grads)) + [("film", g_film)]
    ref32, ref64 = dict(g32, film=f32), dict(g64, film=f64)
    for name, t in named:
        parity.gate_grad(case, name, t.cpu(), ref32[name], ref64[name], tol=parity.GRAD_TOL_SMOOTH,
                         elem_tol=parity.GRAD_ELEM_TOL_SMOOTH)
        parity.gate_grad_samples(case, name, t.cpu(), g[f"g.{name}.idx"], g[f"g.{name}.val"], float(g[f"g.{name}.l2"]),
                                 tol=parity.GRAD_TOL_SMOOTH)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("L", U.DEPTHS)
@pytest.mark.parametrize("use_dir", [True, False])
def test_training_against_reference_and_fp64(golden, L, use_dir):
    g = golden(tag(L, use_dir))
    c = Call(L, use_dir)
    assert U.digest(c.sd, c.film.cpu(), U.grad_rays(), U.t_rand(), *U.cotangents()) == str(g["digest.grad"])
    outs, grads, g_film = c.autograd()
    gate_call(tag(L, use_dir) + ".autograd", g, outs, grads, g_film, c.sd, c.film.cpu())
    # the C-ABI pair, every range saved and none saved: bit-equal to each other and to autograd
    o_all, g_all, f_all = c.c_pair(saved="all")
    o_none, g_none, f_none = c.c_pair(saved="none")
    equal_all(o_all, o_none, "pair output (saved all / none)")
    equal_all(g_all + [f_all], g_none + [f_none], "pair gradient (saved all / none)")
    equal_all(o_all, outs, "pair output vs autograd")
    equal_all(g_all + [f_all], grads + [g_film], "pair gradient vs autograd")
    gate_call(tag(L, use_dir) + ".c_pair", g, o_all, g_all, f_all, c.sd, c.film.cpu())


@pytest.mark.timeout(600)
@pytest.mark.parametrize("L", [4, 12])
def test_image_cut_into_parts(golden, L):
    """Ranges smaller than a group (32 rays x 8 samples = 256 points per image and pass): every image is cut into parts whose
    FiLM gradients add up.  The depth-8 test (test_gpu_cabi_train.test_small_ranges) asserts bit equality with autograd under
    the same split only, not with the uncut call: so here the cut call stays inside the same gates."""
    g = golden(tag(L, True))
    c = Call(L, True)
    outs, grads, g_film = c.c_pair(saved="none", range_points=100)
    o_un, _, _ = c.c_pair(saved="all")
    equal_all(outs, o_un, "outputs of the cut call")
    gate_call(tag(L, True) + ".parts", g, outs, grads, g_film, c.sd, c.film.cpu())


# ---- depth 8 through the macro is kinds 2 / 3 ----------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("use_dir", [True, False])
def test_depth_8_macro_gives_the_bits_of_kinds_2_and_3(use_dir):
    from mirender import fields
    a, b = Call(8, use_dir), Call(8, use_dir, kind=U.kind_of(8, use_dir))
    assert a.kind in (2, 3) and b.kind == U.kind_of(8, use_dir)
    x = U.sample_points(513, seed=3).to(dev())
    film3 = U.film_rows(3, 8, seed=4).to(dev())
    assert torch.equal(fields.eval_points(a.pf, x, film3), fields.eval_points(b.pf, x, film3))
    oa, ga, fa = a.autograd()
    ob, gb, fb = b.autograd()
    equal_all(oa, ob, "render output")
    equal_all(ga + [fa], gb + [fb], "gradient")
    assert max(float(t.abs().max()) for t in ga) > 0
    oc, gc, fc = b.c_pair(saved="none")
    equal_all(oa, oc, "render output (pair)")
    equal_all(ga + [fa], gc + [fc], "gradient (pair)")


# ---- FusedAdam -----------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_fused_adam_refreshes_depth_4_streams():
    from mirender import _lib, train
    c = Call(4, True)
    opt = train.FusedAdam(c.model, lr=1e-3)
    before = [p.detach().clone() for p in c.pf.params]
    for _ in range(3):
        c.autograd()                                    # leaves p.grad, builds both streams
        opt.step()
    torch.cuda.synchronize()
    assert all(not torch.equal(p, q) for p, q in zip(c.pf.params, before))
    lib = _lib.load()
    arr = (ctypes.c_void_p * len(c.pf.params))(*[p.data_ptr() for p in c.pf.params])
    for packed, fn in ((c.pf.packed, lib.mi_field_pack), (c.pf.packed_bwd, lib.mi_field_pack_bwd)):
        fresh = torch.empty_like(packed)
        _lib.check(fn(c.kind, arr, len(c.pf.params), c.pf.w_0, _lib.ptr(fresh), _lib.stream_ptr(dev())), "pack")
        torch.cuda.synchronize()
        assert torch.equal(fresh, packed), f"{int((fresh != packed).sum())} stream positions are stale after the scatter refresh"


# ---- Generator, look-alike -----------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_generator_depth_6_trains():
    from mirender import pigan
    torch.manual_seed(0)
    gen = pigan.Generator(64, 16, near=0.5, far=1.5, coarse_samples=12, fine_samples=24, hidden_layers=6).to(dev())
    img = gen(torch.randn(2, 64, device=dev()), thetas=[0.2, -0.1], phis=[0.05, -0.1], seed=1)
    assert tuple(img.shape) == (2, 3, 16, 16) and bool(torch.isfinite(img).all())
    (img * torch.randn_like(img)).sum().backward()
    for name, p in gen.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert float(gen.mapping_network.output_layers[6].weight.grad.abs().max()) > 0
    assert float(gen.film_siren_nerf.hidden_layers[4].weight.grad.abs().max()) > 0


@pytest.mark.timeout(300)
def test_reference_shaped_depth_4_runs_the_fused_kernels():
    from mirender import fields, render_core
    from test_film_depth_host import _RefLookAlike
    sd = U.state_dict(4, True, seed=404, head="medium")
    ref = _RefLookAlike(4)
    ref.load_state_dict(sd)
    ref = ref.to(dev())
    ours = module(4, True, sd)
    pf = fields.as_packed_field(ref)
    assert pf is not None and pf.kind == U.kind_of(4, True)
    film = U.film_rows(2, 4, seed=9).to(dev())
    rays, tr = U.grad_rays().to(dev()), U.t_rand().to(dev())
    with torch.no_grad():
        a = render_core.render_rays(rays, U.NEAR, U.FAR, ref, ref, U.NC, U.NF, t_rand=tr, film=film)
        b = render_core.render_rays(rays, U.NEAR, U.FAR, ours, ours, U.NC, U.NF, t_rand=tr, film=film)
    equal_all(list(a), list(b), "look-alike vs FilmSirenNeRF output")

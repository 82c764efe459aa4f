"""GPU: mi_field_input_grad and mi_field_input_grad_rays (csrc/ray_grad.hip) against the oracle field's autograd.

One training forward and one mi_field_backward per case through the C ABI, as mirender.autograd calls them, then the input
gradient from the acts / grads_ws they left behind.  Reference: torch.autograd.grad of the CPU oracle with respect to x
[P,6] (point form) or rays [n,2,3] (ray form: pts = o + d z, view = d / |d|, nerf/render.py:122,134), in fp32 and fp64,
with a random cotangent on all four outputs.  Gate: parity.gate_grad with the tolerance class of the kind's parameter
gradients - GRAD_TOL_RELU for the ReLU kinds, GRAD_TOL_SMOOTH with GRAD_ELEM_TOL_SMOOTH per element for the sin kinds - and
the fp64 reference, so the fp64-anchored bound is active.

Sizes: 2 x 333 points (no multiple of a point tile or of the kernels' 4-point / 32-point steps; two FiLM groups, one group
of 666 points for the other kinds) and 2 x 37 rays x 9 samples (9 = two full 4-sample steps and a ragged one)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import film_depth_util as U
from oracle import fields as ofields, parity, synth

pytestmark = pytest.mark.gpu

KINDS = ["nerf", "tiny_nerf", "siren_nerf", "film_siren_nerf", "film_siren_nerf_nodir", "film_L4_nodir", "film_L12_dir"]
PPG, RPG, S = 333, 37, 9


def dev():
    return torch.device("cuda", 0)


_SETUP = {}


def setup(kind):
    """(module on the device, packed field, n_groups, FiLM table or None, oracle(dtype) -> f(x, group))."""
    from mirender import fields
    if kind in _SETUP:
        return _SETUP[kind]
    if kind.startswith("film_L"):
        L, use_dir = int(kind.split("_")[1][1:]), kind.endswith("_dir")
        sd, film = U.state_dict(L, use_dir, seed=300 + L, head="medium"), U.film_rows(2, L, seed=400 + L)
        m = fields.FilmSirenNeRF(hidden_layers=L, use_dir=use_dir)

        def oracle(dt):
            sd_t = {k: v.to(dt) for k, v in sd.items()}
            return lambda x, g: U.forward(sd_t, film[g].to(dt), x)
    else:
        sd = synth.state_dict(kind, 21, "medium", 0.05)
        film = synth.film_params(2, seed=22) if kind.startswith("film") else None
        m = fields.FilmSirenNeRF(use_dir=False) if kind == "film_siren_nerf_nodir" else {
            "nerf": fields.NeRF, "tiny_nerf": fields.TinyNeRF, "siren_nerf": fields.SirenNeRF,
            "film_siren_nerf": fields.FilmSirenNeRF}[kind]()

        def oracle(dt):
            sd_t = {k: v.to(dt) for k, v in sd.items()}
            return lambda x, g: ofields.make_field(kind, sd_t, None if film is None else film[g].to(dt))(x)
    m.load_state_dict(sd)
    m = m.to(dev())
    _SETUP[kind] = (m, fields.as_packed_field(m), 2 if film is not None else 1, film, oracle)
    return _SETUP[kind]


def hip_backward(pf, film, n_groups, per_group, x=None, rays=None, z=None, g_raw=None):
    """Training forward + mi_field_backward; returns (acts, grads_ws, parameter pointer array, film on the device)."""
    from mirender import _lib
    lib = _lib.load()
    k = pf.kind
    P = g_raw.shape[0]
    film_d = None if film is None else film.to(dev()).contiguous()
    acts = torch.empty(lib.mi_field_train_acts_floats(k) * P, device=dev())
    raw = torch.empty(P, 4, device=dev())
    stream = _lib.stream_ptr(dev())
    if x is not None:
        _lib.check(lib.mi_field_eval_points_train(k, _lib.ptr(pf.refresh()), _lib.ptr(film_d), _lib.ptr(x), n_groups, per_group,
                                                  _lib.ptr(raw), _lib.ptr(acts), stream), "mi_field_eval_points_train")
        ppg = per_group
    else:
        _lib.check(lib.mi_field_eval_rays_train(k, _lib.ptr(pf.refresh()), _lib.ptr(film_d), _lib.ptr(rays), _lib.ptr(z),
                                                n_groups, per_group, S, _lib.ptr(raw), _lib.ptr(acts), stream),
                   "mi_field_eval_rays_train")
        ppg = per_group * S
    gws = torch.empty(lib.mi_field_train_grads_floats(k) * P, device=dev())
    part = torch.empty(lib.mi_field_bwd_partial_floats_kind(k, P), device=dev())
    out = [torch.empty_like(p) for p in pf.params]
    arr = (ctypes.c_void_p * len(out))(*[t.data_ptr() for t in out])
    par = (ctypes.c_void_p * len(out))(*[p.data_ptr() for p in pf.params])
    fp = gfilm = None
    if film is not None:
        fp = torch.empty(lib.mi_field_film_partial_floats_kind(k, n_groups, ppg), device=dev())
        gfilm = torch.empty_like(film_d)
    _lib.check(lib.mi_field_backward(k, _lib.ptr(pf.refresh_bwd()), _lib.ptr(film_d), _lib.ptr(acts), _lib.ptr(gws),
                                     _lib.ptr(raw), _lib.ptr(g_raw), n_groups, ppg, _lib.ptr(part), _lib.ptr(fp), arr,
                                     par if film is not None else None, len(out), _lib.ptr(gfilm), stream), "mi_field_backward")
    return acts, gws, par, film_d, out


def gate(case, name, kind, got, r32, r64):
    smooth = kind not in ("nerf", "tiny_nerf")
    return parity.gate_grad(case, name, got.cpu(), r32, r64, tol=parity.GRAD_TOL_SMOOTH if smooth else parity.GRAD_TOL_RELU,
                            elem_tol=parity.GRAD_ELEM_TOL_SMOOTH if smooth else None)


def oracle_grad_x(oracle, x, cot, n_groups, dt):
    xr = x.to(dt).clone().requires_grad_(True)
    per = x.shape[0] // n_groups
    out = torch.cat([oracle(dt)(xr[g * per:(g + 1) * per], g) for g in range(n_groups)])
    (out * cot.to(dt)).sum().backward()
    return xr.grad


def rays_to_x(rays, z):
    o, d = rays[:, 0], rays[:, 1]
    pts = o[:, None, :] + d[:, None, :] * z[:, :, None]
    view = (d / torch.norm(d, dim=-1, keepdim=True))[:, None].expand_as(pts)
    return torch.cat([pts, view], -1).reshape(-1, 6)


@pytest.mark.parametrize("kind", KINDS)
def test_point_form_vs_oracle_autograd(kind):
    from mirender import _lib
    lib = _lib.load()
    m, pf, ng, film, oracle = setup(kind)
    P = 2 * PPG
    x = U.sample_points(P, seed=5, scale=1.2)
    g = torch.Generator().manual_seed(6)
    cot = torch.randn(P, 4, generator=g)
    acts, gws, par, film_d, _ = hip_backward(pf, film, ng, P // ng, x=x.to(dev()), g_raw=cot.to(dev()).contiguous())
    g_x = torch.full((P, 6), float("nan"), device=dev())
    _lib.check(lib.mi_field_input_grad(pf.kind, par, len(pf.params), _lib.ptr(film_d), _lib.ptr(acts), _lib.ptr(gws), ng,
                                       P // ng, _lib.ptr(g_x), _lib.stream_ptr(dev())), "mi_field_input_grad")
    assert torch.isfinite(g_x).all()
    r32, r64 = (oracle_grad_x(oracle, x, cot, ng, dt) for dt in (torch.float32, torch.float64))
    case = f"input grad points {kind} {ng}x{P // ng}"
    gate(case, "g_x position", kind, g_x[:, :3], r32[:, :3], r64[:, :3])
    if kind.endswith("nodir"):
        assert torch.equal(g_x[:, 3:], torch.zeros(P, 3, device=dev())), "no direction input: exactly zero"
        assert float(r64[:, 3:].abs().max()) == 0.0
    else:
        gate(case, "g_x direction", kind, g_x[:, 3:], r32[:, 3:], r64[:, 3:])


@pytest.mark.parametrize("kind", KINDS)
def test_ray_form_vs_oracle_autograd_and_point_form(kind):
    from mirender import _lib
    lib = _lib.load()
    m, pf, ng, film, oracle = setup(kind)
    n = 2 * RPG
    rng = np.random.Generator(np.random.PCG64(9))
    o = rng.normal(size=(n, 3)).astype(np.float32) * 0.1 + np.array([0, 0, 1], np.float32)
    d = (rng.uniform(-0.2, 0.2, size=(n, 3)).astype(np.float32) - o) * rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    rays = torch.from_numpy(np.stack([o, d], 1))                                  # non-unit directions
    z = torch.from_numpy(np.sort(rng.uniform(0.3, 1.0, size=(n, S)).astype(np.float32), -1))
    cot = torch.from_numpy(rng.normal(size=(n * S, 4)).astype(np.float32))
    rays_d, z_d = rays.to(dev()).contiguous(), z.to(dev()).contiguous()
    acts, gws, par, film_d, _ = hip_backward(pf, film, ng, n // ng, rays=rays_d, z=z_d, g_raw=cot.to(dev()).contiguous())
    stream = _lib.stream_ptr(dev())

    def ray_form(accumulate, into):
        _lib.check(lib.mi_field_input_grad_rays(pf.kind, par, len(pf.params), _lib.ptr(film_d), _lib.ptr(acts), _lib.ptr(gws),
                                                _lib.ptr(rays_d), _lib.ptr(z_d), ng, n // ng, S, accumulate, _lib.ptr(into),
                                                stream), "mi_field_input_grad_rays")
        return into

    g_rays = ray_form(0, torch.full((n, 2, 3), float("nan"), device=dev()))
    assert torch.isfinite(g_rays).all()
    refs = {}
    for dt in (torch.float32, torch.float64):
        rr = rays.to(dt).clone().requires_grad_(True)
        xr = rays_to_x(rr, z.to(dt))
        per = xr.shape[0] // ng
        out = torch.cat([oracle(dt)(xr[g * per:(g + 1) * per], g) for g in range(ng)])
        (out * cot.to(dt)).sum().backward()
        refs[dt] = rr.grad
    case = f"input grad rays {kind} {ng}x{n // ng}x{S}"
    gate(case, "g_rays origin", kind, g_rays[:, 0], refs[torch.float32][:, 0], refs[torch.float64][:, 0])
    gate(case, "g_rays direction", kind, g_rays[:, 1], refs[torch.float32][:, 1], refs[torch.float64][:, 1])

    # accumulate = 1 onto a known tensor adds exactly; run to run the same bits
    base = torch.randn(n, 2, 3, device=dev())
    assert torch.equal(ray_form(1, base.clone()), base + g_rays)
    assert torch.equal(ray_form(0, torch.empty(n, 2, 3, device=dev())), g_rays)

    # The ray form equals the point form of the same buffers reduced in torch (float64), to within fp32 summation order.
    # Both forms add the same 256 (+ 256 + 128) products per point and component, in different orders (per lane and then
    # across lanes, before or after the sum over the samples).  Reordering a K-term fp32 sum of terms with mixed signs moves
    # it by about sqrt(K) u times the terms' root sum of squares, which is the size of the sum itself: 2 sqrt(256) u = 32 u of
    # a point's gradient for the two forms together; the sum over the S samples adds 2 sqrt(S) u (as composite_gates takes
    # for its sums) and z g_pos, the projection and the division by |d| another 8 u.  A component that cancels within a
    # point has no scale of its own, so the scale is the ray's largest component: per ray
    #     bound = (32 + 2 sqrt(S) + 8) u max_j sum_s |term_s,j|
    # with term_s = g_pos,s for g_o, and z_s g_pos,s and g_dir,s / |d| (twice: v v^T g is as large at most) for g_d.
    g_x = torch.empty(n * S, 6, device=dev())
    _lib.check(lib.mi_field_input_grad(pf.kind, par, len(pf.params), _lib.ptr(film_d), _lib.ptr(acts), _lib.ptr(gws), ng,
                                       n * S // ng, _lib.ptr(g_x), stream), "mi_field_input_grad")
    gp, gv = g_x[:, :3].double().reshape(n, S, 3), g_x[:, 3:].double().reshape(n, S, 3)
    zz, dd = z_d.double(), rays_d[:, 1].double()
    nrm = dd.norm(dim=-1, keepdim=True)
    v = dd / nrm
    sv = gv.sum(1)
    want_o = gp.sum(1)
    want_d = (zz[..., None] * gp).sum(1) + (sv - v * (v * sv).sum(-1, keepdim=True)) / nrm
    u = 2.0 ** -24
    c = (32 + 2 * math.sqrt(S) + 8) * u
    b_o = c * gp.abs().sum(1).amax(-1, keepdim=True) + 1e-37
    b_d = c * ((zz[..., None] * gp.abs()).sum(1) + 2 * gv.abs().sum(1) / nrm).amax(-1, keepdim=True) + 1e-37
    r_o = float(((g_rays[:, 0].double() - want_o).abs() / b_o).max())
    r_d = float(((g_rays[:, 1].double() - want_d).abs() / b_d).max())
    parity.record(case=case, stage="ray form vs reduced point form", qty="g_rays", err_over_bound=max(r_o, r_d),
                  active=f"({32 + 8} + 2 sqrt(S)) u sum |terms|", passed=bool(max(r_o, r_d) <= 1.0))
    assert r_o <= 1.0 and r_d <= 1.0, (r_o, r_d)
    if kind.endswith("nodir"):
        assert torch.equal(g_x[:, 3:], torch.zeros_like(g_x[:, 3:]))

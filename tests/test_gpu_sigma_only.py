"""GPU: mi_render_rays without the coarse outputs.

A caller that keeps only the fine outputs (render_image, render_video, render_image_dist) passes rgb_c = NULL.  With two
different fields the coarse pass then feeds nothing but sample_fine's weights, which depend on sigma alone: the library
runs the coarse field's sigma-only forward (the trunk and the sigma head) and a weights-only composite.  Sigma is final
before the colour branch starts, so the fine outputs must be the SAME BITS as those of a call that asks for all six:

* NeRF / TinyNeRF / SirenNeRF pairs, 64 + 128 and small odd sample counts, 65 coarse samples (two passes of the
  weights-only composite: its carry of T), point counts that leave a partial 128-point tile, seeded jitter and t_rand;
* depth_c / acc_c asked for while rgb_c is NULL: bit-equal to the all-six call's;
* the fallbacks (one shared field, Nf = 0 with one field, a FiLM pair) give the same bits too;
* render_image / render_image_dist equal render_rays(...)[3:6]."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import render_ref as R, synth  # noqa: E402


def dev():
    return torch.device("cuda", 0)


def _field(kind, seed):
    from mirender import fields
    return fields.field_from_state_dict(synth.state_dict(kind, seed=seed, sharp="medium", bias_jitter=0.05), dev())


def _rays(n, film):
    pose = synth.pose_radians(1.0, 0.2, -0.1) if film else synth.pose_degrees(4.0, 20.0, -30.0)
    return torch.from_numpy(R.rays_from_camera(40, 40, 180.0 if film else 55.0, pose)[:n]).to(dev())


def _abi(pf_c, pf_f, rays, near, far, nc, nf, tr, seed, coarse, film=None, groups=1):
    """mi_render_rays with the coarse outputs named by `coarse` ("rgb", "depth", "acc") and NULL for the others."""
    from mirender import _lib, ops
    lib = _lib.load()
    n = rays.shape[0]
    ws_bytes = lib.mi_render_workspace_bytes(n, nc, nf)
    if pf_c is pf_f:
        ws_bytes += lib.mi_render_shared_field_extra_bytes(n, nc, nf)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
    shapes = {"rgb": (n, 3), "depth": (n,), "acc": (n,)}
    outs = [torch.full(shapes[k], float("nan"), device=dev()) if k in coarse else None for k in ("rgb", "depth", "acc")]
    outs += [torch.empty(s, dtype=torch.float32, device=dev()) for s in ((n, 3), (n,), (n,))]
    zl, ul = ops.linspace_table(near, far, nc, dev()), ops.linspace_table(0.0, 1.0, nf, dev())
    rc = lib.mi_render_rays(pf_c.kind, _lib.ptr(pf_c.refresh()), pf_f.kind, _lib.ptr(pf_f.refresh()), _lib.ptr(film),
                            _lib.ptr(rays), groups, n // groups, near, far, nc, nf, _lib.ptr(zl), _lib.ptr(ul), _lib.ptr(tr),
                            seed, 0, *[_lib.ptr(o) for o in outs], _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dev()))
    assert rc == 0, lib.mi_last_error()
    return outs


def _assert_same(a, b):
    for x, y in zip(a, b):
        assert x is not None and y is not None and torch.equal(x, y)


@pytest.mark.parametrize("kind,n,nc,nf,jitter", [("nerf", 257, 64, 128, "seed"), ("nerf", 33, 5, 3, "t_rand"),
                                                 ("tiny_nerf", 130, 7, 11, "seed"), ("tiny_nerf", 64, 64, 128, "t_rand"),
                                                 ("siren_nerf", 101, 9, 0, "t_rand"), ("siren_nerf", 257, 64, 128, "seed"),
                                                 ("nerf", 1, 3, 1, "seed"), ("tiny_nerf", 130, 65, 16, "t_rand")])
def test_sigma_only_coarse_pass_gives_the_same_fine_bits(kind, n, nc, nf, jitter):
    from mirender import fields, ops
    pf_c, pf_f = fields.as_packed_field(_field(kind, 5)), fields.as_packed_field(_field(kind, 6))
    rays = _rays(n, False)
    tr = synth.t_rand(n, nc, seed=9).to(dev()) if jitter == "t_rand" else None
    with torch.no_grad():
        full = ops.render_rays_fused(pf_c, pf_f, rays, 2.0, 6.0, nc, nf, None, tr, seed=1234)
        fine = ops.render_rays_fused(pf_c, pf_f, rays, 2.0, 6.0, nc, nf, None, tr, seed=1234, coarse_outputs=False)
    assert fine[:3] == (None, None, None)
    assert all(bool(torch.isfinite(o).all()) for o in full)
    _assert_same(full[3:], fine[3:])
    # depth_c / acc_c without rgb_c: from the weights-only composite, the same bits as the all-six call's
    for coarse in (("depth", "acc"), ("depth",), ("acc",)):
        outs = _abi(pf_c, pf_f, rays, 2.0, 6.0, nc, nf, tr, 1234, coarse)
        _assert_same(full[3:], outs[3:])
        if "depth" in coarse:
            assert torch.equal(outs[1], full[1])
        if "acc" in coarse:
            assert torch.equal(outs[2], full[2])


@pytest.mark.parametrize("case", ["shared", "shared_nf0", "film_pair", "film_shared"])
def test_fallbacks_give_the_same_bits(case):
    from mirender import fields, ops
    film_kind = case.startswith("film")
    kind = "film_siren_nerf" if film_kind else "nerf"
    n, nc, nf = (130, 12, 0) if case == "shared_nf0" else (130, 12, 24)
    pf_c = fields.as_packed_field(_field(kind, 5))
    pf_f = pf_c if case in ("shared", "shared_nf0", "film_shared") else fields.as_packed_field(_field(kind, 6))
    film = synth.film_params(2, seed=3).to(dev()) if film_kind else None
    near, far = (0.5, 1.5) if film_kind else (2.0, 6.0)
    rays, tr = _rays(n, film_kind), synth.t_rand(n, nc, seed=9).to(dev())
    with torch.no_grad():
        full = ops.render_rays_fused(pf_c, pf_f, rays, near, far, nc, nf, film, tr)
        fine = ops.render_rays_fused(pf_c, pf_f, rays, near, far, nc, nf, film, tr, coarse_outputs=False)
    assert fine[:3] == (None, None, None)
    _assert_same(full[3:], fine[3:])
    outs = _abi(pf_c, pf_f, rays, near, far, nc, nf, tr, 0, ("depth", "acc"), film, 2 if film_kind else 1)
    _assert_same(full[1:], outs[1:])
    if case == "shared_nf0":                   # one field, Nf = 0: the coarse outputs are the fine outputs
        _assert_same(full[:3], full[3:])


def test_coarse_rgb_needs_depth_and_acc():
    from mirender import _lib, fields, ops
    lib = _lib.load()
    pf_c, pf_f = fields.as_packed_field(_field("nerf", 5)), fields.as_packed_field(_field("nerf", 6))
    n, nc, nf = 16, 8, 8
    rays = _rays(n, False)
    ws_bytes = lib.mi_render_workspace_bytes(n, nc, nf)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
    o3, o1 = torch.empty((n, 3), device=dev()), torch.empty(n, device=dev())
    rc = lib.mi_render_rays(pf_c.kind, _lib.ptr(pf_c.refresh()), pf_f.kind, _lib.ptr(pf_f.refresh()), None, _lib.ptr(rays),
                            1, n, 2.0, 6.0, nc, nf, None, None, None, 0, 0, _lib.ptr(o3), None, _lib.ptr(o1),
                            _lib.ptr(o3), _lib.ptr(o1), _lib.ptr(o1), _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dev()))
    assert rc == -1 and b"null pointer" in lib.mi_last_error()
    rc = lib.mi_render_rays(pf_c.kind, _lib.ptr(pf_c.refresh()), pf_f.kind, _lib.ptr(pf_f.refresh()), None, _lib.ptr(rays),
                            1, n, 2.0, 6.0, nc, nf, None, None, None, 0, 0, None, None, None,
                            None, _lib.ptr(o1), _lib.ptr(o1), _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dev()))
    assert rc == -1 and b"null pointer" in lib.mi_last_error()                # the fine outputs stay mandatory


@pytest.mark.parametrize("kind", ["nerf", "tiny_nerf"])
def test_render_image_paths_equal_render_rays(kind):
    from mirender import dist, ops, render_core
    cm, fm = _field(kind, 5), _field(kind, 6)
    w, h, focal = 37, 23, 30.0
    pose = synth.pose_degrees(4.0, 20.0, -30.0)
    with torch.no_grad():
        ref = render_core.render_rays(ops.gen_rays(w, h, focal, pose, dev()), 2.0, 6.0, cm, fm, 16, 24, seed=77)
    rgb, depth, acc = render_core.render_image(w, h, focal, pose, 2.0, 6.0, cm, fm, 16, 24, seed=77)
    assert np.array_equal(rgb.reshape(-1, 3), ref[3].cpu().numpy())
    assert np.array_equal(depth.reshape(-1), ref[4].cpu().numpy())
    assert np.array_equal(acc.reshape(-1), ref[5].cpu().numpy())
    out = dist.render_image_dist(w, h, focal, pose, 2.0, 6.0, cm, fm, 16, 24, seed=77)
    for a, b in zip(out, ref[3:]):
        assert torch.equal(a.reshape(b.shape), b)

"""GPU: the training (backward) path against autograd of the CPU oracle and the golden gradient fixtures."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fields as ofields, parity, render_ref as R, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device("cuda", 0)


def _nerf_render():
    spec = importlib.util.spec_from_file_location(
        "mi_nerf_render_t", os.path.join(ROOT, "msra-practice-project_amd", "nerf", "render.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def model(kind, sd):
    from mirender import fields
    if kind == "film_siren_nerf_nodir":
        m = fields.FilmSirenNeRF(use_dir=False)
    else:
        m = {"nerf": fields.NeRF, "tiny_nerf": fields.TinyNeRF, "siren_nerf": fields.SirenNeRF,
             "film_siren_nerf": fields.FilmSirenNeRF}[kind]()
    m.load_state_dict(sd)
    return m.to(dev())


def _assert_close_last_and_interior(got, ref):
    """2e-5 of the largest gradient, the last sample of a ray and the samples before it each on their own scale: the
    last delta is 1e10 |d| (render.py:94), so d/dsigma of a last sample with sigma == 0 is about 1e10, and on that scale
    every other element would pass as 0 (per element against float64: test_gpu_composite_stages.py)."""
    for part in (slice(-1, None), slice(0, -1)):
        g, r = got[:, part], ref[:, part]
        if r.numel():
            assert float((g - r).abs().max()) <= 2e-5 * max(1.0, float(r.abs().max())), part


@pytest.mark.parametrize("S", [1, 13, 64, 192])
def test_composite_bwd_vs_oracle_autograd(S):
    from mirender import autograd as A
    rng = np.random.Generator(np.random.PCG64(S))
    n = 257
    raw = rng.uniform(0, 1, size=(n, S, 4)).astype(np.float32)
    raw[..., 3] = rng.exponential(2.0, size=(n, S)).astype(np.float32) * (rng.random((n, S)) < 0.5)
    z = np.sort(rng.uniform(2, 6, size=(n, S)).astype(np.float32), -1)
    rd = rng.normal(size=(n, 3)).astype(np.float32)
    g = [torch.from_numpy(rng.normal(size=s).astype(np.float32)) for s in ((n, 3), (n,), (n,))]
    rt = torch.from_numpy(raw).requires_grad_(True)
    rgb, depth, acc, _ = R.composite(rt, torch.from_numpy(z), torch.from_numpy(rd))
    (rgb * g[0]).sum().add((depth * g[1]).sum()).add((acc * g[2]).sum()).backward()
    rays = torch.from_numpy(np.stack([np.zeros_like(rd), rd], 1)).to(dev())
    got = A._composite_bwd(torch.from_numpy(raw).to(dev()), torch.from_numpy(z).to(dev()), rays,
                           g[0].to(dev()), g[1].to(dev()), g[2].to(dev())).cpu()
    _assert_close_last_and_interior(got, rt.grad)
    # partial cotangents (None) behave as zeros
    got2 = A._composite_bwd(torch.from_numpy(raw).to(dev()), torch.from_numpy(z).to(dev()), rays, g[0].to(dev()),
                            None, None).cpu()
    rt.grad = None
    rgb, _, _, _ = R.composite(rt, torch.from_numpy(z), torch.from_numpy(rd))
    (rgb * g[0]).sum().backward()
    _assert_close_last_and_interior(got2, rt.grad)


def _grad_check(case, named_got, g, prefix, tol=2e-4):
    """Fixture grads are stored as 512 strided samples + L2 norm per tensor (tests/golden/make_golden.py).  Every
    tensor leaves a record (oracle/parity.py:gate_grad_samples); the first failure is raised after all were recorded."""
    recs = [parity.gate_grad_samples(case, prefix + name, t.detach().cpu().numpy(), g[f"g.{prefix}{name}.idx"],
                                     g[f"g.{prefix}{name}.val"], g[f"g.{prefix}{name}.l2"], tol, check=False)
            for name, t in named_got]
    bad = [r for r in recs if not r["passed"]]
    assert not bad, bad[0]
    return max(max(r["max_sample_err_over_norm"], r["norm_err_over_norm"]) for r in recs)


def test_nerf_loss_grads_golden(golden):
    """Fixture F7: train_nerf.py:158-167 loss (use_alpha, fine model on) on a 48-ray batch, 64+128 samples;
    gradients of every weight of both models from the reference's autograd."""
    g = golden("nerf_grad_f7")
    render = _nerf_render()
    nc, nf = int(g["n_coarse"]), int(g["n_fine"])
    cm = model("nerf", synth.state_dict("nerf", 50, True, 0.05))
    fm = model("nerf", synth.state_dict("nerf", 51, True, 0.05))
    out = render.render_rays(torch.from_numpy(g["rays"]).to(dev()), 2.0, 6.0, cm, fm, nc, nf,
                             t_rand=torch.from_numpy(g["t_rand"]).to(dev()))
    rgb_c, _, acc_c, rgb_f, _, acc_f = out
    assert rgb_f.requires_grad
    tgt = torch.from_numpy(g["target"]).to(dev())
    loss = sum(torch.mean((rgb - tgt[:, :3]) ** 2) + 0.1 * torch.mean((acc - tgt[:, 3]) ** 2)
               for rgb, acc in ((rgb_f, acc_f), (rgb_c, acc_c)))
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-4
    # coarse gradients do not depend on the ill-conditioned resampling: tight (achieved 4.6e-5 of a tensor's norm); fine: the
    # reference's resampled depths differ from the HIP path's on a few rays (the x50 head: DESIGN.md section 2), which moves a
    # tensor's gradient by up to 9.4e-4 of its norm (fine.layers_pos.2.bias; profiles/r04_parity.json) - gated at 5e-3,
    # ~5x that (round 3 had 2e-2 here: a 10x regression of the backward through resampling would have passed)
    case = f"F7 nerf loss gradients, 48 rays {nc}+{nf}, sharp heads (end to end through resampling)"
    _grad_check(case, [(k, p.grad) for k, p in cm.named_parameters()], g, "coarse.", tol=5e-4)
    _grad_check(case, [(k, p.grad) for k, p in fm.named_parameters()], g, "fine.", tol=5e-3)


@pytest.mark.parametrize("kind,n,nc,nf,sharp", [("nerf", 37, 16, 24, True), ("tiny_nerf", 130, 8, 8, True),
                                                 ("tiny_nerf", 130, 8, 8, False), ("nerf", 300, 12, 20, False),
                                                 ("siren_nerf", 61, 12, 20, True), ("film_siren_nerf", 64, 12, 24, True),
                                                 ("film_siren_nerf_nodir", 50, 6, 6, True)])
def test_field_grads_vs_oracle_autograd_injected(kind, n, nc, nf, sharp):
    """Same cotangents through the oracle (CPU autograd, fp32 and fp64) and through the HIP path with the
    depths injected.  ReLU derivatives are 0/1 switches on the sign of a pre-activation, so any two fp32
    pipelines disagree on a handful of (point, unit) pairs and each such flip moves a tensor's gradient by
    ~1e-3 of its norm: the gate is the fp64 truth, with the fp32 oracle's own distance from it as the scale
    (3x that, or 5e-3 of the tensor's norm, whichever is larger)."""
    from mirender import autograd as A, fields, ops
    sd_f = synth.state_dict(kind, 7, sharp, 0.05)
    rays = torch.from_numpy(R.rays_from_camera(24, 24, 33.0, synth.pose_degrees(4.0, 15.0, -30.0))[100:100 + n])
    rng = np.random.Generator(np.random.PCG64(1))
    z = torch.from_numpy(np.sort(rng.uniform(2, 6, size=(n, nc + nf)).astype(np.float32), -1))
    cot = [torch.from_numpy(rng.normal(size=s).astype(np.float32)) for s in ((n, 3), (n,), (n,))]
    is_film = kind.startswith("film")
    n_img = 2 if is_film else 1                      # FiLM: two groups (images) of n/2 rays each
    film0 = synth.film_params(n_img, seed=8) if is_film else None
    refs = {}
    for dt in (torch.float32, torch.float64):
        sd_req = {k: v.clone().to(dt).requires_grad_(True) for k, v in sd_f.items()}
        film_req = film0.clone().to(dt).requires_grad_(True) if is_film else None
        ro, rd = rays[:, 0].to(dt), rays[:, 1].to(dt)
        pts, view = R.points_on_rays(ro, rd, z.to(dt)), rd / torch.norm(rd, dim=-1, keepdim=True)
        if is_film:
            half = n // 2
            raw = torch.cat([R.query_field(pts[i * half:(i + 1) * half], view[i * half:(i + 1) * half],
                                           ofields.make_field(kind, sd_req, film_req[i])) for i in range(2)])
        else:
            raw = R.query_field(pts, view, ofields.make_field(kind, sd_req))
        rgb, depth, acc, _ = R.composite(raw, z.to(dt), rd)
        ((rgb * cot[0].to(dt)).sum() + (depth * cot[1].to(dt)).sum() + (acc * cot[2].to(dt)).sum()).backward()
        refs[dt] = {k: v.grad.double() for k, v in sd_req.items()}
        if is_film:
            refs[dt]["__film__"] = film_req.grad.double()

    m = model(kind, sd_f)
    pf = fields.as_packed_field(m)
    rays_d, z_d = rays.to(dev()), z.to(dev())
    film_d = film0.to(dev()) if is_film else None
    raw_d = ops.field_eval_rays(pf, rays_d, z_d, film_d)
    g_raw = A._composite_bwd(raw_d, z_d, rays_d, *[c.to(dev()) for c in cot])
    got, got_film = A._field_backward(pf, rays_d, z_d, raw_d, g_raw, film_d)
    names = []
    for key, _ in fields.SPECS[pf.kind]:
        names += [key + ".weight", key + ".bias"]
    pairs = list(zip(names, got)) + ([("__film__", got_film)] if is_film else [])
    smooth = kind not in ("nerf", "tiny_nerf")       # sin activations have no derivative switches
    case = f"injected-depth gradients {kind} {n} rays S={nc + nf} sharp={sharp}"
    recs = [parity.gate_grad(case, name, t.cpu(), refs[torch.float32][name], refs[torch.float64][name],
                             tol=parity.GRAD_TOL_SMOOTH if smooth else parity.GRAD_TOL_RELU,
                             elem_tol=parity.GRAD_ELEM_TOL_SMOOTH if smooth else None, check=False) for name, t in pairs]
    bad = [r for r in recs if not r["passed"]]
    assert not bad, bad[0]
    # most tensors see no flip at all and agree to fp32 rounding: with the fp64 oracle, or - where the fp32 oracle itself sits
    # further from it than that - with the fp32 oracle.  The kernels evaluate the oracle's fp32 points o + d z bit for bit
    # (tests/test_gpu_prologue_gates.py), and the rounding of a point is 2^9 times larger in the encoding's last frequency
    # than anything the layers add: on 300 rays the oracle's own fp32 gradients are 6e-4 .. 1.7e-3 from fp64 in 20 of 24
    # tensors, and the HIP path's with them (measured: at most 2e-4 from the fp32 oracle's, 1.7e-3 from fp64 like its own).
    for r, (name, t) in zip(recs, pairs):
        r32 = refs[torch.float32][name].reshape(-1)
        r["rel_l2_vs_oracle32"] = float(torch.linalg.norm(t.cpu().double().reshape(-1) - r32) / max(float(torch.linalg.norm(r32)), 1e-30))
    assert sum(r["rel_l2_err"] <= 3e-4 or (r["oracle32_rel_l2_from_fp64"] > 3e-4 and r["rel_l2_vs_oracle32"] <= 3e-4)
               for r in recs) >= len(pairs) // 2
    # the recompute path (above: nothing kept) gives the same gradients as the kept-activation path
    if not is_film:
        raw_s, saved = A._forward_pass(pf, rays_d, z_d, film_d, 1 << 40)
        assert saved and torch.equal(raw_s, raw_d)
        got2, _ = A._field_backward(pf, rays_d, z_d, raw_s, g_raw, film_d, saved)
        for a_, b_ in zip(got, got2):
            assert torch.equal(a_, b_)


def test_pigan_image_and_grads_golden(golden):
    """Fixture F6: pi_GAN Generator.forward loop (modules.py:179-181) without the mapping network: two 16x16
    images from one FilmSirenNeRF, FiLM tables as leaf tensors; image and gradients of sum(img*cot) w.r.t. the
    FiLM tables and every field weight from the reference's autograd.  End to end (resampling included)."""
    g = golden("pigan_grad_f6")
    spec = importlib.util.spec_from_file_location(
        "mi_pigan_render_t", os.path.join(ROOT, "msra-practice-project_amd", "pi_GAN", "render.py"))
    pr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pr)
    res, nc, nf = int(g["res"]), int(g["n_coarse"]), int(g["n_fine"])
    m = model("film_siren_nerf", synth.state_dict("film_siren_nerf", seed=40, sharp=True))
    film = torch.from_numpy(g["film"]).to(dev()).requires_grad_(True)
    focal = res / 2 / np.tan(float(g["fov"]) / 2 * np.pi / 180)         # np.float64, as Renderer computes it
    imgs = []
    for i in range(film.shape[0]):
        m.set_film_params(film[i])
        pose = pr.camera_pos_to_transform_matrix(1, float(g["thetas"][i]), float(g["phis"][i]))
        imgs.append(pr.render_image(res, res, focal, pose, float(g["near"]), float(g["far"]), m, m, nc, nf,
                                    t_rand=torch.from_numpy(g["t_rand"][i]).to(dev())))
    img = torch.stack(imgs)
    assert img.requires_grad and tuple(img.shape) == tuple(g["image"].shape)
    d = (img.detach().cpu() - torch.from_numpy(g["image"])).abs()
    assert float((d > 1e-4).double().mean()) <= 0.05
    (img * torch.from_numpy(g["cotangent"]).to(dev())).sum().backward()
    case = f"F6 pi_GAN image gradients, 2 images {res}x{res} {nc}+{nf}, sharp head (end to end through resampling)"
    # end to end through the resampling of a x50 head: achieved 2.4e-4 (FiLM table) and at worst 1.1e-3 of a tensor's norm
    # (output_layer_sigma.0.bias); gated at 2e-3 / 5e-3 (round 3: 5e-2 for both)
    parity.gate_grad(case, "film table", film.grad.cpu(), g["grad_film"], tol=2e-3)
    _grad_check(case, [(k, p.grad) for k, p in m.named_parameters()], g, "", tol=5e-3)


def test_shared_model_and_unused_outputs():
    """coarse_model is fine_model (train_nerf.py:91,94 with use_fine_model false) and a loss on rgb_f only
    (pi_GAN consumes only the fine rgb, pi_GAN/render.py:203): gradients flow once, coarse pass is skipped."""
    render = _nerf_render()
    sd = synth.state_dict("tiny_nerf", 3, True, 0.05)
    m = model("tiny_nerf", sd)
    rays = torch.from_numpy(R.rays_from_camera(16, 16, 22.0, synth.pose_degrees(4.0, 0.0, -30.0))).to(dev())
    tr = synth.t_rand(256, 8, 1).to(dev())
    out = render.render_rays(rays, 2.0, 6.0, m, m, 8, 8, t_rand=tr)
    out[3].sum().backward()
    g1 = [p.grad.clone() for p in m.parameters()]
    assert all(torch.isfinite(g).all() for g in g1) and any(float(g.abs().max()) > 0 for g in g1)
    for p in m.parameters():
        p.grad = None
    out = render.render_rays(rays, 2.0, 6.0, m, m, 8, 8, t_rand=tr)
    (out[3].sum() + out[0].sum()).backward()
    g2 = [p.grad for p in m.parameters()]
    assert any(float((a - b).abs().max()) > 0 for a, b in zip(g1, g2))     # coarse pass now contributes
    with torch.no_grad():
        out = render.render_rays(rays, 2.0, 6.0, m, m, 8, 8, t_rand=tr)
    assert not out[3].requires_grad


def test_pigan_generator_batched_matches_per_image_and_trains():
    """Generator.forward (pi_GAN/modules.py:176-184) renders the batch in one call; it must equal the reference's
    per-image loop (same poses, same jitter) and carry gradients back into the mapping network."""
    from mirender import pigan
    torch.manual_seed(0)
    res, nc, nf, b = 16, 12, 24, 3
    gen = pigan.Generator(32, res, near=0.5, far=1.5, fov=12, coarse_samples=nc, fine_samples=nf).to(dev())
    gen.film_siren_nerf.load_state_dict(synth.state_dict("film_siren_nerf", seed=40, sharp=True))
    z = torch.randn(b, 32, device=dev())
    tr = synth.t_rand(b * res * res, nc, seed=11).to(dev())
    thetas, phis = [0.2, -0.1, 0.05], [0.0, 0.1, -0.05]
    img = gen(z, thetas, phis, t_rand=tr)
    assert tuple(img.shape) == (b, 3, res, res) and img.requires_grad
    # per-image loop like the reference: set_film_params + renderer(...)
    film = gen.get_mapping(z)
    for i in range(b):
        gen.set_film_params(film[i])
        pose = pigan.camera_pos_to_transform_matrix(1, thetas[i], phis[i])
        from mirender import render_core
        one = render_core.render_image_tensor(res, res, gen.renderer.focal, pose, 0.5, 1.5, gen.film_siren_nerf,
                                              gen.film_siren_nerf, nc, nf, t_rand=tr[i * res * res:(i + 1) * res * res])
        assert float((one.permute(2, 0, 1) - img[i]).detach().abs().max()) <= 1e-6
    img.square().mean().backward()
    g = [p.grad for p in gen.mapping_network.parameters()]
    assert all(x is not None and torch.isfinite(x).all() for x in g) and any(float(x.abs().max()) > 0 for x in g)
    assert gen.film_siren_nerf.hidden_layers[3].weight.grad is not None
    # oracle check of the forward image for image 0 (CPU restatement, same weights / film / pose / jitter)
    sd = {k: v.detach().cpu() for k, v in gen.film_siren_nerf.state_dict().items()}
    f = ofields.make_field("film_siren_nerf", sd, film[0].detach().cpu())
    rays = torch.from_numpy(R.rays_from_camera(res, res, gen.renderer.focal,
                                               pigan.camera_pos_to_transform_matrix(1, thetas[0], phis[0])))
    with torch.no_grad():
        ref = R.render_rays(rays, 0.5, 1.5, f, f, nc, nf, tr[:res * res].cpu())
    d = (img[0].permute(1, 2, 0).reshape(-1, 3).detach().cpu() - ref.rgb_f).abs()
    assert float((d > 1e-4).double().mean()) <= 0.05
    # NumPy-RNG pose draws follow the reference's order
    np.random.seed(3)
    a = [np.random.randn() * 0.3, np.random.randn() * 0.15]
    np.random.seed(3)
    pose = gen.renderer.sample_pose()
    assert np.array_equal(pose, pigan.camera_pos_to_transform_matrix(1, a[0], a[1]))


@pytest.mark.parametrize("kind", ["nerf", "film_siren_nerf"])
def test_partial_save_and_recompute_give_the_same_gradients(kind, monkeypatch):
    """The forward keeps layer inputs for as many ray ranges as its budget holds and backward recomputes the rest:
    all kept, none kept and a mix must agree (the split into ranges is the same in all three, so the sums are too)."""
    from mirender import autograd, fields, render_core
    sd = synth.state_dict(kind, seed=33)
    m = fields.field_from_state_dict(sd, dev())
    film = synth.film_params(4, seed=2).to(dev()).requires_grad_(True) if kind.startswith("film") else None
    n, nc, nf = 4 * 96, 8, 16
    rays = torch.from_numpy(R.rays_from_camera(24, 16, 33.3, synth.pose_degrees(4.0 if film is None else 1.0, 20.0, -30.0))[:n]).to(dev())
    near, far = (2.0, 6.0) if film is None else (0.5, 1.5)
    tr = synth.t_rand(n, nc, seed=5).to(dev())
    lib_acts = 4 * autograd._lib.load().mi_field_train_acts_floats(fields.as_packed_field(m).kind)
    per_range = 96 * (nc + nf)                              # points per range: 4 ranges per fine pass
    monkeypatch.setattr(autograd, "_max_points_per_chunk", lambda pf: per_range)
    results = []
    for budget_ranges in (4, 0, 2):
        monkeypatch.setattr(autograd, "SAVE_FINE_BYTES", lib_acts * per_range * budget_ranges)
        monkeypatch.setattr(autograd, "SAVE_COARSE_BYTES", 1 << 40 if budget_ranges == 4 else 0)
        for p in m.parameters():
            p.grad = None
        if film is not None:
            film.grad = None
        out = render_core.render_rays(rays, near, far, m, m, nc, nf, t_rand=tr, film=film)
        (out[3].square().mean() + out[0].mean() + out[5].mean()).backward()
        results.append([p.grad.clone() for p in m.parameters()] + ([] if film is None else [film.grad.clone()]))
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a, b)
    # ranges smaller than one FiLM image (an image split into parts): same gradients up to the order of the sums
    monkeypatch.setattr(autograd, "_max_points_per_chunk", lambda pf: 40 * (nc + nf))
    monkeypatch.setattr(autograd, "SAVE_FINE_BYTES", lib_acts * 32 * (nc + nf) * 5)       # keeps 5 of the 12 parts
    for p in m.parameters():
        p.grad = None
    if film is not None:
        film.grad = None
    out = render_core.render_rays(rays, near, far, m, m, nc, nf, t_rand=tr, film=film)
    (out[3].square().mean() + out[0].mean() + out[5].mean()).backward()
    split = [p.grad.clone() for p in m.parameters()] + ([] if film is None else [film.grad.clone()])
    for a, b in zip(results[0], split):
        assert float((a - b).abs().max()) <= 2e-5 * max(1e-3, float(a.abs().max()))


@pytest.mark.parametrize("fail_at", [3, 4])
def test_out_of_memory_in_backward_falls_back_to_recompute(monkeypatch, fail_at):
    """the forward's save budget is an estimate of what the allocator can still give; if backward cannot
    allocate a range's gradient rows next to the kept layer inputs, it gives the remaining kept inputs back and
    recomputes them (same gradients bit for bit) instead of failing in the middle of the pass.
    fail_at = 3: the second range's FIRST allocation fails.  fail_at = 4: its SECOND one does, i.e. the
    range's gradient rows had already been allocated - the retry must start with them released (it runs outside the
    `except` block: inside it the exception's traceback would keep the failed call's frame, and those rows, alive exactly
    when memory is shortest)."""
    import weakref
    from mirender import autograd, fields, render_core
    m = fields.field_from_state_dict(synth.state_dict("film_siren_nerf", seed=34), dev())
    film = synth.film_params(4, seed=3).to(dev()).requires_grad_(True)
    n, nc, nf = 4 * 96, 8, 16
    rays = torch.from_numpy(R.rays_from_camera(24, 16, 33.3, synth.pose_degrees(1.0, 20.0, -30.0))[:n]).to(dev())
    tr = synth.t_rand(n, nc, seed=6).to(dev())
    monkeypatch.setattr(autograd, "_max_points_per_chunk", lambda pf: 96 * (nc + nf))      # 4 ranges, all kept
    results, real, calls = [], autograd._guarded, {"n": 0, "raised": 0, "rows": None, "rows_alive_at_retry": None}

    def flaky(nfloats, d):
        calls["n"] += 1
        if calls["armed"] and calls["n"] == fail_at:
            calls["raised"] += 1
            raise torch.cuda.OutOfMemoryError("injected by the test")
        if calls["armed"] and calls["n"] == fail_at + 1:     # the retry's first allocation
            calls["rows_alive_at_retry"] = calls["rows"] is not None and calls["rows"]() is not None
        out = real(nfloats, d)
        if calls["armed"] and calls["n"] == 3:               # the second range's gradient rows
            calls["rows"] = weakref.ref(out[0])
        return out
    monkeypatch.setattr(autograd, "_guarded", flaky)
    for armed in (False, True):
        calls.update(n=0, armed=False)
        for p in m.parameters():
            p.grad = None
        film.grad = None
        out = render_core.render_rays(rays, 0.5, 1.5, m, m, nc, nf, t_rand=tr, film=film)
        calls.update(n=0, armed=armed)                       # count (and fail) backward's allocations only
        out[3].square().mean().backward()
        results.append([p.grad.clone() for p in m.parameters()] + [film.grad.clone()])
    assert calls["raised"] == 1
    if fail_at == 4:
        assert calls["rows_alive_at_retry"] is False          # the failed attempt's rows were released before the retry
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_film_parameter_optimisation_through_generator_render():
    """pi_GAN/synthesis.py:83-107: GAN inversion optimises ONE image's FiLM parameters directly (a [9,512] leaf,
    Adam lr 1e-4 there) through `generator.set_film_params(film_params); generator.render(0, 0)` and a second render at
    a random pose.  Same loop here: through the reference-shaped calls (seeded jitter), and - with the jitter injected -
    against the same loop on CPU autograd through the oracle: losses within 1 %, optimised FiLM parameters within 1e-3."""
    from mirender import pigan, render_core
    torch.manual_seed(0)
    res, nc, nf = 12, 6, 12
    gen = pigan.Generator(32, res, near=0.5, far=1.5, fov=12, coarse_samples=nc, fine_samples=nf).to(dev())
    sd = synth.state_dict("film_siren_nerf", seed=40, sharp="medium")
    gen.film_siren_nerf.load_state_dict(sd)
    film0 = synth.film_params(2, seed=9)
    pose0 = pigan.camera_pos_to_transform_matrix(1, 0, 0)
    focal = gen.renderer.focal
    rays0 = torch.from_numpy(R.rays_from_camera(res, res, focal, pose0))
    tr = [synth.t_rand(res * res, nc, seed=700 + i) for i in range(8)]
    with torch.no_grad():                                   # the image to invert: another FiLM table's render
        f_t = ofields.make_field("film_siren_nerf", sd, film0[1])
        target = R.render_rays(rays0, 0.5, 1.5, f_t, f_t, nc, nf, synth.t_rand(res * res, nc, seed=699)).rgb_f.reshape(res, res, 3)

    # (a) the reference-shaped loop: set_film_params + render(0, 0) + render() at a NumPy-drawn pose
    film = film0[0].clone().to(dev()).requires_grad_(True)           # synthesis.py:83-84
    opt = torch.optim.Adam(params=[film], lr=3e-3)
    np.random.seed(1)
    losses = []
    for step in range(8):
        gen.set_film_params(film)
        torch.manual_seed(step)
        image = gen.render(0, 0)
        rec = torch.mean((image - target.to(dev())) ** 2)
        other = gen.render().mean()                                   # stand-in for the discriminator term
        loss = 1e2 * rec + 0.1 * other
        opt.zero_grad()
        loss.backward()
        assert film.grad is not None and bool(torch.isfinite(film.grad).all()) and float(film.grad.abs().max()) > 0
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < 0.8 * losses[0], losses

    # (b) the reconstruction term with injected jitter, HIP vs CPU autograd through the oracle
    def run(hip):
        film = (film0[0].clone().to(dev()) if hip else film0[0].clone()).requires_grad_(True)
        opt = torch.optim.Adam(params=[film], lr=3e-3)
        out = []
        for step in range(8):
            if hip:
                gen.set_film_params(film)
                image = render_core.render_image_tensor(res, res, focal, pose0, 0.5, 1.5, gen.film_siren_nerf,
                                                        gen.film_siren_nerf, nc, nf, t_rand=tr[step].to(dev()))
                loss = 1e2 * torch.mean((image - target.to(dev())) ** 2)
            else:
                f = ofields.make_field("film_siren_nerf", sd, film)
                image = R.render_rays(rays0, 0.5, 1.5, f, f, nc, nf, tr[step]).rgb_f.reshape(res, res, 3)
                loss = 1e2 * torch.mean((image - target) ** 2)
            opt.zero_grad()
            loss.backward()
            opt.step()
            out.append(float(loss.detach()))
        return out, film.detach().cpu()
    l_hip, f_hip = run(True)
    l_cpu, f_cpu = run(False)
    for a, b in zip(l_hip, l_cpu):
        assert abs(a - b) <= 1e-2 * abs(b), (l_hip, l_cpu)
    assert float((f_hip - f_cpu).norm() / (f_cpu - film0[0]).norm()) <= 2e-2       # relative to how far Adam moved them
    assert float((f_hip - f_cpu).abs().max()) <= 1e-3

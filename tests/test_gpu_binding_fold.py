"""GPU: one autograd Function per training path (DESIGN.md 4.3 "Python", 4.8).  Ray gradients are a property of the call - rays
that require grad - not of a subclass, so what the tests of the three surfaces hold bit for bit is held here launch for launch;
and the two changes that came with the fold: the grid path refuses a backward over weights that moved since its forward, and
the merged backwards refuse to be differentiated twice.

The smallest shapes at which tiles and lists are partial: 37 rays, Nc = 8, Nf = 16 (296 and 888 points), a TinyNeRF pair and
one TinyNeRF for both passes, a grid of 5 x 6 x 7 cells with a ball occupied, so both counts lie strictly inside (0, capacity).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import occupancy_train_ref as tref  # noqa: E402
from oracle import render_ref as R, synth  # noqa: E402

NEAR, FAR = 2.0, 6.0
N, NC, NF = 37, 8, 16
BOX = ((-4.0,) * 3, (4.0,) * 3)              # holds every sample of the rays below (camera at radius 4, depths 2..6)
DIMS, BALL_RADIUS = (5, 6, 7), 1.7
RAY_LAUNCHES = ("mi_composite_bwd_rays", "mi_field_input_grad_rays", "mi_field_input_grad")


def dev():
    return torch.device("cuda", 0)


def rays_of(n=N, grad=False):
    r = torch.from_numpy(R.rays_from_camera(40, 40, 55.0, synth.pose_degrees(4.0, 20.0, -30.0)))
    idx = (torch.arange(n) * 1600 // n + 20) % 1600
    return r[idx].contiguous().to(dev()).requires_grad_(grad)


def models_of(shape):
    """Fresh modules (the tests move their weights): "pair" = two TinyNeRFs, "shared" = one for both passes."""
    from mirender import fields
    make = lambda seed: fields.field_from_state_dict(synth.state_dict("tiny_nerf", seed=seed, sharp="medium", bias_jitter=0.05), dev())  # noqa: E731
    mc = make(5)
    return (mc, mc) if shape == "shared" else (mc, make(6))


def ball_grid():
    """The cells of DIMS over BOX whose centre lies within BALL_RADIUS of the origin."""
    from mirender import occupancy
    axes = [(np.arange(d) + 0.5) * (BOX[1][k] - BOX[0][k]) / d + BOX[0][k] for k, d in enumerate(DIMS)]
    x, y, z = np.meshgrid(*axes, indexing="ij")
    dense = x * x + y * y + z * z <= BALL_RADIUS ** 2
    assert 0 < dense.sum() < dense.size
    return occupancy.OccupancyGrid.from_dense(dense, BOX[0], BOX[1], dev())


def t_rand():
    return synth.t_rand(N, NC, seed=9).to(dev())


def loss_of(outs):
    return sum((o * c.to(dev())).sum() for o, c in zip(outs, tref.case_cots(N)))


def surfaces(mc, mf, grid):
    """name -> fn(rays) -> the six outputs, every surface of a training call over this pair."""
    from mirender import occupancy_train, pose, render_core
    a, kw = (NEAR, FAR, mc, mf, NC, NF), dict(t_rand=t_rand())
    return {"render_core": lambda rays: render_core.render_rays(rays, *a, **kw),
            "occupancy_train": lambda rays: occupancy_train.render_rays(rays, *a, grid=grid, **kw),
            "pose": lambda rays: pose.render_rays(rays, *a, **kw),
            "pose_grid": lambda rays: pose.render_rays(rays, *a, grid=grid, **kw)}


@pytest.fixture
def calls(monkeypatch):
    """The names that pass through _lib.call from here on, in order."""
    from mirender import _lib
    names, real = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", recording)
    return names


def step(fn, rays, calls, models):
    """One training step (forward, loss, backward): the names it sent through _lib.call."""
    for m in models:
        m.zero_grad(set_to_none=True)
    rays.grad = None
    del calls[:]
    loss_of(fn(rays)).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for m in models for p in m.parameters())
    return list(calls)


def test_the_grid_lists_part_of_each_pass():
    from mirender import occupancy_train
    for shape in ("pair", "shared"):
        mc, mf = models_of(shape)
        _, counts = occupancy_train.render_rays(rays_of(), NEAR, FAR, mc, mf, NC, NF, grid=ball_grid(), t_rand=t_rand(),
                                                return_counts=True)
        (c, f), = counts.tolist()
        assert 0 < c < N * NC and 0 < f < N * (NC + NF), (shape, c, f)


@pytest.mark.parametrize("shape", ["pair", "shared"])
def test_ray_gradient_launches_only_when_asked(shape, calls):
    mc, mf = models_of(shape)
    run = surfaces(mc, mf, ball_grid())
    plain_rays, grad_rays = rays_of(), rays_of(grad=True)
    for name in ("render_core", "occupancy_train"):                 # the first steps pack the weight streams
        step(run[name], plain_rays, calls, (mc, mf))
    plain = step(run["render_core"], plain_rays, calls, (mc, mf))
    assert "mi_field_backward" in plain and "mi_composite_bwd" in plain
    assert not set(plain) & set(RAY_LAUNCHES), plain
    with_grid = step(run["occupancy_train"], plain_rays, calls, (mc, mf))
    assert with_grid.count("mi_render_rays_occupancy_train") == 1 and with_grid.count("mi_render_rays_occupancy_backward") == 1
    assert "mi_render_rays_occupancy_backward_rays" not in with_grid
    # pose on rays that ask for nothing: the two lists above
    assert step(run["pose"], plain_rays, calls, (mc, mf)) == plain
    assert step(run["pose_grid"], plain_rays, calls, (mc, mf)) == with_grid
    # ... and on rays that require grad: the ray forms
    asked = step(run["pose"], grad_rays, calls, (mc, mf))
    assert "mi_composite_bwd_rays" in asked and "mi_field_input_grad_rays" in asked
    assert [c for c in asked if c not in RAY_LAUNCHES] == plain     # the same calls otherwise
    g = grad_rays.grad
    assert g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any())
    asked = step(run["pose_grid"], grad_rays, calls, (mc, mf))
    assert asked == [c + "_rays" if c == "mi_render_rays_occupancy_backward" else c for c in with_grid]
    g = grad_rays.grad
    assert g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any())


@pytest.mark.parametrize("change", ["add_", "fused_adam"])
@pytest.mark.parametrize("surface", ["occupancy_train", "pose_grid"])
@pytest.mark.parametrize("shape", ["pair", "shared"])
def test_stale_weights_are_refused_on_the_grid_path(shape, surface, change, calls):
    from mirender import train
    mc, mf = models_of(shape)
    fn = surfaces(mc, mf, ball_grid())[surface]
    rays = rays_of(grad=surface == "pose_grid")
    loss_of(fn(rays)).backward()                                    # the untouched control backpropagates
    assert all(p.grad is not None for p in mc.parameters())
    loss = loss_of(fn(rays))
    if change == "add_":
        with torch.no_grad():
            next(iter(mf.parameters())).add_(0)
    else:
        train.FusedAdam([mc] if mc is mf else [mc, mf]).step()
    del calls[:]
    with pytest.raises(RuntimeError, match="modified in place"):
        loss.backward()
    assert calls == []                                              # refused before anything was launched
    loss_of(fn(rays)).backward()                                    # a forward over the new weights is fine again


def test_double_backward_is_refused():
    from mirender import render_core
    mc, mf = models_of("pair")
    params = list(mc.parameters()) + list(mf.parameters())
    outs = render_core.render_rays(rays_of(), NEAR, FAR, mc, mf, NC, NF, t_rand=t_rand())
    first = torch.autograd.grad((outs[3] ** 2).sum() + (outs[0] ** 2).sum(), params, create_graph=True)
    assert all(bool(torch.isfinite(g).all()) for g in first)
    assert all(g.requires_grad for g in first)                      # they look differentiable; what stands behind them refuses
    with pytest.raises(RuntimeError, match="differentiate twice"):
        sum((g ** 2).sum() for g in first).backward()

"""CPU: the binding's two rules for calls under stream capture, with torch.cuda.is_current_stream_capturing patched to True.

1 the workspace rule (ops._workspace): a call under capture gets a fresh buffer of exactly the requested size and neither reads
  nor fills ops._Workspace's cache - a cached buffer's address baked into a graph is freed under it by the next larger call or
  by _Workspace.release().
2 the refusals (_lib.refuse_capture): FusedAdam.step, LiveOccupancyGrid.update and every render call that would draw a fresh
  host seed raise MiRenderError by name BEFORE their first _lib.call / _lib.query and before anything is allocated - each hands
  the library a host value (a step count, an epoch, a seed) that a replay would silently repeat.

The GPU halves are tests/test_gpu_graph_train.py and tests/test_gpu_graph_occupancy.py.
"""
import types

import pytest
import torch

from mirender import _lib, occupancy, occupancy_train, ops, pose, render_core, train


@pytest.fixture
def capturing(monkeypatch):
    """A host on which the current stream is being captured and any launch, size query or seed draw fails the test."""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)

    def no(what):
        def fail(*a, **k):
            pytest.fail(f"{what} reached under capture")
        return fail
    monkeypatch.setattr(_lib, "call", no("_lib.call"))
    monkeypatch.setattr(_lib, "query", no("_lib.query"))
    monkeypatch.setattr(_lib, "load", no("_lib.load"))
    monkeypatch.setattr(render_core, "_fresh_seed", no("the host seed draw"))


def test_workspace_under_capture_is_fresh_exact_and_never_cached(monkeypatch, capturing):
    monkeypatch.delenv("MI_DEBUG_GUARDS", raising=False)
    kept = torch.empty(4096, dtype=torch.uint8)
    monkeypatch.setattr(ops._Workspace, "bufs", {("cpu", 0): kept})
    monkeypatch.setattr(ops._Workspace, "get", classmethod(lambda cls, device, nbytes: pytest.fail("the cache was consulted under capture")))
    for nbytes in (100, 4096, 10000):                        # below, at and above what the cache holds
        ws, guard = ops._workspace("cpu", nbytes)
        assert guard is None and ws is not kept and ws.data_ptr() != kept.data_ptr()
        assert ws.dtype == torch.uint8 and ws.numel() == nbytes
        assert list(ops._Workspace.bufs.items()) == [(("cpu", 0), kept)] and ops._Workspace.bufs[("cpu", 0)] is kept


def test_workspace_outside_capture_comes_from_the_cache(monkeypatch):
    monkeypatch.delenv("MI_DEBUG_GUARDS", raising=False)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    kept = torch.empty(4096, dtype=torch.uint8)
    monkeypatch.setattr(ops._Workspace, "get", classmethod(lambda cls, device, nbytes: kept))
    ws, guard = ops._workspace("cpu", 100)
    assert ws is kept and guard is None


def test_fused_adam_step_refuses_before_it_touches_anything(capturing):
    opt = object.__new__(train.FusedAdam)                    # no field, no state: the check has to come before it needs either
    with pytest.raises(_lib.MiRenderError, match=r"FusedAdam\.step cannot be captured into a graph: the step count"):
        opt.step()


def test_live_grid_update_refuses_before_it_touches_anything(capturing):
    live = object.__new__(occupancy.LiveOccupancyGrid)
    with pytest.raises(_lib.MiRenderError, match=r"LiveOccupancyGrid\.update cannot be captured into a graph: the epoch"):
        live.update(None)


RAYS = torch.zeros(4, 2, 3)
PF = types.SimpleNamespace(device="cpu")                     # as much of a PackedField as _render_calls reads before its check
UNSEEDED = {
    "render_core.render_rays": lambda **kw: render_core.render_rays(RAYS, 2.0, 6.0, None, None, 8, 16, **kw),
    "render_core.render_image": lambda **kw: render_core.render_image(4, 4, 5.0, None, 2.0, 6.0, None, None, 8, 16, **kw),
    "render_core.render_image_tensor": lambda **kw: render_core.render_image_tensor(4, 4, 5.0, None, 2.0, 6.0, None, None, 8, 16, **kw),
    "occupancy_train.render_rays": lambda **kw: occupancy_train.render_rays(RAYS, 2.0, 6.0, None, None, 8, 16, grid=None, **kw),
    "occupancy_train._render_calls": lambda seed=None, t_rand=None: occupancy_train._render_calls(
        PF, PF, RAYS, 2.0, 6.0, 8, 16, None, t_rand, seed, 0, None, None, 1),
    "pose.render_rays": lambda **kw: pose.render_rays(RAYS, 2.0, 6.0, None, None, 8, 16, **kw),
    "pose.render_rays(grid=)": lambda **kw: pose.render_rays(RAYS, 2.0, 6.0, None, None, 8, 16, grid=object(), **kw),
    "pose.render_image_tensor": lambda **kw: pose.render_image_tensor(4, 4, 5.0, None, 2.0, 6.0, None, None, 8, 16, **kw),
}


@pytest.mark.parametrize("name", sorted(UNSEEDED))
def test_a_render_call_that_would_draw_a_host_seed_refuses(capturing, name):
    with pytest.raises(_lib.MiRenderError, match="cannot be captured into a graph: with neither seed= nor t_rand="):
        UNSEEDED[name]()


@pytest.mark.parametrize("name", sorted(UNSEEDED))
@pytest.mark.parametrize("jitter", ["seed", "t_rand"])
def test_an_explicit_seed_or_t_rand_is_not_refused(capturing, name, jitter):
    """seed= and t_rand= stay allowed under capture: the call goes past the check (and here, on a host without a device and with
    models that are none, fails on something else)."""
    kw = dict(seed=5) if jitter == "seed" else dict(t_rand=torch.zeros(4, 8))
    with pytest.raises(Exception) as e:
        UNSEEDED[name](**kw)
    assert "cannot be captured" not in str(e.value)

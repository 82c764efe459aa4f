"""GPU: what mi_render_rays (csrc/render_path.hip) does that no other test pins, bit for bit.

* One field with Nf = 0, where the fine pass IS the coarse pass: Nc = 1 and 2 (legitimate there only) and 5, over 130 rays (Nc = 1:
  two point tiles, the second with two points), NeRF and FilmSirenNeRF (2 groups of 65 rays).  The fine outputs are mi_composite
  of mi_field_eval_rays' raw at mi_sample_coarse's depths, the coarse outputs are copies of them, and a call that asks for no
  coarse output gives the same fine outputs.
* mi_render_set_mlp_events: the four events bracket the two field passes in stream order.

One field with Nf > 0 in a workspace with and without the shared-field regions (new samples + merge against the whole fine pass)
is tests/test_gpu_shared_field.py::test_shared_field_inference_equals_evaluating_every_point, which compares all six outputs.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import render_ref as R, synth  # noqa: E402

N = 130


def dev():
    return torch.device("cuda", 0)


def _field(kind, seed):
    from mirender import fields
    m = fields.field_from_state_dict(synth.state_dict(kind, seed=seed, sharp="medium", bias_jitter=0.05), dev())
    return m, fields.as_packed_field(m)


def _rays(n, film):
    pose = synth.pose_radians(1.0, 0.2, -0.1) if film else synth.pose_degrees(4.0, 20.0, -30.0)
    return torch.from_numpy(R.rays_from_camera(40, 40, 180.0 if film else 55.0, pose)[:n]).to(dev())


def _outs(n, count):
    return [torch.full(s, float("nan"), dtype=torch.float32, device=dev()) for s in ((n, 3), (n,), (n,))[:3] * count]


@pytest.mark.parametrize("kind", ["nerf", "film_siren_nerf"])
@pytest.mark.parametrize("nc", [1, 2, 5])
def test_one_field_without_new_samples_is_one_composite(kind, nc):
    from mirender import _lib, ops
    lib = _lib.load()
    is_film = kind.startswith("film")
    _, pf = _field(kind, 5)
    groups = 2 if is_film else 1
    film = synth.film_params(groups, seed=3).to(dev()) if is_film else None
    near, far = (0.5, 1.5) if is_film else (2.0, 6.0)
    rays, tr = _rays(N, is_film), synth.t_rand(N, nc, seed=9).to(dev())
    zl, stream, packed = ops.linspace_table(near, far, nc, dev()), _lib.stream_ptr(dev()), _lib.ptr(pf.refresh())
    # the stages, one by one
    z = torch.empty(N, nc, device=dev())
    raw = torch.empty(N, nc, 4, device=dev())
    want = _outs(N, 1)
    assert lib.mi_sample_coarse(N, near, far, nc, _lib.ptr(zl), _lib.ptr(tr), 0, 0, _lib.ptr(z), stream) == 0, lib.mi_last_error()
    assert lib.mi_field_eval_rays(pf.kind, packed, _lib.ptr(film), _lib.ptr(rays), _lib.ptr(z), groups, N // groups, nc, _lib.ptr(raw),
                                  stream) == 0, lib.mi_last_error()
    assert lib.mi_composite(N, nc, _lib.ptr(raw), _lib.ptr(z), _lib.ptr(rays), *[_lib.ptr(o) for o in want], None, stream) == 0, \
        lib.mi_last_error()
    # the fused call, with and without the coarse outputs, in a workspace with and without the shared-field regions
    base = lib.mi_render_workspace_bytes(N, nc, 0)
    for ws_bytes in (base, base + lib.mi_render_shared_field_extra_bytes(N, nc, 0)):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
        for coarse_outputs in (True, False):
            got = _outs(N, 2)
            coarse = [_lib.ptr(o) for o in got[:3]] if coarse_outputs else [None, None, None]
            rc = lib.mi_render_rays(pf.kind, packed, pf.kind, packed, _lib.ptr(film), _lib.ptr(rays), groups, N // groups, near, far,
                                    nc, 0, _lib.ptr(zl), None, _lib.ptr(tr), 0, 0, *coarse, *[_lib.ptr(o) for o in got[3:]],
                                    _lib.ptr(ws), ws_bytes, stream)
            assert rc == 0, lib.mi_last_error()
            for name, w, g_c, g_f in zip(("rgb", "depth", "acc"), want, got[:3], got[3:]):
                assert torch.equal(g_f, w), (name, "fine", coarse_outputs)
                if coarse_outputs:
                    assert torch.equal(g_c, w), (name, "coarse")


def test_mlp_events_bracket_the_two_field_passes():
    from mirender import _lib, ops
    lib = _lib.load()
    n, nc, nf = 256, 8, 8
    (_, pc), (_, pfine) = _field("nerf", 5), _field("nerf", 6)
    rays, tr = _rays(n, False), synth.t_rand(n, nc, seed=2).to(dev())
    zl, ul = ops.linspace_table(2.0, 6.0, nc, dev()), ops.linspace_table(0.0, 1.0, nf, dev())
    ws_bytes = lib.mi_render_workspace_bytes(n, nc, nf)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev())
    outs = _outs(n, 2)
    ev = [lib.mi_event_create() for _ in range(4)]
    try:
        assert all(ev), lib.mi_last_error()
        lib.mi_render_set_mlp_events(*ev)
        rc = lib.mi_render_rays(pc.kind, _lib.ptr(pc.refresh()), pfine.kind, _lib.ptr(pfine.refresh()), None, _lib.ptr(rays), 1, n,
                                2.0, 6.0, nc, nf, _lib.ptr(zl), _lib.ptr(ul), _lib.ptr(tr), 0, 0, *[_lib.ptr(o) for o in outs],
                                _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dev()))
        assert rc == 0, lib.mi_last_error()
        torch.cuda.current_stream(dev()).synchronize()
        ms = []
        for a, b in ((0, 1), (1, 2), (2, 3)):
            t = ctypes.c_float(-1.0)
            assert lib.mi_event_elapsed_ms(ev[a], ev[b], ctypes.byref(t)) == 0, lib.mi_last_error()
            ms.append(t.value)
        print("coarse field, between, fine field [ms]:", ms)
        assert all(t >= 0 for t in ms), ms
        assert ms[0] > 0 and ms[2] > 0, ms
    finally:
        lib.mi_render_set_mlp_events(None, None, None, None)
        for e in ev:
            lib.mi_event_destroy(e)
    assert all(bool(torch.isfinite(o).all()) for o in outs)

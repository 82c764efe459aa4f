"""CPU: the host side of mi_render_rays and of the two backwards' shared checks (csrc/render_path.h).  No GPU, no launch.

* mi_render_rays refuses bad arguments with MI_EINVAL and a message that names it before it launches anything (a launch on
  this machine would come back as MI_EHIP): an unknown kind, a FiLM kind without a table, a workspace one byte short, rgb_c
  without depth_c, and Nc < 3 wherever a fine pass has to be sampled - which it once noticed only after the coarse pass;
* a call without rays returns MI_OK whatever else it is given;
* mi_render_rays_backward and mi_render_rays_occupancy_backward check a field's gradient arrays with one helper: the same
  words, apart from the function's name, for a missing gradient array and for a null gradient pointer, on either field.
"""
import ctypes

from mirender import _lib as binding

MI_EINVAL = -1
FAKE = ctypes.c_void_p(0x10000)        # a non-null "device pointer": every call below must fail before it is used
FAKE2 = ctypes.c_void_p(0x20000)       # a second packed stream: two fields
NERF, FILM = 0, 2
N, NC, NF = 64, 8, 16


def _lib():
    return binding.load()


def _refused(rc, lib, *words):
    msg = lib.mi_last_error()
    assert rc == MI_EINVAL, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)
    return msg


def _render(lib, kind_c=NERF, kind_f=NERF, packed_f=FAKE2, film=None, n=N, nc=NC, nf=NF, rgb_c=FAKE, depth_c=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.mi_render_workspace_bytes(n, nc, nf) + lib.mi_render_shared_field_extra_bytes(n, nc, nf)
    return lib.mi_render_rays(kind_c, FAKE, kind_f, packed_f, film, FAKE, 1, n, 2.0, 6.0, nc, nf, None, None, None, 0, 0,
                              rgb_c, depth_c, FAKE, FAKE, FAKE, FAKE, FAKE, ws_bytes, None)


def test_render_rays_refuses_before_any_launch():
    lib = _lib()
    me = b"mi_render_rays:"
    _refused(_render(lib, kind_c=99), lib, me, b"unknown field kind 99")
    _refused(_render(lib, kind_f=99), lib, me, b"unknown field kind 99")
    _refused(_render(lib, kind_c=FILM), lib, me, b"FiLM kind needs a film table")
    _refused(_render(lib, kind_f=FILM), lib, me, b"FiLM kind needs a film table")
    base = lib.mi_render_workspace_bytes(N, NC, NF)
    _refused(_render(lib, ws_bytes=base - 1), lib, me, b"workspace of", str(base).encode())
    _refused(_render(lib, depth_c=None), lib, me, b"null pointer")                      # rgb_c without depth_c
    _refused(_render(lib, packed_f=None), lib, me, b"null pointer")
    # Nc of 1 or 2 cannot feed sample_pdf: two fields with or without new samples, one field with new samples
    for nc in (1, 2):
        _refused(_render(lib, nc=nc, nf=0), lib, me, b"Nc >= 3")
        _refused(_render(lib, nc=nc, nf=3), lib, me, b"Nc >= 3")
        _refused(_render(lib, packed_f=FAKE, nc=nc, nf=3), lib, me, b"Nc >= 3")
        # ... in a workspace without the shared-field regions too (the whole fine pass is sampled just the same)
        _refused(_render(lib, packed_f=FAKE, nc=nc, nf=3, ws_bytes=lib.mi_render_workspace_bytes(N, nc, 3)), lib, me, b"Nc >= 3")
    _refused(_render(lib, nc=0), lib, me, b"bad sizes")


def test_render_rays_without_rays_returns_ok():
    lib = _lib()
    for groups, rpg in ((0, 100), (3, 0), (0, 0)):
        assert lib.mi_render_rays(NERF, None, NERF, None, None, None, groups, rpg, 2.0, 6.0, NC, NF, None, None, None, 0, 0,
                                  None, None, None, None, None, None, None, 0, None) == 0


def _grads(n_par, present, hole):
    if not present:
        return None
    a = (ctypes.c_void_p * n_par)(*([0x30000] * n_par))
    if hole is not None:
        a[hole] = None
    return a


def _plain_backward(lib, gp_c=True, gp_f=True, hole_c=None, hole_f=None):
    n_par = lib.mi_field_num_params(NERF)
    params = (ctypes.c_void_p * n_par)(*([0x40000] * n_par))
    written = ctypes.c_int(7)
    rc = lib.mi_render_rays_backward(NERF, FAKE, FAKE, params, NERF, FAKE2, FAKE, params, None, FAKE, 1, N, NC, NF, 4096, 4096, FAKE,
                                     lib.mi_render_workspace_bytes(N, NC, NF), None, 0, FAKE, None, None, FAKE, None, None,
                                     _grads(n_par, gp_c, hole_c), _grads(n_par, gp_f, hole_f), None, FAKE, 1 << 40,
                                     ctypes.byref(written), None)
    assert written.value == 0
    return rc


def _occupancy_backward(lib, gp_c=True, gp_f=True, hole_c=None, hole_f=None):
    n_par = lib.mi_field_num_params(NERF)
    written = ctypes.c_int(7)
    rc = lib.mi_render_rays_occupancy_backward(NERF, FAKE, NERF, FAKE, 0, FAKE, N, NC, NF, FAKE, 1 << 40, FAKE, 1 << 40, FAKE, None, None,
                                               FAKE, None, None, _grads(n_par, gp_c, hole_c), _grads(n_par, gp_f, hole_f), FAKE,
                                               1 << 40, ctypes.byref(written), None)
    assert written.value == 0
    return rc


def test_the_two_backwards_word_their_gradient_checks_alike():
    lib = _lib()
    cases = ((dict(gp_c=False), b"the coarse field gets a cotangent but has no gradient array"),
             (dict(gp_f=False), b"the fine field gets a cotangent but has no gradient array"),
             (dict(hole_c=3), b"coarse gradient pointer 3 is null"),
             (dict(hole_f=3), b"fine gradient pointer 3 is null"))
    for kw, words in cases:
        plain = _refused(_plain_backward(lib, **kw), lib, b"mi_render_rays_backward: ", words)
        grid = _refused(_occupancy_backward(lib, **kw), lib, b"mi_render_rays_occupancy_backward: ", words)
        assert plain.split(b": ", 1)[1] == grid.split(b": ", 1)[1], (plain, grid)

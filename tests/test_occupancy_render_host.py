"""CPU: the host side of rendering with an occupancy grid (include/mi_render.h).  No GPU, no launch.

* mi_render_occupancy_extra_bytes against its formula: one list of n * (Nc + Nf) ints and two counts, each region rounded up
  to whole 256-byte blocks;
* mi_occupancy_mark_rays, mi_field_eval_rays_list and mi_render_rays_occupancy refuse bad arguments with MI_EINVAL and a
  message before they launch anything (a launch on this machine would come back as MI_EHIP): a null pointer, bad grid dims, a
  FiLM kind, more than 2^31 - 1 points, a workspace one byte short;
* tests/occupancy_render_ref.py, the torch restatement of "which points are occupied" that tests/test_gpu_occupancy_render.py
  holds the kernels against, is itself checked on cases counted by hand.
"""
import ctypes

import numpy as np
import torch

import occupancy_render_ref as ref
from mirender import _lib as binding

MI_EINVAL = -1
FAKE = ctypes.c_void_p(0x10000)        # a non-null "device pointer": every call below must fail before it is used
NERF, SIREN, FILM, FILM_NODIR, TINY = 0, 1, 2, 3, 4


def _lib():
    return binding.load()


def _i3(*v):
    return (ctypes.c_int * 3)(*v)


def _f3(*v):
    return (ctypes.c_float * 3)(*v)


def _refused(rc, lib, *words):
    msg = lib.mi_last_error()
    assert rc == MI_EINVAL, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_extra_bytes_formula():
    lib = _lib()
    for n, nc, nf in ((1, 3, 0), (37, 5, 0), (130, 64, 128), (1000, 64, 128), (640000, 64, 128)):
        want = ((n * (nc + nf) + 63) // 64 * 64 + 64) * 4
        assert lib.mi_render_occupancy_extra_bytes(n, nc, nf) == want, (n, nc, nf)
    assert lib.mi_render_occupancy_extra_bytes(0, 64, 128) == 0
    assert lib.mi_abi_version() == 4


def _render(lib, kind_c=NERF, kind_f=NERF, packed_c=FAKE, rays=FAKE, n=100, nc=8, nf=16, bits=FAKE, dims=None, lo=None,
            inv=None, rgb_c=FAKE, depth_c=FAKE, acc_c=FAKE, rgb_f=FAKE, ws=FAKE, ws_bytes=None):
    dims = _i3(16, 16, 16) if dims is None else dims
    lo = _f3(-1, -1, -1) if lo is None else lo
    inv = _f3(8, 8, 8) if inv is None else inv
    if ws_bytes is None:
        ws_bytes = lib.mi_render_workspace_bytes(n, nc, nf) + lib.mi_render_occupancy_extra_bytes(n, nc, nf)
    return lib.mi_render_rays_occupancy(kind_c, packed_c, kind_f, FAKE, rays, n, 2.0, 6.0, nc, nf, None, None, None, 0, 0, bits,
                                        dims, lo, inv, rgb_c, depth_c, acc_c, rgb_f, FAKE, FAKE, None, ws, ws_bytes, None)


def test_render_argument_checks():
    lib = _lib()
    _refused(_render(lib, packed_c=None), lib, b"null pointer")
    _refused(_render(lib, rays=None), lib, b"null pointer")
    _refused(_render(lib, bits=None), lib, b"null pointer")
    _refused(_render(lib, rgb_f=None), lib, b"null pointer")
    _refused(_render(lib, ws=None), lib, b"null pointer")
    _refused(_render(lib, depth_c=None), lib, b"null pointer")              # rgb_c without depth_c
    _refused(_render(lib, lo=ctypes.POINTER(ctypes.c_float)()), lib, b"null pointer")
    _refused(_render(lib, dims=ctypes.POINTER(ctypes.c_int)()), lib, b"null grid dims")
    _refused(_render(lib, dims=_i3(0, 16, 16)), lib, b"grid dims")
    _refused(_render(lib, dims=_i3(2048, 2048, 512)), lib, b"2^31 cells")
    for kc, kf in ((FILM, NERF), (NERF, FILM_NODIR), (FILM, FILM)):
        _refused(_render(lib, kind_c=kc, kind_f=kf), lib, b"FiLM")
    _refused(_render(lib, kind_c=99), lib, b"unknown field kind")
    _refused(_render(lib, n=(2 ** 31 - 1) // 192 + 1, nc=64, nf=128, ws_bytes=1 << 60), lib, b"2^31 - 1")
    need = lib.mi_render_workspace_bytes(100, 8, 16) + lib.mi_render_occupancy_extra_bytes(100, 8, 16)
    _refused(_render(lib, ws_bytes=need - 1), lib, b"workspace of", str(need).encode())
    _refused(_render(lib, ws_bytes=lib.mi_render_workspace_bytes(100, 8, 16)), lib, b"workspace of")   # the base alone
    _refused(_render(lib, nc=2), lib, b"bad sizes")
    assert _render(lib, n=0) == 0                                            # no rays: nothing to launch


def test_mark_and_list_argument_checks():
    lib = _lib()
    d, lo, inv = _i3(5, 7, 3), _f3(0, 0, 0), _f3(1, 1, 1)
    mark = lib.mi_occupancy_mark_rays
    _refused(mark(None, d, lo, inv, FAKE, FAKE, 10, 4, FAKE, FAKE, None, None), lib, b"null pointer")
    _refused(mark(FAKE, d, lo, inv, FAKE, FAKE, 10, 4, None, FAKE, None, None), lib, b"null pointer")
    _refused(mark(FAKE, d, lo, inv, FAKE, FAKE, 10, 4, FAKE, None, None, None), lib, b"null pointer")
    _refused(mark(FAKE, _i3(5, 0, 3), lo, inv, FAKE, FAKE, 10, 4, FAKE, FAKE, None, None), lib, b"grid dims")
    _refused(mark(FAKE, d, lo, inv, FAKE, FAKE, 10, 0, FAKE, FAKE, None, None), lib, b"bad sizes")
    _refused(mark(FAKE, d, lo, inv, FAKE, FAKE, (2 ** 31 - 1) // 192 + 1, 192, FAKE, FAKE, None, None), lib, b"2^31 - 1")
    ev = lib.mi_field_eval_rays_list
    for kind in (FILM, FILM_NODIR):
        _refused(ev(kind, FAKE, FAKE, FAKE, 10, 4, FAKE, FAKE, FAKE, None), lib, b"no list-driven forward")
    _refused(ev(NERF, FAKE, FAKE, FAKE, 10, 4, None, FAKE, FAKE, None), lib, b"null pointer")
    _refused(ev(SIREN, FAKE, FAKE, FAKE, 10, 4, FAKE, None, FAKE, None), lib, b"null pointer")
    _refused(ev(TINY, FAKE, FAKE, FAKE, (2 ** 31 - 1) // 192 + 1, 192, FAKE, FAKE, FAKE, None), lib, b"2^31 - 1")
    assert ev(NERF, FAKE, FAKE, FAKE, 0, 4, FAKE, FAKE, FAKE, None) == 0     # no rays: nothing to launch


def test_restatement_counted_by_hand():
    dims = (5, 7, 3)
    lo, hi = np.float32([0, 0, 0]), np.float32([5, 7, 3])                   # unit cells: t = p
    inv = ref.inv_cell_of(lo, hi, dims)
    assert np.array_equal(inv, np.float32([1, 1, 1]))
    dense = np.zeros(dims, bool)
    dense[0, 0, 0] = dense[4, 6, 2] = dense[2, 3, 1] = True
    nan = float("nan")
    p = torch.tensor([[0.0, 0.0, 0.0],        # exactly on lo: inside, cell (0, 0, 0), set
                      [5.0, 7.0, 3.0],        # exactly on hi: outside
                      [4.5, 6.5, 3.0],        # on hi along one axis: outside
                      [4.999, 6.999, 2.999],  # the last cell (4, 6, 2), set
                      [2.5, 3.5, 1.5],        # cell (2, 3, 1), set
                      [2.5, 3.5, 0.5],        # cell (2, 3, 0), clear
                      [-1e-7, 0.0, 0.0],      # just below lo: outside (floor would be -1)
                      [nan, 0.0, 0.0],        # NaN: not inside
                      [0.5, nan, 0.5],
                      [float("inf"), 0.0, 0.0],
                      [0.999, 0.999, 0.999]])
    want = [True, False, False, True, True, False, False, False, False, False, True]
    assert ref.occupied_points(p, lo, inv, dense).tolist() == want
    assert not ref.occupied_points(p, lo, inv, np.zeros(dims, bool)).any()
    ones = ref.occupied_points(p, lo, inv, np.ones(dims, bool)).tolist()    # all ones = "inside the box"
    assert ones == [True, False, False, True, True, True, False, False, False, False, True]
    assert ref.cells_of(p, lo, inv, dims).tolist() == [[0, 0, 0], [4, 6, 2], [2, 3, 1], [2, 3, 0], [0, 0, 0]]
    # rays: o = (0.5, 0.5, -1), d = (0, 0, 2): z = 0.5 is exactly on lo (cell iz = 0), z = 2 exactly on hi
    rays = torch.tensor([[[0.5, 0.5, -1.0], [0.0, 0.0, 2.0]]])
    z = torch.tensor([[0.25, 0.5, 0.75, 1.25, 1.75, 2.0]])
    col = np.zeros(dims, bool)
    col[0, 0, 0] = col[0, 0, 2] = True
    assert ref.occupied_mask(rays, z, lo, inv, col).tolist() == [[False, True, True, False, True, False]]
    # a box that does not start at 0, cells 0.5 wide: inv_cell = 2
    lo2, hi2 = np.float32([-1.5, -1.0, 0.25]), np.float32([1.0, 2.5, 1.75])
    inv2 = ref.inv_cell_of(lo2, hi2, dims)
    assert np.array_equal(inv2, np.float32([2, 2, 2]))
    d2 = np.zeros(dims, bool)
    d2[1, 2, 0] = True
    q = torch.tensor([[-1.0, 0.0, 0.25], [-0.75, 0.25, 0.5], [-0.5, 0.0, 0.25], [-1.0, 0.5, 0.25]])
    assert ref.occupied_points(q, lo2, inv2, d2).tolist() == [True, True, False, False]

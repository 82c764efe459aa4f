"""CPU: the host side of occupancy-grid construction (include/mi_render.h, mirender/occupancy.py).  No GPU, no launch.

* the construction calls refuse bad arguments before they launch anything: bad grid dims, null dims, a sub-sample count out of
  range, cells past the grid, a workspace one byte short;
* the size queries need no GPU;
* pack_dense / unpack_dense (OccupancyGrid.from_dense / to_dense) round-trip, at dims that are no multiple of a word's 32 bits;
* `dense_reference`, the numpy restatement of mi_occupancy_pack (threshold, 6-neighbourhood dilation clipped at the box),
  which tests/test_gpu_occupancy.py holds the kernel against bit for bit, is itself checked on cases small enough to count
  by hand.
"""
import ctypes

import numpy as np
import pytest

from mirender import _lib as binding

MI_EINVAL = -1
FAKE = ctypes.c_void_p(0x10000)        # a non-null "device pointer": every call below must fail before it is used


def _lib():
    return binding.load()


def _i3(*v):
    return (ctypes.c_int * 3)(*v)


def _f3(*v):
    return (ctypes.c_float * 3)(*v)


def dense_reference(sigma, dims, k, threshold, dilate):
    """mi_occupancy_pack restated: sigma [cells * k^3] (cell-major, cell index (ix * Gy + iy) * Gz + iz) -> bool [Gx,Gy,Gz].
    A cell is occupied iff any sub-sample is strictly above the threshold; then `dilate` steps of 6-neighbourhood dilation,
    clipped at the box."""
    occ = (np.asarray(sigma, dtype=np.float32).reshape(-1, k ** 3) > np.float32(threshold)).any(1).reshape(dims)
    for _ in range(dilate):
        out = occ.copy()
        out[1:] |= occ[:-1]; out[:-1] |= occ[1:]                              # noqa: E702
        out[:, 1:] |= occ[:, :-1]; out[:, :-1] |= occ[:, 1:]                  # noqa: E702
        out[:, :, 1:] |= occ[:, :, :-1]; out[:, :, :-1] |= occ[:, :, 1:]      # noqa: E702
        occ = out
    return occ


@pytest.mark.parametrize("dims", [(0, 16, 16), (16, -1, 16), (2048, 2048, 512), (1 << 30, 2, 1)])
def test_bad_dims_are_refused(dims):
    lib = _lib()
    d = _i3(*dims)
    assert lib.mi_occupancy_words(d) == MI_EINVAL and lib.mi_occupancy_pack_workspace_bytes(d, 1) == MI_EINVAL
    assert lib.mi_occupancy_cell_points(d, _f3(0, 0, 0), _f3(1, 1, 1), 2, 0, 1, FAKE, None) == MI_EINVAL
    assert lib.mi_occupancy_pack(FAKE, d, 2, 0.0, 1, FAKE, FAKE, 1 << 40, None) == MI_EINVAL


def test_construction_arguments():
    lib = _lib()
    d = _i3(3, 5, 7)
    lo, cell = _f3(0, 0, 0), _f3(1, 1, 1)
    assert lib.mi_occupancy_cell_points(d, lo, cell, 0, 0, 1, FAKE, None) == MI_EINVAL           # supersample < 1
    assert lib.mi_occupancy_cell_points(d, lo, cell, 9, 0, 1, FAKE, None) == MI_EINVAL           # ... > 8
    assert lib.mi_occupancy_cell_points(d, lo, cell, 2, 100, 6, FAKE, None) == MI_EINVAL         # past the last cell
    assert lib.mi_occupancy_cell_points(d, lo, cell, 2, 0, 1, None, None) == MI_EINVAL
    assert lib.mi_occupancy_cell_points(d, lo, cell, 2, 105, 0, None, None) == 0                 # no cells: nothing to launch
    need = lib.mi_occupancy_pack_workspace_bytes(d, 1)
    assert lib.mi_occupancy_pack(FAKE, d, 2, 0.0, 1, FAKE, FAKE, need - 1, None) == MI_EINVAL
    assert lib.mi_occupancy_pack(FAKE, d, 2, 0.0, -1, FAKE, FAKE, need, None) == MI_EINVAL
    assert lib.mi_occupancy_pack(None, d, 2, 0.0, 1, FAKE, FAKE, need, None) == MI_EINVAL


def test_size_queries_need_no_gpu():
    lib = _lib()
    assert lib.mi_occupancy_words(_i3(1, 1, 1)) == 1 and lib.mi_occupancy_words(_i3(3, 5, 7)) == 4
    assert lib.mi_occupancy_words(_i3(33, 2, 2)) == 5 and lib.mi_occupancy_words(_i3(128, 128, 128)) == 65536
    assert lib.mi_occupancy_words(_i3(2048, 2048, 511)) == 2048 * 2048 * 511 // 32
    # one byte per cell, twice with dilation (ping-pong), in whole 256-byte blocks
    assert lib.mi_occupancy_pack_workspace_bytes(_i3(3, 5, 7), 0) == 256 and lib.mi_occupancy_pack_workspace_bytes(_i3(3, 5, 7), 2) == 512
    assert lib.mi_occupancy_pack_workspace_bytes(_i3(16, 16, 16), 1) == 2 * 4096
    assert lib.mi_occupancy_words(ctypes.POINTER(ctypes.c_int)()) == MI_EINVAL and b"null grid dims" in lib.mi_last_error()
    assert lib.mi_abi_version() == 4


@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 5, 7), (33, 2, 2)])
def test_pack_and_unpack_round_trip(dims):
    from mirender import occupancy
    rng = np.random.Generator(np.random.PCG64(7))
    for dense in (rng.random(dims) < 0.5, np.ones(dims, bool), np.zeros(dims, bool)):
        words = occupancy.pack_dense(dense)
        assert words.dtype == np.uint32 and words.size == (dense.size + 31) // 32
        flat = dense.reshape(-1)
        for i in range(flat.size):                              # the documented position of every cell's bit
            assert bool((int(words[i >> 5]) >> (i & 31)) & 1) == bool(flat[i])
        if dense.size % 32:
            assert int(words[-1]) >> (dense.size % 32) == 0      # spare bits of the last word
        assert np.array_equal(occupancy.unpack_dense(words, dims), dense)


def test_dense_reference_counted_by_hand():
    dims, k = (3, 5, 7), 2
    sig = np.zeros((105, 8), np.float32)
    sig[0, 5] = 1.0                                             # one hot sub-sample in the corner cell (0, 0, 0)
    assert dense_reference(sig, dims, k, 0.0, 0).sum() == 1
    assert dense_reference(sig, dims, k, 1.0, 0).sum() == 0     # strict >: a value equal to the threshold is not above it
    d1 = dense_reference(sig, dims, k, 0.0, 1)
    assert d1.sum() == 4 and d1[0, 0, 0] and d1[1, 0, 0] and d1[0, 1, 0] and d1[0, 0, 1]      # clipped at three faces
    assert dense_reference(sig, dims, k, 0.0, 2).sum() == 10    # |i| + |j| + |l| <= 2 inside the box
    mid = np.zeros((105, 8), np.float32)
    mid[(1 * 5 + 2) * 7 + 3, 0] = 2.0                           # cell (1, 2, 3): nothing clipped
    assert dense_reference(mid, dims, k, 0.0, 1).sum() == 7
    # (33, 2, 2): dilation along the short axes saturates at once
    line = np.zeros((132, 1), np.float32)
    line[(16 * 2 + 0) * 2 + 0] = 1.0
    d = dense_reference(line, (33, 2, 2), 1, 0.5, 1)
    assert d.sum() == 5 and d[15, 0, 0] and d[17, 0, 0] and d[16, 1, 0] and d[16, 0, 1] and not d[16, 1, 1]

"""CPU: the host side of a live occupancy grid (include/mi_render.h "a live grid").  No GPU, no launch.

* Philox4x32-10 of tests/occupancy_live_ref.py against the published known answers;
* mi_occupancy_draw_points / _density_update / _density_pack refuse every bad argument before they launch anything, and
  mi_occupancy_density_workspace_bytes answers its documented formula;
* the inputs tests/test_gpu_occupancy_live.py runs the kernels on have the properties that make those tests mean something;
* the comparison that file uses (bit equality against the restatement) rejects five planted mistakes on those inputs.
"""
import ctypes

import numpy as np
import pytest

import occupancy_live_ref as ref
from mirender import _lib as binding

MI_EINVAL = -1
FAKE = ctypes.c_void_p(0x10000)        # a non-null "device pointer": every call below must fail before it is used
NAN = float("nan")


def _lib():
    return binding.load()


def _i3(*v):
    return (ctypes.c_int * 3)(*v)


def _f3(*v):
    return (ctypes.c_float * 3)(*v)


# ---- Philox ------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    assert ref.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert ref.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_stream_words_are_the_blocks_in_order():
    seed, stream = 0x299F31D0A4093822, 0x85A308D3243F6A88
    w = ref.stream_words(seed, stream, 12)
    for j in range(3):
        assert w[4 * j:4 * j + 4] == ref.philox4x32_10((0x243F6A88, 0x85A308D3, j, 0), (0xA4093822, 0x299F31D0))
    assert ref.stream_words(seed, stream, 5) == w[:5]


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def _draw(lib, **kw):
    a = dict(bits=FAKE, dims=_i3(3, 5, 7), lo=_f3(0, 0, 0), cell=_f3(1, 1, 1), seed=1, epoch=0, mode=1, row0=0, count=10,
             n_uniform=5, cell_ids=FAKE, points=FAKE)
    a.update(kw)
    return lib.mi_occupancy_draw_points(*a.values(), None)


@pytest.mark.parametrize("dims", [(0, 16, 16), (16, -1, 16), (2048, 2048, 512), (1 << 30, 2, 1)])
def test_bad_dims_are_refused(dims):
    lib = _lib()
    d = _i3(*dims)
    assert lib.mi_occupancy_density_workspace_bytes(d, 0) == MI_EINVAL
    assert _draw(lib, dims=d) == MI_EINVAL
    assert lib.mi_occupancy_density_update(FAKE, FAKE, 1, d, 0.95, FAKE, FAKE, 1 << 40, None) == MI_EINVAL
    assert lib.mi_occupancy_density_pack(FAKE, d, 0.01, 1, 0, FAKE, FAKE, 1 << 40, None) == MI_EINVAL
    null = ctypes.POINTER(ctypes.c_int)()
    assert lib.mi_occupancy_density_workspace_bytes(null, 0) == MI_EINVAL and _draw(lib, dims=null) == MI_EINVAL


def test_draw_arguments():
    lib = _lib()
    for bad in (dict(lo=None), dict(cell=None), dict(cell_ids=None), dict(points=None), dict(bits=None), dict(count=-1),
                dict(row0=-1), dict(n_uniform=-1), dict(mode=2), dict(mode=-1),
                dict(mode=0, row0=100, count=6),                       # a sweep past the last of the 105 cells
                dict(row0=(1 << 31) - 9, count=10),                    # rows past 2^31, in draw mode too
                dict(row0=1 << 62, count=1 << 62)):
        assert _draw(lib, **bad) == MI_EINVAL, bad
        assert lib.mi_last_error().startswith(b"mi_occupancy_draw_points")
    # bits may be null where no row reads it; count == 0 is a no-op
    assert _draw(lib, bits=None, mode=0, count=0) == 0 and _draw(lib, bits=None, n_uniform=10, count=0) == 0
    assert _draw(lib, bits=None, n_uniform=9, row0=9, count=0) == 0
    assert _draw(lib, bits=None, n_uniform=9, row0=9, count=1) == MI_EINVAL          # row 9 is an occupied-share row
    assert _draw(lib, count=0) == 0 and _draw(lib, mode=0, row0=105, count=0) == 0


def test_density_update_arguments():
    lib = _lib()
    d = _i3(3, 5, 7)
    need = lib.mi_occupancy_density_workspace_bytes(d, 0)

    def update(sigma=FAKE, ids=FAKE, count=10, decay=0.95, density=FAKE, ws=FAKE, ws_bytes=need):
        return lib.mi_occupancy_density_update(sigma, ids, count, d, decay, density, ws, ws_bytes, None)
    for bad in (dict(sigma=None), dict(ids=None), dict(density=None), dict(ws=None), dict(count=-1), dict(decay=-0.01),
                dict(decay=1.01), dict(decay=NAN), dict(decay=float("inf")), dict(ws_bytes=need - 1)):
        assert update(**bad) == MI_EINVAL, bad
        assert lib.mi_last_error().startswith(b"mi_occupancy_density_update")
    assert update(count=0) == 0 and update(count=0, decay=0.0) == 0 and update(count=0, decay=1.0) == 0


def test_density_pack_arguments():
    lib = _lib()
    d = _i3(3, 5, 7)
    for dilate in (0, 2):
        need = lib.mi_occupancy_density_workspace_bytes(d, dilate)
        assert lib.mi_occupancy_density_pack(FAKE, d, 0.01, 1, dilate, FAKE, FAKE, need - 1, None) == MI_EINVAL
        assert b"workspace" in lib.mi_last_error()
    need = lib.mi_occupancy_density_workspace_bytes(d, 1)
    assert lib.mi_occupancy_density_pack(None, d, 0.01, 1, 1, FAKE, FAKE, need, None) == MI_EINVAL
    assert lib.mi_occupancy_density_pack(FAKE, d, 0.01, 1, 1, None, FAKE, need, None) == MI_EINVAL
    assert lib.mi_occupancy_density_pack(FAKE, d, 0.01, 1, 1, FAKE, None, need, None) == MI_EINVAL
    assert lib.mi_occupancy_density_pack(FAKE, d, 0.01, 1, -1, FAKE, FAKE, 1 << 40, None) == MI_EINVAL
    assert lib.mi_occupancy_density_workspace_bytes(d, -1) == MI_EINVAL


@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 5, 7), (33, 2, 2), (16, 16, 16), (128, 128, 128), (129, 127, 130)])
def test_workspace_query_matches_its_formula(dims):
    lib = _lib()
    d = _i3(*dims)
    cells = dims[0] * dims[1] * dims[2]

    def r256(n):
        return (n + 255) // 256 * 256
    for dilate in (0, 1, 3):
        want = r256(4 * cells) + r256(8 * ((cells + 4095) // 4096)) + 256 + lib.mi_occupancy_pack_workspace_bytes(d, dilate)
        assert lib.mi_occupancy_density_workspace_bytes(d, dilate) == want
    assert lib.mi_abi_version() == 4


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", ref.DIMS)
def test_draw_inputs_accept_on_every_try_and_fall_back(dims):
    bits = ref.draw_bits("random", dims)
    cells = dims[0] * dims[1] * dims[2]
    lo, cell = np.float32([-1.5, -1.0, 0.25]), np.float32([0.1, 0.2, 0.3])
    ids, pts, tries = ref.draw(bits, dims, lo, cell, ref.SEED, 0, 1, 0, 1000, 0)
    assert set(tries.tolist()) == set(range(9))                            # tries 0..7 and the fall-back, 8
    for i in np.flatnonzero(tries < 8):
        assert ref.bit_of(bits, int(ids[i]))
    for i in np.flatnonzero(tries == 8):
        assert not ref.bit_of(bits, int(ids[i]))
    assert ids.min() >= 0 and ids.max() < cells and len(set(ids.tolist())) > 1
    # a point lies in its cell (the far face included: float(i) + u may round up)
    t = (pts[:, :3].astype(np.float64) - lo) / cell
    ijk = np.stack([ids // (dims[1] * dims[2]), (ids // dims[2]) % dims[1], ids % dims[2]], -1)
    assert np.all(t >= ijk - 1e-4) and np.all(t <= ijk + 1 + 1e-4) and not pts[:, 3:].any()
    # uniform rows: every cell index is drawn from the whole grid, occupied or not
    uid, _, utries = ref.draw(bits, dims, lo, cell, ref.SEED, 0, 1, 0, 1000, 1000)
    assert (utries == -1).all() and any(not ref.bit_of(bits, int(c)) for c in uid) and any(ref.bit_of(bits, int(c)) for c in uid)


def test_fold_inputs_hit_every_special_value():
    density, sigma, ids = ref.fold_inputs()
    assert density.shape == (ref.FOLD_CELLS,) and len(set(density.tolist())) == ref.FOLD_CELLS and density.min() > 0
    assert sigma.shape == ids.shape == (ref.FOLD_ROWS,)
    counts = np.bincount(ids, minlength=ref.FOLD_CELLS)
    assert all(counts[c] == 0 for c in ref.FOLD_UNSAMPLED) and (np.delete(counts, ref.FOLD_UNSAMPLED) >= 3).all()
    rows = {c: sigma[ids == c] for c in range(9)}
    neg_zero = np.float32(-0.0).tobytes()
    assert all(v.tobytes() == neg_zero for v in rows[ref.ALL_NEG_ZERO])
    assert (rows[ref.ALL_NEGATIVE] < 0).all() and np.isnan(rows[ref.ALL_NAN]).all()
    assert np.isposinf(rows[ref.HAS_INF]).any()
    assert rows[ref.MAX_FIRST].argmax() == 0 and rows[ref.MAX_FIRST][0] > rows[ref.MAX_FIRST][1:].max()
    last = len(rows[ref.MAX_LAST]) - 1
    assert rows[ref.MAX_LAST].argmax() == last and rows[ref.MAX_LAST][last] > rows[ref.MAX_LAST][:last].max()
    assert np.isnan(rows[ref.NAN_AND_POSITIVE]).any() and np.nanmax(rows[ref.NAN_AND_POSITIVE]) > 0
    assert 0 < rows[ref.BELOW_OLD].max() < np.float32(0.95) * density[ref.BELOW_OLD]
    assert any(v.tobytes() == neg_zero for v in rows[ref.NEG_ZERO_AND_POSITIVE]) and rows[ref.NEG_ZERO_AND_POSITIVE].max() > 0
    # what the rule makes of them
    out = ref.fold(density, sigma, ids, 0.95)
    for c in (ref.ALL_NEG_ZERO, ref.ALL_NEGATIVE, ref.ALL_NAN, ref.BELOW_OLD):
        assert out[c] == np.float32(density[c] * np.float32(0.95))
    assert np.isposinf(out[ref.HAS_INF]) and out[ref.MAX_FIRST] == 50.0 and out[ref.MAX_LAST] == 60.0
    assert out[ref.NAN_AND_POSITIVE] == 9.5 and out[ref.NEG_ZERO_AND_POSITIVE] == 7.25
    for c in ref.FOLD_UNSAMPLED:
        assert out[c] == density[c]
    zero = ref.fold(density, sigma, ids, 0.0)
    assert zero[ref.ALL_NEG_ZERO].tobytes() == np.float32(0.0).tobytes() and not np.isnan(zero).any()
    assert ref.same_bits(ref.fold(density, sigma, ids, 1.0)[ref.ALL_NAN], density[ref.ALL_NAN])


@pytest.mark.parametrize("dims", ref.DIMS)
def test_pack_inputs_sum_exactly_in_any_order(dims):
    d = ref.pack_inputs(dims)
    units = d.astype(np.float64) * 1024.0
    assert np.array_equal(units, np.round(units)) and d.max() < 1024 and d.min() >= 0
    total = int(units.astype(np.int64).sum())
    assert total < 2 ** 53                                                  # every partial sum is an integer fp64 holds
    rng = np.random.Generator(np.random.PCG64(1))
    for order in (np.arange(d.size), np.arange(d.size)[::-1], rng.permutation(d.size)):
        s = 0.0
        for v in d[order].astype(np.float64):
            s += v
        assert s * 1024.0 == total
    assert float(np.sum(d.astype(np.float64))) * 1024.0 == total
    mean = np.float32(total / 1024.0 / d.size)
    for name, threshold, relative in ref.PACK_CASES:
        got_mean, thr = ref.threshold_of(d, threshold, relative)
        assert got_mean == mean
        if name == "mean below the threshold":
            assert mean < threshold and thr == mean
        else:
            assert thr == np.float32(threshold) and (d == thr).any() and (relative == 0 or mean > threshold)
        dense, _ = ref.pack(d, dims, threshold, relative, 0)
        assert 0 < dense.sum() < d.size
    assert not ref.pack(np.zeros_like(d), dims, 0.01, 1, 2)[0].any()        # 0 > min(0.01, 0) is false


# ---- planted mistakes: the GPU test's comparison rejects each ------------------------------------------------------------------
def _fold_by_int_max(density, sigma, ids, decay, keep_neg_zero=False, last_writer=False, decay_all=False):
    """The three kernels as they run, with room for a mistake: the scratch ints at -1, an integer maximum of the floats'
    bits (or the last writer), the per-cell fold."""
    scratch = np.full(density.size, -1, np.int64)
    for s, c in zip(sigma, ids):
        v = s if (s > 0 or (keep_neg_zero and s == 0)) else np.float32(0.0)
        b = int(np.float32(v).view(np.int32))
        scratch[c] = b if last_writer else max(scratch[c], b)
    out = density.copy()
    with np.errstate(invalid="ignore"):
        for c in range(density.size):
            if scratch[c] >= 0:
                out[c] = np.fmax(np.float32(density[c] * np.float32(decay)), np.int32(scratch[c]).view(np.float32))
            elif decay_all:
                out[c] = np.float32(density[c] * np.float32(decay))
    return out


@pytest.mark.parametrize("decay", [0.95, 1.0, 0.0])
def test_the_three_kernels_are_the_rule(decay):
    density, sigma, ids = ref.fold_inputs()
    assert ref.same_bits(_fold_by_int_max(density, sigma, ids, decay), ref.fold(density, sigma, ids, decay))


@pytest.mark.parametrize("mistake", ["decay_all", "last_writer", "keep_neg_zero"])
def test_fold_comparison_rejects(mistake):
    density, sigma, ids = ref.fold_inputs()
    assert not ref.same_bits(_fold_by_int_max(density, sigma, ids, 0.95, **{mistake: True}), ref.fold(density, sigma, ids, 0.95))


@pytest.mark.parametrize("dims", ref.DIMS)
def test_pack_comparison_rejects_a_loose_comparison(dims):
    d = ref.pack_inputs(dims)
    for name, threshold, relative in ref.PACK_CASES[1:]:                    # the two whose threshold is a density
        assert not ref.same_bits(ref.pack(d, dims, threshold, relative, 0, strict=False)[1], ref.pack(d, dims, threshold, relative, 0)[1])


@pytest.mark.parametrize("dims", ref.DIMS)
def test_draw_comparison_rejects_a_stream_without_the_epoch(dims):
    bits = ref.draw_bits("random", dims)
    lo, cell = np.float32([-1.5, -1.0, 0.25]), np.float32([0.1, 0.2, 0.3])
    for mode, count in ((0, 100), (1, 255)):
        right = ref.draw(bits, dims, lo, cell, ref.SEED, 3, mode, 0, count, count // 2)
        wrong = ref.draw(bits, dims, lo, cell, ref.SEED, 3, mode, 0, count, count // 2, epoch_in_stream=False)
        assert not ref.same_bits(right[1], wrong[1])
        assert mode == 0 or not ref.same_bits(right[0], wrong[0])

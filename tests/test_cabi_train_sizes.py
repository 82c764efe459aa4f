"""CPU: the size queries of the C-ABI training pair (mi_render_train_saved_bytes, mi_render_backward_workspace_bytes) and
the argument checks of mi_render_rays_train / mi_render_rays_backward, which return MI_EINVAL before anything touches a
device (the pointers below are never dereferenced)."""
import ctypes

import pytest

from mirender import _lib, fields

KINDS = sorted(fields.SPECS)
MI_EINVAL = -1
FAKE = ctypes.c_void_p(1 << 20)             # a non-null address no call may reach


def lib():
    return _lib.load()


def acts(kind):
    return lib().mi_field_train_acts_floats(kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,nc,nf", [(1, 3, 0), (1000, 64, 128), (4096, 12, 24), (777, 16, 0)])
def test_saved_bytes_cover_every_pass(kind, n, nc, nf):
    L = lib()
    assert L.mi_render_train_saved_bytes(kind, kind, 0, n, nc, nf) == 4 * acts(kind) * n * (nc + (nc + nf))
    assert L.mi_render_train_saved_bytes(kind, kind, 1, n, nc, nf) == 4 * acts(kind) * n * (nc + nf)
    other = (kind + 1) % len(KINDS)
    assert L.mi_render_train_saved_bytes(kind, other, 0, n, nc, nf) == 4 * n * (acts(kind) * nc + acts(other) * (nc + nf))


def _bwd_bytes(kind, shared, groups, rpg, nc, nf, rp):
    return lib().mi_render_backward_workspace_bytes(kind, kind, shared, groups, rpg, nc, nf, rp, rp)


def largest_range(film, groups, rpg, s, rp):
    """Rays in the largest range of a pass of s samples per ray (autograd._chunk_ranges)."""
    n, max_rays = groups * rpg, max(1, rp // s)
    if not film:
        return min(n, max_rays)
    if max_rays >= rpg:
        return min(n, max_rays // rpg * rpg)
    parts = -(-rpg // max_rays)
    return -(-rpg // parts)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shared", [0, 1])
def test_backward_workspace_grows_with_range_points(kind, shared):
    L = lib()
    groups, rpg, nc, nf = (4, 4096, 12, 24) if fields.is_film(kind) else (1, 8192, 32, 64)
    sizes = [_bwd_bytes(kind, shared, groups, rpg, nc, nf, rp) for rp in (64, 4096, 65536, 1 << 20, 1 << 26)]
    assert all(b > 0 for b in sizes)
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    for rp, b in zip((64, 4096, 65536, 1 << 20, 1 << 26), sizes):
        # never below one range's layer inputs + per-layer gradients + dW partial sums (the largest range of the passes)
        s = max(nc, nf if shared else nc + nf)
        pts = largest_range(fields.is_film(kind), groups, rpg, s, rp) * s
        one_range = 4 * (pts * (acts(kind) + L.mi_field_train_grads_floats(kind)) + L.mi_field_bwd_partial_floats(pts))
        assert b >= one_range, (rp, b, one_range)


def test_unknown_kind_and_bad_range_points():
    L = lib()
    assert L.mi_render_train_saved_bytes(9, 0, 0, 10, 8, 8) == MI_EINVAL
    assert b"unknown field kind" in L.mi_last_error()
    assert L.mi_render_backward_workspace_bytes(0, -1, 0, 1, 10, 8, 8, 4096, 4096) == MI_EINVAL
    assert b"unknown field kind" in L.mi_last_error()
    for rp_c, rp_f in ((0, 4096), (4096, 0), (-5, -5)):
        assert L.mi_render_backward_workspace_bytes(0, 0, 0, 1, 10, 8, 8, rp_c, rp_f) == MI_EINVAL
        assert b"points per range" in L.mi_last_error()


N, NC, NF = 64, 8, 16


def _ws(shared):
    L = lib()
    return L.mi_render_workspace_bytes(N, NC, NF) + (L.mi_render_shared_field_extra_bytes(N, NC, NF) if shared else 0)


def _train(kind=0, shared=False, ws_bytes=None, rp=4096, film=None):
    packed_f = FAKE if shared else ctypes.c_void_p(2 << 20)
    outs = [ctypes.c_void_p((3 + i) << 20) for i in range(6)]
    return lib().mi_render_rays_train(kind, FAKE, kind, packed_f, film, FAKE, 1, N, 2.0, 6.0, NC, NF, None, None, None, 0, 0,
                                      *outs, FAKE, _ws(shared) if ws_bytes is None else ws_bytes, rp, rp, None, 0, None)


def _ptrs(k):
    return (ctypes.c_void_p * k)(*[(10 + i) << 20 for i in range(k)])


def _backward(kind=0, shared=False, ws_bytes=None, bwd_bytes=None, params=True, grads_c=True, grads_f=True, rp=4096,
              cots=(1, 1, 1, 1, 1, 1), groups=1, grad_film=True):
    L = lib()
    npar = max(0, L.mi_field_num_params(kind))
    packed_f = FAKE if shared else ctypes.c_void_p(2 << 20)
    film = FAKE if fields.is_film(kind) else None
    bw = _bwd_bytes(kind, int(shared), groups, N // groups, NC, NF, rp) if bwd_bytes is None else bwd_bytes
    cot = [ctypes.c_void_p((40 + i) << 20) if c else None for i, c in enumerate(cots)]
    written = ctypes.c_int(-1)
    rc = L.mi_render_rays_backward(kind, FAKE, FAKE, _ptrs(npar) if params else None, kind, packed_f, FAKE,
                                   _ptrs(npar) if params else None, film, FAKE, groups, N // groups, NC, NF, rp, rp, FAKE,
                                   _ws(shared) if ws_bytes is None else ws_bytes, None, 0, *cot,
                                   _ptrs(npar) if grads_c else None, _ptrs(npar) if grads_f else None,
                                   FAKE if grad_film else None, FAKE, bw, ctypes.byref(written), None)
    return rc, written.value


def test_training_forward_rejects_bad_arguments():
    L = lib()
    assert _train(kind=7) == MI_EINVAL and b"unknown field kind" in L.mi_last_error()
    assert _train(rp=0) == MI_EINVAL and b"points per range" in L.mi_last_error()
    # one field for both passes (same kind, same stream) needs the shared-field extra on top of the workspace
    assert _train(shared=True, ws_bytes=_ws(False)) == MI_EINVAL
    assert b"mi_render_shared_field_extra_bytes" in L.mi_last_error()
    assert _train(ws_bytes=_ws(False) - 1) == MI_EINVAL and b"workspace" in L.mi_last_error()
    assert _train(kind=2) == MI_EINVAL and b"film" in L.mi_last_error()


def test_backward_rejects_bad_arguments():
    L = lib()
    assert _backward(kind=-1)[0] == MI_EINVAL and b"unknown field kind" in L.mi_last_error()
    assert _backward(rp=0)[0] == MI_EINVAL and b"points per range" in L.mi_last_error()
    assert _backward(shared=True, ws_bytes=_ws(False))[0] == MI_EINVAL
    assert b"mi_render_shared_field_extra_bytes" in L.mi_last_error()
    assert _backward(ws_bytes=_ws(False) - 1)[0] == MI_EINVAL
    # a FiLM kind without its parameter array (d gamma = <W, dW_image> + b . db_image needs the weights)
    rc, written = _backward(kind=2, shared=True, params=False, groups=2)
    assert rc == MI_EINVAL and b"parameter array" in L.mi_last_error() and written == 0
    assert _backward(kind=2, shared=True, groups=2, grad_film=False)[0] == MI_EINVAL and b"grad_film" in L.mi_last_error()
    # a NULL gradient array for a field that receives a cotangent ...
    assert _backward(grads_f=False)[0] == MI_EINVAL and b"fine field gets a cotangent" in L.mi_last_error()
    assert _backward(grads_c=False)[0] == MI_EINVAL and b"coarse field gets a cotangent" in L.mi_last_error()
    assert _backward(shared=True, grads_c=False, cots=(0, 0, 0, 1, 0, 0))[0] == MI_EINVAL
    # ... and a backward workspace one byte short
    full = _bwd_bytes(0, 0, 1, N, NC, NF, 4096)
    rc, _ = _backward(bwd_bytes=full - 1)
    assert rc == MI_EINVAL and b"mi_render_backward_workspace_bytes" in L.mi_last_error()


def test_backward_without_cotangents_launches_nothing():
    # no cotangent at all: nothing to do, nothing written (a NULL gradient array is then fine), no device touched
    rc, written = _backward(grads_c=False, grads_f=False, cots=(0,) * 6)
    assert rc == 0 and written == 0


# ---- the dW scratch query against the planner, for every FiLM depth --------------------------------------------------
FILM_DEPTHS = list(range(4, 13))


def _film_sizes(kind):
    import bwd_gates as G
    caps = [256 * G.group_plan(kind, grp, 1)[2] for grp in G.group_jobs(kind)]
    return sorted({1, 257, 9217, 128 * 128 * 36, 1 << 21} | {c + d for c in caps for d in (-5, 37)} | {c // 2 + 37 for c in caps})


@pytest.mark.parametrize("use_dir", [True, False])
@pytest.mark.parametrize("depth", FILM_DEPTHS)
def test_bwd_partial_query_covers_the_planner_at_every_depth(depth, use_dir):
    """mi_field_bwd_partial_floats_kind against a replay of the planner (bwd_gates.film_scratch_plan: the image pass of
    `depth` GEMM jobs of at most ceil(256 / depth) slabs and its thin jobs, the head pass over all images) at every size
    where the plan changes.  Depths 5, 6 and 7 plan 260, 258 and 259 job-slabs where the fixed kinds' figure was written
    for 256: that figure still covers them, through the NeRF plan in its maximum, which is asserted here as well."""
    import bwd_gates as G
    L = lib()
    kind = G.depth_name(depth, use_dir)
    k = G.KIND_IDS[kind]
    assert L.mi_field_film_partial_floats_kind(k, 2, 4096) == depth * (256 * 256 + 256) + 2 * 1024 + 256
    worst_units = 0
    for ppg in _film_sizes(kind):
        for n_img in (1, 2, 3):
            plan, query = G.film_scratch_plan(kind, ppg, n_img), L.mi_field_bwd_partial_floats_kind(k, n_img * ppg)
            assert query >= plan, (ppg, n_img, plan, query)
            assert query >= L.mi_field_bwd_partial_floats(n_img * ppg)
            if depth <= 8:
                assert L.mi_field_bwd_partial_floats(n_img * ppg) >= plan, (ppg, n_img)
            worst_units = max(worst_units, depth * G.group_plan(kind, "g422_img", ppg)[1])
    assert worst_units == depth * -(-256 // depth)
    if depth == 8:
        for P in (1, 8229, 1 << 20):
            assert L.mi_field_bwd_partial_floats_kind(2 if use_dir else 3, P) == L.mi_field_bwd_partial_floats_kind(k, P) \
                == L.mi_field_bwd_partial_floats(P)

"""CPU: the host side of training with an occupancy grid (include/mi_render.h "training with a grid").  No GPU, no launch.

* the new size queries against their formulas;
* every argument check of the new calls refused with MI_EINVAL and a message before anything is launched (a launch on a
  machine without a GPU would come back as MI_EHIP);
* the device slab rule of the counted weight-gradient kernels, restated in tests/occupancy_train_ref.py: with count ==
  capacity it gives the host planner's slab length (bwd_gates.slab_pts_for), and n_slabs * slab_len >= count always;
* tests/occupancy_train_ref.py, the reference the GPU gradients are gated against: an all-true mask is no mask, a masked
  sample gets no gradient, and the two planted mistakes (no mask, a mask shifted by one sample) are rejected by the project's
  gradient gates (a small case of its own: 12 rays x 8 depths, an 8^3 grid);
* the GPU test's own gradient cases (occupancy_train_ref.GRAD_CASES: its kinds, seeds, head variants, rays, grids, jitter and
  cotangents, at the depths the fp32 oracle samples): the fp32 oracle under the mask stays inside the HARD gates against its
  fp64 self in every tensor, so the GPU test may demand the hard gate too and the 3x fp64-bound fallback never decides.
"""
import ctypes

import numpy as np
import pytest
import torch

import bwd_gates as G
import occupancy_render_ref as ref
import occupancy_train_ref as tref
from mirender import _lib as binding
from oracle import parity, render_ref as R, synth

MI_EINVAL = -1
FAKE = ctypes.c_void_p(0x10000)        # a non-null "device pointer": every call below must fail before it is used
NERF, SIREN, FILM, FILM_NODIR, TINY = 0, 1, 2, 3, 4
MARK_BLOCK = 4096                      # points per workgroup of the mark kernels (csrc/occupancy.hip: kMarkBlock)


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


def _up64(x):
    return (x + 63) // 64 * 64


def _ordered_ints(points):
    return points + (points + MARK_BLOCK - 1) // MARK_BLOCK


def test_size_queries_against_their_formulas():
    lib = _lib()
    for n, s in ((1, 3), (37, 5), (130, 192), (1024, 192), (640000, 192)):
        assert lib.mi_occupancy_ordered_list_ints(n, s) == _ordered_ints(n * s), (n, s)
    assert lib.mi_occupancy_ordered_list_ints((2 ** 31 - 1) // 192 + 1, 192) == MI_EINVAL
    for n, nc, nf in ((1, 3, 0), (37, 5, 0), (130, 64, 128), (1024, 64, 128)):
        want = (_up64(_ordered_ints(n * nc)) + _up64(_ordered_ints(n * (nc + nf))) + 64) * 4
        assert lib.mi_render_occupancy_train_extra_bytes(n, nc, nf) == want, (n, nc, nf)
        for kc, kf in ((NERF, NERF), (TINY, SIREN), (SIREN, NERF)):
            saved = 4 * (lib.mi_field_train_acts_floats(kc) * n * nc + lib.mi_field_train_acts_floats(kf) * n * (nc + nf))
            assert lib.mi_render_occupancy_train_saved_bytes(kc, kf, n, nc, nf) == saved
            for shared in (0, 1):
                if shared and kc != kf:
                    continue
                pc, pf = n * nc, n * (nc + nf)
                params = 0
                for i in range(lib.mi_field_num_params(kc)):
                    rows, cols = ctypes.c_int64(), ctypes.c_int64()
                    assert lib.mi_field_param_shape(kc, i, rows, cols) == 0
                    params += _up64(rows.value * cols.value)
                want_b = (_up64(pc * 4) + _up64(pf * 4)
                          + _up64(max(pc * lib.mi_field_train_grads_floats(kc), pf * lib.mi_field_train_grads_floats(kf)))
                          + _up64(max(lib.mi_field_bwd_partial_floats_kind(kc, pc), lib.mi_field_bwd_partial_floats_kind(kf, pf)))
                          + (params if shared else 0)) * 4
                assert lib.mi_render_occupancy_backward_workspace_bytes(kc, kf, shared, n, nc, nf) == want_b, (n, nc, nf, kc, kf)
    assert lib.mi_render_occupancy_train_extra_bytes(0, 64, 128) == 0
    _refused(lib.mi_render_occupancy_train_saved_bytes(FILM, NERF, 10, 8, 8), lib, b"FiLM")
    _refused(lib.mi_render_occupancy_backward_workspace_bytes(NERF, FILM_NODIR, 0, 10, 8, 8), lib, b"FiLM")
    assert lib.mi_abi_version() == 4


def _train(lib, kind_c=NERF, kind_f=NERF, packed_c=FAKE, rays=FAKE, n=100, nc=8, nf=16, bits=FAKE, dims=None, lo=None, inv=None,
           rgb_c=FAKE, rgb_f=FAKE, ws=FAKE, ws_bytes=None, saved=FAKE, saved_bytes=None):
    dims = _i3(16, 16, 16) if dims is None else dims
    lo = _f3(-1, -1, -1) if lo is None else lo
    inv = _f3(8, 8, 8) if inv is None else inv
    if ws_bytes is None:
        ws_bytes = lib.mi_render_workspace_bytes(n, nc, nf) + lib.mi_render_occupancy_train_extra_bytes(n, nc, nf)
    if saved_bytes is None:
        saved_bytes = max(lib.mi_render_occupancy_train_saved_bytes(NERF, NERF, min(n, 1000), nc, nf), 0)
    return lib.mi_render_rays_occupancy_train(kind_c, packed_c, kind_f, FAKE, rays, n, 2.0, 6.0, nc, nf, None, None, None, 0, 0,
                                              bits, dims, lo, inv, rgb_c, FAKE, FAKE, rgb_f, FAKE, FAKE, None, ws, ws_bytes, saved,
                                              saved_bytes, None)


def test_train_argument_checks():
    lib = _lib()
    _refused(_train(lib, packed_c=None), lib, b"null pointer")
    _refused(_train(lib, rays=None), lib, b"null pointer")
    _refused(_train(lib, bits=None), lib, b"null pointer")
    _refused(_train(lib, rgb_c=None), lib, b"null pointer")
    _refused(_train(lib, rgb_f=None), lib, b"null pointer")
    _refused(_train(lib, lo=ctypes.POINTER(ctypes.c_float)()), lib, b"null pointer")
    _refused(_train(lib, dims=ctypes.POINTER(ctypes.c_int)()), lib, b"grid dims")
    _refused(_train(lib, dims=_i3(0, 16, 16)), lib, b"grid dims")
    _refused(_train(lib, dims=_i3(2048, 2048, 512)), lib, b"grid dims")
    for kc, kf in ((FILM, NERF), (NERF, FILM_NODIR), (FILM, FILM)):
        _refused(_train(lib, kind_c=kc, kind_f=kf), lib, b"FiLM")
    _refused(_train(lib, kind_c=99), lib, b"unknown field kind")
    _refused(_train(lib, n=(2 ** 31 - 1) // 192 + 1, nc=64, nf=128, ws_bytes=1 << 60, saved_bytes=1 << 60), lib, b"2^31 - 1")
    _refused(_train(lib, nc=2), lib, b"bad sizes")
    need = lib.mi_render_workspace_bytes(100, 8, 16) + lib.mi_render_occupancy_train_extra_bytes(100, 8, 16)
    _refused(_train(lib, ws_bytes=need - 1), lib, b"workspace of", str(need).encode())
    _refused(_train(lib, ws=None), lib, b"workspace of")
    # the inference call's workspace is too small: each pass keeps its own list
    _refused(_train(lib, ws_bytes=lib.mi_render_workspace_bytes(100, 8, 16) + lib.mi_render_occupancy_extra_bytes(100, 8, 16)), lib,
             b"workspace of")
    sv = lib.mi_render_occupancy_train_saved_bytes(NERF, NERF, 100, 8, 16)
    _refused(_train(lib, saved_bytes=sv - 1), lib, b"saved buffer of", str(sv).encode())
    _refused(_train(lib, saved=None), lib, b"saved buffer of")
    assert _train(lib, n=0) == 0                                            # no rays: nothing to launch


def _backward(lib, kind_c=NERF, kind_f=NERF, shared=0, pb_c=FAKE, pb_f=FAKE, rays=FAKE, n=100, nc=8, nf=16, ws=FAKE, ws_bytes=None,
              saved=FAKE, saved_bytes=None, g_rgb_c=FAKE, g_rgb_f=FAKE, gp_c="ok", gp_f="ok", bws=FAKE, bws_bytes=None, null_at=None):
    n_par = 24
    def arr(v, hole):
        if v != "ok":
            return v
        a = (ctypes.c_void_p * n_par)(*([0x10000] * n_par))
        if hole is not None:
            a[hole] = None
        return a
    if ws_bytes is None:
        ws_bytes = lib.mi_render_workspace_bytes(n, nc, nf) + lib.mi_render_occupancy_train_extra_bytes(n, nc, nf)
    if saved_bytes is None:
        saved_bytes = max(lib.mi_render_occupancy_train_saved_bytes(NERF, NERF, min(n, 1000), nc, nf), 0)
    if bws_bytes is None:
        bws_bytes = max(lib.mi_render_occupancy_backward_workspace_bytes(NERF, NERF, 1, min(n, 1000), nc, nf), 0)
    written = ctypes.c_int(7)
    rc = lib.mi_render_rays_occupancy_backward(kind_c, pb_c, kind_f, pb_f, shared, rays, n, nc, nf, ws, ws_bytes, saved, saved_bytes,
                                               g_rgb_c, None, None, g_rgb_f, None, None, arr(gp_c, null_at), arr(gp_f, None), bws,
                                               bws_bytes, ctypes.byref(written), None)
    assert written.value == 0                                               # nothing was written by a refused call
    return rc


def test_backward_argument_checks():
    lib = _lib()
    _refused(_backward(lib, rays=None), lib, b"null pointer")
    _refused(_backward(lib, pb_c=None), lib, b"coarse field has no transposed stream")
    _refused(_backward(lib, pb_f=None), lib, b"fine field has no transposed stream")
    _refused(_backward(lib, gp_c=None), lib, b"coarse field gets a cotangent but has no gradient array")
    _refused(_backward(lib, gp_f=None), lib, b"fine field gets a cotangent")
    _refused(_backward(lib, null_at=5), lib, b"coarse gradient pointer 5 is null")
    for kc, kf in ((FILM, NERF), (NERF, FILM_NODIR)):
        _refused(_backward(lib, kind_c=kc, kind_f=kf), lib, b"FiLM")
    _refused(_backward(lib, kind_f=TINY, shared=1), lib, b"one field for both passes has one kind")
    _refused(_backward(lib, n=(2 ** 31 - 1) // 192 + 1, nc=64, nf=128, ws_bytes=1 << 60, saved_bytes=1 << 60, bws_bytes=1 << 60), lib,
             b"2^31 - 1")
    need = lib.mi_render_workspace_bytes(100, 8, 16) + lib.mi_render_occupancy_train_extra_bytes(100, 8, 16)
    _refused(_backward(lib, ws_bytes=need - 1), lib, b"workspace of")
    sv = lib.mi_render_occupancy_train_saved_bytes(NERF, NERF, 100, 8, 16)
    _refused(_backward(lib, saved_bytes=sv - 1), lib, b"saved buffer of")
    bw = lib.mi_render_occupancy_backward_workspace_bytes(NERF, NERF, 0, 100, 8, 16)
    _refused(_backward(lib, bws_bytes=bw - 1), lib, b"backward workspace of", str(bw).encode())
    _refused(_backward(lib, bws=None), lib, b"backward workspace of")
    # one field: the fine pass's scratch copy of the gradients is part of the workspace
    assert lib.mi_render_occupancy_backward_workspace_bytes(NERF, NERF, 1, 100, 8, 16) > bw
    _refused(_backward(lib, shared=1, bws_bytes=bw), lib, b"backward workspace of")
    assert _backward(lib, n=0) == 0
    assert _backward(lib, g_rgb_c=None, g_rgb_f=None) == 0                  # no cotangent: nothing to launch


def test_stage_argument_checks():
    lib = _lib()
    d, lo, inv = _i3(5, 7, 3), _f3(0, 0, 0), _f3(1, 1, 1)
    mark = lib.mi_occupancy_mark_rays_ordered
    _refused(mark(None, d, lo, inv, FAKE, FAKE, 10, 4, FAKE, FAKE, None, None), lib, b"null pointer")
    _refused(mark(FAKE, d, lo, inv, FAKE, FAKE, 10, 4, None, FAKE, None, None), lib, b"null pointer")
    _refused(mark(FAKE, d, lo, inv, FAKE, FAKE, 10, 4, FAKE, None, None, None), lib, b"null pointer")
    _refused(mark(FAKE, _i3(5, 0, 3), lo, inv, FAKE, FAKE, 10, 4, FAKE, FAKE, None, None), lib, b"grid dims")
    _refused(mark(FAKE, d, lo, inv, FAKE, FAKE, 10, 0, FAKE, FAKE, None, None), lib, b"bad sizes")
    _refused(mark(FAKE, d, lo, inv, FAKE, FAKE, (2 ** 31 - 1) // 192 + 1, 192, FAKE, FAKE, None, None), lib, b"2^31 - 1")
    ev = lib.mi_field_eval_rays_list_train
    for kind in (FILM, FILM_NODIR):
        _refused(ev(kind, FAKE, FAKE, FAKE, 10, 4, FAKE, FAKE, FAKE, FAKE, None), lib, b"no list-driven forward")
    _refused(ev(NERF, FAKE, FAKE, FAKE, 10, 4, None, FAKE, FAKE, FAKE, None), lib, b"null pointer")
    _refused(ev(SIREN, FAKE, FAKE, FAKE, 10, 4, FAKE, FAKE, FAKE, None, None), lib, b"null pointer")     # no acts
    _refused(ev(TINY, FAKE, FAKE, FAKE, (2 ** 31 - 1) // 192 + 1, 192, FAKE, FAKE, FAKE, FAKE, None), lib, b"2^31 - 1")
    assert ev(NERF, FAKE, FAKE, FAKE, 0, 4, FAKE, FAKE, FAKE, FAKE, None) == 0
    bw = lib.mi_field_backward_list
    gp = (ctypes.c_void_p * 24)(*([0x10000] * 24))
    for kind in (FILM, FILM_NODIR):
        _refused(bw(kind, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 100, FAKE, gp, None), lib, b"no counted backward")
    _refused(bw(NERF, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, 100, FAKE, gp, None), lib, b"null pointer")
    _refused(bw(NERF, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, 100, FAKE, gp, None), lib, b"null pointer")
    _refused(bw(NERF, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2 ** 31, FAKE, gp, None), lib, b"capacity")
    gp[3] = None
    _refused(bw(NERF, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 100, FAKE, gp, None), lib, b"gradient pointer 3 is null")
    gp[3] = 0x10000
    assert bw(NERF, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, FAKE, gp, None) == 0


@pytest.mark.parametrize("kind", ["nerf", "tiny_nerf", "siren_nerf"])
def test_device_slab_rule(kind):
    """slab_len = ceil32(ceil(count / n_slabs)) with n_slabs planned from the capacity."""
    caps = {1, 31, 33, 259, 2561, 2600, 2688, 2817, 8193, 1024 * 64, 1024 * 192, 500_009}
    caps |= {t + d for t in G.cap_thresholds(kind) for d in (-5, 0, 37)}
    for cap in sorted(caps):
        for group in G.group_jobs(kind):
            slab, n_slabs, _ = G.group_plan(kind, group, cap)
            assert tref.counted_slab_len(cap, n_slabs) == slab, (kind, group, cap)         # count == capacity: the host's plan
            for count in {0, 1, 31, 32, 33, cap - 1, cap // 20, cap // 2}:
                if not 0 <= count <= cap:
                    continue
                got = tref.counted_slab_len(count, n_slabs)
                assert got % 32 == 0 and n_slabs * got >= count, (kind, group, cap, count)
                assert got <= slab                                                        # never past what the buffers plan for
                if count:
                    assert (n_slabs - 1) * (got - 32) < count                             # an equal share: no slab a stage too long


# ---- the reference ------------------------------------------------------------------------------------------------------------
def _case(kind, seed=7, n=12, s=8):
    sd = synth.state_dict(kind, seed, "medium", 0.05)
    rays = torch.from_numpy(R.rays_from_camera(24, 24, 33.0, synth.pose_degrees(4.0, 15.0, -30.0))[100:100 + n])
    rng = np.random.Generator(np.random.PCG64(1))
    z = torch.from_numpy(np.sort(rng.uniform(2, 6, size=(n, s)).astype(np.float32), -1))
    cot = [torch.from_numpy(rng.normal(size=sh).astype(np.float32)) for sh in ((n, 3), (n,), (n,))]
    dense = rng.random((8, 8, 8)) < 0.5
    lo, hi = (-2.0,) * 3, (2.0,) * 3
    mask = ref.occupied_mask(rays, z, np.float32(lo), ref.inv_cell_of(lo, hi, dense.shape), dense)
    assert 0 < int(mask.sum()) < mask.numel()
    return sd, rays, z, cot, mask


def _gates(kind):
    smooth = kind == "siren_nerf"
    return dict(tol=parity.GRAD_TOL_SMOOTH if smooth else parity.GRAD_TOL_RELU,
                elem_tol=parity.GRAD_ELEM_TOL_SMOOTH if smooth else None)


@pytest.mark.parametrize("kind", ["tiny_nerf", "siren_nerf"])
def test_reference_and_planted_mistakes(kind):
    sd, rays, z, cot, mask = _case(kind)
    names = tref.param_names(kind, sd)
    r64 = tref.pass_grads(kind, sd, rays, z, mask, cot, torch.float64)
    r32 = tref.pass_grads(kind, sd, rays, z, mask, cot, torch.float32)
    # an all-true mask is no mask, bit for bit
    a, b = tref.pass_grads(kind, sd, rays, z, torch.ones_like(mask), cot), tref.pass_grads(kind, sd, rays, z, None, cot)
    assert all(torch.equal(a[k], b[k]) for k in names)
    # an all-false mask: the background, and no gradient at all
    none = tref.pass_grads(kind, sd, rays, z, torch.zeros_like(mask), cot)
    assert all(float(none[k].abs().max()) == 0.0 for k in names)
    rgb, depth, acc = none["__outs__"]
    assert bool((rgb == 1).all()) and bool((depth == 0).all()) and bool((acc == 0).all())
    # the fp32 oracle under the mask stays inside the gates against its fp64 self
    for k in names:
        parity.gate_grad(f"host {kind} masked oracle fp32 vs fp64", k, r32[k], r32[k], r64[k], check=True, **_gates(kind))
    # the planted mistakes are rejected by the same gates (in at least one tensor, as a wrong kernel would be)
    for what, wrong_mask in (("no mask", None), ("mask shifted by one sample", tref.shifted(mask))):
        wrong = tref.pass_grads(kind, sd, rays, z, wrong_mask, cot, torch.float32)
        recs = [parity.gate_grad(f"host {kind} planted: {what}", k, wrong[k], r32[k], r64[k], check=False, **_gates(kind)) for k in names]
        assert any(not r["passed"] for r in recs), what


@pytest.mark.parametrize("case", sorted(tref.GRAD_CASES))
def test_fp32_oracle_of_the_gpu_cases_is_inside_the_hard_gates(case):
    kind = tref.GRAD_CASES[case][0]
    z_c, m_c, z_f, m_f = tref.oracle_depths(case)
    full = case.endswith("_ones")
    for m in (m_c, m_f):
        assert bool(m.all()) if full else 0 < int(m.sum()) < m.numel(), (case, int(m.sum()), m.numel())
    refs = tref.case_refs(case, z_c, m_c, z_f, m_f)
    worst = 0.0
    for f, (r32, r64) in enumerate(zip(refs[torch.float32], refs[torch.float64])):
        for name in r32:
            rec = parity.gate_grad(f"host {case}: masked oracle fp32 vs fp64", ("coarse." if f == 0 else "fine.") + name, r32[name],
                                   r32[name], r64[name], check=True, **tref.case_gates(kind))
            assert rec["active"] == "hard", rec
            assert float(r64[name].abs().max()) > 0, (case, name)             # the case really exercises the tensor
            worst = max(worst, rec["rel_l2_err"])
    print(f"{case}: fp32 oracle within {worst:.3g} (rel l2) of fp64")

"""CPU: the host side of clipping each ray's sampling range to an occupancy grid (include/mi_render.h "clipping").  No GPU,
no launch.

* every argument check of the new calls refused with MI_EINVAL and a message before anything is launched (a launch on a
  machine without a GPU would come back as MI_EHIP), and the extra-bytes formula;
* tests/occupancy_clip_ref.py, the restatement the GPU test holds the kernel to, counted by hand on a (4,4,4) grid with one
  occupied cell and 8 probes: a ray through the cell, a ray that misses, a NaN direction, pad clamped at both ends, b == M
  returning far itself;
* the four planted mistakes (k1 for k1 + 1, probes at bin edges, pad not clamped, `<=` at the upper face) give other bounds
  than the rule on the GPU test's own inputs, so the bit comparison there rejects a kernel that makes them;
* the GPU test's inputs: at least 4 rays that miss, at least 4 hit rays whose bounds are the whole range, at least 4 with both
  bounds strictly inside, near_r < far_r on every ray;
* the restated samplers: constant bounds give the scalar formulas, and the clipped training cases' fp32 oracle stays inside the
  HARD gradient gates against its fp64 self, so the GPU test may demand the hard gate.
"""
import ctypes

import numpy as np
import pytest
import torch

import occupancy_clip_ref as cref
import occupancy_render_ref as ref
import occupancy_train_ref as tref
from mirender import _lib as binding
from oracle import parity, render_ref as R, synth

MI_EINVAL = -1
FAKE = ctypes.c_void_p(0x10000)        # a non-null "device pointer": every call below must fail before it is used
NERF, SIREN, FILM, FILM_NODIR, TINY = 0, 1, 2, 3, 4
F = np.float32


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


# ---- the C ABI: sizes and refusals -----------------------------------------------------------------------------------------------
def test_extra_bytes_formula():
    lib = _lib()
    for n in (1, 5, 31, 32, 33, 37, 130, 1024, 640000):
        assert lib.mi_render_occupancy_clip_extra_bytes(n) == _up64(2 * n) * 4, n
    assert lib.mi_render_occupancy_clip_extra_bytes(0) == 0 and lib.mi_render_occupancy_clip_extra_bytes(-3) == 0
    assert lib.mi_abi_version() == 4


def _clip(lib, bits=FAKE, dims=None, lo=None, inv=None, rays=FAKE, n=100, near=2.0, far=6.0, probes=64, pad=1, bounds=FAKE):
    dims = _i3(16, 16, 16) if dims is None else dims
    lo = _f3(-1, -1, -1) if lo is None else lo
    inv = _f3(8, 8, 8) if inv is None else inv
    return lib.mi_occupancy_clip_rays(bits, dims, lo, inv, rays, n, near, far, probes, pad, bounds, None)


def test_clip_rays_argument_checks():
    lib = _lib()
    for probes in (0, -1, 4097):
        _refused(_clip(lib, probes=probes), lib, b"probes")
    _refused(_clip(lib, pad=-1), lib, b"pad")
    for near, far in ((6.0, 2.0), (2.0, 2.0), (float("nan"), 6.0), (2.0, float("nan"))):
        _refused(_clip(lib, near=near, far=far), lib, b"near < far")
    _refused(_clip(lib, bounds=None), lib, b"null pointer")
    _refused(_clip(lib, rays=None), lib, b"null pointer")
    _refused(_clip(lib, bits=None), lib, b"null pointer")
    _refused(_clip(lib, dims=_i3(0, 16, 16)), lib, b"grid dims")
    _refused(_clip(lib, dims=_i3(2048, 2048, 512)), lib, b"grid dims")
    _refused(_clip(lib, dims=ctypes.POINTER(ctypes.c_int)()), lib, b"grid dims")
    _refused(_clip(lib, n=-1), lib, b"n =")
    assert _clip(lib, n=0) == 0                                             # no rays: nothing to launch
    assert _clip(lib, n=0, probes=4096, pad=0) == 0 and _clip(lib, n=0, probes=1) == 0


def test_bounds_sampler_argument_checks():
    lib = _lib()
    _refused(lib.mi_sample_coarse_bounds(10, None, 8, None, 0, 0, FAKE, None), lib, b"bounds")
    _refused(lib.mi_sample_coarse_bounds(10, FAKE, 8, None, 0, 0, None, None), lib, b"bad arguments")
    _refused(lib.mi_sample_coarse_bounds(10, FAKE, 0, None, 0, 0, FAKE, None), lib, b"bad arguments")
    assert lib.mi_sample_coarse_bounds(0, FAKE, 8, None, 0, 0, FAKE, None) == 0
    _refused(lib.mi_sample_fine_bounds(10, None, 8, 4, None, FAKE, FAKE, None, FAKE, None, None), lib, b"bounds")
    _refused(lib.mi_sample_fine_bounds(10, FAKE, 2, 4, None, FAKE, FAKE, None, FAKE, None, None), lib, b"Nc >= 3")
    _refused(lib.mi_sample_fine_bounds(10, FAKE, 8, 4, None, FAKE, FAKE, None, None, None, None), lib, b"bad arguments")
    assert lib.mi_sample_fine_bounds(0, FAKE, 8, 4, None, FAKE, FAKE, None, FAKE, None, None) == 0


def _render(lib, train, kind_c=NERF, kind_f=NERF, n=100, nc=8, nf=16, near=2.0, far=6.0, probes=64, pad=1, bits=FAKE, dims=None,
            rgb_f=FAKE, ws=FAKE, ws_bytes=None):
    dims = _i3(16, 16, 16) if dims is None else dims
    extra = lib.mi_render_occupancy_train_extra_bytes if train else lib.mi_render_occupancy_extra_bytes
    if ws_bytes is None:
        ws_bytes = lib.mi_render_workspace_bytes(n, nc, nf) + extra(n, nc, nf) + lib.mi_render_occupancy_clip_extra_bytes(n)
    head = (kind_c, FAKE, kind_f, FAKE, FAKE, n, near, far, nc, nf, probes, pad, None, None, 0, 0, bits, dims, _f3(-1, -1, -1),
            _f3(8, 8, 8), FAKE, FAKE, FAKE, rgb_f, FAKE, FAKE, None, ws, ws_bytes)
    if train:
        return lib.mi_render_rays_occupancy_clip_train(*head, FAKE, 1 << 60, None)
    return lib.mi_render_rays_occupancy_clip(*head, None)


@pytest.mark.parametrize("train", [False, True])
def test_clipped_render_argument_checks(train):
    lib = _lib()
    for probes in (0, 4097):
        _refused(_render(lib, train, probes=probes), lib, b"probes")
    _refused(_render(lib, train, pad=-2), lib, b"pad")
    _refused(_render(lib, train, near=6.0, far=2.0), lib, b"near < far")
    _refused(_render(lib, train, near=float("nan")), lib, b"near < far")
    for kc, kf in ((FILM, NERF), (NERF, FILM_NODIR)):
        _refused(_render(lib, train, kind_c=kc, kind_f=kf), lib, b"FiLM")
    _refused(_render(lib, train, bits=None), lib, b"null pointer")
    _refused(_render(lib, train, dims=_i3(0, 16, 16)), lib, b"grid dims")
    _refused(_render(lib, train, rgb_f=None), lib, b"null pointer")
    extra = lib.mi_render_occupancy_train_extra_bytes if train else lib.mi_render_occupancy_extra_bytes
    unclipped = lib.mi_render_workspace_bytes(100, 8, 16) + extra(100, 8, 16)
    need = unclipped + lib.mi_render_occupancy_clip_extra_bytes(100)
    _refused(_render(lib, train, ws_bytes=need - 1), lib, b"workspace of", str(need).encode(), b"clip_extra_bytes")
    _refused(_render(lib, train, ws_bytes=unclipped), lib, b"workspace of")             # the unclipped call's is too small
    # as in the unclipped calls: the inference call counts a null workspace among its null pointers, the training call sizes it
    _refused(_render(lib, train, ws=None), lib, b"workspace of" if train else b"null pointer")
    assert _render(lib, train, n=0) == 0


# ---- the restatement, counted by hand --------------------------------------------------------------------------------------------
# A (4,4,4) grid over [0,4)^3 (cells of edge 1, inv_cell 1) with the one occupied cell (2,1,1), near = 0, far = 8, M = 8: h = 1,
# probe k at depth k + 0.5.
LO, HI, DIMS = (0.0,) * 3, (4.0,) * 3, (4, 4, 4)
DENSE = np.zeros(DIMS, bool)
DENSE[2, 1, 1] = True
INV = ref.inv_cell_of(LO, HI, DIMS)


def _hand(rays, pad, dense=DENSE, plant=None, m=8, near=0.0, far=8.0):
    return cref.clip_bounds(torch.tensor(rays, dtype=torch.float32).reshape(-1, 2, 3), near, far, F(LO), INV, dense, m, pad, plant)


def test_restatement_by_hand():
    assert np.array_equal(INV, np.ones(3, F))
    assert np.array_equal(cref.probe_depths(0.0, 8.0, 8), np.arange(8, dtype=F) + F(0.5))
    # along +x from x = -1 at y = z = 1.5: probe k at x = k - 0.5; the cell 2 <= x < 3 holds probe 3 alone: k0 = k1 = 3
    through = [[-1.0, 1.5, 1.5], [1.0, 0.0, 0.0]]
    mask = cref.probe_mask(torch.tensor([through]), 0.0, 8.0, F(LO), INV, DENSE, 8)
    assert mask.tolist() == [[False, False, False, True, False, False, False, False]]
    assert _hand(through, 0).tolist() == [[3.0, 4.0]]                         # a = 3, b = 4
    assert _hand(through, 1).tolist() == [[2.0, 5.0]]                         # a = 2, b = 5
    assert _hand(through, 3).tolist() == [[0.0, 7.0]]                         # a = max(0, 0), b = 7
    assert _hand(through, 4).tolist() == [[0.0, 8.0]]                         # a = max(-1, 0) = 0; b = min(8, 8) = M: far itself
    assert _hand(through, 100).tolist() == [[0.0, 8.0]]                       # pad clamped at both ends
    # the same ray at y = 2.5 passes the cell's neighbour: no probe is occupied, the bounds are (near, far)
    assert _hand([[-1.0, 2.5, 1.5], [1.0, 0.0, 0.0]], 1).tolist() == [[0.0, 8.0]]
    # a NaN direction: every point is a NaN, a NaN is outside
    assert _hand([[-1.0, 1.5, 1.5], [float("nan"), 0.0, 0.0]], 1).tolist() == [[0.0, 8.0]]
    # b == M returns far ITSELF, not near + M * h: near = 0.9, far = 2.78, M = 10 give fl(near + 10 * h) = 2.7799997 != 2.78
    near, far = F(0.9), F(2.78)
    h = (far - near) / F(10)
    assert F(near + F(10) * h) != far
    full = np.ones(DIMS, bool)
    inside = [[1.5, 1.5, 1.5], [0.25, 0.0, 0.0]]                             # every probe inside the box
    got = _hand(inside, 0, dense=full, m=10, near=near, far=far)
    assert got[0, 0] == near and got[0, 1] == far
    # the last probe alone occupied, pad 0: b = M
    last = [[-5.0, 1.5, 1.5], [1.0, 0.0, 0.0]]                               # probe 7 at x = 2.5
    assert _hand(last, 0).tolist() == [[7.0, 8.0]]
    assert _hand(last, 2).tolist() == [[5.0, 8.0]]
    # the first probe alone occupied
    first = [[2.0, 1.5, 1.5], [1.0, 0.0, 0.0]]                               # probe 0 at x = 2.5, probe 1 at 3.5
    assert _hand(first, 0).tolist() == [[0.0, 1.0]]
    assert _hand(first, 2).tolist() == [[0.0, 3.0]]
    # the planted mistakes, on the ray through the cell
    assert _hand(through, 0, plant="k1_not_k1_plus_1").tolist() == [[3.0, 3.0]]
    assert _hand(through, 4, plant="pad_not_clamped").tolist() == [[-1.0, 8.0]]
    # probes at the bin edges: probe k at x = k - 1, the cell holds probe 3 (x = 2) as well - but a ray offset by half a bin does not
    half = [[-0.5, 1.5, 1.5], [1.0, 0.0, 0.0]]                               # midpoints at x = k: probe 2 (x = 2) in [2, 3)
    assert _hand(half, 0).tolist() == [[2.0, 3.0]]
    assert _hand(half, 0, plant="probes_at_bin_edges").tolist() == [[3.0, 4.0]]  # edges at x = k - 0.5: probe 3 (x = 2.5)
    # `<=` at the upper face: a probe exactly on x = 4 of a full grid counts as inside
    face = [[-0.5, 1.5, 1.5], [1.0, 0.0, 0.0]]                               # probe 0 at x = 0 (inside: 0 <= t) .. probe 4 at x = 4.0 (outside)
    assert _hand(face, 0, dense=full).tolist() == [[0.0, 4.0]]
    assert _hand(face, 0, dense=full, plant="hi_inclusive").tolist() == [[0.0, 5.0]]


def test_restated_samplers():
    # linspace_at: the symmetric halves of ATen's scalar formula, by hand for 5 steps over [2, 6]
    assert cref.linspace_at([2.0], [6.0], 5).tolist() == [[2.0, 3.0, 4.0, 5.0, 6.0]]
    assert cref.linspace_at([2.0], [6.0], 1).tolist() == [[2.0]]
    lin = cref.linspace_at([0.1, 2.0], [0.7, 6.0], 4)
    step = (F(0.7) - F(0.1)) / F(3)
    assert lin[0].tolist() == [F(0.1), F(F(0.1) + step * F(1)), F(F(0.7) - step * F(1)), F(0.7)]
    # u = 0 gives the lower edges, the first being the range's own start; depths ascend inside each ray's range
    b = np.array([[2.0, 6.0], [3.0, 3.5]], F)
    z0 = cref.sample_coarse_bounds(b, 5, torch.zeros(2, 5))
    assert z0[:, 0].tolist() == [2.0, 3.0] and z0[0].tolist() == [2.0, 2.5, 3.5, 4.5, 5.5]
    z = cref.sample_coarse_bounds(b, 5, synth.t_rand(2, 5, seed=1))
    assert bool((np.diff(z, axis=1) > 0).all()) and bool((z >= b[:, :1]).all()) and bool((z <= b[:, 1:]).all())
    # every ray on (near, far): the oracle's stratified depths, to the 1 ulp by which ATen's vectorised linspace may differ
    tr = synth.t_rand(7, 16, seed=2)
    zo, _ = R.stratified_z(7, 2.0, 6.0, 16, tr)
    zb = cref.sample_coarse_bounds(np.tile(np.array([[2.0, 6.0]], F), (7, 1)), 16, tr)
    assert float(np.abs(zb - zo.numpy()).max()) <= 2 * float(np.spacing(F(6.0)))
    # the fine sampler: Nc + Nf ascending depths that contain the coarse ones, inside the ray's range
    w = torch.rand(2, 5, generator=torch.Generator().manual_seed(3))
    zs, zf = cref.sample_fine_bounds(b, torch.from_numpy(z), w, 3)
    assert tuple(zs.shape) == (2, 3) and tuple(zf.shape) == (2, 8) and bool((zf[:, 1:] >= zf[:, :-1]).all())
    assert bool((zs >= torch.from_numpy(b[:, :1])).all()) and bool((zs <= torch.from_numpy(b[:, 1:])).all())


# ---- the GPU test's own inputs ---------------------------------------------------------------------------------------------------
def _all_cases(n):
    """{(M, grid index, pad): (bounds, hit)} of the kernel test's cases at n rays."""
    rays = cref.case_rays(n)
    out = {}
    for _n, m, name, dims, box in cref.clip_cases((n,)):
        gi = cref.CLIP_GRIDS.index((name, dims, box))
        mask = cref.probe_mask(rays, cref.NEAR, cref.FAR, F(box[0]), ref.inv_cell_of(box[0], box[1], dims), cref.case_dense(name, dims), m)
        k0, k1, hit = cref.first_last(mask)
        for pad in cref.CLIP_PAD:
            out[(m, gi, pad)] = (cref.bounds_from(k0, k1, hit, cref.NEAR, cref.FAR, m, pad), hit)
    return out


def test_conditions_on_the_gpu_inputs():
    near, far = F(cref.NEAR), F(cref.FAR)
    n = max(cref.CLIP_N)
    cases = _all_cases(n)
    assert len(cases) == len(cref.CLIP_M) * len(cref.CLIP_GRIDS) * len(cref.CLIP_PAD)
    fewest = dict(miss=n, whole=n, inside=n)                                  # over the cases in which some ray hits
    most_inside, kinds = 0, set()
    for (m, gi, pad), (b, hit) in cases.items():
        assert b.dtype == np.float32 and b.shape == (n, 2)
        assert bool((b[:, 0] < b[:, 1]).all()), (m, gi, pad)                  # near_r < far_r on every ray
        assert bool((b[:, 0] >= near).all()) and bool((b[:, 1] <= far).all())
        assert bool((b[~hit] == np.array([near, far])).all())
        kinds.add("none" if not hit.any() else "all" if hit.all() else "some")
        if not hit.any():
            continue
        fewest["miss"] = min(fewest["miss"], int((~hit).sum()))
        most_inside = max(most_inside, int((hit & (b[:, 0] > near) & (b[:, 1] < far)).sum()))
    assert kinds == {"none", "some"}                                          # the NaN ray never hits; the empty grid: nobody does
    assert fewest["miss"] >= 4, fewest                                        # in EVERY case: the NaN ray and the three that point away
    # the special rays do what their descriptions say, at 64 probes under the full 16^3 grid over BOX
    full = cref.CLIP_GRIDS.index(("ones", (16, 16, 16), cref.BOX))
    b, hit = cases[(64, full, 0)]
    assert hit[:cref.N_SPECIAL].tolist() == [True, False, False, False, False, True]
    assert b[0].tolist() == [2.0, 2.0 + 10.0 / 16.0]                          # probes 0..9 in front of the face x = 4, probe 10 on it
    rest = slice(cref.N_SPECIAL, None)
    assert bool(hit[rest].all()) and bool((b[rest] == np.array([near, far])).all())   # BOX holds every sample of the camera's rays
    assert int(hit[rest].sum()) >= 4                                          # hit rays whose bounds are the whole range
    # both bounds strictly inside: the box the rays partly leave, 64 probes, pad 1
    small = cref.CLIP_GRIDS.index(("ones", (16, 16, 16), cref.SMALL))
    b, hit = cases[(64, small, 1)]
    strictly = hit & (b[:, 0] > near) & (b[:, 1] < far)
    print(f"SMALL box, 64 probes, pad 1: {int(strictly.sum())} of {n} rays with both bounds strictly inside; most in any case {most_inside}")
    assert int(strictly.sum()) >= 4


@pytest.mark.parametrize("plant", cref.PLANTS)
def test_planted_mistakes_change_the_gpu_cases(plant):
    """Each mistake gives other bits than the rule in some case of the kernel test, at every n but the single ray (whose one
    ray is the ray with a probe on the face: it tells `<=` from `<` and k1 from k1 + 1)."""
    for n in cref.CLIP_N:
        rays = cref.case_rays(n)
        differs = 0
        for _n, m, name, dims, box in cref.clip_cases((n,)):
            lo, inv, dense = F(box[0]), ref.inv_cell_of(box[0], box[1], dims), cref.case_dense(name, dims)
            for pad in cref.CLIP_PAD:
                want = cref.clip_bounds(rays, cref.NEAR, cref.FAR, lo, inv, dense, m, pad)
                got = cref.clip_bounds(rays, cref.NEAR, cref.FAR, lo, inv, dense, m, pad, plant)
                differs += not np.array_equal(want.view(np.int32), got.view(np.int32))
        print(f"{plant}: n = {n}: {differs} cases differ")
        assert differs > 0, (plant, n)


# ---- the clipped training cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(tref.GRAD_CASES))
def test_fp32_oracle_of_the_clipped_training_cases_is_inside_the_hard_gates(case):
    kind = tref.GRAD_CASES[case][0]
    b = cref.train_case_bounds(case)
    full = case.endswith("_ones")
    whole = (b == np.array([tref.NEAR, tref.FAR], F)).all(1)
    assert bool(whole.all()) if full else int((~whole).sum()) >= 4, (case, int(whole.sum()))   # the clip really moves bounds
    z_c, m_c, z_f, m_f = cref.train_oracle_depths(case)
    for m in (m_c, m_f):
        assert bool(m.all()) if full else 0 < int(m.sum()) < m.numel(), (case, int(m.sum()), m.numel())
    refs = tref.case_refs(case, z_c, m_c, z_f, m_f)
    worst = 0.0
    for f, (r32, r64) in enumerate(zip(refs[torch.float32], refs[torch.float64])):
        for name in r32:
            rec = parity.gate_grad(f"host clipped {case}: masked oracle fp32 vs fp64", ("coarse." if f == 0 else "fine.") + name,
                                   r32[name], r32[name], r64[name], check=True, **tref.case_gates(kind))
            assert rec["active"] == "hard", rec
            assert float(r64[name].abs().max()) > 0, (case, name)
            worst = max(worst, rec["rel_l2_err"])
    print(f"clipped {case}: fp32 oracle within {worst:.3g} (rel l2) of fp64")

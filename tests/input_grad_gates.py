"""Stage D of the field backward: the gradient to a point's six inputs and to the rays (csrc/ray_grad.hip), rebuilt in
float64 from the kernels' OWN inputs - the dA rows of the input-consuming layers, those layers' weights, the saved encoding
rows and the FiLM table - and gated per element (test_gpu_input_grad_gates.py, test_input_grad_gates_host.py): torch only.

The consuming layers, their dA regions, weight columns and FiLM rows are read from bwd_gates.network(kind): the `In`s whose
region is E_pos, E_dir or xin.  Nothing flips between the kernel and this restatement (the ReLU switches are already in dA),
so the gate is |got - ref64| <= gamma_c mag with gamma_c = c u / (1 - c u), u = 2^-24, mag the reference's expression over
absolute values and c COUNTED from ray_grad.hip: the number of fp32 roundings on the longest path from a product to the
stored float (a fused multiply-add rounds once where the count below takes two, so contraction only shortens a path).

  lin kernel (sin kinds), per point and component
      position   1 gamma (.) dA  + 1 product + 3 adds of a lane's four features + 1 add of the skip layer's row   =  6 in the lane
      direction  1 + 1 + 3                                                                                         =  5 in the lane
      point form: + 6 levels of wave_sum                                          position 12, direction 11
  PE kernel (ReLU kinds), per point and component
      dE         pe_contract is ONE sequential fmaf chain over all K dA features of a lane's encoding column: the first
                 product is rounded K times; K = 256 per position layer (NeRF: both layers run into the same chain, 512;
                 TinyNeRF 256), 128 for the direction layer
      t          (dE * E_mate) * (+-2^i): 1 rounding, the power of two is exact                 K + 1 in the lane
      point form: + 6 levels of wave_sum                                          position K + 7, direction 135
  ray form, per ray (S samples), from the in-lane counts above (lane_pos, lane_dir)
      g_o        lane_pos + S adds into the lane's sum + 6 levels                                lane_pos + S + 6
      g_d, z     lane_pos + 1 (z_s *) + S + 6 + 1 (store_ray's final add)                        lane_pos + S + 8
      g_d, sv    lane_dir + S + 6 + store_ray's longest path, 18: |d| = sqrt(d . d) carries 3 (two adds, the root halves
                 the sum's 3 and rounds once), v_i = d_i / |d| 4, v_i sv_i 5, two adds 7, v_j (v . sv) 12, sv_j - . 13,
                 / |d| 17, sz_j + . 18 (hipcc's default fp32 division and square root are correctly rounded)
                                                                                                  lane_dir + S + 24

The launch's own formulas (launch_input_grad) are mirrored in `launch_plan`, as bwd_gates.slabs_for mirrors the planner."""
from __future__ import annotations

import torch

import bwd_gates as G
from oracle import parity

U = G.U
CHUNK = 32                      # points of a point-form unit (kChunk)
PE_WAVES, LIN_WAVES = 16, 4     # waves (= units in flight) of a block: kPeThreads / 64, 256 / 64
LIN_BLOCKS_PER_CU = 8
WAVE_SUM = 6                    # levels of the butterfly over 64 lanes
C_STORE_RAY = 18                # store_ray's longest path (module docstring)
PE_KINDS = ("nerf", "tiny_nerf")


def gamma_c(c: float) -> float:
    """The bound on (1 + d_1) .. (1 + d_c) - 1 with every |d_i| <= u."""
    return c * U / (1.0 - c * U)


# ---- the launch ------------------------------------------------------------------------------------------------------
def units_for(ray_form: bool, n_groups: int, per_group: int) -> int:
    """Units of a launch: rays, or chunks of CHUNK points that do not straddle a group."""
    return n_groups * (per_group if ray_form else -(-per_group // CHUNK))


def sweep_units(pe: bool, cus: int) -> int:
    """Units the largest grid takes at once; past it a wave's loop runs `u += stride`."""
    return PE_WAVES * cus if pe else LIN_WAVES * LIN_BLOCKS_PER_CU * cus


def launch_plan(pe: bool, units: int, cus: int):
    """(blocks, units per sweep = the loop's stride) of launch_input_grad."""
    per_block = PE_WAVES if pe else LIN_WAVES
    cap = cus if pe else LIN_BLOCKS_PER_CU * cus
    blocks = min(-(-units // per_block), cap)
    return blocks, blocks * per_block


# ---- the consuming layers --------------------------------------------------------------------------------------------
def consumers(kind: str):
    """([(layer, In)] reading the position, (layer, In) reading the direction or None), from the kind's network."""
    pos, dr = [], None
    for lay in G.network(kind):
        for r in lay.ins:
            if r.region == "E_pos" or (r.region == "xin" and r.c0 == 0):
                pos.append((lay, r))
            elif r.region in ("E_dir", "xin"):
                assert dr is None, kind
                dr = (lay, r)
    assert 1 <= len(pos) <= 2, kind
    return pos, dr


def roundings(kind: str, n_samples: int = 0) -> dict:
    """The counted constants: point form {"pos", "dir"}; ray form (n_samples > 0) {"o", "d_z", "d_sv"}."""
    pos, dr = consumers(kind)
    if kind in PE_KINDS:
        lane_pos, lane_dir = 256 * len(pos) + 1, 128 + 1
    else:
        lane_pos, lane_dir = 1 + 1 + 3 + (len(pos) - 1), 1 + 1 + 3
    if not n_samples:
        return {"pos": lane_pos + WAVE_SUM, "dir": lane_dir + WAVE_SUM}
    return {"o": lane_pos + n_samples + WAVE_SUM, "d_z": lane_pos + 1 + n_samples + WAVE_SUM + 1,
            "d_sv": lane_dir + n_samples + WAVE_SUM + C_STORE_RAY}


# ---- the reference ---------------------------------------------------------------------------------------------------
def _contract(lay, r, D, params, film, ppg, dtype):
    """dA W over the layer's input columns r, and the same over absolute values; gamma of the point's image for FiLM."""
    dA = D[lay.grad].to(dtype)
    if lay.film is not None:
        P = dA.shape[0]
        img = torch.arange(P, device=dA.device) // ppg
        dA = dA * film[:, lay.film, :256].to(dtype)[img]
    W = lay.weight_cols(params[2 * lay.p], r).to(dtype)
    return dA @ W, dA.abs() @ W.abs()


def _through_encoding(E, dE, mag_dE, freqs):
    """dx_c = sum_i 2^i (E[6i+3+c] dE[6i+c] - E[6i+c] dE[6i+3+c]) and its magnitude, from the saved rows E."""
    P = E.shape[0]
    E = E[:, :6 * freqs].to(dE.dtype).reshape(P, freqs, 6)
    dE, mag_dE = dE.reshape(P, freqs, 6), mag_dE.reshape(P, freqs, 6)
    s = (2.0 ** torch.arange(freqs, device=E.device, dtype=dE.dtype)).view(1, freqs, 1)
    g = (s * (E[:, :, 3:] * dE[:, :, :3] - E[:, :, :3] * dE[:, :, 3:])).sum(1)
    mag = (s * (E[:, :, 3:].abs() * mag_dE[:, :, :3] + E[:, :, :3].abs() * mag_dE[:, :, 3:])).sum(1)
    return g, mag


def stage_d_points(kind, A, D, params, film, ppg, dtype=torch.float64):
    """(g_pos [P,3], its magnitude, g_dir [P,3], its magnitude) of every point, in `dtype` (float64: the reference;
    float32: torch's evaluation of the same contraction, recorded beside the kernel's error).  A, D: bwd_gates.regions of
    acts and grads_ws; film [groups, rows, 512] or None; ppg: points per group."""
    pos, dr = consumers(kind)
    g = mag = None
    for lay, r in pos:
        t, m = _contract(lay, r, D, params, film, ppg, dtype)
        g, mag = (t, m) if g is None else (g + t, mag + m)
    if kind in PE_KINDS:
        g, mag = _through_encoding(A["E_pos"], g, mag, 10)
    if dr is None:
        z = torch.zeros_like(g)
        return g, mag, z, z.clone()
    gd, magd = _contract(dr[0], dr[1], D, params, film, ppg, dtype)
    if kind in PE_KINDS:
        gd, magd = _through_encoding(A["E_dir"], gd, magd, 4)
    return g, mag, gd, magd


def stage_d_rays(g_pos, mag_pos, g_dir, mag_dir, rays, z):
    """Per ray, from the points' values [n * S, 3]: (g_o, mag_o, g_d, mag of g_d's z part, mag of its sv part)."""
    n, S = z.shape
    dt = g_pos.dtype
    zz = z.to(dt)[..., None]
    gp, mp = g_pos.reshape(n, S, 3), mag_pos.reshape(n, S, 3)
    d = rays[:, 1].to(dt)
    nrm = d.norm(dim=-1, keepdim=True)
    v = d / nrm
    sv, msv = g_dir.reshape(n, S, 3).sum(1), mag_dir.reshape(n, S, 3).sum(1)
    g_d = (zz * gp).sum(1) + (sv - v * (v * sv).sum(-1, keepdim=True)) / nrm
    mag_sv = (msv + v.abs() * (v.abs() * msv).sum(-1, keepdim=True)) / nrm
    return gp.sum(1), mp.sum(1), g_d, (zz.abs() * mp).sum(1), mag_sv


# ---- the gate ----------------------------------------------------------------------------------------------------------
def _rms(x) -> float:
    return float(x.double().pow(2).mean().sqrt()) if x.numel() else 0.0


def gate_d(case: str, tensor: str, got, ref, bound, active: str, ref32=None) -> bool:
    """One parity record like bwd_gates.gate's, with the kernel's RMS error against fp64 and, where ref32 is given, that of
    torch's fp32 evaluation of the same contraction (err_vs_fp32_reference: recorded, not gated)."""
    worst, where = G.worst_ratio(got, ref, bound)
    extra = {}
    if ref32 is not None:
        extra = dict(rms_err_vs_fp64=_rms(got.double() - ref), err_vs_fp32_reference=_rms(ref32.double() - ref))
    rec = parity.record(case=case, stage="D input grad", qty=tensor, err_over_bound=worst, active=active,
                        elements=int(got.numel()), worst_index=where, passed=bool(worst <= 1.0), **extra)
    return rec["passed"]


def check_points(case, kind, got, A, D, params, film, ppg, with_fp32=True) -> bool:
    """Gate g_x [P,6] of the point form; exact zeros where every consumed dA row of a point is zero and for a kind without
    a direction input."""
    c = roundings(kind)
    gp, mp, gd, md = stage_d_points(kind, A, D, params, film, ppg)
    r32 = stage_d_points(kind, A, D, params, film, ppg, torch.float32) if with_fp32 else None
    ok = gate_d(case, "g_x position", got[:, :3], gp, gamma_c(c["pos"]) * mp, f"gamma({c['pos']}) mag",
                None if r32 is None else r32[0])
    ok &= gate_d(case, "g_x direction", got[:, 3:], gd, gamma_c(c["dir"]) * md, f"gamma({c['dir']}) mag",
                 None if r32 is None else r32[2])
    ok &= _exact_zeros(case, kind, got, D, 1)
    return bool(ok)


def check_rays(case, kind, got, A, D, params, film, rpg, rays, z, with_fp32=True) -> bool:
    """Gate g_rays [n,2,3] of the ray form (accumulate = 0)."""
    S = z.shape[1]
    c = roundings(kind, S)

    def ref(dtype):
        return stage_d_rays(*stage_d_points(kind, A, D, params, film, rpg * S, dtype), rays, z)

    g_o, m_o, g_d, m_z, m_sv = ref(torch.float64)
    r32 = ref(torch.float32) if with_fp32 else None
    ok = gate_d(case, "g_rays origin", got[:, 0], g_o, gamma_c(c["o"]) * m_o, f"gamma({c['o']}) mag",
                None if r32 is None else r32[0])
    ok &= gate_d(case, "g_rays direction", got[:, 1], g_d, gamma_c(c["d_z"]) * m_z + gamma_c(c["d_sv"]) * m_sv,
                 f"gamma({c['d_z']}) mag_z + gamma({c['d_sv']}) mag_sv", None if r32 is None else r32[2])
    ok &= _exact_zeros(case, kind, got.reshape(-1, 6), D, S, ray_form=True)
    return bool(ok)


def _exact_zeros(case, kind, got, D, S, ray_form=False) -> bool:
    """A point / ray whose consumed dA rows are all zero gives exactly 0 (+0 or -0); the point form of a kind without a
    direction input gives exactly 0 in columns 3..5."""
    pos, dr = consumers(kind)
    live = None
    for lay, _ in pos + ([dr] if dr else []):
        nz = (D[lay.grad] != 0).any(1)
        live = nz if live is None else live | nz
    dead = ~live.reshape(-1, S).any(1)
    ok = bool((got[dead] == 0).all())
    if dr is None and not ray_form:
        ok &= bool((got[:, 3:] == 0).all())
    rec = parity.record(case=case, stage="D input grad", qty="exact zeros", err_over_bound=0.0 if ok else float("inf"),
                        active="exact", elements=int(dead.sum()), worst_index=-1, passed=ok)
    return rec["passed"]

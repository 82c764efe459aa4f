"""GPU: device marching cubes (mirender.mesh) against skimage.measure.marching_cubes_lewiner (fixtures F11,
tests/golden/make_golden_mesh.py), at scale, past 2^31 voxels, and create_mesh's PLY end to end."""
import os

import numpy as np
import pytest
import torch

from mirender import fields, mesh
from mirender.grid import density_grid
from mesh_gates import (boundary_gate, closed_manifold, decider_zero_cubes, edge_keys, parse_ply, tie_cubes,
                        touches_border, vertex_gate)
from oracle import parity, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SURFACES = ["m1", "m2", "m3", "m4", "m5"]


def fixture(name):
    return dict(np.load(os.path.join(GOLDEN, f"mesh_f11_{name}.npz")))


def run(d, **kw):
    out = mesh.marching_cubes(torch.from_numpy(d["volume"]).cuda(), float(d["level"]), tuple(d["spacing"]), **kw)
    return [t.cpu().numpy() for t in out]


def gradient_normals(vol, level, verts, spacing):
    """The documented normal: np.gradient interpolated along the vertex's edge, normalised, toward lower values.
    Returns (normals, mask of the vertices it applies to: edge vertices)."""
    g = np.stack(np.gradient(vol.astype(np.float64)), -1)
    X, Y, Z = vol.shape
    keys = edge_keys(verts, vol.shape, spacing)
    ok = keys >= 0
    c, a = np.divmod(keys[ok], 3)
    lo = np.stack([c // (Y * Z), (c // Z) % Y, c % Z], 1)
    hi = lo.copy()
    hi[np.arange(len(hi)), a] += 1
    a0 = vol[tuple(lo.T)].astype(np.float64) - level
    a1 = vol[tuple(hi.T)].astype(np.float64) - level
    t = (-a0 / (a1 - a0))[:, None]
    n = g[tuple(lo.T)] + t * (g[tuple(hi.T)] - g[tuple(lo.T)])
    return -n / np.linalg.norm(n, axis=1, keepdims=True), ok


@pytest.mark.parametrize("name", SURFACES)
def test_matches_skimage(name):
    d = fixture(name)
    shape, sp = d["volume"].shape, tuple(d["spacing"])
    verts, faces, normals, values = run(d)
    assert verts.dtype == np.float32 and faces.dtype == np.int32 and normals.dtype == np.float32
    max_ulp = 0 if sp == (1.0, 1.0, 1.0) else 1
    vr = vertex_gate(d["verts"], verts, shape, sp, max_ulp=max_ulp)
    ties = tie_cubes(d["volume"], float(d["level"]))
    ex = decider_zero_cubes(d["volume"], float(d["level"])) | ties
    br = boundary_gate(d["verts"], d["faces"], verts, faces, shape, sp, exempt=ex)
    gn, on_edge = gradient_normals(d["volume"], float(d["level"]), verts, sp)
    nerr = float(np.abs(normals[on_edge] - gn).max())
    # values: skimage stores max - min of one cube holding the edge; ours is the first such cube in C order
    same_value = float(np.mean(values[vr["index_got"]] == d["values"][vr["index_ref"]]))
    parity.record(case=f"F11 {name}", stage="marching_cubes", qty="verts", err_vs_oracle32=float(vr["max_ulp"]),
                  tol=float(max_ulp), active="hard", passed=vr["passed"], matched=vr["matched"],
                  centre_vertices=vr["centre_vertices"], tie_vertices=vr["tie_vertices"], cubes=br["cubes"],
                  cubes_differ=br["differ"], skipped_cubes=br["skipped_cubes"], exempt_cubes=br["exempt_cubes"],
                  unassigned_ref=br["unassigned_ref"], normals_err=nerr, values_equal_skimage=same_value)
    print(name, {k: v for k, v in vr.items() if not k.startswith("index")}, br, "normals", nerr, "values", same_value)
    if name == "m4":
        # integer volume: ties put vertices on corners, and some of Lewiner's centre vertices land on two integer
        # coordinates (so they look like edge vertices); every edge vertex of ours is skimage's, bit for bit
        assert vr["extra"] == 0 and vr["missing"] <= vr["centre_vertices"] and vr["max_ulp"] == 0, vr
    else:
        assert vr["passed"], vr
    assert br["passed"], br
    assert nerr < 1e-5


@pytest.mark.parametrize("name", ["m1", "m2", "m3", "m5"])
def test_whole_mesh(name):
    d = fixture(name)
    shape, sp = d["volume"].shape, tuple(d["spacing"])
    verts, faces, _, _ = run(d)
    closed, euler, comps = closed_manifold(faces, len(verts))
    if not touches_border(d["verts"], shape, sp):
        assert closed
    if name in ("m1", "m2", "m5"):
        ref = closed_manifold(d["faces"], len(d["verts"]))
        assert (euler, comps) == ref[1:], (euler, comps, ref)
        if name == "m1":
            assert (euler, comps) == (2, 1)
        if name == "m2":
            assert euler == 0
    else:
        rc, centre, _ = __import__("mesh_gates").cube_triangles(d["verts"], d["faces"], shape, sp)
        print(f"{name}: {len(centre)} cubes whose interior Lewiner tunnels through a centre vertex")


def test_deterministic_and_ascent():
    d = fixture("m3")
    a = run(d)
    b = run(d)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    asc = run(d, gradient_direction="ascent")
    assert np.array_equal(asc[0], a[0]) and np.array_equal(asc[1], a[1][:, [0, 2, 1]])


def test_level_outside_range():
    d = fixture("m6")
    assert str(d["error"]) == mesh.RANGE_ERROR
    with pytest.raises(ValueError, match="Surface level must be within volume data range."):
        mesh.marching_cubes(d["volume"], float(d["level"]))


def test_sphere_256():
    n, r, c = 256, 100.0, 127.3
    ax = torch.arange(n, device="cuda", dtype=torch.float64) - c
    vol = (torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - r).float()
    verts, faces, _, _ = mesh.marching_cubes(vol, 0.0)
    v, f = verts.double(), faces.long()
    closed, euler, comps = closed_manifold(faces.cpu().numpy(), len(verts))
    assert closed and euler == 2 and comps == 1
    area = 0.5 * torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).norm(dim=1).sum().item()
    assert abs(area / (4 * np.pi * r * r) - 1) < 0.01, area
    # trilinear value at each vertex (on an edge: linear along it) equals the level
    vn = vol.double()
    lo = v.floor().long().clamp(max=n - 2)
    t = v - lo
    val = torch.zeros(len(v), dtype=torch.float64, device="cuda")
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                w = (t[:, 0] if dx else 1 - t[:, 0]) * (t[:, 1] if dy else 1 - t[:, 1]) * (t[:, 2] if dz else 1 - t[:, 2])
                val += w * vn[lo[:, 0] + dx, lo[:, 1] + dy, lo[:, 2] + dz]
    err = val.abs().max().item()
    parity.record(case="sphere 256^3", stage="marching_cubes", qty="trilinear level", err_vs_oracle32=err, tol=1e-5,
                  active="hard", passed=err < 1e-5, area_ratio=area / (4 * np.pi * r * r))
    assert err < 1e-5


def test_index_width_past_2_31_voxels():
    X, Y, Z = 2048, 2048, 520
    vol = torch.empty((X, Y, Z), dtype=torch.float32, device="cuda")
    vol.copy_((torch.arange(X, device="cuda", dtype=torch.float32) - 1000.25).view(X, 1, 1).expand(X, Y, Z))
    assert vol.numel() > 2 ** 31
    verts, faces, _, _ = mesh.marching_cubes(vol, 0.0)
    del vol
    assert verts.shape == (Y * Z, 3) and faces.shape == (2 * (Y - 1) * (Z - 1), 3)
    assert bool((verts[:, 0] == 1000.25).all())
    yz = torch.arange(Y * Z, device="cuda")
    assert torch.equal(verts[:, 1], (yz // Z).float()) and torch.equal(verts[:, 2], (yz % Z).float())
    assert int(faces.min()) == 0 and int(faces.max()) == Y * Z - 1


def test_create_mesh_ply_end_to_end(tmp_path):
    d = fixture("m5")
    sd = synth.state_dict(str(d["field_kind"]), seed=int(d["field_seed"]), sharp=bool(d["field_sharp"]))
    film = synth.film_params(1, seed=int(d["field_film_seed"]))[0].cuda()
    field = fields.FilmSirenNeRF(use_dir=True).cuda()
    field.load_state_dict(sd)
    vs = 0.2 / 47
    sdf = density_grid(field, 48, 65536, film=film)
    path = tmp_path / "mesh.ply"
    mesh.convert_sdf_samples_to_ply(sdf, [-0.1, -0.1, -0.1], vs, str(path), level=float(d["level"]))
    _, pv, pf = parse_ply(path.read_bytes())
    got = (pv.astype(np.float64) + 0.1) / vs
    ref = d["verts"].astype(np.float64) / vs
    kr, kg = edge_keys(ref, d["volume"].shape), edge_keys(np.round(got * 1e3) / 1e3, d["volume"].shape)
    common, ir, ig = np.intersect1d(kr[kr >= 0], kg[kg >= 0], return_indices=True)
    e = np.abs(ref[kr >= 0][ir] - got[kg >= 0][ig]).max(1)
    frac = len(common) / (kr >= 0).sum()
    within = float(np.mean(e <= 1e-3))
    # The HIP field and the oracle differ at fp32 rounding, amplified by the x50 sigma head of this field: an edge
    # whose corners are both within that noise of the level can gain or lose its crossing, and a near-flat crossing
    # moves.  Measured on the MI355X: 99.66 % of the oracle mesh's edges are shared.
    parity.record(case="F11 m5 create_mesh PLY", stage="marching_cubes", qty="verts / voxel",
                  err_vs_oracle32=float(e.max()), tol=1e-3, active="hard", passed=bool(frac >= 0.995 and within >= 0.999),
                  frac_edges_shared=float(frac), frac_within_tol=within)
    print("create_mesh PLY vs M5: edges shared", frac, "within 1e-3 voxel", within, "max", e.max())
    assert frac >= 0.995 and within >= 0.999, (frac, within, e.max())
    assert len(pf) > 500

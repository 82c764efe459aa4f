"""Mesh gates of the marching-cubes tests (test_mesh_host.py, test_gpu_mesh.py): numpy only.

A marching-cubes vertex lies on a grid edge: two of its index-space coordinates are integers.  Its edge key is
(linear index of the edge's low corner) * 3 + axis.  Vertices with three integer coordinates (a corner AT the level)
get key -2, Lewiner's cube-centre vertices (fewer than two integer coordinates) key -1."""
from collections import Counter, defaultdict

import numpy as np

TIE, CENTRE = -2, -1


def edge_keys(verts, shape, spacing=(1.0, 1.0, 1.0)):
    q = np.asarray(verts, np.float64) / np.asarray(spacing, np.float64)
    r = np.round(q)
    integral = np.abs(q - r) <= 1e-6 * np.maximum(1.0, np.abs(q))
    n_int = integral.sum(1)
    axis = np.argmin(integral, 1)
    lo = np.where(integral, r, np.floor(q)).astype(np.int64)
    X, Y, Z = shape
    keys = ((lo[:, 0] * Y + lo[:, 1]) * Z + lo[:, 2]) * 3 + axis
    keys[n_int == 3] = TIE
    keys[n_int < 2] = CENTRE
    return keys


def ulp_diff(a, b):
    """|a - b| in units in the last place of fp32 (both fp32-representable)."""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def vertex_gate(ref_verts, got_verts, shape, spacing=(1.0, 1.0, 1.0), max_ulp=0):
    """Every edge vertex of the reference has one on the same edge in `got` (and no other), positions within max_ulp.
    Returns a record dict; record['passed'] is the verdict."""
    kr, kg = edge_keys(ref_verts, shape, spacing), edge_keys(got_verts, shape, spacing)
    er, eg = kr >= 0, kg >= 0
    rec = dict(ref_vertices=len(kr), got_vertices=len(kg), centre_vertices=int((kr == CENTRE).sum()),
               tie_vertices=int((kr == TIE).sum()))
    if len(np.unique(kg[eg])) != eg.sum() or len(np.unique(kr[er])) != er.sum():
        rec.update(passed=False, why="two vertices on one edge")
        return rec
    sr, sg = set(kr[er].tolist()), set(kg[eg].tolist())
    rec.update(missing=len(sr - sg), extra=len(sg - sr))
    common = np.array(sorted(sr & sg), np.int64)
    ir = np.argsort(kr[er])[np.searchsorted(np.sort(kr[er]), common)]
    ig = np.argsort(kg[eg])[np.searchsorted(np.sort(kg[eg]), common)]
    vr = np.asarray(ref_verts)[er][ir].astype(np.float32)
    vg = np.asarray(got_verts)[eg][ig].astype(np.float32)
    u = int(ulp_diff(vr, vg).max()) if len(common) else 0
    rec.update(max_ulp=u, matched=len(common), index_ref=np.flatnonzero(er)[ir], index_got=np.flatnonzero(eg)[ig])
    rec["passed"] = rec["missing"] == 0 and rec["extra"] == 0 and u <= max_ulp
    return rec


def _cube_of(keys, shape):
    X, Y, Z = shape
    c = keys // 3
    a = keys % 3
    pts = np.stack([c // (Y * Z), (c // Z) % Y, c % Z], 1)
    lo = pts.min(0)
    d = pts - lo
    if (d > 1).any() or (d[np.arange(len(a)), a] != 0).any():
        return None
    return int((lo[0] * Y + lo[1]) * Z + lo[2])


def _cubes_holding(keys, shape):
    """Every cube that holds all the given edges."""
    X, Y, Z = shape
    sets = []
    for key in keys.tolist():
        c, a = divmod(key, 3)
        p = [c // (Y * Z), (c // Z) % Y, c % Z]
        o = [k for k in range(3) if k != a]
        cubes = set()
        for d0 in (0, 1):
            for d1 in (0, 1):
                q = list(p)
                q[o[0]] -= d0
                q[o[1]] -= d1
                if all(0 <= q[k] <= shape[k] - 2 for k in range(3)):
                    cubes.add((q[0] * Y + q[1]) * Z + q[2])
        sets.append(cubes)
    return set.intersection(*sets) if sets else set()


def tie_cubes(volume, level):
    """Cubes with a corner exactly at the level (its vertices sit on corners; no edge identifies them)."""
    t = np.asarray(volume, np.float64) == level
    X, Y, Z = t.shape
    bad = np.zeros((X - 1, Y - 1, Z - 1), bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                bad |= t[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz]
    idx = np.flatnonzero(bad.ravel())
    x, r = np.divmod(idx, (Y - 1) * (Z - 1))
    y, z = np.divmod(r, Z - 1)
    return set(((x * Y + y) * Z + z).tolist())


def _boundary(tris):
    cnt = Counter()
    for t in tris:
        for i in range(3):
            cnt[(t[i], t[(i + 1) % 3])] += 1
    return frozenset(e for e, n in cnt.items() if n == 1 and cnt[(e[1], e[0])] == 0)


def cube_triangles(verts, faces, shape, spacing=(1.0, 1.0, 1.0)):
    """{cube: [triangle as edge-key triple]}; also the cubes that cannot be compared (they hold a centre-vertex
    triangle, a triangle lying in a face shared by two cubes, or a vertex on a corner) and the count of triangles
    that cannot be assigned to one cube."""
    keys = edge_keys(verts, shape, spacing)
    out, centre, unassigned = defaultdict(list), set(), 0
    for f in np.asarray(faces):
        k = keys[f]
        if (k == TIE).any():
            unassigned += 1
            for v in np.asarray(verts, np.float64)[f[k == TIE]] / np.asarray(spacing, np.float64):
                p = np.round(v).astype(np.int64)
                for d in range(8):
                    q = p - np.array([(d >> 2) & 1, (d >> 1) & 1, d & 1])
                    if (q >= 0).all() and (q <= np.asarray(shape) - 2).all():
                        centre.add(int((q[0] * shape[1] + q[1]) * shape[2] + q[2]))
            continue
        if (k >= 0).all() and len(_cubes_holding(k, shape)) > 1:
            unassigned += 1
            centre |= _cubes_holding(k, shape)
            continue
        if (k == CENTRE).any():
            centre |= _cubes_holding(k[k >= 0], shape)
            continue
        cb = _cube_of(k, shape)
        if cb is None:
            unassigned += 1
            continue
        out[cb].append(tuple(k.tolist()))
    return out, centre, unassigned


def decider_zero_cubes(volume, level):
    """Cubes with an ambiguous face whose asymptotic decider is exactly 0."""
    v = np.asarray(volume, np.float64) - level
    X, Y, Z = v.shape
    bad = np.zeros((X - 1, Y - 1, Z - 1), bool)
    c = [[[v[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz] for dz in (0, 1)] for dy in (0, 1)] for dx in (0, 1)]
    faces = []
    for s in (0, 1):
        faces.append((c[s][0][0], c[s][1][0], c[s][1][1], c[s][0][1]))
        faces.append((c[0][s][0], c[1][s][0], c[1][s][1], c[0][s][1]))
        faces.append((c[0][0][s], c[1][0][s], c[1][1][s], c[0][1][s]))
    for a0, a1, a2, a3 in faces:
        i0, i1, i2, i3 = a0 > 0, a1 > 0, a2 > 0, a3 > 0
        amb = (i0 == i2) & (i1 == i3) & (i0 != i1)
        bad |= amb & (a0 * a2 - a1 * a3 == 0)
    idx = np.flatnonzero(bad.ravel())
    x, r = np.divmod(idx, (Y - 1) * (Z - 1))
    y, z = np.divmod(r, Z - 1)
    return set(((x * Y + y) * Z + z).tolist())


def boundary_gate(ref_verts, ref_faces, got_verts, got_faces, shape, spacing=(1.0, 1.0, 1.0), exempt=()):
    """Per cube, the directed boundary edges (triangle edges used by one triangle of that cube) are the same."""
    rc, centre, un_r = cube_triangles(ref_verts, ref_faces, shape, spacing)
    gc, centre_g, un_g = cube_triangles(got_verts, got_faces, shape, spacing)
    skip = centre | centre_g | set(exempt)
    cubes = (set(rc) | set(gc)) - skip
    differ = sorted(c for c in cubes if _boundary(rc.get(c, ())) != _boundary(gc.get(c, ())))
    return dict(cubes=len(cubes), differ=len(differ), first_differ=differ[:5], ref_skipped_cubes=len(centre),
                exempt_cubes=len(set(exempt) & (set(rc) | set(gc))), unassigned_ref=un_r, unassigned_got=un_g,
                skipped_cubes=len(skip), passed=not differ)


def closed_manifold(faces, n_verts):
    """Every undirected edge in exactly two faces, in opposite directions; returns (closed, euler, components)."""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    cnt = Counter(map(tuple, d.tolist()))
    closed = all(n == 1 and cnt.get((b, a), 0) == 1 for (a, b), n in cnt.items())
    used = np.unique(f)
    E = len(cnt) // 2
    parent = np.arange(n_verts)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in d.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    comps = len({find(int(u)) for u in used})
    return closed, len(used) - E + len(f), comps


def touches_border(verts, shape, spacing=(1.0, 1.0, 1.0)):
    q = np.asarray(verts, np.float64) / np.asarray(spacing, np.float64)
    return bool((q.min(0) <= 1e-6).any() or (q.max(0) >= np.asarray(shape) - 1 - 1e-6).any())


def parse_ply(data: bytes):
    """(header lines, verts [V,3] f32, faces [F,3] i32) of a binary little-endian triangle PLY."""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    nv = int(next(h for h in header if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in header if h.startswith("element face")).split()[-1])
    verts = np.frombuffer(data, "<f4", nv * 3, end).reshape(nv, 3)
    rows = np.frombuffer(data, [("n", "u1"), ("i", "<i4", (3,))], nf, end + nv * 12)
    assert len(data) == end + nv * 12 + nf * 13
    assert (rows["n"] == 3).all()
    return header, verts, rows["i"].copy()

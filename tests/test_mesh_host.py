"""CPU: the PLY writer, the marching-cubes workspace query and the mesh gates (tests/mesh_gates.py) - the gates are
shown to fail on deliberately broken copies of a fixture, so the GPU tests that use them can fail."""
import os

import numpy as np
import pytest

from mirender import _lib, mesh
from mesh_gates import boundary_gate, closed_manifold, parse_ply, vertex_gate

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture(name):
    return dict(np.load(os.path.join(GOLDEN, f"mesh_f11_{name}.npz")))


HEADER = ["ply", "format binary_little_endian 1.0", "element vertex {}", "property float x", "property float y",
          "property float z", "element face {}", "property list uchar int vertex_indices", "end_header"]


def test_ply_round_trip(tmp_path):
    d = fixture("m1")
    path = tmp_path / "m.ply"
    mesh.write_ply(str(path), d["verts"], d["faces"])
    header, v, f = parse_ply(path.read_bytes())
    assert header == [h.format(len(d["verts"])) if "vertex" in h and "element" in h else
                      h.format(len(d["faces"])) if "face" in h and "element" in h else h for h in HEADER]
    assert np.array_equal(v, d["verts"].astype(np.float32)) and np.array_equal(f, d["faces"])


def test_ply_empty_mesh(tmp_path):
    path = tmp_path / "e.ply"
    mesh.write_ply(str(path), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    header, v, f = parse_ply(path.read_bytes())
    assert "element vertex 0" in header and "element face 0" in header and v.shape == (0, 3) and f.shape == (0, 3)


def test_workspace_query_needs_no_gpu():
    lib = _lib.load()
    small = lib.mi_mc_workspace_bytes(17, 23, 31)
    assert small >= 2 * 17 * 23 * 31
    assert lib.mi_mc_workspace_bytes(2048, 2048, 520) >= 2 * 2048 * 2048 * 520     # int64 sizes
    assert lib.mi_mc_workspace_bytes(1, 5, 5) < 0 and b"at least 2" in lib.mi_last_error()


@pytest.mark.parametrize("name", ["m1", "m3"])
def test_gates_pass_on_the_fixture_itself(name):
    d = fixture(name)
    assert vertex_gate(d["verts"], d["verts"], d["volume"].shape)["passed"]
    assert boundary_gate(d["verts"], d["faces"], d["verts"], d["faces"], d["volume"].shape)["differ"] == 0


def test_gates_fail_on_broken_copies():
    d = fixture("m1")
    shape = d["volume"].shape
    v, f = d["verts"], d["faces"]
    flipped = f.copy()
    flipped[100] = flipped[100, ::-1]
    assert boundary_gate(v, f, v, flipped, shape)["differ"] >= 1
    assert not closed_manifold(flipped, len(v))[0]
    dropped = np.delete(f, 200, axis=0)
    assert boundary_gate(v, f, v, dropped, shape)["differ"] >= 1
    assert not closed_manifold(dropped, len(v))[0]
    moved = v.astype(np.float32).copy()
    ax = int(np.argmax(moved[7] != np.round(moved[7])))
    moved[7, ax] = np.nextafter(moved[7, ax], np.float32(np.inf))
    rec = vertex_gate(v, moved, shape)
    assert not rec["passed"] and rec["max_ulp"] == 1
    assert closed_manifold(f, len(v)) == (True, 2, 1)

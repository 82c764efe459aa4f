"""CPU: the four MFMA kernel units (the forward's three kernel families and the backward chain) depend, among the project's
files, on exactly the headers DESIGN.md 4.1 allows them, so an edit of a launcher declaration, of the render paths, of the
registry's host side or of an entry point in the public header recompiles none of them.  The prerequisites are the compiler's
own: the unit's dependency file under csrc/_obj when a build left a fresh one, else a preprocess-only run with csrc/build.py's
flags into a temporary directory."""
import os
import re
import shutil
import subprocess

import pytest

from test_build_deps import B, PKG

ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
SHARED = {"field_mlp_device.h", "field_layout.h", "field_kinds.h", "mi_math.h", "mi_device.h", "mi_host.h"}
UNITS = {
    "field_mlp_nerf.hip": "field_mlp_instances.h",
    "field_mlp_siren.hip": "field_mlp_instances.h",
    "field_mlp_film.hip": "field_mlp_instances.h",
    "field_bwd_chain.hip": "field_bwd.h",
}
FORBIDDEN = {"msra-practice-project_amd/csrc/launchers.h", "msra-practice-project_amd/csrc/render_path.h",
             "msra-practice-project_amd/csrc/field_kinds_host.h", "include/mi_render.h"}


def _allowed(unit):
    return {f"msra-practice-project_amd/csrc/{n}" for n in SHARED | {unit, UNITS[unit]}} | {"include/mi_render_kinds.h"}


def _project_deps(unit, tmp_path):
    """The files under the repository that the compiler names as prerequisites of `unit`, relative to the repository."""
    src = os.path.join(CSRC, unit)
    obj, dep = (os.path.join(B.OBJ, unit.replace(".hip", ext)) for ext in (".o", ".d"))
    if B.unit_stale(obj, src, dep) is not None:                     # no build, or one older than the sources: ask the compiler
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not (os.path.exists(hipcc) or shutil.which(hipcc)):
            pytest.skip("no hipcc and no fresh dependency file")
        dep = str(tmp_path / "unit.d")
        subprocess.check_call([hipcc, *B.COMMON, *B.SOURCES[unit], "-E", "-MD", "-MF", dep, src, "-o", str(tmp_path / "unit.i")],
                              timeout=600)
    with open(dep) as f:
        deps = {os.path.realpath(os.path.join(CSRC, d)) for d in B.parse_depfile(f.read())}
    deps.add(os.path.realpath(src))
    root = os.path.realpath(ROOT) + os.sep
    return {d[len(root):] for d in deps if d.startswith(root)}


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_mfma_unit_depends_on_its_allow_list_only(unit, tmp_path):
    deps = _project_deps(unit, tmp_path)
    assert deps == _allowed(unit)
    assert not deps & FORBIDDEN


def test_mi_common_is_gone():
    assert not os.path.exists(os.path.join(CSRC, "mi_common.h"))
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if os.path.isfile(path) and name.endswith((".h", ".hip", ".py")):
            with open(path) as f:
                assert not re.search(r'#\s*include\s*["<][^">\n]*mi_common\.h[">]', f.read()), f"{name} includes mi_common.h"

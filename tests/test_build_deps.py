"""csrc/build.py decides what to recompile from the dependency file the compiler wrote for each translation unit
(-MD -MF): the parser, and the staleness rule on files with set times.  No compiler, a temporary directory."""
import importlib.util
import os

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "msra-practice-project_amd")


def _build_module():
    spec = importlib.util.spec_from_file_location("mi_csrc_build", os.path.join(PKG, "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


B = _build_module()


def _touch(path, t):
    with open(path, "a"):
        pass
    os.utime(path, (t, t))
    return str(path)


def _unit(tmp_path, listed=("a.h", "b.h")):
    """A unit whose object (time 100) is newer than its source and both listed headers (time 50); returns obj, src, depfile."""
    src = _touch(tmp_path / "unit.hip", 50)
    hdrs = [_touch(tmp_path / h, 50) for h in listed]
    obj = _touch(tmp_path / "unit.o", 100)
    dep = tmp_path / "unit.d"
    dep.write_text(f"{obj}: {src} \\\n  " + " \\\n  ".join(hdrs) + "\n")
    return obj, src, str(dep)


def test_parse_depfile_continuation_lines():
    text = "_obj/unit.o: csrc/unit.hip csrc/a.h \\\n  /opt/include/hip/hip_runtime.h csrc/with\\ space.h\n"
    assert B.parse_depfile(text) == ["csrc/unit.hip", "csrc/a.h", "/opt/include/hip/hip_runtime.h", "csrc/with space.h"]
    assert B.parse_depfile("") == []


def test_fresh_unit_is_reused(tmp_path):
    obj, src, dep = _unit(tmp_path)
    assert B.unit_stale(obj, src, dep) is None


def test_listed_header_newer_than_object_is_stale(tmp_path):
    obj, src, dep = _unit(tmp_path)
    _touch(tmp_path / "b.h", 200)
    assert B.unit_stale(obj, src, dep)


def test_source_newer_than_object_is_stale(tmp_path):
    obj, src, dep = _unit(tmp_path)
    _touch(src, 200)
    assert B.unit_stale(obj, src, dep)


def test_unlisted_file_newer_is_not_stale(tmp_path):
    obj, src, dep = _unit(tmp_path)
    _touch(tmp_path / "unrelated.h", 200)
    assert B.unit_stale(obj, src, dep) is None


def test_missing_depfile_is_stale(tmp_path):
    obj, src, dep = _unit(tmp_path)
    os.remove(dep)
    assert B.unit_stale(obj, src, dep)


def test_missing_object_or_listed_file_is_stale(tmp_path):
    obj, src, dep = _unit(tmp_path)
    os.remove(tmp_path / "a.h")
    assert B.unit_stale(obj, src, dep)
    os.remove(obj)
    assert B.unit_stale(obj, src, dep)


def test_depfile_of_another_copy_of_the_tree_is_stale(tmp_path):
    """A built tree copied elsewhere: object and dependency file come along, and the file still names the first tree's source
    and headers - fresh, existing, and not what this tree's object would be compiled from."""
    first, second = tmp_path / "first", tmp_path / "second"
    first.mkdir(), second.mkdir()
    obj, src, dep = _unit(first)
    copy = [_touch(second / n, t) for n, t in (("unit.o", 100), ("unit.hip", 50), ("a.h", 50), ("b.h", 50))]
    (second / "unit.d").write_text(open(dep).read())
    assert B.unit_stale(obj, src, dep) is None
    assert "another tree" in B.unit_stale(copy[0], copy[1], str(second / "unit.d"))

"""CPU: the conventions of the Python binding that exist once - the size query, the debug guard, the buffers of a render
call, the decisions about a pair of fields and the pointer array.  No GPU: CPU tensors, and a stub in place of the loaded
library where a call is involved."""
import ctypes
import types

import pytest
import torch

from mirender import _lib, fields, ops


class StubLib:
    """What _lib.load() returns while a test runs: size queries that answer `value`, and a last-error text."""

    def __init__(self, value):
        self.value, self.asked = value, []

    def mi_some_bytes(self, *args):
        self.asked.append(args)
        return self.value

    def mi_last_error(self):
        return b"stub: kind 99 has no such size"


def test_query_returns_the_value_and_raises_with_the_last_error(monkeypatch):
    stub = StubLib(4096)
    monkeypatch.setattr(_lib, "_lib", stub)                   # load() hands out what it has loaded before
    got = _lib.query("mi_some_bytes", 3, 5)
    assert got == 4096 and type(got) is int and stub.asked == [(3, 5)]
    stub.value = 0
    assert _lib.query("mi_some_bytes") == 0                   # an empty buffer is not an error
    stub.value = -1
    with pytest.raises(_lib.MiRenderError, match="mi_some_bytes.*stub: kind 99 has no such size"):
        _lib.query("mi_some_bytes", 99)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_guard_off_is_a_plain_buffer(monkeypatch, dtype):
    monkeypatch.delenv("MI_DEBUG_GUARDS", raising=False)
    view, whole = _lib.guarded(100, dtype, "cpu")
    assert whole is None and view.numel() == 100 and view.dtype == dtype and view.untyped_storage().nbytes() == 100 * dtype.itemsize
    _lib.check_guard(whole, "nothing to check")


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
@pytest.mark.parametrize("n", [0, 1, 100, 4097])
def test_guard_catches_one_changed_unit_anywhere_in_the_tail(monkeypatch, dtype, n):
    monkeypatch.setenv("MI_DEBUG_GUARDS", "1")
    tail = _lib.GUARD_BYTES // dtype.itemsize                # 4 096 floats and 16 384 bytes are the same tail
    view, whole = _lib.guarded(n, dtype, "cpu")
    assert view.numel() == n and view.dtype == dtype and whole.numel() == n + tail
    # the first n units of the guarded buffer, not a copy
    assert view.untyped_storage().data_ptr() == whole.untyped_storage().data_ptr() and view.storage_offset() == 0
    view.fill_(0)                                            # writing all the caller asked for touches no sentinel
    _lib.check_guard(whole, "untouched")
    for at in (0, 1, tail // 2, tail - 1):
        keep = whole[n + at].clone()
        whole[n + at] = 0
        with pytest.raises(_lib.MiRenderError, match=f"rows of layer 3.* wrote {(at + 1) * dtype.itemsize} bytes past the end"):
            _lib.check_guard(whole, "rows of layer 3")
        whole[n + at] = keep
        _lib.check_guard(whole, "restored")


def test_autograd_keeps_the_float_guard_under_its_names(monkeypatch):
    from mirender import autograd
    monkeypatch.setenv("MI_DEBUG_GUARDS", "1")
    view, whole = autograd._guarded(100, "cpu")
    assert view.dtype == torch.float32 and view.numel() == 100 and whole.numel() == 100 + 4096
    autograd._check_guard(whole, "untouched")
    whole[100 + 5] = 0.0
    with pytest.raises(_lib.MiRenderError, match="touched.*past the end"):
        autograd._check_guard(whole, "touched")
    monkeypatch.delenv("MI_DEBUG_GUARDS")
    view, whole = autograd._guarded(7, "cpu")
    assert whole is None and view.numel() == 7


@pytest.mark.parametrize("n", [0, 1, 129])
def test_render_outputs(n):
    outs = ops._render_outputs(n, "cpu")
    assert [tuple(o.shape) for o in outs] == [(n, 3), (n,), (n,), (n, 3), (n,), (n,)]
    assert all(o.dtype == torch.float32 and o.device.type == "cpu" for o in outs)
    fine_only = ops._render_outputs(n, "cpu", coarse_outputs=False)
    assert fine_only[:3] == [None, None, None]
    assert [tuple(o.shape) for o in fine_only[3:]] == [(n, 3), (n,), (n,)]


def test_t_rand_is_converted_and_checked():
    assert ops._t_rand(None, 4, 8, "cpu") is None
    t = ops._t_rand(torch.rand(4, 8, dtype=torch.float64).t().contiguous().t(), 4, 8, "cpu")
    assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (4, 8)
    for bad in (torch.rand(4, 7), torch.rand(5, 8), torch.rand(32)):
        with pytest.raises(_lib.MiRenderError, match=r"t_rand must be \[4,8\]"):
            ops._t_rand(bad, 4, 8, "cpu")


def test_lin_tables():
    zl, ul = ops._lin_tables(2.0, 6.0, 8, 16, "cpu")
    assert torch.equal(zl, torch.linspace(2.0, 6.0, 8)) and torch.equal(ul, torch.linspace(0.0, 1.0, 16))
    assert ops._lin_tables(2.0, 6.0, 8, 0, "cpu")[1] is None          # Nf = 0: no inverse CDF
    assert ops._lin_tables(2.0, 6.0, 8, 16, "cpu", exact_linspace=False) == (None, None)


def packed(model):
    """What the functions over a pair read of a PackedField (which itself needs the model on a device)."""
    return types.SimpleNamespace(kind=model.KIND, params=list(model.parameters()), device=torch.device("cpu"))


def test_resolve_film():
    film_m, plain_m = fields.FilmSirenNeRF(), fields.NeRF()
    film_pf, plain_pf = packed(film_m), packed(plain_m)
    own = torch.arange(9 * 512, dtype=torch.float32).reshape(9, 512)
    explicit = torch.zeros(2, 9, 512)
    assert fields.resolve_film(None, (plain_pf, plain_m), (plain_pf, plain_m)) is None
    assert fields.resolve_film(explicit, (plain_pf, plain_m)) is None                 # non-FiLM kinds take no table
    with pytest.raises(ValueError):                                                    # unset, as the reference
        fields.resolve_film(None, (film_pf, film_m), (film_pf, film_m))
    assert fields.resolve_film(explicit, (film_pf, film_m), (film_pf, film_m)) is explicit     # ... but an explicit one wins
    film_m.set_film_params(own)
    assert fields.resolve_film(explicit, (plain_pf, plain_m), (film_pf, film_m)) is explicit
    for pair in (((film_pf, film_m), (plain_pf, plain_m)), ((plain_pf, plain_m), (film_pf, film_m)),
                 ((None, lambda x: x), (film_pf, film_m)), ((film_pf, film_m),)):
        got = fields.resolve_film(None, *pair)                                         # from the coarse / the fine model
        assert tuple(got.shape) == (1, 9, 512) and torch.equal(got.reshape(9, 512), own)


def test_film_groups():
    film_pf, plain_pf = packed(fields.FilmSirenNeRF()), packed(fields.NeRF())
    assert fields.film_groups(plain_pf, torch.zeros(2, 9, 512), 10) == (None, 1, 10)
    table, groups, per = fields.film_groups(film_pf, torch.zeros(2 * 9, 512, dtype=torch.float64), 10)
    assert (groups, per) == (2, 5) and tuple(table.shape) == (2, 9, 512) and table.dtype == torch.float32
    with pytest.raises(_lib.MiRenderError, match="rays must split evenly over the FiLM groups"):
        fields.film_groups(film_pf, torch.zeros(3, 9, 512), 10)
    with pytest.raises(ValueError):
        fields.film_groups(film_pf, None, 10)


def test_pair_params_and_needs_graph():
    a, b = packed(fields.TinyNeRF()), packed(fields.TinyNeRF())
    shared, two = fields.pair_params(a, a), fields.pair_params(a, b)
    assert len(shared) == len(a.params) and all(p is q for p, q in zip(shared, a.params))
    assert len(two) == len(a.params) + len(b.params) and all(p is q for p, q in zip(two, a.params + b.params))
    assert shared is not a.params                                                      # a list of its own
    assert fields.needs_graph(None, a, b)
    with torch.no_grad():
        assert not fields.needs_graph(None, a, b)
    for p in a.params + b.params:
        p.requires_grad_(False)
    assert not fields.needs_graph(None, a, b) and not fields.needs_graph(torch.zeros(1, 9, 512), a)
    assert fields.needs_graph(torch.zeros(1, 9, 512, requires_grad=True), a)
    b.params[-1].requires_grad_(True)
    assert fields.needs_graph(None, a, b) and not fields.needs_graph(None, a)


@pytest.mark.parametrize("n", [37, 0])
def test_occupancy_workspace_bytes_is_the_sum_of_the_library_queries(n):
    lib, nc, nf = _lib.load(), 8, 16
    seen = set()
    for train in (False, True):
        for clip in (None, (64, 1)):
            want = lib.mi_render_workspace_bytes(n, nc, nf)
            want += (lib.mi_render_occupancy_train_extra_bytes if train else lib.mi_render_occupancy_extra_bytes)(n, nc, nf)
            want += lib.mi_render_occupancy_clip_extra_bytes(n) if clip else 0
            got = ops._occupancy_workspace_bytes(train, clip, n, nc, nf)
            assert got == want and type(got) is int and (got > 0) == (n > 0), (train, clip)
            seen.add(got)
    assert len(seen) == (4 if n else 1)                       # the four calls' workspaces differ; without rays there is none


GRID_REFUSALS = {
    "rendering": ("rendering with an occupancy grid is not built for callables with no known layout (the generic path): both "
                  "models must be NeRF, SirenNeRF or TinyNeRF fields",
                  "rendering with an occupancy grid is not built for FiLM fields (a FiLM field's table is per image, a per-scene "
                  "grid has no meaning there)"),
    "training": ("training with an occupancy grid is not built for generic callables (models with no known layout): both models "
                 "must be NeRF, SirenNeRF or TinyNeRF fields",
                 "training with an occupancy grid is not built for FiLM kinds (a FiLM field's table is per image, a per-scene grid "
                 "has no meaning there)"),
}


@pytest.mark.parametrize("doing", sorted(GRID_REFUSALS))
def test_refuse_grid_call_says_what_each_call_always_said(doing):
    film_pf, plain_pf = packed(fields.FilmSirenNeRF()), packed(fields.TinyNeRF())
    here, there = types.SimpleNamespace(device="cpu"), types.SimpleNamespace(device="cuda:1")
    no_layout, film_kinds = GRID_REFUSALS[doing]

    def said(*args):
        with pytest.raises(_lib.MiRenderError) as e:
            fields.refuse_grid_call(doing, *args)
        return str(e.value)
    assert said(here, None, plain_pf) == no_layout and said(here, plain_pf, None) == no_layout
    assert said(here, film_pf, plain_pf) == film_kinds and said(here, plain_pf, film_pf) == film_kinds
    assert said(there, plain_pf, plain_pf) == "the occupancy grid is on cuda:1, the fields are on cpu"
    # the caller's own refusals rank behind the two about the models and ahead of the one about the device
    def own():
        raise _lib.MiRenderError("the caller's own")
    assert said(here, None, plain_pf, own) == no_layout and said(here, film_pf, plain_pf, own) == film_kinds
    assert said(there, plain_pf, plain_pf, own) == "the caller's own"
    fields.refuse_grid_call(doing, here, plain_pf, plain_pf)


def test_pose_defines_no_function_but_get_rays():
    from mirender import pose
    own = [name for name, v in vars(pose).items()
           if isinstance(v, type) and issubclass(v, torch.autograd.Function) and v.__module__ == pose.__name__]
    assert own == ["_GetRaysFn"]


def test_wants_grad_and_f32c_keep_or_cut_the_graph():
    x = torch.ones(2, 3, dtype=torch.float64, requires_grad=True)
    assert _lib.wants_grad(x) and not _lib.wants_grad(x.detach()) and not _lib.wants_grad(None) and not _lib.wants_grad([1.0])
    with torch.no_grad():
        assert not _lib.wants_grad(x)
    kept, cut = _lib.f32c(x.t(), "cpu", detach=False), _lib.f32c(x.t(), "cpu")
    assert kept.requires_grad and not cut.requires_grad and torch.equal(kept.detach(), cut)
    assert all(t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (3, 2) for t in (kept, cut))
    assert _lib.f32c(None, "cpu", detach=False) is None


def test_ptr_array():
    ts = [torch.zeros(3), None, torch.zeros(5, dtype=torch.int32)]
    arr = _lib.ptr_array(ts)
    assert len(arr) == 3 and isinstance(arr, ctypes.Array) and arr._type_ is ctypes.c_void_p
    assert arr[0] == ts[0].data_ptr() and arr[1] is None and arr[2] == ts[2].data_ptr()
    assert len(_lib.ptr_array([])) == 0


def test_seed64():
    assert _lib.seed64(0) == 0 and _lib.seed64(-1) == 2 ** 64 - 1 and _lib.seed64(2 ** 64 + 5) == 5

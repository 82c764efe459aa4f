"""ctypes binding of libmirender.so (the C ABI declared in include/mi_render.h).

The HIP library is the product: there is no CPU or PyTorch fallback.  If the shared object
is missing or a symbol is absent, importing/using this module raises immediately.
torch must be imported first so the process has ONE HIP runtime (torch's bundled
libamdhip64.so.7 satisfies libmirender's NEEDED entry by SONAME).
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (loads libamdhip64 before libmirender)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmirender.so")

c_f32p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_f32 = ctypes.c_float
_f64 = ctypes.c_double
_u64 = ctypes.c_uint64
_u32 = ctypes.c_uint32
_vp = ctypes.c_void_p

# name -> (restype, argtypes): every symbol include/mi_render.h declares
SIGNATURES = {
    "mi_abi_version": (_int, []),
    "mi_last_error": (ctypes.c_char_p, []),
    "mi_field_num_params": (_int, [_int]),
    "mi_field_packed_floats": (_i64, [_int]),
    "mi_field_macs": (_i64, [_int]),
    "mi_field_film_layers": (_int, [_int]),
    "mi_field_param_shape": (_int, [_int, _int, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "mi_field_pack": (_int, [_int, ctypes.POINTER(_vp), _int, _f32, _vp, _vp]),
    "mi_field_eval_points": (_int, [_int, _vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "mi_field_eval_rays": (_int, [_int, _vp, _vp, _vp, _vp, _i64, _i64, _int, _vp, _vp]),
    "mi_gen_rays": (_int, [_int, _int, _f64, ctypes.POINTER(_f32), _i64, _i64, _vp, _int, _vp]),
    "mi_sample_coarse": (_int, [_i64, _f32, _f32, _int, _vp, _vp, _u64, _u64, _vp, _vp]),
    "mi_composite": (_int, [_i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mi_sample_fine": (_int, [_i64, _f32, _f32, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mi_sample_fine_pos": (_int, [_i64, _f32, _f32, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mi_merge_raw": (_int, [_i64, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "mi_split_grad": (_int, [_i64, _int, _int, _vp, _vp, _vp, _int, _vp, _vp]),
    "mi_sample_pdf": (_int, [_i64, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "mi_image_metrics_workspace_floats": (_i64, [_int, _int, _int, _int]),
    "mi_image_metrics": (_int, [_vp, _vp, _int, _int, _int, _int, _vp, _int, _vp, _vp, _vp]),
    "mi_grid_points": (_int, [_int, _vp, _f32, _i64, _i64, _vp, _vp]),
    "mi_nerf_loss_workspace_floats": (_i64, [_i64]),
    "mi_nerf_loss": (_int, [_i64, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mi_ray_bank": (_int, [_int, _int, _f64, _vp, _vp, _int, _i64, _vp, _int, _vp]),
    "mi_adam_step": (_int, [_int, ctypes.POINTER(_int), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                            ctypes.POINTER(_vp), ctypes.POINTER(_i64), _f32, _f32, _f32, _f32, _f32, _f32,
                            ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp]),
    "mi_render_workspace_bytes": (_i64, [_i64, _int, _int]),
    "mi_render_shared_field_extra_bytes": (_i64, [_i64, _int, _int]),
    "mi_render_deferred_colour_extra_bytes": (_i64, [_i64, _int, _int]),
    "mi_field_has_deferred_colour": (_int, [_int]),
    "mi_render_rays": (_int, [_int, _vp, _int, _vp, _vp, _vp, _i64, _i64, _f32, _f32, _int, _int, _vp, _vp, _vp,
                              _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "mi_composite_bwd": (_int, [_i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mi_field_packed_bwd_floats": (_i64, [_int]),
    "mi_field_pack_bwd": (_int, [_int, ctypes.POINTER(_vp), _int, _f32, _vp, _vp]),
    "mi_field_train_acts_floats": (_i64, [_int]),
    "mi_field_train_grads_floats": (_i64, [_int]),
    "mi_field_bwd_partial_floats": (_i64, [_i64]),
    "mi_field_bwd_partial_floats_kind": (_i64, [_int, _i64]),
    "mi_field_eval_rays_train": (_int, [_int, _vp, _vp, _vp, _vp, _i64, _i64, _int, _vp, _vp, _vp]),
    "mi_field_eval_points_train": (_int, [_int, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    "mi_field_film_partial_floats": (_i64, [_i64, _i64]),
    "mi_field_film_partial_floats_kind": (_i64, [_int, _i64, _i64]),
    "mi_field_backward": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, ctypes.POINTER(_vp),
                                 ctypes.POINTER(_vp), _int, _vp, _vp]),
    "mi_field_input_grad": (_int, [_int, ctypes.POINTER(_vp), _int, _vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "mi_field_input_grad_rays": (_int, [_int, ctypes.POINTER(_vp), _int, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int,
                                        _vp, _vp]),
    "mi_composite_bwd_rays": (_int, [_i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp]),
    "mi_render_train_saved_bytes": (_i64, [_int, _int, _int, _i64, _int, _int]),
    "mi_render_backward_workspace_bytes": (_i64, [_int, _int, _int, _i64, _i64, _int, _int, _i64, _i64]),
    "mi_render_rays_train": (_int, [_int, _vp, _int, _vp, _vp, _vp, _i64, _i64, _f32, _f32, _int, _int, _vp, _vp, _vp,
                                    _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp]),
    "mi_render_rays_backward": (_int, [_int, _vp, _vp, ctypes.POINTER(_vp), _int, _vp, _vp, ctypes.POINTER(_vp), _vp, _vp,
                                       _i64, _i64, _int, _int, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                       _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, _i64,
                                       ctypes.POINTER(_int), _vp]),
    "mi_mc_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "mi_marching_cubes_count": (_int, [_vp, _i64, _i64, _i64, _f64, _vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), _vp]),
    "mi_marching_cubes_emit": (_int, [_vp, _i64, _i64, _i64, _f64, ctypes.POINTER(_f64), _int, _vp, _vp, _vp, _vp, _vp,
                                      _vp]),
    "mi_event_create": (_vp, []),
    "mi_event_destroy": (None, [_vp]),
    "mi_event_record": (_int, [_vp, _vp]),
    "mi_event_elapsed_ms": (_int, [_vp, _vp, ctypes.POINTER(_f32)]),
    "mi_render_set_mlp_events": (None, [_vp, _vp, _vp, _vp]),
    "mi_field_eval_rays_deferred": (_int, [_int, _vp, _vp, _vp, _vp, _i64, _i64, _int, _vp, _vp, _i64, _vp]),
    "mi_render_set_colour_chunk_rows": (None, [_i64]),
    "mi_occupancy_words": (_i64, [ctypes.POINTER(_int)]),
    "mi_occupancy_pack_workspace_bytes": (_i64, [ctypes.POINTER(_int), _int]),
    "mi_occupancy_cell_points": (_int, [ctypes.POINTER(_int), ctypes.POINTER(_f32), ctypes.POINTER(_f32), _int, _i64, _i64,
                                        _vp, _vp]),
    "mi_occupancy_pack": (_int, [_vp, ctypes.POINTER(_int), _int, _f32, _int, _vp, _vp, _i64, _vp]),
    "mi_occupancy_draw_points": (_int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_f32), ctypes.POINTER(_f32), _u64, _u32, _int,
                                        _i64, _i64, _i64, _vp, _vp, _vp]),
    "mi_occupancy_density_workspace_bytes": (_i64, [ctypes.POINTER(_int), _int]),
    "mi_occupancy_density_update": (_int, [_vp, _vp, _i64, ctypes.POINTER(_int), _f32, _vp, _vp, _i64, _vp]),
    "mi_occupancy_density_pack": (_int, [_vp, ctypes.POINTER(_int), _f32, _int, _int, _vp, _vp, _i64, _vp]),
    "mi_occupancy_mark_rays": (_int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_f32), ctypes.POINTER(_f32), _vp, _vp, _i64,
                                      _int, _vp, _vp, _vp, _vp]),
    "mi_field_eval_rays_list": (_int, [_int, _vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp]),
    "mi_render_occupancy_extra_bytes": (_i64, [_i64, _int, _int]),
    "mi_render_rays_occupancy": (_int, [_int, _vp, _int, _vp, _vp, _i64, _f32, _f32, _int, _int, _vp, _vp, _vp, _u64, _u64,
                                        _vp, ctypes.POINTER(_int), ctypes.POINTER(_f32), ctypes.POINTER(_f32), _vp, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "mi_occupancy_ordered_list_ints": (_i64, [_i64, _int]),
    "mi_occupancy_mark_rays_ordered": (_int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_f32), ctypes.POINTER(_f32), _vp, _vp,
                                              _i64, _int, _vp, _vp, _vp, _vp]),
    "mi_field_eval_rays_list_train": (_int, [_int, _vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp]),
    "mi_field_backward_list": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, ctypes.POINTER(_vp), _vp]),
    "mi_render_occupancy_train_extra_bytes": (_i64, [_i64, _int, _int]),
    "mi_render_occupancy_train_saved_bytes": (_i64, [_int, _int, _i64, _int, _int]),
    "mi_render_occupancy_backward_workspace_bytes": (_i64, [_int, _int, _int, _i64, _int, _int]),
    "mi_render_rays_occupancy_train": (_int, [_int, _vp, _int, _vp, _vp, _i64, _f32, _f32, _int, _int, _vp, _vp, _vp, _u64,
                                              _u64, _vp, ctypes.POINTER(_int), ctypes.POINTER(_f32), ctypes.POINTER(_f32),
                                              _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp]),
    "mi_render_rays_occupancy_backward": (_int, [_int, _vp, _int, _vp, _int, _vp, _i64, _int, _int, _vp, _i64, _vp, _i64,
                                                 _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                                 _vp, _i64, ctypes.POINTER(_int), _vp]),
    "mi_field_input_grad_rays_list": (_int, [_int, ctypes.POINTER(_vp), _int, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _int,
                                             _int, _vp, _vp]),
    "mi_render_rays_occupancy_backward_rays": (_int, [_int, _vp, _int, _vp, _int, _vp, _i64, _int, _int, _vp, _i64, _vp, _i64,
                                                      _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                                      _vp, _i64, ctypes.POINTER(_int), ctypes.POINTER(_vp), _int,
                                                      ctypes.POINTER(_vp), _int, _vp, _vp]),
    "mi_occupancy_clip_rays": (_int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_f32), ctypes.POINTER(_f32), _vp, _i64, _f32, _f32,
                                      _int, _int, _vp, _vp]),
    "mi_sample_coarse_bounds": (_int, [_i64, _vp, _int, _vp, _u64, _u64, _vp, _vp]),
    "mi_sample_fine_bounds": (_int, [_i64, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mi_render_occupancy_clip_extra_bytes": (_i64, [_i64]),
    "mi_render_rays_occupancy_clip": (_int, [_int, _vp, _int, _vp, _vp, _i64, _f32, _f32, _int, _int, _int, _int, _vp, _vp, _u64,
                                             _u64, _vp, ctypes.POINTER(_int), ctypes.POINTER(_f32), ctypes.POINTER(_f32), _vp, _vp,
                                             _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "mi_render_rays_occupancy_clip_train": (_int, [_int, _vp, _int, _vp, _vp, _i64, _f32, _f32, _int, _int, _int, _int, _vp, _vp,
                                                   _u64, _u64, _vp, ctypes.POINTER(_int), ctypes.POINTER(_f32),
                                                   ctypes.POINTER(_f32), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64,
                                                   _vp]),
}

ABI_VERSION = 4      # include/mi_render.h as of this binding (mi_abi_version() of the library must equal it)

_lib = None


class MiRenderError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle; raises if the HIP library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MiRenderError(
            f"{LIB_PATH} not found: build it with `python msra-practice-project_amd/csrc/build.py` "
            "(the HIP library is required; there is no fallback path)")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    # the signatures below are those of ONE ABI version: a stale or foreign library (MI_DIAG_LIB in tests/conftest.py makes
    # loading another one a supported path) must be refused before any call passes it arguments in the wrong order
    try:
        lib.mi_abi_version.restype = ctypes.c_int
        have = lib.mi_abi_version()
    except AttributeError:
        have = None
    if have != ABI_VERSION:
        raise MiRenderError(f"{LIB_PATH} has ABI version {have}, this binding is written against {ABI_VERSION}: rebuild it "
                            "with `python msra-practice-project_amd/csrc/build.py --force`")
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().mi_last_error().decode(errors="replace")
        raise MiRenderError(f"{what} failed ({rc}): {msg}")


def ptr(t):
    """Device pointer of a tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ----------------------------------------------------------------------------------------------------------------
# The calling conventions of the package, each said once.  A new entry point plugs in here: its launches go through
# call(), its *_bytes / *_floats queries through query(), its caller-sized buffers through guarded() / check_guard().
# ----------------------------------------------------------------------------------------------------------------
def call(name: str, device, *args):
    """Launch entry point `name` on `device`: the device is selected, the calling thread's current stream of that device is
    appended as the last argument (where every launching entry point of include/mi_render.h takes it) and a non-zero
    return raises MiRenderError under the same name."""
    with torch.cuda.device(device):
        check(getattr(load(), name)(*args, stream_ptr(device)), name)


def query(name: str, *args) -> int:
    """A *_bytes / *_floats / *_ints / *_words size query: the int, or MiRenderError with mi_last_error() when the library
    answers with a negative error code (which must never reach torch.empty as a size)."""
    n = int(getattr(load(), name)(*args))
    if n < 0:
        check(n, name)
    return n


def capturing() -> bool:
    """Is the calling thread's current stream being captured into a graph?  On a host without a device torch's query raises
    instead of answering; nothing can be captured there (the callers go on to their own "no ROCm device" errors)."""
    try:
        return torch.cuda.is_current_stream_capturing()
    except RuntimeError:
        return False


def refuse_capture(who: str, why: str):
    """Raise MiRenderError when the calling thread's current stream is being captured into a graph.  For the calls that hand
    the library a value the HOST computes anew on every call (a step count, an epoch, a fresh seed): a graph records the
    value of the captured call and every replay would repeat it - wrong results, no error.  Called before the function's
    first launch or allocation, so a refused call leaves the capture as it was."""
    if capturing():
        raise MiRenderError(f"{who} cannot be captured into a graph: {why}")


def ptr_array(tensors):
    """void*[len] of the tensors' device pointers (NULL for a None entry); valid while the caller keeps the tensors."""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def seed64(seed) -> int:
    """A Python int of any sign as the uint64 the Philox-keyed entry points take."""
    return int(seed) & (2 ** 64 - 1)


def f32c(t, device, detach=True):
    """A tensor as the library reads it: detached, fp32, contiguous, on `device` (None stays None).  detach=False keeps the
    graph to `t`: rays or points whose gradient the call's Function produces (mirender.pose), or a callable's own torch ops
    (the generic path)."""
    if t is None:
        return None
    return (t.detach() if detach else t).to(device=device, dtype=torch.float32).contiguous()


def wants_grad(t) -> bool:
    """Is `t` a tensor whose gradient a call made now would have to produce?"""
    return isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled()


# MI_DEBUG_GUARDS=1 (tests/test_gpu_guards.py): every buffer whose size the caller takes from a query gets GUARD_BYTES of a
# sentinel byte behind it, checked after the call - the library never allocates, so a kernel writing past what a query
# promised would otherwise corrupt a neighbouring tensor silently.  The check is the only place that reads back.
GUARD_BYTES = 16384
_SENTINEL = 0xA5


def guards_on() -> bool:
    return os.environ.get("MI_DEBUG_GUARDS") == "1"


def guarded(n: int, dtype, device):
    """(torch.empty(n, dtype) on device, None); with MI_DEBUG_GUARDS=1 (the first n units of a buffer whose tail is the
    sentinel, that whole buffer - for check_guard after the call)."""
    n = int(n)
    if not guards_on():
        return torch.empty(n, dtype=dtype, device=device), None
    whole = torch.empty(n + GUARD_BYTES // dtype.itemsize, dtype=dtype, device=device)
    whole[n:].view(torch.uint8).fill_(_SENTINEL)
    return whole[:n], whole


def check_guard(whole, what: str):
    """Raise if the library touched the sentinel tail of guarded()'s `whole` (None: guards are off), naming the buffer."""
    if whole is None:
        return
    hit = (whole[whole.numel() - GUARD_BYTES // whole.dtype.itemsize:].view(torch.uint8) != _SENTINEL).nonzero()
    if hit.numel():
        raise MiRenderError(f"{what}: the library wrote {int(hit[-1]) + 1} bytes past the end of the buffer")

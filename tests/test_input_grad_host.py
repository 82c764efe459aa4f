"""CPU: the ray / input gradient entry points (include/mi_render.h, csrc/ray_grad.hip) are exported, bound and validate
their arguments without a GPU; mirender.pose imports and refuses a model that is not on a device.  No kernel is launched:
every call below is refused before it reaches one."""
import ctypes

import pytest
import torch

NEW = ("mi_field_input_grad", "mi_field_input_grad_rays", "mi_composite_bwd_rays")


def _lib():
    import test_abi
    return test_abi.ensure_built()


def test_symbols_exported_and_bound():
    _l = _lib()
    import test_abi
    raw = ctypes.CDLL(_l.LIB_PATH)
    for s in NEW:
        assert s in test_abi.declared_symbols() and s in _l.SIGNATURES and hasattr(raw, s), s
    assert _l.load().mi_abi_version() == 4 == _l.ABI_VERSION


def _params(n, null_at=None):
    keep = [torch.zeros(4) for _ in range(n)]
    arr = (ctypes.c_void_p * n)(*[None if i == null_at else t.data_ptr() for i, t in enumerate(keep)])
    return arr, keep


def test_input_grad_argument_checks():
    _l = _lib()
    lib = _l.load()
    buf = torch.zeros(64)
    p = ctypes.c_void_p(buf.data_ptr())
    arr, _keep = _params(24)

    def refused(rc, word):
        assert rc == -1, rc
        assert word.encode() in lib.mi_last_error(), lib.mi_last_error()

    # bad kinds
    refused(lib.mi_field_input_grad(99, arr, 24, None, p, p, 1, 8, p, None), "unknown field kind")
    refused(lib.mi_field_input_grad_rays(0x100 + 2 * 3, arr, 24, p, p, p, p, p, 1, 8, 4, 0, p, None), "outside the supported range")
    # null pointers
    refused(lib.mi_field_input_grad(0, None, 24, None, p, p, 1, 8, p, None), "null pointer")
    refused(lib.mi_field_input_grad(0, arr, 24, None, None, p, 1, 8, p, None), "null pointer")
    refused(lib.mi_field_input_grad(0, arr, 24, None, p, None, 1, 8, p, None), "null pointer")
    refused(lib.mi_field_input_grad(0, arr, 24, None, p, p, 1, 8, None, None), "null pointer")
    refused(lib.mi_field_input_grad_rays(0, arr, 24, None, p, p, None, p, 1, 8, 4, 0, p, None), "null pointer")
    refused(lib.mi_field_input_grad_rays(0, arr, 24, None, p, p, p, None, 1, 8, 4, 0, p, None), "null pointer")
    bad, _k2 = _params(24, null_at=5)
    refused(lib.mi_field_input_grad(0, bad, 24, None, p, p, 1, 8, p, None), "parameter 5 is null")
    # bad shapes
    refused(lib.mi_field_input_grad(0, arr, 22, None, p, p, 1, 8, p, None), "expects 24 parameter tensors")
    refused(lib.mi_field_input_grad(0, arr, 24, None, p, p, 1, -8, p, None), "negative size")
    refused(lib.mi_field_input_grad(0, arr, 24, None, p, p, 2, 8, p, None), "only FiLM kinds have groups")
    refused(lib.mi_field_input_grad_rays(0, arr, 24, None, p, p, p, p, 1, 8, 0, 0, p, None), "n_samples must be positive")
    film_arr, _k3 = _params(22)
    refused(lib.mi_field_input_grad(2, film_arr, 22, None, p, p, 1, 8, p, None), "FiLM kind needs a film table")
    # nothing to do is not an error, and touches nothing
    assert lib.mi_field_input_grad(0, arr, 24, None, p, p, 1, 0, p, None) == 0
    assert lib.mi_field_input_grad_rays(0, arr, 24, None, p, p, p, p, 1, 0, 4, 1, p, None) == 0


def test_composite_bwd_rays_argument_checks():
    lib = _lib().load()
    buf = torch.zeros(64)
    p = ctypes.c_void_p(buf.data_ptr())
    for args in ((-1, 4, p, p, p, p, p, p, p, 0, p, None), (2, 0, p, p, p, p, p, p, p, 0, p, None),
                 (2, 4097, p, p, p, p, p, p, p, 0, p, None), (2, 4, None, p, p, p, p, p, p, 0, p, None),
                 (2, 4, p, None, p, p, p, p, p, 0, p, None), (2, 4, p, p, None, p, p, p, p, 0, p, None),
                 (2, 4, p, p, p, p, p, p, p, 0, None, None)):
        assert lib.mi_composite_bwd_rays(*args) == -1
        assert b"mi_composite_bwd_rays" in lib.mi_last_error()
    assert lib.mi_composite_bwd_rays(0, 4, p, p, p, None, None, None, None, 0, p, None) == 0      # no rays


def test_pose_module_imports_and_refuses_cpu_models():
    import mirender
    from mirender import _lib, fields, pose
    assert mirender.pose is pose and "pose" in mirender.__all__
    for name in ("get_rays", "render_rays", "render_image_tensor", "field_eval_points"):
        assert callable(getattr(pose, name))
    rays = torch.zeros(4, 2, 3, requires_grad=True)
    with pytest.raises(_lib.MiRenderError, match="needs the model on a ROCm device"):
        pose.render_rays(rays, 2.0, 6.0, fields.NeRF(), fields.NeRF(), 4, 4, seed=0)
    with pytest.raises(_lib.MiRenderError, match="generic path"):
        pose.render_rays(rays, 2.0, 6.0, lambda x: x[:, :4], lambda x: x[:, :4], 4, 4, seed=0)
    with pytest.raises(_lib.MiRenderError, match="ROCm device"):
        pose.get_rays(4, 4, 5.0, torch.eye(4))

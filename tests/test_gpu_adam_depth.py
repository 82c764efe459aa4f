"""GPU: mi_adam_step's scatter of the updated parameters into both weight streams on the FiLM depth kinds
(adam_pack_kernel<DEPTH = true>, which computes every stream item with film_item() instead of reading a constant table).

Called through the C ABI with a non-zero gradient on every element and a learning rate that moves every parameter; after
each step both streams must equal a fresh mi_field_pack / mi_field_pack_bwd of the updated parameters bit for bit - a
stale position would make training use an old weight for part of a layer - and parameters and moments must match
torch.optim.Adam at the tolerances of test_gpu_trainloop.test_fused_adam_matches_torch_adam_and_keeps_the_streams_current.

Cases: every depth 4..12 with and without the view direction as a single field with its transposed stream; depths 5 and 12
with packed_bwd = NULL; a fixed kind paired with a depth kind, in both orders, one with field 1's transposed stream absent;
two distinct depth-12 fields (60 of the kernel's 64 tensor slots)."""
import ctypes
import math

import pytest
import torch

import bwd_gates as G
import film_depth_util as U
from oracle import parity, synth

pytestmark = pytest.mark.gpu

LR, BETAS, EPS, STEPS = 1e-2, (0.9, 0.999), 1e-8, 3


def dev():
    return torch.device("cuda", 0)


def L_(L, use_dir):
    return G.depth_name(L, use_dir)


# (field kinds, which of them have a transposed stream; None: the packed_bwd array itself is NULL)
CASES = [((L_(L, d),), (True,)) for L in range(G.DEPTH_MIN, G.DEPTH_MAX + 1) for d in (True, False)]
CASES += [((L_(L, d),), None) for L in (5, 12) for d in (True, False)]
CASES += [(("nerf", L_(5, False)), (True, True)),
          ((L_(7, True), "tiny_nerf"), (True, False)),
          ((L_(12, True), L_(12, True)), (True, True))]


def case_id(kinds, bwd):
    tag = "no_bwd_array" if bwd is None else "".join("b" if x else "-" for x in bwd)
    return "+".join(k.replace("film_depth_", "") for k in kinds) + "-" + tag


def module(kind, seed):
    from mirender import fields
    d = G.depth_of(kind)
    if d is None:
        sd = synth.state_dict(kind, seed=seed, sharp="medium", bias_jitter=0.05)
    else:
        sd = U.state_dict(d[0], d[1], seed=seed, head="medium")
    return fields.field_from_state_dict(sd, dev())


def stale_positions(lib, pf, packed, pack_fn):
    """Positions of a stream the scatter patched in place that differ from a fresh pack of the current parameters."""
    from mirender import _lib
    arr = (ctypes.c_void_p * len(pf.params))(*[p.data_ptr() for p in pf.params])
    fresh = torch.empty_like(packed)
    _lib.check(pack_fn(pf.kind, arr, len(pf.params), pf.w_0, _lib.ptr(fresh), _lib.stream_ptr(dev())), "pack")
    torch.cuda.synchronize()
    return int((fresh.view(torch.int32) != packed.view(torch.int32)).sum())


@pytest.mark.parametrize("kinds,bwd", CASES, ids=[case_id(*c) for c in CASES])
def test_adam_scatter_keeps_depth_streams_current(kinds, bwd):
    from mirender import _lib, fields
    lib = _lib.load()
    mods = [module(k, 80 + i) for i, k in enumerate(kinds)]
    pfs = [fields.as_packed_field(m) for m in mods]
    # a depth-8 module is kinds 2 / 3; its streams under the macro id are the same streams (mi_render.h), so take that id
    pfs = [pf if pf.kind == G.KIND_IDS[k] else fields.PackedField(G.KIND_IDS[k], pf.params, pf.w_0) for pf, k in zip(pfs, kinds)]
    assert all(pf.kind == G.KIND_IDS[k] or G.depth_of(k)[0] == 8 for pf, k in zip(pfs, kinds))
    fwd = [pf.refresh() for pf in pfs]
    has_bwd = (False,) * len(pfs) if bwd is None else bwd
    tr = [pf.refresh_bwd() if h else None for pf, h in zip(pfs, has_bwd)]
    params = [p.detach() for pf in pfs for p in pf.params]
    ref_params = [p.clone().requires_grad_(True) for p in params]
    ref = torch.optim.Adam(ref_params, lr=LR, betas=BETAS, eps=EPS)
    m1, m2 = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    n = len(params)
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    c_kinds = (ctypes.c_int * len(pfs))(*[pf.kind for pf in pfs])
    numel = (ctypes.c_int64 * n)(*[p.numel() for p in params])
    gen = torch.Generator(device=dev()).manual_seed(1)
    # one sign per element for all steps: the first moment never cancels, so every step moves every parameter by a sizeable
    # part of LR (far above the parameters' fp32 spacing)
    signs = [torch.where(torch.randn(p.shape, device=dev(), generator=gen) < 0, -1.0, 1.0) for p in params]
    stale = 0
    for t in range(1, STEPS + 1):
        before = [p.clone() for p in params]
        grads = []
        for p, q, sg in zip(params, ref_params, signs):
            g = (torch.randn(p.shape, device=dev(), generator=gen).abs() + 1e-3) * sg * 10.0 ** float(-(t % 3))  # never zero
            grads.append(g)
            q.grad = g.clone()
        _lib.check(lib.mi_adam_step(len(pfs), c_kinds, arr(params), arr(grads), arr(m1), arr(m2), numel,
                                    -LR / (1 - BETAS[0] ** t), 1 - BETAS[0], BETAS[1], 1 - BETAS[1], EPS,
                                    math.sqrt(1 - BETAS[1] ** t), arr(fwd), None if bwd is None else arr(tr),
                                    _lib.stream_ptr(dev())), "mi_adam_step")
        ref.step()
        torch.cuda.synchronize()
        for p, b in zip(params, before):
            assert bool((p != b).all()), "a parameter the step did not move cannot show a stale stream position"
        for pf, f, r in zip(pfs, fwd, tr):
            stale += stale_positions(lib, pf, f, lib.mi_field_pack)
            if r is not None:
                stale += stale_positions(lib, pf, r, lib.mi_field_pack_bwd)
    parity.record(case=f"adam scatter {case_id(kinds, bwd)}", stage="adam scatter", qty="stale stream positions", stale=stale,
                  steps=STEPS, passed=stale == 0)
    assert stale == 0, f"{stale} stream positions are stale after the scatter refresh"
    for p, q, a, b in zip(params, ref_params, m1, m2):
        sb = ref.state[q]
        assert float((p - q.detach()).abs().max()) <= 1e-7
        assert float((a - sb["exp_avg"]).abs().max()) <= 1e-7 * max(1.0, float(sb["exp_avg"].abs().max()))
        assert float((b - sb["exp_avg_sq"]).abs().max()) <= 1e-7 * max(1.0, float(sb["exp_avg_sq"].abs().max()))

"""GPU: mi_render_rays runs the fine pass's colour branch only on the points with sigma > 0 - and no output bit moves.

With two different fields (NeRF, TinyNeRF) and a workspace that also holds mi_render_deferred_colour_extra_bytes, the fine
pass is evaluated in chunks of whole rays: a trunk-and-spill launch writes {0, 0, 0, sigma} for every point and appends the
points with sigma > 0 (H8 row, index) to the chunk's live list, then a colour launch runs layers_dir and the rgb head over
that list.  A point with sigma == 0 has alpha = 1 - exp(-0 * delta) = 0 and so weight exactly 0: its colour enters rgb_f as
0 * rgb = +0 for any finite rgb.  The yardstick is the undeferred computation assembled from the staged calls:

    sample_coarse -> field_eval_rays -> composite -> sample_fine -> field_eval_rays -> composite

and the final outputs must equal it bit for bit.  Shapes: 257 rays, Nc = 16, Nf = 32 (S = 48), chunk rows forced to 4 096 =
85 rays per chunk: four chunks, the last one of 2 rays, partial 128-point tiles in both kernels.

No case passes vacuously: each one first counts the live (sigma > 0) points in the staged reference alone.  Fine-field seeds
were picked with the CPU oracle (oracle/render_ref.py) at exactly these shapes - rays below, t_rand seed 9, coarse field
`sharp` seed 34 (nerf) / 25 (tiny_nerf), fine field `sharp` with bias_jitter 0.05; live share of the fine points, whole
call and per chunk:
    nerf       fine seed 3:  73.0 %  (72 / 69 / 78 / 58 %); the one ray of the n = 1 case: 35 of 48
    tiny_nerf  fine seed 11: 58.7 %  (57 / 51 / 68 / 49 %)
    nerf fine seed 3 with the sigma bias shifted by -3000: 0 live, by +3000: all live (checked for n = 1 and n = 257)
(nerf fine seeds 6 and 11 give 5 % and 4 %, tiny_nerf 3 and 6 give 17 % and 89 %.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import render_ref as R, synth  # noqa: E402

NEAR, FAR = 2.0, 6.0
N, NC, NF = 257, 16, 32
S = NC + NF
CHUNK = 4096                      # forced chunk rows: 85 rays of 48 samples
COARSE_SEED = {"nerf": 34, "tiny_nerf": 25}
FINE_SEED = {"nerf": 3, "tiny_nerf": 11}


def dev():
    return torch.device("cuda", 0)


def _packed(kind, seed, sigma_bias=0.0):
    from mirender import fields
    sd = synth.state_dict(kind, seed=seed, sharp=True, bias_jitter=0.05)
    if sigma_bias:
        sd["output_layer_sigma.bias"] = sd["output_layer_sigma.bias"] + sigma_bias
    return fields.as_packed_field(fields.field_from_state_dict(sd, dev()))


def _rays(n):
    """n rays spread over a 40x40 view of the volume (n = 1: a ray through its middle)."""
    r = torch.from_numpy(R.rays_from_camera(40, 40, 1.3875 * 40, synth.pose_degrees(4.0, 20.0, -30.0)))
    idx = (torch.arange(n) * 1600 // n + 20) % 1600 if n > 1 else torch.tensor([820])
    return r[idx].contiguous().to(dev())


_REF = {}


def _staged(kind, n, sigma_bias=0.0):
    """The undeferred computation, stage by stage; computed once per key, shared and left unchanged."""
    key = (kind, n, sigma_bias)
    if key not in _REF:
        from mirender import ops
        pf_c, pf_f = _packed(kind, COARSE_SEED[kind]), _packed(kind, FINE_SEED[kind], sigma_bias)
        rays, tr = _rays(n), synth.t_rand(n, NC, seed=9).to(dev())
        with torch.no_grad():
            z_c = ops.sample_coarse(n, NEAR, FAR, NC, dev(), tr, seed=0)
            raw_c = ops.field_eval_rays(pf_c, rays, z_c)
            _, depth_c, acc_c, w_c = ops.composite(raw_c, z_c, rays)
            z_f = ops.sample_fine(z_c, w_c, NEAR, FAR, NF)
            raw_f = ops.field_eval_rays(pf_f, rays, z_f)
            rgb_f, depth_f, acc_f, _ = ops.composite(raw_f, z_f, rays, want_weights=False)
        _REF[key] = dict(pf_c=pf_c, pf_f=pf_f, rays=rays, tr=tr, z_f=z_f, raw_f=raw_f, live=raw_f[..., 3] > 0,
                         outs=(depth_c, acc_c, rgb_f, depth_f, acc_f))
    return _REF[key]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same_bits(got, ref):
    for name, a, b in zip(("depth_c", "acc_c", "rgb_f", "depth_f", "acc_f"), got, ref["outs"]):
        assert torch.equal(_bits(a), _bits(b)), name


class _ChunkRows:
    """mi_render_set_colour_chunk_rows for the length of a with block; back to the build constant afterwards."""

    def __init__(self, rows):
        self.rows = rows

    def __enter__(self):
        from mirender import _lib
        _lib.load().mi_render_set_colour_chunk_rows(self.rows)

    def __exit__(self, *exc):
        from mirender import _lib
        _lib.load().mi_render_set_colour_chunk_rows(0)


def _align64(x):
    return (x + 63) // 64 * 64


def _chunk_rays(n, rows):
    return min(n, max(1, min(rows, n * S) // S)) if rows else n


def _counts(extra, n, rows):
    """The per-chunk live counts the call left in its extra buffer (rows [cap, 256] | idx [cap] | counts)."""
    cr = _chunk_rays(n, rows)
    cap, n_chunks = max(cr * S, min(rows if rows else n * S, n * S)), (n + cr - 1) // cr
    off = (_align64(cap * 256) + _align64(cap)) * 4
    return extra[off:off + 4 * n_chunks].view(torch.int32).cpu(), cr


def _want_counts(ref, n, cr):
    return torch.tensor([int(ref["live"][i:i + cr].sum()) for i in range(0, n, cr)], dtype=torch.int32)


class _Call:
    """mi_render_rays with rgb_c = NULL into fixed buffers (so that a graph can replay it)."""

    def __init__(self, ref, n, extra=True):
        from mirender import _lib, ops
        self.lib, self.ref, self.n = _lib.load(), ref, n
        self.base = self.lib.mi_render_workspace_bytes(n, NC, NF)
        self.extra = self.lib.mi_render_deferred_colour_extra_bytes(n, NC, NF) if extra else 0
        self.ws = torch.zeros(self.base + self.extra, dtype=torch.uint8, device=dev())
        self.outs = [torch.full(s, float("nan"), device=dev()) for s in ((n,), (n,), (n, 3), (n,), (n,))]
        self.zl, self.ul = ops.linspace_table(NEAR, FAR, NC, dev()), ops.linspace_table(0.0, 1.0, NF, dev())
        self.pc, self.pf = _lib.ptr(ref["pf_c"].refresh()), _lib.ptr(ref["pf_f"].refresh())

    def __call__(self):
        from mirender import _lib
        r = self.ref
        rc = self.lib.mi_render_rays(r["pf_c"].kind, self.pc, r["pf_f"].kind, self.pf, None, _lib.ptr(r["rays"]), 1, self.n,
                                     NEAR, FAR, NC, NF, _lib.ptr(self.zl), _lib.ptr(self.ul), _lib.ptr(r["tr"]), 0, 0, None,
                                     *[_lib.ptr(o) for o in self.outs], _lib.ptr(self.ws), self.base + self.extra,
                                     _lib.stream_ptr(dev()))
        assert rc == 0, self.lib.mi_last_error()
        return self.outs

    def counts(self, rows):
        return _counts(self.ws[self.base:], self.n, rows)


def _mixed(ref):
    share = float(ref["live"].float().mean())
    assert 0.1 <= share <= 0.9, share


def test_stage_nerf_mixed_field():
    """mi_field_eval_rays_deferred against mi_field_eval_rays on the same z_f."""
    from mirender import _lib
    lib = _lib.load()
    ref = _staged("nerf", N)
    _mixed(ref)
    with _ChunkRows(CHUNK):
        nbytes = lib.mi_render_deferred_colour_extra_bytes(N, NC, NF)
        extra = torch.zeros(nbytes, dtype=torch.uint8, device=dev())
        raw = torch.full((N, S, 4), float("nan"), device=dev())
        rc = lib.mi_field_eval_rays_deferred(ref["pf_f"].kind, _lib.ptr(ref["pf_f"].refresh()), None, _lib.ptr(ref["rays"]),
                                             _lib.ptr(ref["z_f"]), 1, N, S, _lib.ptr(raw), _lib.ptr(extra), nbytes,
                                             _lib.stream_ptr(dev()))
        assert rc == 0, lib.mi_last_error()
        assert lib.mi_field_eval_rays_deferred(ref["pf_f"].kind, _lib.ptr(ref["pf_f"].refresh()), None, _lib.ptr(ref["rays"]),
                                               _lib.ptr(ref["z_f"]), 1, N, S, _lib.ptr(raw), _lib.ptr(extra), nbytes - 1,
                                               _lib.stream_ptr(dev())) == -1
        got, cr = _counts(extra, N, CHUNK)
    want, live = ref["raw_f"], ref["live"]
    assert torch.equal(_bits(raw[..., 3]), _bits(want[..., 3]))
    assert torch.equal(_bits(raw[..., :3][live]), _bits(want[..., :3][live]))
    assert torch.equal(_bits(raw[..., :3][~live]), torch.zeros_like(_bits(raw[..., :3][~live])))
    assert cr == 85 and torch.equal(got, _want_counts(ref, N, cr))


@pytest.mark.parametrize("kind", ["nerf", "tiny_nerf"])
def test_whole_call_mixed_field(kind):
    """mi_render_rays with the extra workspace, four chunks - and with a base-only workspace (the whole forward)."""
    ref = _staged(kind, N)
    _mixed(ref)
    with _ChunkRows(CHUNK):
        call = _Call(ref, N)
        _assert_same_bits(call(), ref)
        got, cr = call.counts(CHUNK)
        assert len(got) == 4 and torch.equal(got, _want_counts(ref, N, cr))
        _assert_same_bits(_Call(ref, N, extra=False)(), ref)


@pytest.mark.parametrize("bias,share", [(-3000.0, 0.0), (3000.0, 1.0)])
def test_all_dead_and_all_live(bias, share):
    """No live point: every count is 0.  Every point live: every chunk's list is full, the buffer's worst case."""
    ref = _staged("nerf", N, bias)
    assert float(ref["live"].float().mean()) == share
    with _ChunkRows(CHUNK):
        call = _Call(ref, N)
        _assert_same_bits(call(), ref)
        got, cr = call.counts(CHUNK)
    assert got.tolist() == ([0, 0, 0, 0] if share == 0.0 else [85 * S, 85 * S, 85 * S, 2 * S])


def test_one_chunk():
    """Hook at 0: the chunk is capped at n * S."""
    ref = _staged("nerf", N)
    _mixed(ref)
    call = _Call(ref, N)
    assert call.extra >= N * S * 1028
    _assert_same_bits(call(), ref)
    got, cr = call.counts(0)
    assert cr == N and got.tolist() == [int(ref["live"].sum())]


def test_one_ray():
    ref = _staged("nerf", 1)
    live = int(ref["live"].sum())
    assert 1 <= live <= S - 1, live
    with _ChunkRows(CHUNK):
        call = _Call(ref, 1)
        _assert_same_bits(call(), ref)
        assert call.counts(CHUNK)[0].tolist() == [live]


def test_graph_replays():
    """The whole call captured on one stream and replayed twice: the counts are cleared inside the graph."""
    ref = _staged("nerf", N)
    _mixed(ref)
    with _ChunkRows(CHUNK):
        call = _Call(ref, N)
        call()                                                    # warm-up outside the capture (kernel attributes)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        for _ in range(2):
            for o in call.outs:
                o.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            _assert_same_bits(call.outs, ref)
            got, cr = call.counts(CHUNK)
            assert torch.equal(got, _want_counts(ref, N, cr))

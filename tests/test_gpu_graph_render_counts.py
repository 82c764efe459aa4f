"""GPU: mi_render_rays without coarse colours inside a HIP graph, with live counts that change between replays - at every size
of its two count clears.

On the frame path (two fields, rgb_c = NULL) the call keeps two sets of counters in its workspace and clears each once per
call: one count per window of the windowed coarse pass (4 * ceil(Nc / 8) bytes, at an address whose alignment depends on n and
Nc) and one per chunk of the deferred colour branch (4 * n_chunks bytes, 256-byte aligned).  A clear that does not happen on
replay is invisible to a replay of the capture's own inputs: the stale count only re-lists rays or points that are listed
anyway, and every result depends on its own ray alone.  It shows when the counts CHANGE - so here the field streams, the rays
and the jitter the graph reads are rewritten in place between replays, in the order

    eager warm-up, empty (every count 0) | capture | replay mixed, empty, full, mixed with other rays, empty

which makes the first stale count visible while every index is still inside its list: the replay of `empty` right behind
`mixed` must read back zeros.  After every replay the counts are read from the workspace (torch.zeros, so a stale list entry is a
valid ray or point index) and asserted - against the eager call's counts and against the counts derived on the CPU from the
staged reference's sigma alone - before the next replay is started.  The outputs equal the eager call bit for bit.

tools/probes/graph_memset_probe.py is why this file exists: on this runtime a captured hipMemsetAsync of more than 12 bytes, or
one that crosses a 16-byte line, clears its bytes on the first replay only (profiles/graph_memset_probe.log, DESIGN.md 4.8
"In a graph").  Both clears are kernels now (render_stages.hip: clear_floats_kernel); a change that turns one back into a memset
node, or that sizes a launch from a count the host knew at capture, fails here at the second replay.

  (a) window counts: Nc in {9, 20, 33, 48, 56, 80} = 2, 3, 5, 6, 7, 10 windows (8 to 40 bytes), n in {67, 130}, Nf = 8, nerf and
      siren_nerf, want = () (the 2^-42 rule, kStopBelowPdfEps) and ("depth_c",) (the 2^-151 rule).  Count r >= 1 is the number
      of rays whose first sample with a product <= threshold in front of it lies behind 8 r (tests/test_gpu_sampler_stop.py:
      _first_below).
  (b) chunk counts: n = 67, Nc = 16, Nf = 32, nerf, the chunk rows forced so that there are 3, 5, 6, 7 and 10 chunks; the FINE
      field switches between mixed, sigma_bias -3000 (no point live) and +3000 (every point live).  Count i is the number of
      points with sigma > 0 in chunk i of the staged reference.
  (c) ops.render_rays_fused(coarse_outputs=False), captured as tests/test_gpu_graph.py does, Nc = 48, n = 67: outputs only - its
      workspace lives in the graph's pool, so its counts cannot be watched, and it runs only behind a passed case (a) of the
      same (n, Nc, kind).

No replay passes vacuously: each first asserts on the staged reference alone what it claims - all stopped, none stopped,
10 - 90 % stopped in front of the last window (live share of the fine points in (b)) - and a count vector other than the
previous replay's.

Seeds: the CPU oracle (oracle/render_ref.py) at exactly these rays (graph_replay.rays_of(0) and (3)), jitter and shapes, `sharp`
sigma head; share of rays stopped in front of the last window, smallest .. largest over the 12 (n, Nc) and both replays:
    2^-42:   nerf seed 4: 13 .. 43 %        siren_nerf seed 4: 32 .. 54 %
    2^-151:  nerf seed 89: 28 .. 75 %       siren_nerf seed 16: 28 .. 64 %
(for 2^-151, nerf seed 3 stops no ray at n = 67, Nc = 48 with the rays of replay 3 and siren_nerf seed 14 stops 9 %; of seeds
0 .. 99 searched the same way, nerf 45, 52, 89, 93 and siren_nerf 16, 22, 32, 40, 67, ... hold the share everywhere.)  The
`empty` head (seed 5 sharp, sigma_bias +3000) leaves every product <= 2^-151 in front of sample 3; the `full` one (seed 5,
sharp=False) stops no ray.  (b): coarse seed 34, fine seed 3 as tests/test_gpu_deferred_colour.py: 70 - 76 % of the fine points
live at these rays."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import graph_replay as G  # noqa: E402
import test_gpu_deferred_colour as DC  # noqa: E402
import test_gpu_sampler_stop as SS  # noqa: E402
from oracle import parity, synth  # noqa: E402

dev = G.dev
WINDOW, STOP, ZERO = SS.WINDOW, SS.STOP, SS.ZERO
NEAR, FAR = G.NEAR, G.FAR
ORDER = ("mixed", "empty", "full", "mixed", "empty")          # replay k reads rays_of(k) and t_rand_of(k)
MIXED_SEED = {("nerf", ()): 4, ("nerf", ("depth_c",)): 89, ("siren_nerf", ()): 4, ("siren_nerf", ("depth_c",)): 16}

_FIELDS = {}
_PASSED = set()                                               # the cases (a) that passed in this session: (kind, n, nc, want)


def _packed(kind, seed, sharp, sigma_bias=0.0):
    """One PackedField per description, shared and left unchanged (the static streams are clones)."""
    key = (kind, seed, sharp, sigma_bias)
    if key not in _FIELDS:
        from mirender import fields
        sd = synth.state_dict(kind, seed=seed, sharp=sharp, bias_jitter=0.05)
        if sigma_bias:
            sd["output_layer_sigma.bias"] = sd["output_layer_sigma.bias"] + sigma_bias
        _FIELDS[key] = fields.as_packed_field(fields.field_from_state_dict(sd, dev()))
    return _FIELDS[key]


def _coarse_variants(kind, want):
    return {"mixed": _packed(kind, MIXED_SEED[(kind, want)], True), "empty": _packed(kind, 5, True, 3000.0),
            "full": _packed(kind, 5, False)}


class _Call:
    """mi_render_rays with rgb_c = NULL into fixed buffers: static clones of the two packed streams, static rays and t_rand,
    a zeroed workspace.  want: which of depth_c / acc_c the call asks for; extra: the deferred colour branch's buffer."""

    def __init__(self, pf_c, pf_f, n, nc, nf, want=(), extra=False):
        from mirender import _lib, ops
        self.lib, self.n, self.nc, self.nf = _lib.load(), n, nc, nf
        self.kinds = (pf_c.kind, pf_f.kind)
        self.stream_c, self.stream_f = pf_c.refresh().clone(), pf_f.refresh().clone()
        self.rays, self.tr = torch.zeros(n, 2, 3, device=dev()), torch.zeros(n, nc, device=dev())
        self.base = self.lib.mi_render_workspace_bytes(n, nc, nf)
        self.extra = self.lib.mi_render_deferred_colour_extra_bytes(n, nc, nf) if extra else 0
        self.ws = torch.zeros(self.base + self.extra, dtype=torch.uint8, device=dev())
        assert self.ws.data_ptr() % 256 == 0
        self.coarse = {k: torch.full((n,), float("nan"), device=dev()) for k in want}
        self.fine = [torch.full(s, float("nan"), device=dev()) for s in ((n, 3), (n,), (n,))]
        self.zl, self.ul = ops.linspace_table(NEAR, FAR, nc, dev()), ops.linspace_table(0.0, 1.0, nf, dev())

    def fill(self, pf_c, pf_f, k):
        """What replay k finds: the two fields' streams, the rays and the jitter, written in place."""
        self.stream_c.copy_(pf_c.refresh())
        self.stream_f.copy_(pf_f.refresh())
        self.rays.copy_(G.rays_of(k, self.n))
        self.tr.copy_(G.t_rand_of(k, self.n, self.nc))

    def __call__(self):
        from mirender import _lib
        c = [_lib.ptr(self.coarse[k]) if k in self.coarse else None for k in ("depth_c", "acc_c")]
        rc = self.lib.mi_render_rays(self.kinds[0], _lib.ptr(self.stream_c), self.kinds[1], _lib.ptr(self.stream_f), None,
                                     _lib.ptr(self.rays), 1, self.n, NEAR, FAR, self.nc, self.nf, _lib.ptr(self.zl),
                                     _lib.ptr(self.ul), _lib.ptr(self.tr), 0, 0, None, *c, *[_lib.ptr(o) for o in self.fine],
                                     _lib.ptr(self.ws), self.base + self.extra, _lib.stream_ptr(dev()))
        assert rc == 0, self.lib.mi_last_error()

    def outputs(self):
        d = dict(self.coarse)
        d.update(rgb_f=self.fine[0], depth_f=self.fine[1], acc_f=self.fine[2])
        return d

    def blank(self):
        for o in self.outputs().values():
            o.fill_(float("nan"))

    # RenderWorkspace (csrc/render_path.h): regions of align64(floats) floats, z_c [n,Nc] first, then raw_c's.
    # coarse_sigma_windows (csrc/render_path.hip): sigma [n,Nc] compact at the start of raw_c's region, two live lists [n]
    # behind it, then one count per window.
    def window_counts_at(self):
        """(byte offset of the window counts in the workspace, their number)"""
        n, nc = self.n, self.nc
        return 4 * (DC._align64(n * nc) + n * nc + 2 * n), (nc + WINDOW - 1) // WINDOW

    def window_counts(self):
        off, rounds = self.window_counts_at()
        return self.ws[off:off + 4 * rounds].view(torch.int32).cpu().tolist()

    def chunk_counts(self, rows):
        return DC._counts(self.ws[self.base:], self.n, rows)[0].tolist()


def _capture(call):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    return graph


def _clear_record(case, nbytes, address):
    """The case's record of its clear; `counts` grows by what each replay read back, `passed` is set by the last one."""
    return parity.record(case=case, stage="graph replay", qty="count clear", bytes=nbytes, address_mod_16=address % 16,
                         counts=[], active="exact", passed=False)


# ---- (a) window counts ------------------------------------------------------------------------------------------------------
_COARSE_REF = {}


def _coarse_ref(pf, n, nc, k):
    """The staged coarse pass of one field at replay k's rays and jitter: z_c and raw_c (its sigma is all that is read), once
    per key, shared and left unchanged."""
    key = (id(pf), n, nc, k)
    if key not in _COARSE_REF:
        from mirender import ops
        rays = G.rays_of(k, n)
        with torch.no_grad():
            z_c = ops.sample_coarse(n, NEAR, FAR, nc, dev(), G.t_rand_of(k, n, nc), seed=0)
            raw_c = ops.field_eval_rays(pf, rays, z_c)
        _COARSE_REF[key] = (dict(z_c=z_c, raw_c=raw_c), rays)
    return _COARSE_REF[key]


def _want_window_counts(pf, n, nc, k, threshold, variant):
    """Count r of the windowed pass from the staged reference alone, on the CPU; asserts what `variant` claims."""
    ref, rays = _coarse_ref(pf, n, nc, k)
    first = SS._first_below(ref, rays, threshold)
    rounds = (nc + WINDOW - 1) // WINDOW
    stopped = int(SS._stopped(first, nc).sum())
    if variant == "empty":
        assert int((first <= WINDOW).sum()) == n
    elif variant == "full":
        assert int((first < nc).sum()) == 0
    else:
        assert 0.1 * n <= stopped <= 0.9 * n, (stopped, n)
    return [0] + [int((first > WINDOW * r).sum()) for r in range(1, rounds)]


@pytest.mark.parametrize("want", [(), ("depth_c",)], ids=["stop42", "stop151"])
@pytest.mark.parametrize("kind", ["nerf", "siren_nerf"])
@pytest.mark.parametrize("n", [67, 130])
@pytest.mark.parametrize("nc", [9, 20, 33, 48, 56, 80])
def test_window_counts_follow_the_replayed_field(nc, n, kind, want):
    nf = 8
    threshold = ZERO if want else STOP
    variants, pf_f = _coarse_variants(kind, want), _packed(kind, 6, "medium")
    name = f"render counts windows {kind} n={n} Nc={nc} {'2^-151' if want else '2^-42'}"
    graphed, eager = _Call(variants["empty"], pf_f, n, nc, nf, want), _Call(variants["empty"], pf_f, n, nc, nf, want)
    off, rounds = graphed.window_counts_at()
    rec = _clear_record(name, 4 * rounds, graphed.ws.data_ptr() + off)
    with G.Case(name) as c:
        graphed.fill(variants["empty"], pf_f, 0)
        graphed()                                              # warm-up outside the capture: every count is left 0
        torch.cuda.synchronize()
        assert graphed.window_counts() == [0] * rounds
        graph = _capture(graphed)
        previous = [0] * rounds
        for k, variant in enumerate(ORDER):
            expect = _want_window_counts(variants[variant], n, nc, k, threshold, variant)
            assert expect != previous, (k, variant, expect)
            for call in (graphed, eager):
                call.fill(variants[variant], pf_f, k)
                call.blank()
            eager()
            graph.replay()
            torch.cuda.synchronize()
            got = graphed.window_counts()
            rec["counts"].append(got)
            print(f"{name}: replay {k} {variant}: counts {got}, eager {eager.window_counts()}, reference {expect}")
            assert got == eager.window_counts(), (k, variant, got, eager.window_counts())
            assert got == expect, (k, variant, got, expect)
            c.check(k, G.snapshot(graphed.outputs()), G.snapshot(eager.outputs()), counts=got)
            assert c.first is None, c.first
            previous = expect
        assert float(graphed.fine[0].std()) > 1e-3            # the last picture has contrast
        rec["passed"] = True
    _PASSED.add((kind, n, nc, want))


# ---- (b) chunk counts -------------------------------------------------------------------------------------------------------
N_B, NC_B, NF_B = 67, DC.NC, DC.NF                            # S = 48, the S that DC._counts mirrors the buffer for
_FINE_REF = {}


def _fine_live(pf_c, pf_f, k):
    """sigma > 0 of the staged fine pass [n, S] at replay k's rays and jitter; once per key, shared and left unchanged."""
    key = (id(pf_c), id(pf_f), k)
    if key not in _FINE_REF:
        from mirender import ops
        rays = G.rays_of(k, N_B)
        with torch.no_grad():
            z_c = ops.sample_coarse(N_B, NEAR, FAR, NC_B, dev(), G.t_rand_of(k, N_B, NC_B), seed=0)
            w_c = ops.composite(ops.field_eval_rays(pf_c, rays, z_c), z_c, rays)[3]
            z_f = ops.sample_fine(z_c, w_c, NEAR, FAR, NF_B)
            _FINE_REF[key] = (ops.field_eval_rays(pf_f, rays, z_f)[..., 3] > 0).cpu()
    return _FINE_REF[key]


@pytest.mark.parametrize("chunk_rays,n_chunks", [(23, 3), (14, 5), (12, 6), (10, 7), (7, 10)])
def test_chunk_counts_follow_the_replayed_field(chunk_rays, n_chunks):
    n, S, rows = N_B, NC_B + NF_B, chunk_rays * (NC_B + NF_B)
    assert (n + chunk_rays - 1) // chunk_rays == n_chunks
    pf_c = _packed("nerf", DC.COARSE_SEED["nerf"], True)
    fine = {"mixed": _packed("nerf", DC.FINE_SEED["nerf"], True), "empty": _packed("nerf", DC.FINE_SEED["nerf"], True, -3000.0),
            "full": _packed("nerf", DC.FINE_SEED["nerf"], True, 3000.0)}
    want = ("depth_c", "acc_c")
    name = f"render counts chunks nerf n={n} S={S} chunks={n_chunks}"
    with DC._ChunkRows(rows), G.Case(name) as c:
        graphed, eager = (_Call(pf_c, fine["empty"], n, NC_B, NF_B, want, extra=True) for _ in range(2))
        at = graphed.ws.data_ptr() + graphed.base + graphed.extra - 4 * DC._align64(n_chunks)
        rec = _clear_record(name, 4 * n_chunks, at)
        graphed.fill(pf_c, fine["empty"], 0)
        graphed()                                              # warm-up outside the capture: every count is left 0
        torch.cuda.synchronize()
        assert graphed.chunk_counts(rows) == [0] * n_chunks
        graph = _capture(graphed)
        previous = [0] * n_chunks
        for k, variant in enumerate(ORDER):
            live = _fine_live(pf_c, fine[variant], k)
            expect = [int(live[i:i + chunk_rays].sum()) for i in range(0, n, chunk_rays)]
            share = float(live.float().mean())
            lo, hi = {"empty": (0.0, 0.0), "full": (1.0, 1.0), "mixed": (0.1, 0.9)}[variant]
            assert lo <= share <= hi, (variant, share)
            assert expect != previous, (k, variant, expect)
            for call in (graphed, eager):
                call.fill(pf_c, fine[variant], k)
                call.blank()
            eager()
            graph.replay()
            torch.cuda.synchronize()
            got = graphed.chunk_counts(rows)
            rec["counts"].append(got)
            print(f"{name}: replay {k} {variant}: counts {got}, eager {eager.chunk_counts(rows)}, reference {expect}")
            assert got == eager.chunk_counts(rows), (k, variant, got, eager.chunk_counts(rows))
            assert got == expect, (k, variant, got, expect)
            c.check(k, G.snapshot(graphed.outputs()), G.snapshot(eager.outputs()), counts=got)
            assert c.first is None, c.first
            if variant == "mixed":                             # a picture with contrast (`empty` is the white background)
                assert float(graphed.fine[0].std()) > 1e-3
            previous = expect
        rec["passed"] = True


# ---- (c) the Python surface -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nerf", "siren_nerf"])
def test_render_rays_fused_without_coarse_outputs_replays(kind):
    from mirender import fields, ops
    n, nc, nf = 67, 48, 8
    if (kind, n, nc, ()) not in _PASSED:
        pytest.skip("its counts cannot be read (the workspace is the graph's): runs only behind a passed case (a) at this shape")
    variants, pf_f = _coarse_variants(kind, ()), _packed(kind, 6, "medium")
    # the captured call's coarse field: a PackedField of its own whose stream is rewritten in place (its parameters never
    # change, so refresh() keeps handing out that stream)
    sd = synth.state_dict(kind, seed=5, sharp=True, bias_jitter=0.05)
    static_c = fields.as_packed_field(fields.field_from_state_dict(sd, dev()))
    stream = static_c.refresh()
    stream.copy_(variants["empty"].refresh())
    s_rays, s_tr = G.rays_of(0, n).clone(), G.t_rand_of(0, n, nc).clone()

    def call(pf_c, rays, tr):
        with torch.no_grad():
            return ops.render_rays_fused(pf_c, pf_f, rays, NEAR, FAR, nc, nf, None, tr, coarse_outputs=False)

    names = ("rgb_c", "depth_c", "acc_c", "rgb_f", "depth_f", "acc_f")
    with G.Case(f"render counts render_rays_fused(coarse_outputs=False) {kind} n={n} Nc={nc}") as c:
        graph, s_out = G.capture(lambda: call(static_c, s_rays, s_tr))
        assert static_c.refresh().data_ptr() == stream.data_ptr()
        for k, variant in enumerate(ORDER):
            stream.copy_(variants[variant].refresh())
            G.refill((s_rays, s_tr), (G.rays_of(k, n), G.t_rand_of(k, n, nc)))
            graph.replay()
            torch.cuda.synchronize()
            got = G.snapshot(dict(zip(names, s_out)))
            c.check(k, got, dict(zip(names, call(variants[variant], G.rays_of(k, n), G.t_rand_of(k, n, nc)))))
            assert c.first is None, c.first
        assert all(got[q] is None for q in names[:3]) and float(got["rgb_f"].std()) > 1e-3

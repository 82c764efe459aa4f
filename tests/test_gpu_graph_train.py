"""GPU: the training calls inside a HIP graph (tests/test_gpu_graph.py holds the inference call to the same promise).

include/mi_render.h and INTEGRATION.md promise that every entry point only enqueues work on the caller's stream, so a call
sequence can be captured and replayed.  Here the sequence is one training step - render_core.render_rays with parameters that
require grad (autograd._RenderRaysFn), train.nerf_loss, loss.backward() - captured once with torch.cuda.graph and replayed with
new contents in its static ray, jitter and target buffers.  The reference of every replay is the eager step on the same inputs
from the same state, bit for bit (tests/graph_replay.py; tests/test_gpu_train.py holds the eager step run-to-run bit-equal).

  A  the plain step         nerf (two fields; once with a point budget that cuts the fine pass into four ranges, two of them
                            recomputed in backward), tiny_nerf (one shared field, Nf = 0 and 16), siren_nerf (two fields),
                            film_siren_nerf (one field, a two-image FiLM table that requires grad)
  B  state changing in place  five steps with an eager FusedAdam.step() between replays against the same loop fully eager:
                            the packed streams are one buffer each, rewritten in place; and torch.optim.Adam between replays,
                            where a replay renders the OLD streams until pf.refresh() / pf.refresh_bwd() ran eagerly
  E  the metrics            metrics.mse / ssim and nerf_loss on their own
  F  the workspace rule     a captured call never takes its workspace from ops._Workspace's cache nor leaves it there
  G  the refusals           FusedAdam.step and a render call that would draw a fresh host seed raise under capture, and work
                            eagerly afterwards with the bits they gave before

Shapes: 67 rays at 8 + 16 samples (536 and 1 608 points: several 32-point tiles with a partial last one, more than one dW
slab); the FiLM case two images of 67 rays at 12 + 24 in [0.5, 1.5] like the other FiLM tests.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import graph_replay as G  # noqa: E402

dev = G.dev


# ---- A. the plain training step -----------------------------------------------------------------------------------------------
PLAIN = {
    "nerf_pair": dict(kind="nerf", shared=False),
    "tiny_nerf_shared_nf0": dict(kind="tiny_nerf", shared=True, nf=0),
    "tiny_nerf_shared": dict(kind="tiny_nerf", shared=True),
    "siren_nerf_pair": dict(kind="siren_nerf", shared=False),
    # two images of 67 rays each: the rays must split evenly over the FiLM groups
    "film_siren_nerf": dict(kind="film_siren_nerf", shared=True, n=2 * G.N, film_images=2, **G.FILM_SHAPE),
}


@pytest.mark.parametrize("case", sorted(PLAIN))
def test_training_step_replayed_equals_eager(case):
    G.replay_against_eager(f"graph train {case}", G.TrainStep(**PLAIN[case]))


def test_training_step_with_recomputed_ranges_replayed_equals_eager(monkeypatch):
    """A point budget of 20 rays' fine samples: the fine pass is cut into four ranges (20, 20, 20, 7 rays), the coarse pass into
    two; the forward keeps the layer inputs of two fine ranges and of no coarse one, so the captured backward re-runs the saving
    forward for the others and adds the ranges' gradients (_foreach_add_) inside the graph."""
    from mirender import autograd, fields
    step = G.TrainStep("nerf", False)
    per_range = 20 * (G.NC + G.NF)
    lib_acts = 4 * autograd._lib.query("mi_field_train_acts_floats", fields.as_packed_field(step.models[0]).kind)
    monkeypatch.setattr(autograd, "_max_points_per_chunk", lambda pf: per_range)
    monkeypatch.setattr(autograd, "SAVE_FINE_BYTES", lib_acts * per_range * 2)
    monkeypatch.setattr(autograd, "SAVE_COARSE_BYTES", 0)
    pf = fields.as_packed_field(step.models[1])
    assert len(autograd._chunk_ranges(pf, G.N, G.NC + G.NF, None)[2]) >= 3
    want, _ = G.replay_against_eager("graph train nerf_pair, four ranges, two recomputed", step)
    # the cut itself moves no output bit (it only reorders the gradient sums): the same step without the budget
    monkeypatch.undo()
    whole = G.snapshot(step(*step.inputs(0)))
    assert all(G.differing(whole[f"out{k}"], want[0][f"out{k}"]) == 0 for k in range(6))


# ---- B. steps with state changing in place ------------------------------------------------------------------------------------
def _state(step, opt_state):
    """Parameters, both Adam moments and both packed streams of every field."""
    from mirender import fields
    d = {}
    for f, m in enumerate(step.models):
        pf = fields.as_packed_field(m)
        d[f"packed{f}"], d[f"packed_bwd{f}"] = pf.packed, pf.packed_bwd
        for i, p in enumerate(m.parameters()):
            d[f"param{f}.{i}"], d[f"exp_avg{f}.{i}"], d[f"exp_avg_sq{f}.{i}"] = p, opt_state[p]["exp_avg"], opt_state[p]["exp_avg_sq"]
    return G.snapshot(d)


def _eager_fused_loop(steps):
    from mirender import train
    step = G.TrainStep("nerf", False)
    opt = train.FusedAdam(list(step.models), lr=5e-4)
    losses = []
    for k in range(steps):
        losses.append(step(*step.inputs(k))["loss"].detach().clone())
        opt.step()
    return losses, _state(step, opt.state)


def test_fused_adam_between_replays_equals_the_eager_loop():
    """FusedAdam.step() rewrites the parameters and both packed streams of both fields in place, in the one buffer each that the
    graph holds: five replays with an eager step between them are the eager loop, bit for bit - every loss, and at the end the
    parameters, both moments and all four streams."""
    from mirender import fields, train
    steps = 5
    with G.Case("graph train: FusedAdam.step between replays, five steps") as c:
        want_losses, want_state = _eager_fused_loop(steps)
        again_losses, again_state = _eager_fused_loop(steps)
        c.eager_pair(dict(want_state, **{f"loss{k}": v for k, v in enumerate(want_losses)}),
                     dict(again_state, **{f"loss{k}": v for k, v in enumerate(again_losses)}))
        step = G.TrainStep("nerf", False)
        opt = train.FusedAdam(list(step.models), lr=5e-4)
        static_in = [t.clone() for t in step.inputs(0)]
        graph, static_out = G.capture(lambda: step(*static_in))
        pfs = [fields.as_packed_field(m) for m in step.models]
        ptrs = [(pf.packed.data_ptr(), pf.packed_bwd.data_ptr()) for pf in pfs]
        for k in range(steps):
            for s, t in zip(static_in, step.inputs(k)):
                s.copy_(t)
            graph.replay()
            c.check(k, {"loss": static_out["loss"].detach().clone()}, {"loss": want_losses[k]})
            opt.step()                                      # eager: its t and bias corrections are host values
        torch.cuda.synchronize()
        assert ptrs == [(pf.packed.data_ptr(), pf.packed_bwd.data_ptr()) for pf in pfs]      # one buffer each, all along
        c.check("end", _state(step, opt.state), want_state)
        assert float(want_losses[0]) != float(want_losses[-1])          # the weights did move


def test_torch_adam_between_replays_needs_an_eager_refresh():
    """With torch.optim.Adam the pack launches are not in the graph (refresh() returned early at capture: the streams were
    current).  After its step a replay still renders the OLD streams - the eager outputs of the old weights, bit for bit - until
    pf.refresh() / pf.refresh_bwd() ran eagerly; they repack into the same buffers, and the replay is the eager step again."""
    from mirender import fields
    with G.Case("graph train: torch.optim.Adam between replays") as c:
        graphed, eager, old = (G.TrainStep("nerf", False) for _ in range(3))       # three copies of one initial state
        opts = [torch.optim.Adam(s.leaves(), lr=5e-3) for s in (graphed, eager)]
        c.eager_pair(G.snapshot(eager(*eager.inputs(0))), G.snapshot(old(*old.inputs(0))))
        static_in = [t.clone() for t in graphed.inputs(0)]
        graph, static_out = G.capture(lambda: graphed(*static_in))
        pfs = [fields.as_packed_field(m) for m in graphed.models]
        ptrs = [(pf.packed.data_ptr(), pf.packed_bwd.data_ptr()) for pf in pfs]
        outputs = [f"out{k}" for k in range(6)] + ["loss", "psnr"]

        def replay(k):
            for s, t in zip(static_in, graphed.inputs(k)):
                s.copy_(t)
            graph.replay()
            torch.cuda.synchronize()
            return G.snapshot(static_out)

        c.check(0, replay(0), G.snapshot(eager(*eager.inputs(0))))
        for opt in opts:
            opt.step()                                      # the same gradients (just checked), so the same new weights
        # no refresh: the old streams
        stale, want_old, want_new = replay(1), G.snapshot(old(*old.inputs(1))), G.snapshot(eager(*eager.inputs(1)))
        c.check("1, not refreshed, against the old weights", {q: stale[q] for q in outputs}, {q: want_old[q] for q in outputs})
        assert G.differing(want_old["out3"], want_new["out3"]) > 0          # the step did change the picture
        for k in (1, 2):
            for pf in pfs:
                pf.refresh()
                pf.refresh_bwd()
            c.check(f"{k}, refreshed", replay(k), want_new if k == 1 else G.snapshot(eager(*eager.inputs(k))))
            for opt in opts:
                opt.step()
        assert ptrs == [(pf.packed.data_ptr(), pf.packed_bwd.data_ptr()) for pf in pfs]


# ---- E. the metrics -----------------------------------------------------------------------------------------------------------
def _images(k):
    g = torch.Generator().manual_seed(40 + k)
    a = torch.rand(2, 3, 24, 31, generator=g)
    return a.to(dev()), (0.8 * a + 0.2 * torch.rand(2, 3, 24, 31, generator=g)).to(dev())


def test_metrics_replayed_equal_eager():
    from mirender import metrics

    def run(a, b):
        return dict(mse=metrics.mse(a, b), ssim=metrics.ssim(a, b), ssim_per_image=metrics.ssim(a, b, size_average=False))
    with G.Case("graph metrics: mse, ssim of 2 x 3 x 24 x 31") as c:
        want = {k: G.snapshot(run(*_images(k))) for k in (0, 1, 2)}
        c.eager_pair(want[0], G.snapshot(run(*_images(0))))
        static_in = [t.clone() for t in _images(0)]
        graph, static_out = G.capture(lambda: run(*static_in))
        for k in (1, 2):
            for s, t in zip(static_in, _images(k)):
                s.copy_(t)
            graph.replay()
            torch.cuda.synchronize()
            c.check(k, G.snapshot(static_out), want[k])
        assert 0.0 < float(static_out["ssim"]) < 1.0 and float(static_out["mse"]) > 0.0


def test_nerf_loss_alone_replayed_equals_eager():
    from mirender import train
    n = G.N

    def inputs(k):
        g = torch.Generator().manual_seed(60 + k)
        outs = [torch.rand(s, generator=g).to(dev()) for s in ((n, 3), (n,), (n,), (n, 3), (n,), (n,))]
        return outs + list(G.target_of(k, n))

    def run(*t):
        loss, psnr = train.nerf_loss(tuple(t[:6]), t[6], t[7], use_alpha=True, use_fine_model=True)
        return dict(loss=loss, psnr=psnr)
    with G.Case("graph metrics: nerf_loss alone") as c:
        want = {k: G.snapshot(run(*inputs(k))) for k in (0, 1, 2)}
        c.eager_pair(want[0], G.snapshot(run(*inputs(0))))
        static_in = [t.clone() for t in inputs(0)]
        graph, static_out = G.capture(lambda: run(*static_in))
        for k in (1, 2):
            for s, t in zip(static_in, inputs(k)):
                s.copy_(t)
            graph.replay()
            torch.cuda.synchronize()
            c.check(k, G.snapshot(static_out), want[k])
        assert float(static_out["loss"]) > 0.0


# ---- F. the workspace rule ----------------------------------------------------------------------------------------------------
def test_a_captured_call_never_uses_the_cached_workspace(monkeypatch):
    """A warm-up on stream s leaves ops._Workspace a cached buffer for (device, s); a capture on s must neither take it nor
    replace it: its workspace is a fresh buffer of the graph's own pool (ops._workspace).  Then the cache grows under the first
    graph (a larger eager call on s), a second, larger graph is captured on s, and first, second, first replayed: each equals
    eager."""
    from mirender import ops
    pf_c, pf_f = G.field("nerf", 3, grad=False)[1], G.field("nerf", 4, grad=False)[1]
    sizes = (G.N, 2 * G.N)

    def inputs(n, k):
        return G.rays_of(k, n), G.t_rand_of(k, n)

    def render(rays, tr):
        with torch.no_grad():
            outs = ops.render_rays_fused(pf_c, pf_f, rays, G.NEAR, G.FAR, G.NC, G.NF, None, tr)
        return {f"out{k}": o for k, o in enumerate(outs)}
    with G.Case("graph workspace rule: two graphs on one warmed stream") as c:
        want = {(n, k): G.snapshot(render(*inputs(n, k))) for n in sizes for k in (0, 1, 2)}
        c.eager_pair(want[(sizes[0], 0)], G.snapshot(render(*inputs(sizes[0], 0))))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        key = (ops._Workspace._name(dev()), s.cuda_stream)
        with torch.cuda.stream(s):
            render(*inputs(sizes[0], 0))                                    # the warm-up that makes the hazard
        cached = ops._Workspace.bufs[key]
        handed, real = [], ops._workspace

        def recording(device, nbytes):
            ws, guard = real(device, nbytes)
            handed.append((ws, int(nbytes)))
            return ws, guard
        monkeypatch.setattr(ops, "_workspace", recording)
        graphs, static_in, static_out = {}, {}, {}
        for n in sizes:
            before = dict(ops._Workspace.bufs)
            del handed[:]
            static_in[n] = [t.clone() for t in inputs(n, 0)]
            graphs[n] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[n], stream=s):
                static_out[n] = render(*static_in[n])
            assert len(handed) == 1
            ws, nbytes = handed[0]
            held = ops._Workspace.bufs[key]
            assert ws is not held and ws.data_ptr() != held.data_ptr() and ws.numel() == nbytes        # fresh, exact, not the cache's
            assert ops._Workspace.bufs.keys() == before.keys() and all(ops._Workspace.bufs[q] is before[q] for q in before)
            if n == sizes[0]:
                with torch.cuda.stream(s):
                    render(*inputs(sizes[1], 0))                            # a larger eager call on s: the cache grows
                s.synchronize()
                assert ops._Workspace.bufs[key] is not cached and ops._Workspace.bufs[key].numel() > cached.numel()
                del cached
        for j, n in enumerate((sizes[0], sizes[1], sizes[0])):
            for st, t in zip(static_in[n], inputs(n, j)):
                st.copy_(t)
            torch.cuda.current_stream().synchronize()
            graphs[n].replay()
            torch.cuda.synchronize()
            c.check(f"{j} ({n} rays)", G.snapshot(static_out[n]), want[(n, j)])


# ---- G. what a replay would silently repeat is refused ------------------------------------------------------------------------
def test_fused_adam_and_unseeded_render_refuse_capture_and_work_afterwards():
    from mirender import _lib, render_core, train
    a, b = G.TrainStep("nerf", False), G.TrainStep("nerf", False)
    for s in (a, b):
        s(*s.inputs(0))                                                     # the same gradients on both
    opt_a, opt_b = train.FusedAdam(list(a.models), lr=5e-4), train.FusedAdam(list(b.models), lr=5e-4)
    opt_a.step()
    rays = G.rays_of(0)
    torch.manual_seed(7)
    with torch.no_grad():
        want = render_core.render_rays(rays, G.NEAR, G.FAR, b.models[0], b.models[1], G.NC, G.NF)
        torch.manual_seed(7)
        x = torch.zeros(8, device=dev())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = x + 1                                                       # so the graph is not empty
            with pytest.raises(_lib.MiRenderError, match="FusedAdam.step cannot be captured.*step count"):
                opt_b.step()
            with pytest.raises(_lib.MiRenderError, match="render_rays cannot be captured.*fresh seed"):
                render_core.render_rays(rays, G.NEAR, G.FAR, b.models[0], b.models[1], G.NC, G.NF)
        graph.replay()
        torch.cuda.synchronize()
        assert bool((y == 1).all())
        assert opt_b._step == 0 and not opt_b.state                         # refused before anything was touched
        got = render_core.render_rays(rays, G.NEAR, G.FAR, b.models[0], b.models[1], G.NC, G.NF)     # the draw the refusal left alone
    assert all(G.differing(g, w) == 0 for g, w in zip(got, want))
    opt_b.step()
    assert opt_b._step == 1
    for pa, pb in zip(a.leaves(), b.leaves()):
        assert G.differing(pa, pb) == 0
    # an explicit seed= stays allowed under capture: its replays repeat that jitter
    with torch.no_grad():
        want = render_core.render_rays(rays, G.NEAR, G.FAR, b.models[0], b.models[1], G.NC, G.NF, seed=5)
        graph, got = G.capture(lambda: render_core.render_rays(rays, G.NEAR, G.FAR, b.models[0], b.models[1], G.NC, G.NF, seed=5))
        graph.replay()
        torch.cuda.synchronize()
    assert all(G.differing(g, w) == 0 for g, w in zip(got, want))

"""Shared by tests/test_gpu_graph_train.py and tests/test_gpu_graph_occupancy.py: the inputs, the capture recipe and the bit
comparison of a call sequence replayed from a HIP graph against the same sequence called eagerly.

The rules of every graph here ("Graph capture"): one stream, captured with torch.cuda.graph, so the graph is a
linear chain; one warm-up on a side stream first, so packed streams and linspace tables exist before the capture; static input
buffers refilled in place between replays; the jitter a static t_rand buffer, never a host seed that changes; no environment
variable, no MI_DEBUG_GUARDS (its check reads back), no empty_cache() / _Workspace.release() between capture and replay.

The reference is the eager call on the same inputs from the same state, compared as torch.equal on int32 views.  Every case
leaves parity records with stage "graph replay": per quantity the number of differing elements over all replays, and the
sample counts each replay saw (cases with an occupancy grid).
"""
import numpy as np
import torch

from oracle import parity, render_ref as R, synth

N, NC, NF = 67, 8, 16                  # 536 coarse points, 1 608 fine: several 32-point tiles with a partial last one
NEAR, FAR = 2.0, 6.0
FILM_SHAPE = dict(near=0.5, far=1.5, nc=12, nf=24)


def dev():
    return torch.device("cuda", 0)


def rays_of(k, n=N):
    """The rays of replay k: n of the 1 600 rays of a 40 x 40 camera, spread over the frame, a different angle per replay."""
    r = torch.from_numpy(R.rays_from_camera(40, 40, 55.0, synth.pose_degrees(4.0, 20.0 + 40.0 * k, -30.0)))
    idx = (torch.arange(n) * 1600 // n + 20) % 1600
    return r[idx].contiguous().to(dev())


def t_rand_of(k, n=N, nc=NC):
    return synth.t_rand(n, nc, seed=10 + k).to(dev())


def target_of(k, n=N):
    g = torch.Generator().manual_seed(100 + k)
    return torch.rand(n, 3, generator=g).to(dev()), torch.rand(n, generator=g).to(dev())


def field(kind, seed, grad=True):
    """A fresh module (not shared between tests: FusedAdam and the optimiser cases rewrite it) and its PackedField."""
    from mirender import fields
    m = fields.field_from_state_dict(synth.state_dict(kind, seed=seed, sharp="medium", bias_jitter=0.05), dev())
    for p in m.parameters():
        p.requires_grad_(grad)
    return m, fields.as_packed_field(m)


def bits(t):
    t = t.detach().contiguous()
    return t if t.dtype == torch.int32 else t.view(torch.int32)


def differing(a, b) -> int:
    """Elements whose bits differ (shape and dtype must agree)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((bits(a) != bits(b)).sum())


def snapshot(named: dict) -> dict:
    """Clones of the named tensors (None stays None): what a replay left in its static outputs, before the next one."""
    return {k: (None if v is None else v.detach().clone()) for k, v in named.items()}


class Case:
    """The comparisons of one test: every check() is recorded, the records are written when the block ends - also when it ends
    in an exception - and a difference fails the test there, naming the side that moved."""

    def __init__(self, name):
        self.name, self.diff, self.counts, self.first = name, {}, [], None

    def __enter__(self):
        return self

    def _note(self, qty, d, where):
        self.diff[qty] = self.diff.get(qty, 0) + d
        if d and self.first is None:
            self.first = (qty, where, d)

    def eager_pair(self, a: dict, b: dict):
        """The precondition: the eager call twice on the same inputs from the same state, bit-equal.  A failure here is the
        eager path moving, not the graph."""
        assert a.keys() == b.keys()
        bad = {k: differing(a[k], b[k]) for k in a if a[k] is not None and differing(a[k], b[k])}
        parity.record(case=self.name, stage="graph replay: eager pair", qty=",".join(sorted(a)), differing=sum(bad.values()),
                      active="bit-exact", passed=not bad)
        assert not bad, (self.name, "two eager runs differ", bad)

    def check(self, k, got: dict, want: dict, counts=None):
        """Replay k against the eager call.  counts: what the replay's passes evaluated (a list), kept for the record."""
        assert got.keys() == want.keys(), (sorted(got), sorted(want))
        for qty in got:
            assert (got[qty] is None) == (want[qty] is None), (self.name, qty, "one side has no value")
            if got[qty] is not None:
                self._note(qty, differing(got[qty], want[qty]), f"replay {k}")
        if counts is not None:
            self.counts.append(counts)

    def __exit__(self, exc_type, exc, tb):
        for qty, d in self.diff.items():
            parity.record(case=self.name, stage="graph replay", qty=qty, differing=d, counts=self.counts, active="bit-exact",
                          passed=d == 0)
        if exc_type is None:
            assert self.first is None, (self.name, "the replay differs from the eager call: (quantity, where, elements)", self.first)
        return False


def capture(fn, warm=True):
    """torch's whole-network recipe: fn() once on a side stream (packs, tables, autograd's own buffers), then captured.  Returns
    (graph, what fn returned under capture: the static outputs)."""
    if warm:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def static_like(t):
    """A static buffer of a captured call holding t's contents; a leaf that requires grad where t is one (pose: the rays)."""
    return t.detach().clone().requires_grad_(t.requires_grad)


def refill(static, new):
    with torch.no_grad():
        for s, t in zip(static, new):
            s.copy_(t)


class TrainStep:
    """One training step over `models` ((m,) for one shared field, (coarse, fine) otherwise): render, train.nerf_loss,
    loss.backward().  The eager call and the captured one are the same function on other tensors.  render() is
    render_core.render_rays; the cases with an occupancy grid or gradients to the rays override it, prepare() (the state a
    replay finds: the grid's bits) and verify() (what a replay must show besides equalling the eager step)."""

    def __init__(self, kind, shared, nc=NC, nf=NF, n=N, near=NEAR, far=FAR, film_images=0, seeds=(3, 4), rays_grad=False):
        self.models = (field(kind, seeds[0])[0],) if shared else (field(kind, seeds[0])[0], field(kind, seeds[1])[0])
        self.film = synth.film_params(film_images, seed=1).to(dev()).requires_grad_(True) if film_images else None
        self.n, self.nc, self.nf, self.near, self.far, self.rays_grad = n, nc, nf, near, far, rays_grad

    def leaves(self):
        return [p for m in self.models for p in m.parameters()] + ([] if self.film is None else [self.film])

    def inputs(self, k):
        rgb, alpha = target_of(k, self.n)
        return rays_of(k, self.n).requires_grad_(self.rays_grad), t_rand_of(k, self.n, self.nc), rgb, alpha

    def prepare(self, k):
        pass

    def verify(self, k, got):
        pass

    def render(self, rays, tr):
        """(the six outputs, the counts of the passes or None)"""
        from mirender import render_core
        return render_core.render_rays(rays, self.near, self.far, self.models[0], self.models[-1], self.nc, self.nf, t_rand=tr,
                                       film=self.film), None

    def __call__(self, rays, tr, rgb, alpha):
        from mirender import train
        for p in self.leaves() + [rays]:
            p.grad = None                                 # gradients start as None: backward writes them, it does not add
        outs, counts = self.render(rays, tr)
        loss, psnr = train.nerf_loss(outs, rgb, alpha, use_alpha=True, use_fine_model=True)
        loss.backward()
        d = {f"out{k}": o for k, o in enumerate(outs)}
        d.update(loss=loss, psnr=psnr)
        for f, m in enumerate(self.models):
            for i, p in enumerate(m.parameters()):
                d[f"grad{f}.{i}"] = p.grad
        if self.film is not None:
            d["film.grad"] = self.film.grad
        if self.rays_grad:
            d["rays.grad"] = rays.grad
        if counts is not None:
            d["counts"] = counts
        return d

    def eager(self, k):
        self.prepare(k)
        return snapshot(self(*self.inputs(k)))


def replay_against_eager(case, step, replays=(0, 1, 2), capture_at=None):
    """The eager step at every replay's inputs and state (at the capture's twice: the precondition), then the capture, then the
    replays, each compared with its eager step and shown to step.verify().  Returns (the eager results by k, the counts the
    replays saw)."""
    capture_at = replays[0] if capture_at is None else capture_at
    with Case(case) as c:
        want = {k: step.eager(k) for k in sorted(set(replays) | {capture_at})}
        c.eager_pair(want[capture_at], step.eager(capture_at))
        step.prepare(capture_at)
        static_in = [static_like(t) for t in step.inputs(capture_at)]
        graph, static_out = capture(lambda: step(*static_in))
        assert all(v is not None for v in static_out.values()), [k for k, v in static_out.items() if v is None]
        for k in replays:
            step.prepare(k)
            refill(static_in, step.inputs(k))
            graph.replay()
            torch.cuda.synchronize()
            got = snapshot(static_out)
            c.check(k, got, want[k], counts=got["counts"].tolist() if "counts" in got else None)
            step.verify(k, got)
        # the case is not degenerate: the last replay's picture has contrast, its gradients are not all zero
        assert float(static_out["out3"].detach().std()) > 1e-3
        assert any(float(v.abs().max()) > 0 for q, v in static_out.items() if q.startswith("grad"))
    return want, c.counts


def ball(dims, fraction):
    """bool [dims]: the cells whose centre lies in a ball about the grid's centre holding about `fraction` of the cells."""
    ax = [np.arange(d) + 0.5 - d / 2.0 for d in dims]
    r2 = ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2
    radius = (fraction * dims[0] * dims[1] * dims[2] * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0)
    return r2 <= radius * radius

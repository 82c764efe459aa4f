"""GPU: rendering and training with an occupancy grid inside a HIP graph, with list counts that change between replays.

DESIGN.md 4.8 says of the list-driven passes: "count read on the device and clamped to the capacity; no read-back ... the launch
is sized from `n`".  Every eager test calls with the count its own call marked, so a launch sized on the host from the data would
pass them all.  Only a replay whose count differs from the count at capture can tell: here a graph is captured over a random
half-full 16^3 grid and replayed after the grid's bits were rewritten IN PLACE - all ones, all zeros, a ball of about a twentieth
of the cells, the half-full grid again - so the counts go partial, full, 0, small, partial, each longer list followed by a shorter
one over the same workspace, which then still holds the previous replay's list and rows (the stale rows the eager tests imitate
with NaN sentinels).  The reference of every replay is the eager call on the same inputs and bits, bit for bit
(tests/graph_replay.py); tests/test_gpu_occupancy_train.py ("two runs") and tests/test_gpu_occupancy_pose.py hold the eager
calls run-to-run bit-equal.

  C  inference (render_rays(grid=), with and without clip_probes=32, two boxes), the training step (occupancy_train.render_rays,
     nerf_loss, backward: nerf pair, tiny_nerf shared, siren_nerf pair; nerf pair with clip_probes=32 and with max_points cutting
     the rays into three calls) and pose.render_rays(grid=) with rays that require grad (and once without a grid)
  D  a LiveOccupancyGrid under the captured training step: eager update() calls rewrite the bits the graph holds
  G  LiveOccupancyGrid.update refuses capture

The replay on all zeros must give the background and exact zero gradients; the replay on all ones lists every sample of the box
that holds every sample and equals the call without a grid where the eager suite states that equality
(test_covering_grid_changes_no_bit, test_pair_with_an_all_ones_grid_equals_plain_training / _pose_without_a_grid).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import graph_replay as G  # noqa: E402

dev = G.dev
DIMS = (16, 16, 16)
BIG = ((-4.0,) * 3, (4.0,) * 3)                # holds every sample of every ray used here (|coordinate| < 3.5)
SMALL = ((-1.5,) * 3, (1.5,) * 3)              # a box the rays partly leave
HALF = np.random.Generator(np.random.PCG64(31)).random(DIMS) < 0.5
# the grid a call finds: replays 0..3, and 4 the capture (the same bits as 3, other rays)
STATES = [np.ones(DIMS, bool), np.zeros(DIMS, bool), G.ball(DIMS, 0.05), HALF, HALF]
ONES, ZEROS, CAPTURE = 0, 1, 4
REPLAYS = (0, 1, 2, 3)


def _bits_of(dense):
    from mirender import occupancy
    return torch.from_numpy(occupancy.pack_dense(dense).view(np.int32)).to(dev())


class _GridMixin:
    """The grid of a case and the bits each replay finds, written in place; what the all-zeros and the all-ones replay owe."""

    def init_grid(self, box, ones_equals_plain):
        from mirender import occupancy
        self.grid = occupancy.OccupancyGrid.from_dense(HALF, box[0], box[1], dev())
        self.box, self.ones_equals_plain = box, ones_equals_plain
        self.ptr = self.grid.bits.data_ptr()
        self.states = [_bits_of(d) for d in STATES]

    def prepare(self, k):
        self.grid.bits.copy_(self.states[k])
        assert self.grid.bits.data_ptr() == self.ptr

    def verify(self, k, got):
        if "counts" not in got:                                               # the one case without a grid
            return
        full = [self.n * self.nc, self.n * (self.nc + self.nf)]
        counts = got["counts"].sum(0).tolist()
        if k == ZEROS:
            assert counts == [0, 0]
            for q in ("out0", "out3"):
                assert bool((got[q] == 1).all()), q                           # the white background
            for q in ("out1", "out2", "out4", "out5"):
                assert bool((got[q] == 0).all()), q
            assert all(bool((v == 0).all()) for q, v in got.items() if "grad" in q)      # exact zeros, parameters and rays
        if k == ONES and self.box is BIG:
            assert counts == full, (counts, full)
        if k == ONES and self.ones_equals_plain:
            plain = self.plain_ones
            same = [q for q in plain if q.startswith("out") or q in ("loss", "psnr") or self.ones_equals_plain == "all"]
            bad = {q: G.differing(got[q], plain[q]) for q in same if G.differing(got[q], plain[q])}
            assert not bad, ("all-ones grid against the call without a grid", bad)


def _check_counts(counts, n, nc, nf, box):
    """The case proves something only if the counts moved: every replay another count than the one before, 0 among them, and -
    in the box that holds every sample - the full count."""
    totals = [np.asarray(c).sum(0).tolist() for c in counts]
    assert all(a != b for a, b in zip(totals, totals[1:])), totals
    assert [0, 0] in totals, totals
    assert all(t[0] > 0 and t[1] > 0 for t in (totals[2], totals[3])), totals              # the ball and the half-full grid list something
    assert totals[3][0] < n * nc and totals[3][1] < n * (nc + nf), totals                  # ... and the half-full grid not everything
    if box is BIG:
        assert [n * nc, n * (nc + nf)] in totals, totals


# ---- C. inference ---------------------------------------------------------------------------------------------------------------
class _Inference(_GridMixin):
    def __init__(self, box, clip):
        self.models = (G.field("nerf", 3, grad=False)[0], G.field("nerf", 4, grad=False)[0])
        self.n, self.nc, self.nf, self.clip = G.N, G.NC, G.NF, clip
        self.init_grid(box, "outputs" if clip is None and box is BIG else None)
        self.plain_ones = self.plain(ONES) if self.ones_equals_plain else None

    def inputs(self, k):
        return G.rays_of(k), G.t_rand_of(k)

    def __call__(self, rays, tr, grid="own"):
        from mirender import render_core
        grid = self.grid if grid == "own" else grid
        with torch.no_grad():
            res = render_core._render_rays(rays, G.NEAR, G.FAR, *self.models, self.nc, self.nf, t_rand=tr, grid=grid,
                                           return_counts=grid is not None, clip_probes=self.clip)
        outs, counts = res if grid is not None else (res, None)
        d = {f"out{k}": o for k, o in enumerate(outs)}
        if counts is not None:
            d["counts"] = counts
        return d

    def plain(self, k):
        return G.snapshot(self(*self.inputs(k), grid=None))

    def eager(self, k):
        self.prepare(k)
        return G.snapshot(self(*self.inputs(k)))


@pytest.mark.parametrize("box,clip", [("big", None), ("small", None), ("big", 32), ("small", 32)])
def test_inference_with_a_grid_replayed_over_changing_counts(box, clip):
    """The atomic mark: the order of the list is not fixed, outputs and counts are."""
    step = _Inference(BIG if box == "big" else SMALL, clip)
    with G.Case(f"graph occupancy inference, {box} box, clip_probes={clip}") as c:
        want = {k: step.eager(k) for k in REPLAYS + (CAPTURE,)}
        c.eager_pair(want[CAPTURE], step.eager(CAPTURE))
        step.prepare(CAPTURE)
        static_in = [t.clone() for t in step.inputs(CAPTURE)]
        graph, static_out = G.capture(lambda: step(*static_in))
        for k in REPLAYS:
            step.prepare(k)
            G.refill(static_in, step.inputs(k))
            graph.replay()
            torch.cuda.synchronize()
            got = G.snapshot(static_out)
            c.check(k, got, want[k], counts=got["counts"].tolist())
            step.verify(k, got)
        _check_counts(c.counts, step.n, step.nc, step.nf, step.box)


# ---- C. the training step and the pose step ---------------------------------------------------------------------------------------
class _GridStep(_GridMixin, G.TrainStep):
    """occupancy_train.render_rays (pose.render_rays(grid=) with rays_grad) + nerf_loss + backward over self.grid."""

    def __init__(self, kind, shared, box=BIG, ones_equals_plain=None, clip=None, max_points=None, rays_grad=False, grid=True):
        G.TrainStep.__init__(self, kind, shared, rays_grad=rays_grad)
        self.clip, self.max_points, self.with_grid = clip, max_points, grid
        self.init_grid(box, ones_equals_plain)
        # the same step without a grid at the all-ones replay's inputs, run before anything is captured
        self.plain_ones = self.plain(ONES) if ones_equals_plain else None

    def render(self, rays, tr):
        from mirender import occupancy_train, pose
        mc, mf = self.models[0], self.models[-1]
        if not self.with_grid:                                                # pose.render_rays without a grid, once
            return pose.render_rays(rays, G.NEAR, G.FAR, mc, mf, self.nc, self.nf, t_rand=tr), None
        kw = dict(grid=self.grid, t_rand=tr, clip_probes=self.clip, max_points=self.max_points)
        if self.rays_grad:
            # pose.render_rays returns the six outputs; the counts of its calls are occupancy_train's on the same inputs
            return pose.render_rays(rays, G.NEAR, G.FAR, mc, mf, self.nc, self.nf, **kw), self._counts(rays, tr)
        return occupancy_train.render_rays(rays, G.NEAR, G.FAR, mc, mf, self.nc, self.nf, return_counts=True, **kw)

    def _counts(self, rays, tr):
        from mirender import occupancy_train
        with torch.no_grad():
            return occupancy_train.render_rays(rays.detach(), G.NEAR, G.FAR, self.models[0], self.models[-1], self.nc, self.nf,
                                               grid=self.grid, t_rand=tr, clip_probes=self.clip, return_counts=True)[1]

    def plain(self, k):
        """The same step without a grid: render_core.render_rays under autograd, or pose.render_rays for the rays' gradient."""
        twin = object.__new__(G.TrainStep)
        twin.__dict__.update(self.__dict__)
        if self.rays_grad:
            from mirender import pose
            twin.render = lambda rays, tr: (pose.render_rays(rays, G.NEAR, G.FAR, self.models[0], self.models[-1], self.nc,
                                                             self.nf, t_rand=tr), None)
        return G.snapshot(twin(*self.inputs(k)))


TRAIN = {
    # two fields, the box that holds every sample: on all ones the outputs AND every gradient are the plain training path's bits
    "nerf_pair": dict(kind="nerf", shared=False, ones_equals_plain="all"),
    # one field: the outputs are, the gradients are other sums (test_pair_with_an_all_ones_grid_equals_plain_training)
    "tiny_nerf_shared": dict(kind="tiny_nerf", shared=True, ones_equals_plain="outputs"),
    "siren_nerf_pair_small_box": dict(kind="siren_nerf", shared=False, box=SMALL),
    "nerf_pair_clip32": dict(kind="nerf", shared=False, clip=32),
    # three calls of 23, 23 and 21 rays; autograd sums their gradients: the outputs are the plain path's, the sums are others
    "nerf_pair_three_calls": dict(kind="nerf", shared=False, max_points=23 * (2 * G.NC + G.NF), ones_equals_plain="outputs"),
    "pose_nerf_pair": dict(kind="nerf", shared=False, rays_grad=True, ones_equals_plain="all"),
    "pose_tiny_nerf_shared_clip32": dict(kind="tiny_nerf", shared=True, rays_grad=True, clip=32),
}


@pytest.mark.parametrize("case", sorted(TRAIN))
def test_training_step_with_a_grid_replayed_over_changing_counts(case):
    step = _GridStep(**TRAIN[case])
    _want, counts = G.replay_against_eager(f"graph occupancy train {case}", step, replays=REPLAYS, capture_at=CAPTURE)
    assert len(counts) == len(REPLAYS) and all(len(c) == (3 if step.max_points else 1) for c in counts)
    _check_counts(counts, step.n, step.nc, step.nf, step.box)


def test_pose_step_without_a_grid_replayed_equals_eager():
    step = _GridStep("nerf", False, rays_grad=True, grid=False)
    want, _ = G.replay_against_eager("graph pose.render_rays without a grid", step)
    assert float(want[0]["rays.grad"].abs().max()) > 0


# ---- D. a live grid under the captured step ----------------------------------------------------------------------------------------
LIVE_STEPS = 6


def _live():
    from mirender import occupancy
    # threshold: the mean density (relative, min(threshold, mean)), so every update leaves a grid that is neither full nor empty
    return occupancy.LiveOccupancyGrid(BIG[0], BIG[1], DIMS[0], dev(), threshold=1e30, relative=True, seed=3)


def _live_update(live, fine, k):
    if k in (0, 2, 4):
        live.update(fine, cells=None if k == 0 else live.grid.cells // 4)       # a sweep once, a quarter of the cells twice


def _live_state(step, live):
    d = dict(density=live.density, bits=live.grid.bits)
    for f, m in enumerate(step.models):
        for i, p in enumerate(m.parameters()):
            d[f"param{f}.{i}"] = p
    return G.snapshot(d)


def _eager_live_loop():
    from mirender import train
    step = _GridStep("nerf", False)
    live = _live()
    step.grid, step.prepare = live.grid, lambda k: None
    opt = train.FusedAdam(list(step.models), lr=5e-4)
    per_step, bits = [], []
    for k in range(LIVE_STEPS):
        _live_update(live, step.models[1], k)
        bits.append(live.grid.bits.clone())
        res = step(*step.inputs(k))
        per_step.append(G.snapshot(dict(loss=res["loss"], counts=res["counts"])))
        opt.step()
    return per_step, _live_state(step, live), bits


def test_live_grid_updates_between_replays_equal_the_eager_loop():
    """Six steps, live.update(fine) before steps 0, 2 and 4 and FusedAdam.step() after each.  The graph holds live.grid, whose
    bits every update rewrites in place (occupancy.py: "a captured graph that holds `live.grid` sees the new bits")."""
    from mirender import train
    with G.Case("graph occupancy train: LiveOccupancyGrid updated between replays") as c:
        want, want_state, bits = _eager_live_loop()
        again, again_state, _ = _eager_live_loop()
        flat = lambda steps, state: dict(state, **{f"{q}{k}": v for k, s in enumerate(steps) for q, v in s.items()})  # noqa: E731
        c.eager_pair(flat(want, want_state), flat(again, again_state))
        # the scenario proves something: every update changed the bits, no grid was full or empty
        assert all(G.differing(bits[a], bits[b]) > 0 for a, b in ((0, 2), (2, 4)))
        step = _GridStep("nerf", False)
        live = _live()
        step.grid, step.prepare = live.grid, lambda k: None
        ptr = live.grid.bits.data_ptr()
        opt = train.FusedAdam(list(step.models), lr=5e-4)
        static_in = [t.clone() for t in step.inputs(0)]
        graph, static_out = G.capture(lambda: step(*static_in))          # over the fresh live grid: every cell occupied
        for k in range(LIVE_STEPS):
            _live_update(live, step.models[1], k)
            assert live.grid.bits.data_ptr() == ptr
            G.refill(static_in, step.inputs(k))
            graph.replay()
            got = G.snapshot(dict(loss=static_out["loss"], counts=static_out["counts"]))
            c.check(k, got, want[k], counts=got["counts"].tolist())
            opt.step()
        torch.cuda.synchronize()
        c.check("end", _live_state(step, live), want_state)
        totals = [np.asarray(x).sum(0).tolist() for x in c.counts]
        full = [step.n * step.nc, step.n * (step.nc + step.nf)]
        assert len({tuple(t) for t in totals}) == LIVE_STEPS, totals         # the counts moved at every step
        assert all(0 < t[0] < full[0] and 0 < t[1] < full[1] for t in totals), (totals, full)


# ---- G. the refusal ------------------------------------------------------------------------------------------------------------------
def test_live_grid_update_refuses_capture_and_works_afterwards():
    from mirender import _lib
    fine = G.field("nerf", 4, grad=False)[0]
    a, b = _live(), _live()
    a.update(fine)
    x = torch.zeros(8, device=dev())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = x + 1                                                              # so the graph is not empty
        with pytest.raises(_lib.MiRenderError, match="LiveOccupancyGrid.update cannot be captured.*epoch"):
            b.update(fine)
    graph.replay()
    torch.cuda.synchronize()
    assert bool((y == 1).all()) and b.updates == 0 and bool((b.density == 0).all())      # refused before anything was touched
    b.update(fine)
    assert b.updates == 1 and G.differing(a.density, b.density) == 0 and G.differing(a.grid.bits, b.grid.bits) == 0

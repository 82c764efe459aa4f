#!/usr/bin/env python3
"""Generate the FiLM depth fixtures by IMPORTING the reference (build container only, CPU fp32).

Run once, here:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_film_depth.py
Outputs tests/golden/film_depth_L{4,6,12}_{dir,nodir}.npz (committed; data only): the reference's own
FilmSirenNeRF(hidden_layers=L, use_dir=...) (pi_GAN/modules.py:70-118)

  field      out.{plain,medium} [257,4] on 257 points for the two sigma-head scalings, FiLM row set 1 of 2
  gradient   the six outputs of the reference's render_rays (pi_GAN/render.py) for 64 rays in 2 images, 8+16 samples, one
             shared field, injected jitter, and autograd's gradients of sum_k <out_k, cot_k> with respect to every parameter
             and the FiLM table (512 strided samples + sum + L2 norm per tensor, like F6: an L = 12 state dict is 3 MB)

Weights, FiLM rows, rays, jitter and cotangents come from tests/film_depth_util.py's seeded generators; the fixture holds
their sha256 digest.

The sigma head sits behind a ReLU: a point whose pre-activation is within fp32 error of 0 has no meaningful gradient gate.
The field points are therefore conditioned: sigma_pre is evaluated by the reference class in fp32 and fp64, and a point with
|sigma_pre64| < 100 x max|sigma_pre32 - sigma_pre64| is redrawn (at most 10 % of the points, else the seed must change).  The
achieved margin and the redraw count are stored; the gradient call's sample points cannot be redrawn one by one, so its margin
and the number of points under it are stored as found.
"""
import contextlib
import os
import sys

os.environ["MKL_CBWR"] = "AVX2,STRICT"      # as tests/conftest.py and make_golden.py

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import film_depth_util as U  # noqa: E402


def load_reference():
    sys.path.insert(0, os.path.join(REF, "pi_GAN"))
    import render as pigan_render  # noqa
    import modules as pigan_modules  # noqa
    sys.path.pop(0)
    return pigan_render, pigan_modules


@contextlib.contextmanager
def injected_rand(queue):
    orig = torch.rand

    def fake(shape, *a, **k):
        t = queue.pop(0)
        assert tuple(t.shape) == tuple(shape), (t.shape, shape)
        return t.clone()
    torch.rand = fake
    try:
        yield
    finally:
        torch.rand = orig


def ref_model(pm, L, use_dir, sd, dtype=torch.float32):
    m = pm.FilmSirenNeRF(hidden_layers=L, use_dir=use_dir)
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)


def sigma_pre(m, film, x):
    """The reference module's sigma pre-activation: its own layers, up to the Linear of output_layer_sigma."""
    m.set_film_params(film)
    fp = m.film_params
    h = m.input_layer(x[:, :3], *fp[0])
    for i in range(m.n_layers):
        h = m.hidden_layers[i](h, *fp[i + 1])
    return m.output_layer_sigma[0](h)


def conditioned_points(pm, L, use_dir, sd, film, seed):
    m32, m64 = ref_model(pm, L, use_dir, sd), ref_model(pm, L, use_dir, sd, torch.float64)
    x = U.sample_points(257, seed)
    spare = U.sample_points(257, seed + 1000)
    redraws = 0
    with torch.no_grad():
        for _ in range(50):
            s32, s64 = sigma_pre(m32, film, x), sigma_pre(m64, film.double(), x.double())
            err = float((s32.double() - s64).abs().max())
            bad = torch.nonzero(s64.abs().reshape(-1) < 100 * err).reshape(-1)
            if not len(bad):
                break
            for i in bad.tolist():
                x[i] = spare[redraws % 257]
                redraws += 1
        else:
            raise SystemExit("points did not settle: change the seed")
    assert redraws <= 25, f"{redraws} redraws > 10 % of 257 points: change the seed, do not raise the cap"
    return x, float(s64.abs().min() / err), redraws


def main():
    torch.set_num_threads(8)
    pr, pm = load_reference()
    for L in U.DEPTHS:
        for use_dir in (True, False):
            out = {}
            film = U.film_rows(2, L, seed=100 + L)
            # ---- field ----
            sds = {h: U.state_dict(L, use_dir, seed=200 + L, head=h) for h in ("plain", "medium")}
            x, margin, redraws = conditioned_points(pm, L, use_dir, sds["medium"], film[1], seed=300 + L)
            with torch.no_grad():
                for h, sd in sds.items():
                    m = ref_model(pm, L, use_dir, sd)
                    m.set_film_params(film[1])
                    out[f"out.{h}"] = m(x).numpy()
                    out[f"digest.{h}"] = np.array(U.digest(sd, film))
            out.update(x=x.numpy(), sigma_margin=np.float64(margin), redraws=np.int64(redraws))
            # ---- gradient ----
            sd = U.state_dict(L, use_dir, seed=400 + L, head="medium")
            gfilm = U.film_rows(U.N_GROUPS, L, seed=500 + L).clone().requires_grad_(True)
            m = ref_model(pm, L, use_dir, sd)
            rays, tr, cot = U.grad_rays(), U.t_rand(), U.cotangents()
            rpg = U.N_RAYS // U.N_GROUPS
            parts = []
            with injected_rand([tr[g * rpg:(g + 1) * rpg] for g in range(U.N_GROUPS)]):
                for g in range(U.N_GROUPS):
                    m.set_film_params(gfilm[g])
                    parts.append(pr.render_rays(rays[g * rpg:(g + 1) * rpg], U.NEAR, U.FAR, m, m, U.NC, U.NF))
            outs = [torch.cat([p[k] for p in parts]) for k in range(6)]
            loss = sum((o * c).sum() for o, c in zip(outs, cot))
            loss.backward()
            for name, o in zip(U.OUT_NAMES, outs):
                out[name] = o.detach().numpy()
            named = [(k, p.grad) for k, p in m.named_parameters()] + [("film", gfilm.grad)]
            for name, g in named:
                g = g.detach().numpy().reshape(-1)
                idx = U.subsample_idx(g.size)
                out[f"g.{name}.idx"], out[f"g.{name}.val"] = idx, g[idx]
                out[f"g.{name}.sum"] = np.float64(g.astype(np.float64).sum())
                out[f"g.{name}.l2"] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
            out["loss"] = loss.detach().numpy()
            out["digest.grad"] = np.array(U.digest(sd, gfilm.detach(), rays, tr, *cot))
            # the restatement must reproduce the reference on the spot (CPU, same torch): the GPU tests lean on it
            r_outs, r_grads, r_gfilm = U.oracle_render_grads(sd, gfilm.detach())
            worst = max(float((a - b).abs().max()) for a, b in zip(r_outs, outs))
            gworst = max(float((r_grads[k] - p.grad).norm() / p.grad.norm()) for k, p in m.named_parameters())
            assert worst <= 1e-6 and gworst <= 1e-5, (L, use_dir, worst, gworst)
            name = f"film_depth_L{L}_{'dir' if use_dir else 'nodir'}"
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, **out)
            print(f"{name}.npz {os.path.getsize(path) / 1024:.1f} KiB margin {margin:.0f} redraws {redraws} "
                  f"restatement: outputs {worst:.1e} grads {gworst:.1e}", flush=True)


if __name__ == "__main__":
    main()

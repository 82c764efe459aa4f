"""Shared helpers of the FiLM depth tests (tests/test_film_depth_host.py, tests/test_gpu_film_depth.py) and of the fixture
generator tests/golden/make_golden_film_depth.py: FilmSirenNeRF(hidden_dim=256, hidden_layers=L) for L other than the
reference's default 8.

Weights and FiLM rows come from a seeded NumPy PCG64 generator with the distributions oracle/synth.py uses for depth 8
(pi_GAN/modules.py:27-31, torch.nn.Linear's default for the two heads), so the fixtures store a sha256 digest instead of
the tensors.  `forward` is the CPU restatement of the depth-L network (modules.py:101-118), in whatever dtype its weights
have: the fp32 and fp64 reference of the GPU tests."""
from __future__ import annotations

import hashlib

import numpy as np
import torch

DEPTHS = (4, 6, 12)                 # the depths with reference-pinned fixtures
NEAR, FAR, NC, NF = 0.5, 1.5, 8, 16  # the gradient fixture's render_rays call: 64 rays in 2 groups, one shared field
N_RAYS, N_GROUPS = 64, 2
# the "", "medium" and sharp head scalings of the F5 family (oracle/synth.py:SIGMA_HEAD)
SIGMA_HEAD = {"plain": (1.0, 0.0), "medium": (8.0, 2.0), "sharp": (50.0, 5.0)}


def kind_of(L: int, use_dir: bool) -> int:
    """MI_FIELD_FILM_DEPTH(L, use_dir) of include/mi_render.h."""
    return 0x100 + 2 * L + (1 if use_dir else 0)


def spec(L: int, use_dir: bool) -> list:
    """(key, (out, in)) per linear layer, the reference's layout for hidden_layers = L (pi_GAN/modules.py:76-94)."""
    return ([("input_layer", (256, 3))] + [(f"hidden_layers.{i}", (256, 256)) for i in range(L - 1)]
            + [("output_layer_sigma.0", (1, 256)), ("hidden_layer_rgb", (256, 259 if use_dir else 256)),
               ("output_layer_rgb.0", (3, 256))])


def macs(L: int, use_dir: bool) -> int:
    return 256 * 3 + (L - 1) * 256 * 256 + 256 + 256 * (259 if use_dir else 256) + 3 * 256


def _uniform(rng, shape, bound):
    return rng.uniform(-bound, bound, size=shape).astype(np.float32)


def state_dict(L: int, use_dir: bool, seed: int, head: str = "plain") -> dict:
    """Synthetic fp32 state dict; `head`: "plain" (the initialiser's sigma head), "medium" (x8, +2) or "sharp" (x50, +5:
    oracle/synth.py)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    scale, shift = SIGMA_HEAD[head]
    sd = {}
    for key, (o, i) in spec(L, use_dir):
        if key in ("output_layer_sigma.0", "output_layer_rgb.0"):
            b = 1.0 / np.sqrt(i)
            w, bias = _uniform(rng, (o, i), b), _uniform(rng, (o,), b)
        else:
            wb = 1.0 / i if key == "input_layer" else np.sqrt(6.0 / i) / 30.0
            w, bias = _uniform(rng, (o, i), wb), _uniform(rng, (o,), np.sqrt(1.0 / i))
        if key == "output_layer_sigma.0":
            w, bias = w * np.float32(scale), bias + np.float32(shift)
        sd[key + ".weight"] = torch.from_numpy(np.ascontiguousarray(w))
        sd[key + ".bias"] = torch.from_numpy(np.ascontiguousarray(bias.astype(np.float32)))
    return sd


def film_rows(n_images: int, L: int, seed: int, spread: float = 0.25) -> torch.Tensor:
    """[n_images, L + 1, 512] FiLM table: gamma around 1, beta around 0 (pi_GAN/modules.py:56-58)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = _uniform(rng, (n_images, L + 1, 512), spread)
    f[:, :, :256] += 1.0
    return torch.from_numpy(f)


def digest(sd: dict, *extra) -> str:
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k].detach().cpu().numpy()).tobytes())
    for t in extra:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def sample_points(n: int, seed: int, scale: float = 1.5) -> torch.Tensor:
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = rng.uniform(-scale, scale, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return torch.from_numpy(np.concatenate([pos, d.astype(np.float32)], -1))


def forward(sd: dict, film: torch.Tensor, x: torch.Tensor, w_0: float = 30.0, want_sigma_pre: bool = False):
    """FilmSirenNeRF.forward (pi_GAN/modules.py:101-118) for one image: film [L + 1, 512], x [M, 6] -> [M, 4]."""
    L = sum(1 for k in sd if k.startswith("hidden_layers.") and k.endswith(".weight")) + 1
    use_dir = sd["hidden_layer_rgb.weight"].shape[1] == 259
    lin = lambda h, key: torch.nn.functional.linear(h, sd[key + ".weight"], sd[key + ".bias"])  # noqa: E731
    siren = lambda h, key, r: torch.sin(w_0 * (film[r, :256] * lin(h, key) + film[r, 256:]))    # noqa: E731
    h = siren(x[:, :3], "input_layer", 0)
    for i in range(L - 1):
        h = siren(h, f"hidden_layers.{i}", i + 1)
    sigma_pre = lin(h, "output_layer_sigma.0")
    h = siren(torch.cat([h, x[:, 3:]], -1) if use_dir else h, "hidden_layer_rgb", L)
    out = torch.cat([torch.sigmoid(lin(h, "output_layer_rgb.0")), torch.relu(sigma_pre)], -1)
    return (out, sigma_pre) if want_sigma_pre else out


def field(sd: dict, film: torch.Tensor):
    """The callable oracle/render_ref.py drives: x [M, 6] -> [M, 4]."""
    return lambda x: forward(sd, film, x)


def to64(sd: dict) -> dict:
    return {k: v.double() for k, v in sd.items()}


def grad_rays(seed: int = 11) -> torch.Tensor:
    """[N_RAYS, 2, 3]: origins on the unit sphere's +z cap looking at the origin (the pi_GAN camera's geometry)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    o = rng.normal(size=(N_RAYS, 3)).astype(np.float32) * 0.15 + np.array([0, 0, 1], np.float32)
    tgt = rng.uniform(-0.2, 0.2, size=(N_RAYS, 3)).astype(np.float32)
    d = tgt - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return torch.from_numpy(np.stack([o, d.astype(np.float32)], 1))


def t_rand(seed: int = 12) -> torch.Tensor:
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.random((N_RAYS, NC), dtype=np.float32))


def cotangents(seed: int = 13) -> list:
    """One fixed cotangent per render_rays output: the loss is sum_k <out_k, cot_k> (F6's scalar loss, on all six)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [torch.from_numpy(rng.normal(size=s).astype(np.float32)) for s in ((N_RAYS, 3), (N_RAYS,), (N_RAYS,)) * 2]


OUT_NAMES = ("rgb_c", "depth_c", "acc_c", "rgb_f", "depth_f", "acc_f")


def subsample_idx(n: int, k: int = 512):
    return np.unique(np.linspace(0, n - 1, min(n, k)).astype(np.int64))


def oracle_render_grads(sd: dict, film: torch.Tensor, dtype=torch.float32):
    """oracle/render_ref.render_rays per image with the injected jitter, one shared field, then autograd of the fixed loss:
    (six outputs, {parameter: grad}, grad of the FiLM table), in `dtype`."""
    from oracle import render_ref as R
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    fl = film.to(dtype).clone().requires_grad_(True)
    rays, tr = grad_rays().to(dtype), t_rand().to(dtype)
    rpg = N_RAYS // N_GROUPS
    outs = []
    for g in range(N_GROUPS):
        f = field(p, fl[g])
        outs.append(R.render_rays(rays[g * rpg:(g + 1) * rpg], NEAR, FAR, f, f, NC, NF, tr[g * rpg:(g + 1) * rpg]).outputs())
    outs = [torch.cat([o[k] for o in outs]) for k in range(6)]
    loss = sum((o * c.to(dtype)).sum() for o, c in zip(outs, cotangents()))
    loss.backward()
    return [o.detach() for o in outs], {k: v.grad for k, v in p.items()}, fl.grad

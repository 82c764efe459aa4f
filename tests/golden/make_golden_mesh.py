#!/usr/bin/env python3
"""Family F11: marching-cubes fixtures (mesh_f11_m1..m6.npz), the mesh half of create_mesh (pi_GAN/utils.py:109-180).

    python tests/golden/make_golden_mesh.py

The volumes are built here (numpy; M5 with the field oracle); skimage.measure.marching_cubes_lewiner runs in a separate
interpreter that has scikit-image 0.18.3 (the last release with it) but no torch: $MI_SKIMAGE_PYTHON, default
/opt/conda/bin/python3.9.  Every file stores the volume, level, spacing and skimage's verts / faces / normals / values
(M6: the ValueError message instead)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SKIMAGE_PY = os.environ.get("MI_SKIMAGE_PYTHON", "/opt/conda/bin/python3.9")

HELPER = r"""
import sys, warnings
warnings.simplefilter("ignore")
import numpy as np
from skimage.measure import marching_cubes_lewiner
d = dict(np.load(sys.argv[1]))
out = {}
try:
    v, f, n, val = marching_cubes_lewiner(d["volume"], level=float(d["level"]), spacing=tuple(d["spacing"].tolist()))
    out = dict(verts=np.asarray(v), faces=f, normals=n, values=val, error=np.array(""))
except ValueError as e:
    out = dict(error=np.array(str(e)))
np.savez(sys.argv[2], **out)
"""

M5_FIELD = dict(kind="film_siren_nerf", seed=11, sharp=True, film_seed=3)   # oracle.synth parameters of M5's field


def m5_volume():
    sys.path.insert(0, ROOT)
    from oracle import fields, grid, synth
    sd = synth.state_dict(M5_FIELD["kind"], seed=M5_FIELD["seed"], sharp=M5_FIELD["sharp"])
    film = synth.film_params(1, seed=M5_FIELD["film_seed"])[0]
    return grid.density_grid(fields.make_field(M5_FIELD["kind"], sd, film), 48).numpy()


def volumes():
    x, y, z = np.mgrid[0:40, 0:40, 0:40].astype(np.float64)
    yield "m1", (np.sqrt((x - 19.3) ** 2 + (y - 20.1) ** 2 + (z - 18.7) ** 2) - 13.2).astype(np.float32), 0.0, (1, 1, 1)
    x, y, z = np.mgrid[0:44, 0:44, 0:24].astype(np.float64)
    r = np.sqrt((x - 21.6) ** 2 + (y - 22.3) ** 2)
    yield "m2", (np.sqrt((r - 13.0) ** 2 + (z - 11.4) ** 2) - 5.1).astype(np.float32), 0.0, (1, 1, 1)
    rng = np.random.Generator(np.random.PCG64(17))
    noise = rng.standard_normal((17, 23, 31))
    k = np.array([0.25, 0.5, 0.25])
    for ax in range(3):
        noise = np.apply_along_axis(lambda a: np.convolve(a, k, mode="same"), ax, noise)
    yield "m3", noise.astype(np.float32), 0.05, (1, 1, 1)
    yield "m4", rng.integers(-3, 4, (9, 11, 13)).astype(np.float32), 1.0, (1, 1, 1)
    vol = m5_volume()
    vs = 0.2 / 47
    level = -20.0 if vol.min() <= -20.0 <= vol.max() else float(np.quantile(vol, 0.05))
    yield "m5", vol, level, (vs, vs, vs)
    yield "m6", np.linspace(-1.0, 1.0, 8 * 9 * 10, dtype=np.float32).reshape(8, 9, 10), 2.5, (1, 1, 1)


def main():
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(os.path.dirname(os.path.dirname(SKIMAGE_PY)), "lib"))
    with tempfile.TemporaryDirectory() as tmp:
        helper = os.path.join(tmp, "mc.py")
        open(helper, "w").write(HELPER)
        for name, vol, level, spacing in volumes():
            src, dst = os.path.join(tmp, name + "_in.npz"), os.path.join(tmp, name + "_out.npz")
            np.savez(src, volume=vol, level=np.float64(level), spacing=np.asarray(spacing, np.float64))
            subprocess.check_call([SKIMAGE_PY, "-W", "ignore", helper, src, dst], env=env, timeout=600)
            out = dict(np.load(dst))
            rec = dict(volume=vol, level=np.float64(level), spacing=np.asarray(spacing, np.float64), **out)
            if name == "m5":
                rec.update({"field_" + k: np.array(v) for k, v in M5_FIELD.items()})
            path = os.path.join(HERE, f"mesh_f11_{name}.npz")
            np.savez_compressed(path, **rec)
            nf = len(out["faces"]) if "faces" in out else 0
            print(f"{path}: volume {vol.shape} level {level:g} faces {nf} error {str(out['error'])!r} "
                  f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

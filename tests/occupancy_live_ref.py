"""A live occupancy grid's three device calls restated in numpy (include/mi_render.h "a live grid"), shared by
tests/test_occupancy_live_host.py (known answers, the inputs' properties, planted mistakes) and
tests/test_gpu_occupancy_live.py (which holds mi_occupancy_draw_points, mi_occupancy_density_update,
mi_occupancy_density_pack and LiveOccupancyGrid against it, bit for bit).

    philox4x32_10 / stream_words   the random words, in Python ints
    draw                           row -> cell and jittered point, fp32 with one operation per rounding
    fold                           density_c = fmax(fl(density_c * decay), max over the cell's rows of (sigma > 0 ? sigma : +0))
    pack                           mean in fp64, thr = fmin(threshold, mean) or threshold, density > thr, dilation, words

and the inputs both test files use: draw_bits, fold_inputs, pack_inputs.
"""
import functools

import numpy as np

from mirender import occupancy
from test_occupancy_host import dense_reference

M32 = 0xFFFFFFFF
SEED = 0x9E3779B97F4A7C15                  # both key words non-zero
DIMS = [(3, 5, 7), (33, 2, 2), (16, 16, 16)]


def philox4x32_10(counter, key):
    """The Philox4x32-10 block (Salmon et al. 2011) of a 4-word counter under a 2-word key: 4 words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


@functools.lru_cache(maxsize=None)
def stream_words(seed, stream, n=12):
    """The first n words of stream R under `seed`: word w is word w & 3 of the block with counter (R_lo, R_hi, w >> 2, 0)."""
    key = (seed & M32, (seed >> 32) & M32)
    out = []
    for j in range((n + 3) // 4):
        out.extend(philox4x32_10((stream & M32, (stream >> 32) & M32, j, 0), key))
    return tuple(out[:n])


def bit_of(bits, cell):
    return (int(bits[cell >> 5]) >> (cell & 31)) & 1


def draw(bits, dims, lo, cell, seed, epoch, mode, row0, count, n_uniform, epoch_in_stream=True):
    """mi_occupancy_draw_points: (cell_ids int32 [count], points float32 [count,6], tries int [count]).  tries[i] is the
    candidate an occupied-share row accepted (8: none, it fell back to the last), -1 for sweep and uniform rows.
    epoch_in_stream=False plants the mistake of a stream that forgets the epoch."""
    cells = dims[0] * dims[1] * dims[2]
    ids, tries = np.zeros(count, np.int32), np.full(count, -1)
    u = np.zeros((count, 3), np.float32)
    for i in range(count):
        r = row0 + i
        w = stream_words(seed, ((epoch if epoch_in_stream else 0) << 32) | r)
        u[i] = [np.float32(w[d] >> 8) * np.float32(2.0 ** -24) for d in range(3)]
        if mode == 0:
            c = r
        elif r < n_uniform:
            c = (w[3] * cells) >> 32
        else:
            cand = [(w[4 + a] * cells) >> 32 for a in range(8)]
            hit = [a for a in range(8) if bit_of(bits, cand[a])]
            tries[i] = hit[0] if hit else 8
            c = cand[hit[0]] if hit else cand[7]
        ids[i] = c
    ijk = np.stack([ids // (dims[1] * dims[2]), (ids // dims[2]) % dims[1], ids % dims[2]], -1).astype(np.float32)
    lo, cell = np.asarray(lo, np.float32).reshape(3), np.asarray(cell, np.float32).reshape(3)
    pts = np.zeros((count, 6), np.float32)
    pts[:, :3] = lo + (ijk + u) * cell                         # an add, a multiply, an add: float32 arrays, each op rounded
    return ids, pts, tries


def fold(density, sigma, cell_ids, decay):
    """mi_occupancy_density_update: the new density [cells] (float32); cells without a row keep their bits."""
    density, sigma = np.asarray(density, np.float32), np.asarray(sigma, np.float32)
    v = np.where(sigma > 0, sigma, np.float32(0.0)).astype(np.float32)      # -0.0, negatives, NaN: +0
    out = density.copy()
    with np.errstate(invalid="ignore"):
        for c in np.unique(cell_ids):
            m = v[cell_ids == c].max()
            out[c] = np.fmax(np.float32(density[c] * np.float32(decay)), m)
    return out


def threshold_of(density, threshold, relative):
    """(mean, thr) of mi_occupancy_density_pack as float32."""
    density = np.asarray(density, np.float32)
    mean = np.float32(np.sum(density.astype(np.float64)) / density.size)
    return mean, (np.fmin(np.float32(threshold), mean) if relative else np.float32(threshold))


def pack(density, dims, threshold, relative, dilate, strict=True):
    """mi_occupancy_density_pack: (dense bool [Gx,Gy,Gz], uint32 words).  strict=False plants >= in place of >."""
    density = np.asarray(density, np.float32)
    _, thr = threshold_of(density, threshold, relative)
    if strict:
        dense = dense_reference(density, dims, 1, thr, dilate)
    else:
        dense = dense_reference((density >= thr).astype(np.float32), dims, 1, 0.5, dilate)
    return dense, occupancy.pack_dense(dense)


def same_bits(a, b):
    """The comparison of the GPU tests: equal shape, dtype and BITS (-0.0 is not +0, a NaN equals itself)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------
def draw_bits(name, dims):
    """uint32 words of the grids the draw is tested on: "random" (30 % occupied), "zeros", "ones"."""
    if name == "random":
        dense = np.random.Generator(np.random.PCG64(21)).random(dims) < 0.3
    else:
        dense = np.ones(dims, bool) if name == "ones" else np.zeros(dims, bool)
    return occupancy.pack_dense(dense)


FOLD_CELLS, FOLD_ROWS = 105, 1000
FOLD_UNSAMPLED = (17, 50, 104)
# cells whose rows are all of one special kind, and the two whose largest sigma is their first / their last row
ALL_NEG_ZERO, ALL_NEGATIVE, ALL_NAN, HAS_INF, MAX_FIRST, MAX_LAST, NAN_AND_POSITIVE, BELOW_OLD, NEG_ZERO_AND_POSITIVE = range(9)


def fold_inputs():
    """(density [105] distinct positive, sigma [1000], cell_ids [1000]): many rows per cell, three cells without any."""
    rng = np.random.Generator(np.random.PCG64(33))
    ids = rng.integers(0, FOLD_CELLS, FOLD_ROWS).astype(np.int32)
    for c in FOLD_UNSAMPLED:
        ids[ids == c] = c + 1 if c + 1 < FOLD_CELLS else 20
    sigma = rng.normal(size=FOLD_ROWS).astype(np.float32) * np.float32(4.0)          # about half negative
    density = (np.float32(0.25) + np.arange(FOLD_CELLS, dtype=np.float32) * np.float32(0.03125))[rng.permutation(FOLD_CELLS)]
    rows = {c: np.flatnonzero(ids == c) for c in range(9)}
    sigma[rows[ALL_NEG_ZERO]] = np.float32(-0.0)
    sigma[rows[ALL_NEGATIVE]] = -np.abs(sigma[rows[ALL_NEGATIVE]]) - np.float32(1.0)
    sigma[rows[ALL_NAN]] = np.float32("nan")
    sigma[rows[HAS_INF][1]] = np.float32("inf")
    sigma[rows[MAX_FIRST]] = np.float32(1.0)
    sigma[rows[MAX_FIRST][0]] = np.float32(50.0)
    sigma[rows[MAX_LAST]] = np.float32(1.0)
    sigma[rows[MAX_LAST][-1]] = np.float32(60.0)
    sigma[rows[NAN_AND_POSITIVE]] = np.float32("nan")
    sigma[rows[NAN_AND_POSITIVE][2]] = np.float32(9.5)
    sigma[rows[BELOW_OLD]] = np.float32(2.0 ** -20)
    sigma[rows[NEG_ZERO_AND_POSITIVE]] = np.float32(-0.0)
    sigma[rows[NEG_ZERO_AND_POSITIVE][1]] = np.float32(7.25)
    return density, sigma, ids


PACK_CASES = [("mean below the threshold", 1000.0, 1), ("mean above the threshold", 2.5, 1), ("absolute", 600.25, 0)]


def pack_inputs(dims):
    """density [cells]: multiples of 2^-10 below 1024 (any order of an fp64 sum is exact), 70 % of them zero; the values 2.5
    and 600.25, the thresholds of two of PACK_CASES, are present."""
    cells = dims[0] * dims[1] * dims[2]
    rng = np.random.Generator(np.random.PCG64(44))
    d = rng.integers(0, 1 << 20, cells).astype(np.float32) * np.float32(2.0 ** -10)
    d[rng.random(cells) < 0.7] = 0.0
    d[5], d[cells - 3] = 2.5, 600.25
    return d

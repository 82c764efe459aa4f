"""Gates of the evaluation stages (csrc/eval_stages.hip; test_eval_gates_host.py, test_gpu_eval_gates.py): torch only,
nothing from the product.

The frame-metrics kernel works in 32x32 tiles and leaves one partial pair {ssim sum, squared-error sum} per tile in its
workspace; the loss kernel leaves four block sums per 256 rays.  Each is rebuilt here in float64 from the kernels' own
float32 inputs, next to a first-order bound built from absolute values (as bwd_gates.py does for the field backward), so
the gates look at every tile, every block and every gradient seed instead of at one mean per image or batch.

Also here, for the CPU test that shows the gates have teeth: a float32 restatement of the kernel's own order (separable
passes, the 4-pixel / butterfly / 4-wave tile sum) with the mistakes a tiled kernel can make as options."""
from __future__ import annotations

import math
from collections import namedtuple
from functools import lru_cache

import torch
import torch.nn.functional as F

U = 2.0 ** -24                 # unit roundoff of fp32
TILE = 32                      # image_metrics_kernel: output pixels per workgroup side
C1, C2 = 1e-4, 9e-4            # pytorch_ssim: 0.01^2, 0.03^2
MAX_WINDOW = 31                # include/mi_render.h: window_size odd and <= 31
SUM_DEPTH = 13                 # additions on the longest path of a tile's sum (4 per thread, 6 butterfly steps, 3 waves)
SE_TILE_U = 15.0               # squared-error tile: two roundings per term + SUM_DEPTH, rigorous, nothing calibrated
MEAN_TOL = 2e-5                # the per-image gate of test_gpu_metrics.py (SSIM_TOL), for the proof of the gap

# The SSIM tile gate |partial - sum m| <= C_TILE (sqrt(sum b^2) + sqrt(13) u sum |m|), calibrated on the CPU against two
# fp32 computations and never against the kernel (test_eval_gates_host.py::test_calibration, every case of CASES).  The
# worst achieved ratio was 0.489 for the reference's 2-D (ws^2-tap) form (oracle.metrics.ssim's map; 96x130, window 27,
# noise) and 0.078 for the separable order the kernel uses (31x33, window 3, noise), so the constant is 3x the larger,
# rounded up to a tenth.  The factor is bwd_gates.py's: room for another valid fp32 association.  The 2-D form stays
# below 0.15 up to window 11 and reaches 0.3-0.5 only with 27 taps and more on noise: its window fl(g[i] g[j]) is
# rounded once for the whole image, an error every pixel of a tile shares, where the quadrature sum assumes independence.
CAL_2D, CAL_SEPARABLE = 0.489, 0.078
C_TILE = 1.5

SEED_U = 8.0                   # loss seeds: fl(fl(wc w) d), w = fl(2 / fl(3 n)), d = fl(x - t): 5 roundings, fl(0.1), 2 slack
BLOCK_U = 14.0                 # loss block sums: d, d^2 (3 u), 2 adds per ray, 6 butterfly steps, 3 waves
OUT_U = 16.0                   # loss outputs: the block sums, the fp64 reduce, one rounding to fp32


# ---- the window ------------------------------------------------------------------------------------------------------
def gaussian(window_size: int, sigma: float = 1.5) -> torch.Tensor:
    """pytorch_ssim.gaussian: the normalised fp32 taps both the reference and mi_image_metrics' callers use."""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)],
                     dtype=torch.float32)
    return g / g.sum()


# ---- float64 reference and bound ---------------------------------------------------------------------------------------
def _band(n: int, g64: torch.Tensor) -> torch.Tensor:
    """[n, n] banded matrix of a zero-padded 1-D correlation with the taps g: T[i, k] = g[k - i + r]."""
    ws = g64.numel()
    t = torch.arange(n)[None, :] - torch.arange(n)[:, None] + ws // 2
    return torch.where((t >= 0) & (t < ws), g64[t.clamp(0, ws - 1)], torch.zeros((), dtype=torch.float64))


def conv64_2d(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """The definition: F.conv2d of x [N,C,H,W] (float64) with the window g[i] g[j] formed in float64, zero padding,
    groups = C.  Slow for wide windows; ssim_map64 applies the same window as two banded-matrix products, which differs
    from this by float64 rounding only (test_eval_gates_host.py holds the two together)."""
    g64 = g.double()
    c = x.shape[1]
    w2 = (g64[:, None] * g64[None, :])[None, None].expand(c, 1, g.numel(), g.numel())
    return F.conv2d(x, w2, padding=g.numel() // 2, groups=c)


def ssim_map64(img1: torch.Tensor, img2: torch.Tensor, g: torch.Tensor):
    """(m, b): pytorch_ssim's map of two fp32 batches [N,C,H,W] in float64 - 2-D window g[i] g[j] formed in float64 from the
    fp32 taps, zero padding, groups = C - and a per-pixel first-order bound on what an fp32 evaluation of it may differ by.
    gamma = (2 ws + 3) u counts the roundings of two separable passes of ws taps (ws products, ws additions per pass and
    the product a a / b b / a b)."""
    assert img1.dtype == torch.float32 and img2.dtype == torch.float32 and g.dtype == torch.float32
    a, b = img1.double(), img2.double()
    ws = g.numel()
    tv, th = _band(a.shape[-2], g.double()), _band(a.shape[-1], g.double()).T
    conv = lambda x: tv @ x @ th  # noqa: E731
    gamma = (2 * ws + 3) * U
    mu1, mu2 = conv(a), conv(b)
    e11, e22, e12 = conv(a * a), conv(b * b), conv(a * b)
    d_mu1, d_mu2 = gamma * conv(a.abs()), gamma * conv(b.abs())
    d_e11, d_e22, d_e12 = gamma * e11, gamma * e22, gamma * conv((a * b).abs())
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    d_s1 = d_e11 + 2 * mu1.abs() * d_mu1 + U * (e11 + mu1 * mu1)
    d_s2 = d_e22 + 2 * mu2.abs() * d_mu2 + U * (e22 + mu2 * mu2)
    d_s12 = d_e12 + mu1.abs() * d_mu2 + mu2.abs() * d_mu1 + U * (e12.abs() + (mu1 * mu2).abs())
    n1, n2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    d1, d2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    d_n1 = 2 * (mu1.abs() * d_mu2 + mu2.abs() * d_mu1) + 2 * U * n1.abs()
    d_n2 = 2 * d_s12 + U * (n2.abs() + C2)
    d_d1 = 2 * (mu1.abs() * d_mu1 + mu2.abs() * d_mu2) + 2 * U * d1
    d_d2 = d_s1 + d_s2 + 2 * U * d2
    m = (n1 * n2) / (d1 * d2)
    bound = (d_n1 * n2.abs() + n1.abs() * d_n2) / (d1 * d2) + m.abs() * (d_d1 / d1 + d_d2 / d2) + 3 * U * m.abs()
    return m, bound


def tile_sums(x: torch.Tensor) -> torch.Tensor:
    """Sums of x [N,C,H,W] over the kernel's 32x32 tiles (the last row and column of tiles ragged), flat in the
    workspace's order ((plane * by + ty) * bx + tx)."""
    n, c, h, w = x.shape
    by, bx = -(-h // TILE), -(-w // TILE)
    x = F.pad(x, (0, bx * TILE - w, 0, by * TILE - h))
    return x.reshape(n * c, by, TILE, bx, TILE).sum((2, 4)).reshape(-1)


def tile_pixels(shape) -> torch.Tensor:
    """In-image pixels of every tile, in tile_sums' order."""
    return tile_sums(torch.ones(shape, dtype=torch.float64))


def ssim_tile_ref(m: torch.Tensor, b: torch.Tensor, c_tile: float = C_TILE):
    """(reference, bound) of the SSIM tile partials: the per-pixel bounds add in quadrature (they are independent rounding
    errors), and sqrt(13) u sum |m| is the statistical form of the depth-13 summation of the tile."""
    return tile_sums(m), c_tile * (torch.sqrt(tile_sums(b * b)) + math.sqrt(SUM_DEPTH) * U * tile_sums(m.abs()))


def se_tile_ref(img1: torch.Tensor, img2: torch.Tensor):
    """(reference, bound) of the squared-error tile partials: 15 u sum d^2, d = a - b in float64."""
    d = img1.double() - img2.double()
    ref = tile_sums(d * d)
    return ref, SE_TILE_U * U * ref


def image_means(partials: torch.Tensor, shape):
    """[N, 2] float64 {mse, mean ssim} the reduce kernel must round to fp32: the fp64 sum of image n's tile partials
    {ssim, se} times 1 / (C H W)."""
    n, c, h, w = shape
    s = partials.double().reshape(n, -1, 2).sum(1) * (1.0 / (float(c) * h * w))
    return torch.stack([s[:, 1], s[:, 0]], 1)


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """One fp32 ulp at |x| (float64 in, float64 out)."""
    x32 = x.abs().float()
    return (torch.nextafter(x32, torch.full_like(x32, math.inf)).double() - x32.double())


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound and its flat index: 0 where the error is 0, inf where only the bound is, inf for a NaN."""
    err = (torch.as_tensor(got).double().cpu() - ref.double()).abs()
    ratio = torch.nan_to_num(torch.where(err == 0, torch.zeros_like(err), err / bound.double()), nan=math.inf)
    if not ratio.numel():
        return 0.0, -1
    return float(ratio.max()), int(ratio.argmax())


# ---- the shape matrix ---------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "h w ws c n content")
# (H, W) x window x channels x images x content, not the full product: every size at each window class, a window wider
# than the image ((1,1), (1,40), (5,7) with 7 and more taps), a single tile ((32,32) and below), a ragged last tile on each
# axis ((33,32), (31,33), (65,31), (37,53)), a 3x3 tile interior ((96,130): 3 x 5 tiles), every window, every channel count.
CASES = [Case(*c) for c in (
    (1, 1, 1, 1, 1, "noise"), (1, 1, 11, 3, 1, "wide"), (1, 1, 31, 1, 3, "noise"),
    (1, 40, 3, 1, 1, "noise"), (1, 40, 27, 3, 1, "smooth"), (1, 40, 11, 4, 3, "white"),
    (5, 7, 1, 3, 1, "wide"), (5, 7, 7, 4, 1, "noise"), (5, 7, 11, 1, 3, "smooth"), (5, 7, 31, 3, 1, "white"),
    (31, 33, 3, 4, 1, "noise"), (31, 33, 11, 3, 1, "smooth"), (31, 33, 27, 1, 1, "wide"), (31, 33, 7, 3, 3, "white"),
    (32, 32, 1, 1, 1, "white"), (32, 32, 7, 3, 3, "noise"), (32, 32, 11, 4, 1, "smooth"), (32, 32, 31, 1, 1, "wide"),
    (32, 32, 29, 3, 1, "noise"),
    (33, 32, 3, 3, 1, "white"), (33, 32, 11, 1, 1, "noise"), (33, 32, 27, 4, 1, "smooth"), (33, 32, 31, 1, 3, "wide"),
    (65, 31, 1, 4, 1, "noise"), (65, 31, 7, 1, 3, "white"), (65, 31, 11, 3, 1, "wide"), (65, 31, 31, 3, 1, "smooth"),
    (37, 53, 3, 1, 1, "smooth"), (37, 53, 7, 3, 1, "wide"), (37, 53, 11, 3, 3, "white"), (37, 53, 27, 3, 1, "noise"),
    (37, 53, 31, 4, 1, "noise"),
    (96, 130, 1, 3, 1, "smooth"), (96, 130, 3, 3, 1, "wide"), (96, 130, 7, 4, 1, "white"), (96, 130, 11, 3, 3, "noise"),
    (96, 130, 27, 1, 1, "noise"), (96, 130, 29, 1, 1, "white"), (96, 130, 31, 3, 1, "white"), (96, 130, 31, 1, 1, "noise"),
)]
# more than 256 tiles per image: the reduce kernel's loop takes a second stride (2 x 4 planes of 9 x 9 tiles = 324 per image)
REDUCE_CASE = Case(260, 270, 3, 4, 2, "smooth")


def case_id(c: Case) -> str:
    return f"{c.h}x{c.w}-w{c.ws}-c{c.c}-n{c.n}-{c.content}"


def case_images(c: Case, seed: int):
    """The two fp32 CPU batches [n, c, h, w] of a case; every plane holds different content.
      noise   uniform noise, independent in the two images
      smooth  5x5-averaged noise and that plus 0.03 gaussian noise, clamped (test_gpu_metrics.py's full frame)
      white   `smooth` under a white background: both images exactly 1.0 on the left third, only the first on the next sixth
      wide    uniform in [-0.5, 1.5]"""
    gen = torch.Generator().manual_seed(1000 + seed)
    shape = (c.n, c.c, c.h, c.w)
    if c.content == "noise":
        return torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)
    if c.content == "wide":
        return torch.rand(shape, generator=gen) * 2 - 0.5, torch.rand(shape, generator=gen) * 2 - 0.5
    a = F.avg_pool2d(torch.rand(shape, generator=gen), 5, stride=1, padding=2)
    b = (a + 0.03 * torch.randn(shape, generator=gen)).clamp(0, 1)
    if c.content == "white":
        x0, x1 = -(-c.w // 3), -(-c.w // 2)
        a, b = a.clone(), b.clone()
        a[..., :x1] = 1.0
        b[..., :x0] = 1.0
    else:
        assert c.content == "smooth", c.content
    return a.contiguous(), b.contiguous()


@lru_cache(maxsize=None)
def case_data(c: Case):
    """(img1, img2, g, m, b) of a case, computed once and shared by the tests: leave them unchanged."""
    seed = (CASES.index(c) if c in CASES else len(CASES))
    a, b = case_images(c, seed)
    g = gaussian(c.ws)
    m, bound = ssim_map64(a, b, g)
    return a, b, g, m, bound


# ---- fp32 restatement of the kernel's order (CPU test only) -------------------------------------------------------------
def _pass32(x, g, axis, lo, hi, mode, drop_last_at_31=False):
    """One separable pass in fp32, taps added first to last, multiply and add un-fused: out[i] = sum_t g[t] x[i + t - lo]
    with `lo` / `hi` pixels of padding in front / behind."""
    pad = (lo, hi, 0, 0) if axis == 3 else (0, 0, lo, hi)
    if mode == "replicate" and (lo or hi):
        for _ in range(max(lo, hi)):                       # one pixel at a time: any width, unlike F.pad's replicate
            step = tuple(min(1, p) for p in pad)
            x = F.pad(x, step, mode="replicate")
            pad = tuple(p - s for p, s in zip(pad, step))
    else:
        x = F.pad(x, pad)
    n = x.shape[axis] - (lo + hi)
    s = torch.zeros_like(x.narrow(axis, 0, n))
    before_last = s
    for t in range(g.numel()):
        before_last = s
        s = s + g[t] * x.narrow(axis, t, n)
    if drop_last_at_31:
        col = torch.arange(n) % TILE == TILE - 1
        s = torch.where(col, before_last, s)
    return s


def ssim_map32(img1, img2, g, pad_mode="zeros", shift=0, drop_tap=False, extend=False):
    """The SSIM map as image_metrics_kernel computes it, in torch fp32: horizontal then vertical pass over the five planes
    a, b, a a, b b, a b, then the map's expression in the kernel's order.  Options are the mistakes of the CPU teeth test:
    pad_mode 'replicate'; shift = 1 reads one tap to the right in the horizontal pass; drop_tap loses the last horizontal
    tap at column 31 of every tile; extend computes the map on the image zero-extended to whole tiles (what a ragged tile
    holds when the in-image test of the third stage is missing)."""
    a, b = img1, img2
    if extend:
        h, w = a.shape[-2:]
        ext = (0, -(-w // TILE) * TILE - w, 0, -(-h // TILE) * TILE - h)
        a, b = F.pad(a, ext), F.pad(b, ext)
    r = g.numel() // 2
    planes = [a, b, a * a, b * b, a * b]
    out = []
    for p in planes:
        hrow = _pass32(p, g, 3, r - shift, r + shift, pad_mode, drop_tap)
        out.append(_pass32(hrow, g, 2, r, r, pad_mode))
    mu1, mu2, e11, e22, e12 = out
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu1_mu2
    c1, c2 = torch.tensor(0.01, dtype=torch.float32) ** 2, torch.tensor(0.03, dtype=torch.float32) ** 2
    return ((2.0 * mu1_mu2 + c1) * (2.0 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))


def tile_partials32(x: torch.Tensor) -> torch.Tensor:
    """fp32 sums of x [N,C,H,W] (fp32) per tile in the kernel's order: thread t adds pixels t, t + 256, t + 512, t + 768
    of the tile (row-major), a 64-lane xor butterfly from offset 32 down to 1, then the four waves first to last."""
    n, c, h, w = x.shape
    by, bx = -(-h // TILE), -(-w // TILE)
    x = F.pad(x, (0, bx * TILE - w, 0, by * TILE - h))
    t = x.reshape(n * c, by, TILE, bx, TILE).permute(0, 1, 3, 2, 4).reshape(-1, 4, 256)
    s = ((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]
    s = s.reshape(-1, 4, 64)
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lane ^ off]
    s = s[:, :, 0]
    return ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]


# ---- the loss -------------------------------------------------------------------------------------------------------------
Loss64 = namedtuple("Loss64", "seeds blocks out")


def loss64(rgb_c, acc_c, rgb_f, acc_f, target, use_alpha: bool, use_fine: bool, n_for_weight=None) -> Loss64:
    """nerf/train_nerf.py:158-167 in float64 from the fp32 inputs (target [n,4] = r, g, b, alpha):
      seeds   d loss / d (rgb_c [n,3], acc_c [n], rgb_f [n,3], acc_f [n])
      blocks  [ceil(n / 256), 4] sums of {se_rgb_c, se_acc_c, se_rgb_f, se_acc_f} over each block of 256 rays
      out     {loss, mean((rgb_f - rgb)^2), loss_coarse, loss_fine}; the coarse terms are reported whatever use_fine is
    n_for_weight: the n of the seeds' 2 / (3 n) and 0.2 / n (the teeth test passes n + 1)."""
    for t in (rgb_c, acc_c, rgb_f, acc_f, target):
        assert t.dtype == torch.float32
    n = rgb_f.shape[0]
    nw = float(n if n_for_weight is None else n_for_weight)
    rgb, alpha = target[:, :3].double(), target[:, 3].double()
    dc, df = rgb_c.double() - rgb, rgb_f.double() - rgb
    dac, daf = acc_c.double() - alpha, acc_f.double() - alpha
    w_rgb, w_acc = 2.0 / (3.0 * nw), (0.1 * 2.0 / nw if use_alpha else 0.0)
    wc = 1.0 if use_fine else 0.0
    seeds = (wc * w_rgb * dc, wc * w_acc * dac, w_rgb * df, w_acc * daf)
    se = torch.stack([(dc * dc).sum(1), dac * dac, (df * df).sum(1), daf * daf], 1)
    nb = -(-n // 256)
    blocks = F.pad(se, (0, 0, 0, nb * 256 - n)).reshape(nb, 256, 4).sum(1)
    tot = se.sum(0)
    mc, mf = tot[0] / (3.0 * n), tot[2] / (3.0 * n)
    lc = mc + (0.1 * tot[1] / n if use_alpha else 0.0)
    lf = mf + (0.1 * tot[3] / n if use_alpha else 0.0)
    out = torch.stack([lf + (lc if use_fine else torch.zeros_like(lc)), mf, lc, lf])
    return Loss64(seeds, blocks, out)


def loss_inputs(n: int):
    """The five fp32 CPU inputs of a loss case (uniform, seeded by n, as test_gpu_trainloop.py's)."""
    gen = torch.Generator().manual_seed(n)
    rgb_c, acc_c, rgb_f, acc_f = (torch.rand(s, generator=gen) for s in ((n, 3), (n,), (n, 3), (n,)))
    return rgb_c, acc_c, rgb_f, acc_f, torch.rand((n, 4), generator=gen)

"""GPU: the kernels of csrc/eval_stages.hip per tile, per block and per element against float64 (tests/eval_gates.py),
through the C ABI with a test-owned workspace so that what the first kernel of each pair leaves behind can be read back.

  image_metrics   every SSIM tile partial within the calibrated tile gate, every squared-error tile partial within
                  15 u sum d^2, the reduce within one fp32 ulp of the fp64 sum of its own inputs; identical images exact;
                  every window the header promises (29 and 31 need more than the default 64 KiB of LDS)
  nerf_loss       every gradient seed within 8 u relative, the seeds that must be zero exactly zero, every block sum within
                  14 u, all four outputs within 16 u; 70 001 rays give the reduce a second stride
  ray_bank        bit-exact against the oracle over several workgroups and a ragged last one

Every case leaves one parity record with the worst achieved ratio (committed extract: profiles/eval_gates_parity.json)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_gates as E  # noqa: E402
from oracle import parity, synth, train_ref as T  # noqa: E402

STAGE = "eval gate"


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def mi():
    from mirender import _lib, train
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    _lib.load()
    return type("MI", (), {"lib": _lib, "train": train})


def image_metrics(mi, a, b, g):
    """mi_image_metrics on two CPU fp32 batches: (tile partials [tiles, 2] = {ssim sum, squared-error sum}, out [N, 2] =
    {mse, mean ssim}), both back on the CPU.  Workspace and output start as NaN: every entry must be written."""
    lib = mi.lib.load()
    n, c, h, w = a.shape
    ad, bd = a.to(dev()).contiguous(), b.to(dev()).contiguous()
    floats = lib.mi_image_metrics_workspace_floats(n, c, h, w)
    assert floats == 2 * n * c * (-(-h // E.TILE)) * (-(-w // E.TILE))
    ws = torch.full((floats,), float("nan"), dtype=torch.float32, device=dev())
    out = torch.full((n, 2), float("nan"), dtype=torch.float32, device=dev())
    g = g.contiguous()
    assert g.device.type == "cpu" and g.dtype == torch.float32
    with torch.cuda.device(dev()):
        rc = lib.mi_image_metrics(mi.lib.ptr(ad), mi.lib.ptr(bd), n, c, h, w, ctypes.c_void_p(g.data_ptr()), g.numel(),
                                  mi.lib.ptr(ws), mi.lib.ptr(out), mi.lib.stream_ptr(dev()))
    assert rc == 0, (rc, lib.mi_last_error())
    return ws.cpu().reshape(-1, 2), out.cpu()


def check_metrics_case(mi, c):
    a, b, g, m, bound = E.case_data(c)
    partials, out = image_metrics(mi, a, b, g)
    ref, gate = E.ssim_tile_ref(m, bound)
    ssim_ratio, ssim_at = E.worst_ratio(partials[:, 0], ref, gate)
    se_ref, se_gate = E.se_tile_ref(a, b)
    se_ratio, se_at = E.worst_ratio(partials[:, 1], se_ref, se_gate)
    want = E.image_means(partials, a.shape)
    reduce_ratio, _ = E.worst_ratio(out, want, E.ulp32(want))
    print(f"{E.case_id(c)}: ssim tile {ssim_ratio:.4f} of the gate ({ssim_ratio * E.C_TILE:.4f} at c = 1, tile {ssim_at}), "
          f"squared-error tile {se_ratio:.4f} (tile {se_at}), reduce {reduce_ratio:.3f} ulp")
    ok = ssim_ratio <= 1.0 and se_ratio <= 1.0 and reduce_ratio <= 1.0
    parity.record(case=f"image_metrics {E.case_id(c)}", stage=STAGE, qty="tile partials {ssim, se}, out",
                  err_over_bound=ssim_ratio, ssim_ratio_at_c1=ssim_ratio * E.C_TILE, se_err_over_bound=se_ratio,
                  reduce_err_ulp=reduce_ratio, tiles=int(partials.shape[0]), worst_index=ssim_at,
                  active=f"{E.C_TILE:g} (sqrt(sum b^2) + sqrt(13) u sum|m|); 15 u sum d^2; 1 ulp", passed=bool(ok))
    assert ssim_ratio <= 1.0, (E.case_id(c), "ssim tile", ssim_ratio, ssim_at)
    assert se_ratio <= 1.0, (E.case_id(c), "squared-error tile", se_ratio, se_at)
    assert reduce_ratio <= 1.0, (E.case_id(c), "reduce", out, want)


@pytest.mark.parametrize("c", E.CASES, ids=[E.case_id(c) for c in E.CASES])
def test_image_metrics_tiles(mi, c):
    check_metrics_case(mi, c)


def test_image_metrics_reduce_second_stride(mi):
    """324 tiles per image: image_metrics_reduce_kernel's loop over the partials takes a second step of 256."""
    c = E.REDUCE_CASE
    assert c.c * (-(-c.h // E.TILE)) * (-(-c.w // E.TILE)) > 256
    check_metrics_case(mi, c)


@pytest.mark.parametrize("shape,ws", [((1, 3, 37, 53), 11), ((2, 1, 96, 130), 11), ((1, 3, 37, 53), 31), ((1, 1, 96, 130), 7)])
def test_identical_images_are_exact(mi, shape, ws):
    """With contraction off N1 == D1 and N2 == D2 bit for bit when the two images are identical, all-zero images included:
    every SSIM tile partial is the number of in-image pixels of its tile, every squared-error partial is +0."""
    img = torch.rand(shape, generator=torch.Generator().manual_seed(ws))
    pixels = E.tile_pixels(shape)
    for a in (img, torch.zeros(shape)):
        partials, out = image_metrics(mi, a, a.clone(), E.gaussian(ws))
        assert torch.equal(partials[:, 0].double(), pixels)
        assert not partials[:, 1].any() and not torch.signbit(partials[:, 1]).any()
        assert torch.equal(out, torch.tensor([[0.0, 1.0]]).expand(shape[0], 2))
    parity.record(case=f"image_metrics identical {shape} w{ws}", stage=STAGE, qty="tile partials", err_over_bound=0.0,
                  active="bit-exact", passed=True)


# ---- the loss ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_alpha,use_fine", [(False, True), (True, True), (True, False), (False, False)])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099, 70001])
def test_nerf_loss_seeds_blocks_and_outputs(mi, n, use_alpha, use_fine):
    lib = mi.lib.load()
    ins = E.loss_inputs(n)
    ref = E.loss64(*ins, use_alpha, use_fine)
    d = [t.to(dev()).contiguous() for t in ins]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev())  # noqa: E731
    seeds = [nan(n, 3), nan(n), nan(n, 3), nan(n)]
    blocks = -(-n // 256)
    assert lib.mi_nerf_loss_workspace_floats(n) == 4 * blocks
    ws, out = nan(4 * blocks), nan(4)
    with torch.cuda.device(dev()):
        rc = lib.mi_nerf_loss(n, *[mi.lib.ptr(t) for t in d], int(use_alpha), int(use_fine), *[mi.lib.ptr(s) for s in seeds],
                              mi.lib.ptr(ws), mi.lib.ptr(out), mi.lib.stream_ptr(dev()))
    assert rc == 0, (rc, lib.mi_last_error())
    names = ("g_rgb_c", "g_acc_c", "g_rgb_f", "g_acc_f")
    zero = {"g_rgb_c": not use_fine, "g_acc_c": not use_fine or not use_alpha, "g_rgb_f": False, "g_acc_f": not use_alpha}
    seed_ratio = 0.0
    for name, got, want in zip(names, seeds, ref.seeds):
        got = got.cpu()
        if zero[name]:
            assert not got.any(), name
            assert not want.any(), name
        ratio, at = E.worst_ratio(got, want, E.SEED_U * E.U * want.abs())
        seed_ratio = max(seed_ratio, ratio)
        assert ratio <= 1.0, (name, ratio, at)
    block_ratio, block_at = E.worst_ratio(ws.cpu().reshape(blocks, 4), ref.blocks, E.BLOCK_U * E.U * ref.blocks)
    out_ratio, out_at = E.worst_ratio(out.cpu(), ref.out, E.OUT_U * E.U * ref.out.abs())
    print(f"nerf_loss n={n} use_alpha={use_alpha} use_fine={use_fine}: seeds {seed_ratio:.3f} of 8 u, blocks {block_ratio:.3f} "
          f"of 14 u, out {out_ratio:.3f} of 16 u")
    ok = seed_ratio <= 1.0 and block_ratio <= 1.0 and out_ratio <= 1.0
    parity.record(case=f"nerf_loss n={n} use_alpha={use_alpha} use_fine={use_fine}", stage=STAGE,
                  qty="seeds, block sums, out[0..3]", err_over_bound=seed_ratio, block_err_over_bound=block_ratio,
                  out_err_over_bound=out_ratio, blocks=blocks, active="8 u |seed|; 14 u block sum; 16 u |out|", passed=bool(ok))
    assert block_ratio <= 1.0, ("block sums", block_ratio, block_at)
    assert out_ratio <= 1.0, ("out", out_ratio, out_at, out.cpu(), ref.out)


# ---- the ray bank ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("images,width,height", [(3, 37, 19), (1, 100, 100)])
@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("focal_type", [float, np.float64])
def test_ray_bank_bit_exact_across_workgroups(mi, images, width, height, white, focal_type):
    """Several workgroups of 256 rows and a ragged last one (2 109 rows = 8 + 61 / 256, 10 000 = 39 + 16 / 256), both
    backgrounds, both focal types (np.float64 makes get_rays, and so the kernel, compute in fp64)."""
    assert (images * width * height) % 256 and images * width * height > 2 * 256
    focal = focal_type(0.5 * width / np.tan(0.5 * 0.6911112))
    poses = np.stack([synth.pose_degrees(4.0, th, -30.0) for th in (37.0, -120.0, 5.0)[:images]]).astype(np.float32)
    imgs = np.random.Generator(np.random.PCG64(7 + images)).random((images, height, width, 4), dtype=np.float32)
    bank = mi.train.RayBank(imgs, poses, focal, dev(), white_bkgd=white)
    want = T.rays_rgba(imgs, poses, width, height, focal, white_bkgd=white)
    got = bank.table.cpu().numpy()
    parity.record(case=f"ray_bank {images}x{height}x{width} white={white} focal={focal_type.__name__}", stage=STAGE,
                  qty="rays_rgba", err_over_bound=float(np.abs(got.astype(np.float64) - want).max()), active="bit-exact",
                  passed=bool(np.array_equal(got, want)))
    assert np.array_equal(got, want)

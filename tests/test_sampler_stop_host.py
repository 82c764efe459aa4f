"""CPU: a coarse weight below 2^-41 is invisible to sample_pdf, so the windowed coarse pass may stop a ray once the
transmittance in front of a window boundary is <= 2^-42 (kStopBelowPdfEps, csrc/launchers.h) whenever sample_fine is the
weights' only reader.

sample_pdf uses a weight only as w + 1e-5f (float32, un-fused).  1e-5f lies in [2^-17, 2^-16): its ulp is 2^-40 and the
rounding boundary above it is half of that, 2^-41: every w strictly below it leaves the sum at 1e-5f, whichever way a
tie would go.  The stop at 2^-42 keeps a factor 2 under that for the error of the device's fp64 product scans.

Part 1 checks the float32 identity where it could break; part 2 checks that the oracle's sample_pdf returns the same
bits whatever stands behind a stop index, as long as it is below 2^-41."""
import numpy as np
import pytest
import torch

from oracle import render_ref as R

EPS = np.float32(1e-5)
HALF_ULP = np.float32(2.0 ** -41)
STOP = np.float32(2.0 ** -42)


def _around(x, count):
    """The `count` float32 bit patterns on either side of x (x included)."""
    b = int(np.float32(x).view(np.uint32))
    return np.arange(b - count, b + count + 1, dtype=np.uint32).view(np.float32)


def _vanishes(w):
    w = np.asarray(w, dtype=np.float32)
    s = w + EPS
    assert s.dtype == np.float32
    return s == EPS


def test_epsilon_is_where_the_argument_puts_it():
    assert np.float32(2.0 ** -17) <= EPS < np.float32(2.0 ** -16)
    assert np.spacing(EPS) == np.float32(2.0 ** -40)
    assert not _vanishes(np.nextafter(HALF_ULP, np.float32(1)))      # above half an ulp the sum moves: the bound is tight


def test_weights_around_the_stop_vanish():
    w = _around(STOP, 4096)
    assert w.min() < STOP < w.max()
    assert _vanishes(w).all()


def test_weights_just_below_half_an_ulp_vanish():
    b = int(HALF_ULP.view(np.uint32))
    w = np.arange(b - 4096, b, dtype=np.uint32).view(np.float32)
    assert w.max() == np.nextafter(HALF_ULP, np.float32(0)) and (w < HALF_ULP).all()
    assert _vanishes(w).all()


def test_zero_and_subnormals_vanish():
    tiny = np.finfo(np.float32).tiny
    sub = np.concatenate([np.arange(0, 4097, dtype=np.uint32),                       # 0 and the smallest subnormals
                          np.arange(0x007FF000, 0x00801000, dtype=np.uint32),        # the largest, and the first normals
                          np.linspace(0, 0x007FFFFF, 4096).astype(np.uint32)]).view(np.float32)
    assert sub[0] == 0 and (sub[1:4097] < tiny).all() and sub.max() > tiny
    assert _vanishes(sub).all()


def test_a_random_draw_below_half_an_ulp_vanishes():
    rng = np.random.default_rng(0)
    bits = rng.integers(0, int(HALF_ULP.view(np.uint32)), size=1 << 20, dtype=np.uint32)    # uniform over the bit patterns
    lin = (rng.random(1 << 20) * float(HALF_ULP)).astype(np.float32)                        # uniform over the values
    lin = lin[lin < HALF_ULP]
    assert _vanishes(bits.view(np.float32)).all() and _vanishes(lin).all()


def _rows(nc, rng, n=64):
    """Weight rows [n, nc] as a coarse pass leaves them (alpha * transmittance of random sigma: a head of ordinary
    weights, a falling tail) and the mids [n, nc - 1] of jittered ascending depths."""
    z = np.sort(2.0 + 4.0 * (np.arange(nc)[None, :] + rng.random((n, nc))) / nc, -1).astype(np.float32)
    alpha = (rng.random((n, nc)) ** 2).astype(np.float32)
    trans = np.cumprod(np.concatenate([np.ones((n, 1), np.float32), 1 - alpha], -1), -1)[:, :-1].astype(np.float32)
    return torch.from_numpy(alpha * trans), torch.from_numpy(0.5 * (z[:, 1:] + z[:, :-1]))


@pytest.mark.parametrize("nf", [128, 3])
@pytest.mark.parametrize("nc", [64, 9])
def test_sample_pdf_ignores_the_tail_behind_a_stop(nc, nf):
    rng = np.random.default_rng(nc * 1000 + nf)
    w, mids = _rows(nc, rng)
    below = np.nextafter(HALF_ULP, np.float32(0))
    checked = 0
    for stop in sorted({1, 2, 4, 8, 16, 24, 40, 56, nc - 2, nc - 1} & set(range(1, nc))):
        tails = {
            "zero": torch.zeros(w.shape[0], nc - stop),
            "largest below 2^-41": torch.full((w.shape[0], nc - stop), float(below)),     # every later alpha = 1
            "random below 2^-41": torch.from_numpy((rng.random((w.shape[0], nc - stop)) * float(below)).astype(np.float32)),
        }
        got = {}
        for name, tail in tails.items():
            assert float(tail.max()) < float(HALF_ULP)
            row = torch.cat([w[:, :stop], tail], -1)
            got[name] = R.sample_pdf(mids, row[:, 1:-1], nf)
            assert got[name].dtype == torch.float32 and got[name].shape == (w.shape[0], nf)
        for name in ("largest below 2^-41", "random below 2^-41"):
            assert torch.equal(got[name], got["zero"]), (stop, name)
        checked += 1
    assert checked >= 4
    # the comparison can fail: a tail of ordinary size moves the samples
    stop = nc // 2
    big = torch.cat([w[:, :stop], torch.from_numpy((rng.random((w.shape[0], nc - stop)) * 1e-3).astype(np.float32))], -1)
    zero = torch.cat([w[:, :stop], torch.zeros(w.shape[0], nc - stop)], -1)
    assert not torch.equal(R.sample_pdf(mids, big[:, 1:-1], nf), R.sample_pdf(mids, zero[:, 1:-1], nf))

"""CPU: tests/sampler_ref.py, the restatement tests/test_gpu_sampler_bits.py holds the inverse-CDF samplers to, checked itself.

    a  it means what the reference means: against oracle.render_ref.sample_pdf every unmasked sample is within
       parity.pdf_conditioning's tolerance; the share of samples that differ at all is printed
    b  the arithmetic render_stages.hip argues in comments: under cdf_like_cumsum's criterion every sum the shuffle scan forms
       fits a double's 53 bits (shown with Python integers), so the scan's order and the sequential order give one cdf; that
       still holds one exponent beyond the criterion (no row can tell the two orders apart there), and two beyond a row does
    c  the CDF-space gate holds for the oracle and for the restatement on every family, no sample left out
    d  planted mistakes: each changes the restatement's bits on a committed case of the GPU test, named here
    e  every weight family takes the kernel path it is meant to take; the sorted-lists merge equals the key ranking wherever
       the kernel takes it
    f  refusals that need no launch: Nc < 3, fewer than 2 bins, and the smallest sizes past the launchers' own LDS formulas
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import sampler_ref as S
from mirender import _lib as binding
from oracle import parity, render_ref as R

F = np.float32
M32 = 0xFFFFFFFF


# ---- a / c: the families of the gate ---------------------------------------------------------------------------------------------
def _lin_mids(nc):
    lin = torch.linspace(2.0, 6.0, nc).numpy()
    return S.mids(lin)


def gate_family(name):
    """(bins [n,nb], weights [n,nb-1], nf) of six families on the render path's own shapes: 64 coarse depths on linspace mids,
    free bins, sparse weights."""
    rng = np.random.Generator(np.random.PCG64(sum(map(ord, name))))
    n = 48
    if name in ("random6 on linspace mids", "single spike", "all zero", "1e-7-scaled"):
        bins = np.tile(_lin_mids(64), (n, 1))
        w = S.power6(rng.random((n, 62)))
        if name == "single spike":
            w[:] = 0
            w[np.arange(n), rng.integers(0, 62, n)] = 1.0
        elif name == "all zero":
            w[:] = 0
        elif name == "1e-7-scaled":
            w = (w * F(1e-7)).astype(F)
        return bins, w, 128
    if name == "64 random sorted bins":
        return np.sort((2.0 + 4.0 * rng.random((n, 64))).astype(F), 1), S.power6(rng.random((n, 63))), 64
    assert name == "128 bins, 10 % dense"
    w = rng.random((n, 127)).astype(F)
    w[rng.random((n, 127)) > 0.1] = 0
    return np.tile(_lin_mids(129), (n, 1)), w, 128


GATE_FAMILIES = ("random6 on linspace mids", "single spike", "all zero", "1e-7-scaled", "64 random sorted bins",
                 "128 bins, 10 % dense")
FINITE = tuple(f for f in S.FAMILIES + ("uniform",) if f not in ("inf_row", "nan_row"))


def _family_inputs(name):
    if name in GATE_FAMILIES:
        return gate_family(name)
    return np.tile(_lin_mids(66), (5, 1)), S.family(name, 5, 64), 65


def _oracle(bins, w, nf):
    return R.sample_pdf(torch.from_numpy(np.ascontiguousarray(bins)), torch.from_numpy(np.ascontiguousarray(w)), nf).numpy()


@pytest.mark.parametrize("name", GATE_FAMILIES + FINITE)
def test_restatement_means_what_the_oracle_means(name):
    bins, w, nf = _family_inputs(name)
    u = torch.linspace(0.0, 1.0, nf).numpy()                                  # the table mirender.ops injects
    got = S.sample_pdf(bins, w, nf, u)[0]
    want = _oracle(bins, w, nf)
    mask, tol = parity.pdf_conditioning(torch.from_numpy(np.ascontiguousarray(bins)), torch.from_numpy(w), nf)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    differ = float((S.bits(got) != S.bits(want)).mean())
    print(f"{name}: {100 * differ:.2f} % of the samples differ by at least a bit, {100 * mask.mean():.2f} % are masked, "
          f"largest unmasked error {float((d / tol)[~mask].max(initial=0.0)):.3g} tolerances")
    assert not ((d > tol) & ~mask).any(), (name, float((d / tol)[~mask].max()))
    # and the gate, which has no mask: the oracle and the restatement, every sample
    e_orc = float(S.cdf_space_error(bins, w, want, u).max())
    e_ref = float(S.cdf_space_error(bins, w, got, u).max())
    print(f"{name}: CDF-space error of the oracle {e_orc:.3g}, of the restatement {e_ref:.3g}")
    assert e_orc <= 1.0 and e_ref <= max(1.0, parity.FP64_FACTOR * e_orc), (name, e_orc, e_ref)


def _gate_rows(c, bins):
    w = c["weights"][:, 1:-1]
    return np.isfinite(w).all(1) & (np.diff(bins, axis=1) > 0).all(1)


def test_gate_holds_on_every_case_of_the_gpu_test():
    """The restatement's own samples and the oracle's, on every ray of every case with finite weights and ascending bins."""
    worst = {}
    for name in sorted(S.CASES):
        c = S.case_inputs(name)
        if c["nf"] == 0:
            continue
        bins = np.ascontiguousarray(S.case_bins(c))
        rows = _gate_rows(c, bins)
        if not rows.any():
            continue
        w = c["weights"][:, 1:-1]
        u = S.u_table(c["nf"]) if c["u"] is None else c["u"]
        e_ref = float(S.cdf_space_error(bins[rows], w[rows], S.reference(c)[0][rows], u).max())
        e_orc = float(S.cdf_space_error(bins[rows], w[rows], _oracle(bins[rows], w[rows], c["nf"]),
                                        torch.linspace(0.0, 1.0, c["nf"]).numpy()).max())
        assert e_orc <= 1.0 and e_ref <= max(1.0, parity.FP64_FACTOR * e_orc), (name, e_orc, e_ref)
        worst[c["family"]] = max(worst.get(c["family"], (0.0, 0.0)), (e_ref, e_orc))
    for fam, (e_ref, e_orc) in sorted(worst.items()):
        print(f"{fam}: largest CDF-space error of the restatement {e_ref:.3g} (the oracle's on that case {e_orc:.3g})")
    assert set(worst) >= set(FINITE)


# ---- b: the exactness criterion --------------------------------------------------------------------------------------------------
def _f32(field, mant, neg=False):
    return np.array([(int(neg) << 31) | (field << 23) | mant], np.uint32).view(F)[0]


def _int_terms(pdf):
    """The fp32 terms as Python integers in units of 2^(gmin - 150), gmin the least exponent field of a non-zero term (a
    denormal's being 1): a term is mantissa * 2^(max(field, 1) - 150)."""
    words = np.asarray(pdf, F).view(np.uint32).tolist()
    fields = [max((x >> 23) & 0xFF, 1) for x in words if (x << 1) & M32]
    gmin = min(fields) if fields else 1
    out = []
    for x in words:
        f, m = (x >> 23) & 0xFF, x & 0x7FFFFF
        assert f < 255
        v = (m | (1 << 23 if f else 0)) << (max(f, 1) - gmin) if (x << 1) & M32 else 0
        out.append(-v if x >> 31 else v)
    return out, gmin


def _scan_ints(terms, nb):
    """cdf_like_cumsum's shuffle scan over integers: (the exclusive prefixes [nb], the largest |value| any lane ever holds)."""
    nw = nb - 1
    peak, carry, out = 0, 0, [0] * nb
    for base in range(0, nb, 64):
        own = [terms[base + k] if base + k < nw else 0 for k in range(64)]
        incl = list(own)
        o = 1
        while o < 64:
            incl = [incl[k] + incl[k - o] if k >= o else incl[k] for k in range(64)]
            peak = max(peak, max(abs(v) for v in incl))
            o <<= 1
        for k in range(64):
            peak = max(peak, abs(incl[k] - own[k]), abs(carry + (incl[k] - own[k])))
            if base + k < nb:
                out[base + k] = carry + (incl[k] - own[k])
        carry += incl[63]
        peak = max(peak, abs(carry))
    return out, peak


def _worst_row(nb, span, low_field=100):
    """The row of nb - 1 terms that makes every partial sum as long as a row of that span can: the largest mantissa at the top
    field everywhere, and in the middle one term at the bottom field whose last mantissa bit is set."""
    row = np.array([_f32(low_field + span, 0x7FFFFF)] * (nb - 1), F)
    row[(nb - 1) // 2] = _f32(low_field, 1)
    return row


def _random_row(nb, span, rng, low_field=100):
    nw = nb - 1
    f = rng.integers(low_field, low_field + span + 1, nw)
    f[rng.integers(0, nw)], f[rng.integers(0, nw)] = low_field, low_field + span
    row = np.array([_f32(int(a), int(m)) for a, m in zip(f, rng.integers(0, 1 << 23, nw))], F)
    if nw > 4:
        row[rng.integers(0, nw)] = 0.0                                   # a zero term: skipped for fmin
    if not (row.view(np.uint32) >> 23 == low_field).any():
        row[0] = _f32(low_field, 1)
    if not (row.view(np.uint32) >> 23 == low_field + span).any():
        row[-1] = _f32(low_field + span, 5)
    return row


def _check_exact(row, nb):
    """Every sum the scan forms fits 53 bits, so both orders, and the exact sum rounded once, give the same cdf."""
    terms, gmin = _int_terms(row)
    prefix, peak = _scan_ints(terms, nb)
    assert peak < 1 << 53, (nb, peak.bit_length())
    exact = np.array([F(math.ldexp(float(p), gmin - 150)) for p in prefix], F)
    assert prefix == [sum(terms[:j]) for j in range(nb)]
    for other in (S.cdf_sequential(row, nb), S.cdf_scan(row, nb)):
        assert np.array_equal(other.view(np.int32), exact.view(np.int32)), nb
    return peak


@pytest.mark.parametrize("nb", [64, 65, 129, 257])
def test_the_exactness_criterion(nb):
    crit = S.crit_span(nb)
    rng = np.random.Generator(np.random.PCG64(nb))
    for excess in (0, 1):
        rows = [_worst_row(nb, crit + excess)] + [_random_row(nb, crit + excess, rng) for _ in range(10)]
        # a denormal at the bottom counts as field 1: the span is measured from there
        rows.append(_worst_row(nb, crit + excess, low_field=1))
        rows[-1][(nb - 1) // 2] = _f32(0, 1)
        for row in rows:
            path = S.cdf_path(row, nb)
            assert path["fmax"] - path["fmin"] == crit + excess and path["log2n"] == (nb - 1).bit_length(), path
            assert path["exact"] == (excess == 0), path
            _check_exact(row, nb)
    # How far the exactness reaches: the worst row needs span + 24 bits for its longest term and up to log2n more for the sum
    # of nb - 1 < 2^log2n of them, 52 under the criterion and 53 one beyond it - still a double's mantissa.  So ONE BEYOND THE
    # CRITERION NO ROW EXISTS on which the two orders differ (shown above for the worst row, which bounds every other); the
    # first span at which a sum can need 54 bits is two beyond when nb - 1 is just below a power of two, three beyond when
    # it is one.
    first = next(e for e in range(8) if _scan_ints(_int_terms(_worst_row(nb, crit + e))[0], nb)[1] >= 1 << 53)
    assert first == (2 if nb == 64 else 3), (nb, first)


def test_one_term_always_qualifies():
    """nb = 2: one term, fmax == fmin whatever it is; there is no row beyond the criterion."""
    for x in (_f32(1, 0), _f32(0, 1), _f32(254, 0x7FFFFF), F(0.0)):
        assert S.cdf_path(np.array([x], F), 2)["exact"]
        _check_exact(np.array([x], F), 2)
    assert not S.cdf_path(np.array([F("inf")], F), 2)["exact"] and not S.cdf_path(np.array([F("nan")], F), 2)["exact"]


def _tie_row(nb, span, seed):
    """A row whose total sits one unit of the smallest term above a tie of the fp32 rounding: the top-field mantissas sum to
    31 mod 64, and two bottom-field terms add 2^24 + 1 units."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = rng.integers(1 << 23, 1 << 24, nb - 3)
    m[0] += (31 - int(m.sum())) % 64
    if m[0] >= 1 << 24:
        m[0] -= 64
    terms = [_f32(100 + span, int(x) & 0x7FFFFF) for x in m] + [_f32(100, 1), _f32(100, 0)]
    return np.array(terms, F)[rng.permutation(nb - 1)]


def test_two_beyond_the_criterion_the_orders_differ():
    """nb = 64, span 24 = (28 - 6) + 2: sums of 54 bits, rounded differently by the two orders, and one entry of the fp32 cdf
    shows it.  The criterion sends such a row down the sequential order."""
    row = _tie_row(64, S.crit_span(64) + 2, 31)
    path = S.cdf_path(row, 64)
    assert not path["exact"] and path["fmax"] - path["fmin"] == S.crit_span(64) + 2
    assert _scan_ints(_int_terms(row)[0], 64)[1] >= 1 << 53
    a, b = S.cdf_sequential(row, 64), S.cdf_scan(row, 64)
    assert np.flatnonzero(a.view(np.int32) != b.view(np.int32)).tolist() == [44]


# ---- d: planted mistakes ---------------------------------------------------------------------------------------------------------
PLANT_CASES = {
    "searchsorted_left": ("pdf-nc66-nf65-n3-uniform-kernel-stratified", "z_samples"),
    "guard_le": ("fine-nc5-nf8-n17-guard_sweep-guard_u-stratified", "z_samples"),
    "guard_on_pdf": ("pdf-nc66-nf8-n17-guard_sweep-guard_u-stratified", "z_samples"),
    "pdf_sum_sequential": ("fine_pos-nc130-nf126-n5-random6-kernel-unsorted", "z_samples"),
    "cdf_fp32": ("pdf-nc130-nf126-n5-random6-injected-stratified", "z_samples"),
    "lerp_fma": ("fine-nc4-nf251-n5-random6-kernel-stratified", "z_samples"),
    "u_plain": ("fine-nc4-nf251-n5-random6-kernel-stratified", "z_samples"),
    "above_unclamped": ("pdf-nc5-nf3-n4-random6-injected-stratified", "z_samples"),
    "sample_before_equal_coarse": ("fine_pos-nc130-nf126-n5-random6-kernel-unsorted", "pos"),
    "pos_offset": ("fine_pos-nc5-nf3-n4-random6-kernel-unsorted", "pos"),
}


def _changed(a, b):
    out = []
    for x, y, what in zip(a, b, ("z_samples", "z_fine", "pos")):
        if x is not None and not (np.array_equal(x, y) if what == "pos" else np.array_equal(S.bits(x), S.bits(y))):
            out.append(what)
    return out


def test_planted_mistakes_change_the_bits():
    assert set(PLANT_CASES) == set(S.PLANTS)
    for plant, (name, what) in PLANT_CASES.items():
        c = S.case_inputs(name)
        assert what in _changed(S.reference(c), S.reference(c, plant=plant)), (plant, name)
    # the tie of the merge's plant is the one the inputs were given: the sample at u = 0 is the first bin, a coarse depth too
    c = S.case_inputs(PLANT_CASES["sample_before_equal_coarse"][0])
    zs = S.reference(c)[0]
    assert (zs[:, 0] == c["z_coarse"][:, 1]).all()
    # guard <= differs from < only where a cdf step IS 1e-5f: the sweep holds such a row
    c = S.case_inputs(PLANT_CASES["guard_le"][0])
    steps = np.stack([S.sample_row(S.case_bins(c)[r], c["weights"][r, 1:-1], c["u"])[2][1] for r in range(c["n"])])
    assert (steps == S.EPS).any()


# ---- e: the paths ----------------------------------------------------------------------------------------------------------------
def _rows_of(fam, entries=("fine", "fine_pos", "bounds", "pdf")):
    for name in sorted(S.CASES):
        c = S.CASES[name]
        if c["family"] == fam and c["entry"] in entries:
            c = S.case_inputs(name)
            bins = S.case_bins(c)
            for r in range(c["weights"].shape[0]):
                yield name, c, r, S.sample_row(bins[r], c["weights"][r, 1:-1], S.u_table(c["nf"]) if c["u"] is None else c["u"])


def test_every_family_takes_its_path():
    seen = {}
    for fam in S.FAMILIES + ("uniform", "guard_sweep"):
        for name, c, r, (zs, pdf, cdf_, path) in _rows_of(fam):
            nw, span = pdf.size, path["fmax"] - path["fmin"]
            key = None
            if fam in ("random6", "zero", "spike", "two_ended", "tiny", "uniform", "guard_sweep"):
                # (the rows of a few thousand bins, there for their LDS requests, leave the criterion 17 - 28 + log2n short)
                assert path["exact"] or nw > 256, (name, r, path)
            elif fam == "span40" and nw >= 2:
                assert not path["exact"] and span == 40, (name, r, path)
            elif fam in ("crit", "crit_plus1", "crit_plus2") and nw >= 2:
                k = ("crit", "crit_plus1", "crit_plus2").index(fam)
                assert span == S.crit_span(nw + 1) + k and path["exact"] == (k == 0), (name, r, path)
            elif fam == "huge":
                if nw >= 2:                 # 2^127 takes the whole pdf; every other entry is a denormal, counted as field 1
                    sub = pdf[(pdf != 0) & (np.abs(pdf) < F(2.0 ** -126))]
                    assert sub.size == nw - 1 and path["fmin"] == 1 and path["fmax"] == 127 and not path["exact"], (name, r, path)
            elif fam in ("inf_row", "nan_row") and c["weights"].shape[0] > 1:
                assert path["exact"] == (r != 1) and (path["fmax"] == 255) == (r == 1), (name, r, path)
                key = "bad row" if r == 1 else "neighbour"
            if fam == "uniform" and c["entry"] != "bounds":
                # every cdf entry is a u: searchsorted right against left decides those brackets
                assert np.isin(cdf_, c["u"] if c["u"] is not None else S.u_table(c["nf"])).all(), (name, r)
            seen.setdefault(fam, set()).add((key, path["exact"], nw > 64, nw > 128))
    assert ("bad row", False, False, False) in seen["inf_row"] and ("neighbour", True, True, False) in seen["nan_row"]
    # both sides of the guard, within 8 ulp of 1e-5f, in the sweep
    ulp = float(np.spacing(S.EPS))
    for nc in (5, 66):
        c = S.case_inputs(f"pdf-nc{nc}-nf8-n17-guard_sweep-guard_u-stratified")
        steps = np.array([S.sample_row(c["bins"][r], c["weights"][r, 1:-1], c["u"])[2][1] for r in range(c["n"])])
        assert (steps < S.EPS).any() and (steps > S.EPS).any() and float(np.abs(steps - S.EPS).max()) <= 8 * ulp, steps


def test_the_merge_branches():
    """Stratified depths take the sorted-lists branch, the unsorted ones and a NaN row full counting; the sorted-lists branch
    equals the key ranking on every row that takes it, and no sample of those rows is a -0 (the one value it ranks otherwise)."""
    took = {True: 0, False: 0}
    totals = set()
    for name in sorted(S.CASES):
        c = S.case_inputs(name)
        if c["entry"] == "pdf":
            continue
        zs, zf, pos = S.reference(c)
        for r in range(zs.shape[0]):
            fast = S.lists_sorted(c["z_coarse"][r], zs[r])
            took[fast] += 1
            if c["coarse"] == "unsorted" and c["nc"] > 3:
                assert not fast, (name, r)
                totals.add(c["nc"] + c["nf"])
            if fast:
                assert not (np.signbit(zs[r]) & (zs[r] == 0)).any(), (name, r)
                f2, p2 = S.merge_sorted_lists(c["z_coarse"][r], zs[r])
                assert np.array_equal(p2, pos[r]) and np.array_equal(S.bits(f2), S.bits(zf[r])), (name, r)
            elif np.isfinite(zs[r]).all() and c["coarse"] == "stratified":
                raise AssertionError((name, r, "a finite stratified row must take the sorted-lists branch"))
    assert took[True] > 100 and took[False] > 100 and {255, 256, 257} <= totals, (took, sorted(totals))


def test_shapes_cover_what_the_issue_names():
    fine = [c for c in S.CASES.values() if c["entry"] != "pdf"]
    assert {c["nc"] for c in fine} >= set(S.NC_ALL) and {c["nf"] for c in fine} >= set(S.NF_ALL)
    assert {c["n"] for c in fine} >= set(S.N_ALL) | {S.BIG_N}
    for entry in ("fine", "fine_pos", "bounds", "pdf"):
        assert {c["tables"] for c in S.CASES.values() if c["entry"] == entry} >= {"injected", "kernel"}, entry
    assert {c["bounds"] for c in S.CASES.values() if c["entry"] == "bounds"} == {"const", "varied", "degenerate"}
    c = S.case_inputs(next(k for k, v in S.CASES.items() if v["bounds"] == "degenerate"))
    assert (c["bounds_arr"][:, 0] == c["bounds_arr"][:, 1]).sum() == 1
    assert S.BIG_N > 4 * 4096 and (S.BIG_N + 3) // 4 > 256 * 16
    assert 4 * 2 * 2048 * 4 == 64 * 1024 and 4 * (2 * 1024 + 2 * 1024) * 4 == 64 * 1024 and 4 * 2 * 5120 * 4 == 160 * 1024


def test_jitter_words():
    """sampler_ref.jitter is the Philox block of the live grid's known-answer tests, read as the kernel reads it."""
    import occupancy_live_ref as lref
    seed, ray = 0x9E3779B97F4A7C15, (1 << 32) + 5
    u = S.jitter(seed, ray, 2, 6)
    for r in range(2):
        for k in range(6):
            word = lref.philox4x32_10(((ray + r) & M32, (ray + r) >> 32, k >> 2, 0), (seed & M32, seed >> 32))[k & 3]
            assert u[r, k] == F(word >> 8) * F(2.0 ** -24) and 0.0 <= u[r, k] < 1.0
    assert binding.seed64(-3) == 2 ** 64 - 3


# ---- f: refusals that need no launch ---------------------------------------------------------------------------------------------
MI_EINVAL = -1
FAKE = ctypes.c_void_p(0x10000)        # a non-null "device pointer": every call below must fail before it is used


def _refused(rc, lib, *words):
    msg = lib.mi_last_error()
    assert rc == MI_EINVAL, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def _fine_calls(lib, nc, nf, n=4):
    yield lib.mi_sample_fine(n, 2.0, 6.0, nc, nf, None, None, FAKE, FAKE, FAKE, FAKE, None)
    yield lib.mi_sample_fine_pos(n, 2.0, 6.0, nc, nf, None, None, FAKE, FAKE, FAKE, FAKE, FAKE, None)
    yield lib.mi_sample_fine_bounds(n, FAKE, nc, nf, None, FAKE, FAKE, FAKE, FAKE, FAKE, None)


def test_refusals():
    lib = binding.load()
    for nc in (0, 1, 2):
        for rc in _fine_calls(lib, nc, 4):
            _refused(rc, lib, b"Nc >= 3")
    for nb in (0, 1):
        _refused(lib.mi_sample_pdf(4, nb, 4, FAKE, FAKE, None, FAKE, None), lib, b"at least 2 bins")
    # the LDS limits, from the launchers' own formulas: the smallest size each refuses
    def fine_lds(nc, nf):
        return 4 * (2 * nc + 2 * (nc + nf)) * 4
    nc0 = next(nc for nc in range(3, 1 << 20) if fine_lds(nc, 0) > 64 * 1024)
    nf64 = next(nf for nf in range(0, 1 << 20) if fine_lds(64, nf) > 64 * 1024)
    assert (nc0, nf64) == (1025, 1921) and fine_lds(nc0 - 1, 0) == 64 * 1024 and fine_lds(64, nf64 - 1) <= 64 * 1024
    for nc, nf in ((nc0, 0), (64, nf64)):
        for rc, who in zip(_fine_calls(lib, nc, nf), (b"sample_fine:", b"sample_fine:", b"sample_fine_bounds:")):
            _refused(rc, lib, who, b"exceed LDS")
    nb0 = next(nb for nb in range(2, 1 << 20) if 4 * 2 * nb * 4 > 160 * 1024)
    assert nb0 == 5121
    _refused(lib.mi_sample_pdf(4, nb0, 4, FAKE, FAKE, None, FAKE, None), lib, b"sample_pdf:", b"exceed LDS")
    # nothing to do is not a refusal
    assert lib.mi_sample_pdf(0, nb0, 4, FAKE, FAKE, None, FAKE, None) == 0
    assert lib.mi_sample_pdf(4, 5, 0, FAKE, FAKE, None, None, None) == 0

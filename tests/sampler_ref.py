"""The inverse-CDF samplers of csrc/render_stages.hip restated on the CPU in numpy fp32 / fp64 (IEEE, every operation rounded on
its own, in the kernel's order), shared by tests/test_sampler_ref_host.py (which holds the restatement to the oracle, proves the
arithmetic the kernel's comments only argue, and plants the mistakes the comparison must reject) and
tests/test_gpu_sampler_bits.py (which holds mi_sample_fine, mi_sample_fine_pos, mi_sample_fine_bounds and mi_sample_pdf to it
bit for bit).  render_stages.hip is compiled without contraction and these functions use no transcendental, so one rounding per
operation is all there is to restate.

    normalise_pdf     t = fl(w + 1e-5f); 64 strided partial sums (lane j % 64, ascending j); xor butterfly 32..1; t / sum
    cdf               cdf[0] = 0, cdf[j] = fp32(fp64 sequential sum of pdf[:j]); cdf_path says which order the kernel takes,
                      cdf_scan is that other order (the shuffle scan), equal to the sequential one wherever the kernel takes it
    draw              the binary search, both clamps, the denom < 1e-5f guard, t = fl(fl(u - c0) / denom),
                      z = fl(b0 + fl(t * fl(b1 - b0)))
    merge             rank by the key (value, index): -0 before +0, a NaN with the sign bit clear last, one with it set first
    sample_pdf / sample_fine / sample_fine_bounds    (z_samples, z_fine, pos) as the C calls return them
    cdf_space_error   the mask-free accuracy measure of DESIGN.md 2: |F64(z) - u| over a scale that holds for every sample

and the inputs both test files use: `family` (the weight rows), `CASES` (every shape x family x entry point of the GPU test).
`plant=` names one of PLANTS: what a subtly wrong kernel would compute instead.
"""
import numpy as np

import occupancy_clip_ref as cref
import occupancy_live_ref as lref

F = np.float32
EPS = F(1e-5)                               # kPdfEps and the guard of draw_inverse_cdf: the same fp32 constant


def quiet():
    return np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore")


PLANTS = ("searchsorted_left", "guard_le", "guard_on_pdf", "pdf_sum_sequential", "cdf_fp32", "lerp_fma", "u_plain",
          "above_unclamped", "sample_before_equal_coarse", "pos_offset")


def bits(a) -> np.ndarray:
    """The int32 view the GPU test compares, NaNs of either sign and any payload made one value (a NaN equals a NaN)."""
    a = np.ascontiguousarray(np.asarray(a, F))
    b = a.view(np.int32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


# ---- the pdf ---------------------------------------------------------------------------------------------------------------------
def normalise_pdf(w, plant=None) -> np.ndarray:
    """float32 [nw]: (w + 1e-5f) / sum, the sum formed as the wave forms it."""
    w = np.asarray(w, F).reshape(-1)
    with quiet():
        t = (w + EPS).astype(F)
        if plant == "pdf_sum_sequential":
            part = F(0.0)
            for x in t:
                part = F(part + x)
        else:
            lanes = np.zeros(64, F)
            for base in range(0, t.size, 64):                     # lane j % 64 adds its terms in ascending j
                seg = t[base:base + 64]
                lanes[:seg.size] = (lanes[:seg.size] + seg).astype(F)
            idx = np.arange(64)
            for o in (32, 16, 8, 4, 2, 1):
                lanes = (lanes + lanes[idx ^ o]).astype(F)
            assert len(set(bits(lanes).tolist())) == 1, "the butterfly must leave every lane with the same sum"
            part = lanes[0]
        return (t / part).astype(F)


# ---- the cdf ---------------------------------------------------------------------------------------------------------------------
def cdf_path(pdf, nb: int) -> dict:
    """The criterion of cdf_like_cumsum restated literally: exponent fields, zero terms skipped for fmin, a denormal counted as
    field 1, field 255 forcing the sequential order.  {"exact", "fmin", "fmax", "log2n"}."""
    u = np.asarray(pdf, F).reshape(-1)[:nb - 1].view(np.uint32)
    fmin, fmax = 255, 0
    for x in u.tolist():
        f = (x >> 23) & 0xFF
        zero = ((x << 1) & 0xFFFFFFFF) == 0
        fmax = max(fmax, f)
        if not zero:
            fmin = min(fmin, max(f, 1))
    log2n = (nb - 1 if nb > 1 else 1).bit_length()
    exact = fmax < 255 and (fmin > fmax or fmax - fmin <= 28 - log2n)
    return dict(exact=bool(exact), fmin=fmin, fmax=fmax, log2n=log2n)


def cdf_sequential(pdf, nb: int, plant=None) -> np.ndarray:
    """float32 [nb]: cdf[j] = fp32(sum of pdf[:j]), the running sum a double (Python floats are IEEE doubles)."""
    pdf = np.asarray(pdf, F).reshape(-1)
    out = np.zeros(nb, F)
    with quiet():
        s = F(0.0) if plant == "cdf_fp32" else 0.0
        for j in range(1, nb):
            s = F(s + pdf[j - 1]) if plant == "cdf_fp32" else s + float(pdf[j - 1])
            out[j] = F(s)
    return out


def cdf_scan(pdf, nb: int) -> np.ndarray:
    """float32 [nb]: the order of the kernel's other branch - per 64 entries a Hillis-Steele scan in fp64 over the lanes
    (steps 1, 2, .., 32), the exclusive prefix as carry + (inclusive - own), the carry advanced by lane 63's inclusive sum."""
    pdf = np.asarray(pdf, F).reshape(-1)
    nw = nb - 1
    out = np.zeros(nb, F)
    carry = np.float64(0.0)
    terms = np.zeros((nb + 63) // 64 * 64)
    terms[:nw] = pdf[:nw]
    with quiet():
        for base in range(0, nb, 64):
            j = base + np.arange(64)
            own = terms[base:base + 64]                                  # 0.0 for a lane past the last term
            incl = own.copy()
            o = 1
            while o < 64:
                up = np.concatenate([np.zeros(o), incl[:-o]])
                incl = np.where(np.arange(64) >= o, incl + up, incl)
                o <<= 1
            val = (carry + (incl - own)).astype(F)
            m = j < nb
            out[j[m]] = val[m]
            carry = carry + incl[63]
    return out


def cdf(pdf, nb: int, plant=None):
    """(cdf float32 [nb], path): the restated cdf - the sequential fp64 sum, which the scan equals wherever the kernel takes it
    (tests/test_sampler_ref_host.py shows that) - and the branch the kernel's criterion picks."""
    return cdf_sequential(pdf, nb, plant), cdf_path(pdf, nb)


# ---- the draw --------------------------------------------------------------------------------------------------------------------
def u_table(nf: int, plant=None) -> np.ndarray:
    """float32 [nf]: linspace_at(0, 1, nf), the in-kernel table."""
    if plant == "u_plain" and nf > 1:
        return (np.arange(nf, dtype=F) / F(nf - 1)).astype(F)
    return cref.linspace_at([0.0], [1.0], nf)[0]


def draw(cdf_, bins, u, pdf=None, plant=None) -> np.ndarray:
    """float32 [len(u)]: draw_inverse_cdf of every u, all samples of the row stepping through the search together."""
    cdf_, bins, u = np.asarray(cdf_, F), np.asarray(bins, F), np.asarray(u, F).reshape(-1)
    nb = cdf_.size
    lo, hi = np.zeros(u.size, np.int64), np.full(u.size, nb, np.int64)
    with quiet():
        while True:
            live = lo < hi
            if not live.any():
                break
            mid = (lo + hi) >> 1
            c = cdf_[np.minimum(mid, nb - 1)]
            right = (c < u) if plant == "searchsorted_left" else (c <= u)          # false for a NaN on either side
            lo = np.where(live & right, mid + 1, lo)
            hi = np.where(live & ~right, mid, hi)
        below = np.maximum(lo - 1, 0)
        above = lo if plant == "above_unclamped" else np.minimum(lo, nb - 1)
        cx, bx = np.append(cdf_, F("nan")), np.append(bins, F("nan"))                 # what lies past the table: poison
        c0, c1 = cx[below], cx[above]
        denom = (c1 - c0).astype(F)
        if plant == "guard_on_pdf":
            guard = np.asarray(pdf, F)[np.minimum(below, nb - 2)] < EPS
        elif plant == "guard_le":
            guard = denom <= EPS
        else:
            guard = denom < EPS
        denom = np.where(guard, F(1.0), denom).astype(F)
        t = ((u - c0).astype(F) / denom).astype(F)
        b0, b1 = bx[below], bx[above]
        if plant == "lerp_fma":      # one rounding: the product of two floats is exact in a double (the sum's own rounding aside)
            return (b0.astype(np.float64) + t.astype(np.float64) * (b1 - b0).astype(F).astype(np.float64)).astype(F)
        return (b0 + (t * (b1 - b0).astype(F)).astype(F)).astype(F)


# ---- the merge -------------------------------------------------------------------------------------------------------------------
def sort_keys(zall, idx) -> np.ndarray:
    b = np.ascontiguousarray(np.asarray(zall, F)).view(np.uint32).astype(np.uint64)
    b = b ^ np.where(b >> np.uint64(31), np.uint64(0xFFFFFFFF), np.uint64(0x80000000))
    return (b << np.uint64(32)) | np.asarray(idx).astype(np.uint64)


def merge(z_coarse, z_samples, plant=None):
    """(z_fine float32 [Nc+Nf], pos int32 [Nc+Nf]): pos[e] = #(keys below element e's), key = (value, index in cat(coarse,
    samples)); z_fine[pos[e]] = element e."""
    zc, zs = np.asarray(z_coarse, F).reshape(-1), np.asarray(z_samples, F).reshape(-1)
    zall = np.concatenate([zc, zs])
    idx = np.arange(zall.size)
    if plant == "sample_before_equal_coarse":
        idx = np.concatenate([idx[:zc.size] + zs.size, idx[zc.size:] - zc.size])
    keys = sort_keys(zall, idx)
    assert np.unique(keys).size == keys.size
    pos = np.empty(zall.size, np.int32)
    pos[np.argsort(keys)] = np.arange(zall.size, dtype=np.int32)
    z_fine = np.empty_like(zall)
    z_fine[pos] = zall
    if plant == "pos_offset":
        pos = pos.copy()
        pos[zc.size:] += 1
    return z_fine, pos


def lists_sorted(z_coarse, z_samples) -> bool:
    """The kernel's `sorted` flag: each list ascending and free of NaN (the pair across the lists' seam is not looked at)."""
    for a in (np.asarray(z_coarse, F).reshape(-1), np.asarray(z_samples, F).reshape(-1)):
        with quiet():
            if np.isnan(a).any() or (a[1:] < a[:-1]).any():
                return False
    return True


def merge_sorted_lists(z_coarse, z_samples):
    """The kernel's branch for two sorted lists: a coarse depth goes behind the samples strictly below it, a sample behind the
    coarse depths at or below it (float compares: -0 == +0).  Equal to `merge` for every row that takes it, except where a
    sample is -0 and a coarse depth +0 (the key order puts that sample first, this branch the coarse depth); no -0 sample can
    come out of ascending bins, and the host test shows that none of the committed rows holds one."""
    zc, zs = np.asarray(z_coarse, F).reshape(-1), np.asarray(z_samples, F).reshape(-1)
    pos = np.empty(zc.size + zs.size, np.int32)
    for e, v in enumerate(zc):
        pos[e] = e + int(np.sum(zs < v))
    for i, v in enumerate(zs):
        pos[zc.size + i] = i + int(np.sum(zc <= v))
    z_fine = np.empty(pos.size, F)
    z_fine[pos] = np.concatenate([zc, zs])
    return z_fine, pos


# ---- the public functions: (z_samples, z_fine, pos) ------------------------------------------------------------------------------
def mids(lin) -> np.ndarray:
    lin = np.asarray(lin, F)
    return (F(0.5) * (lin[..., 1:] + lin[..., :-1]).astype(F)).astype(F)


def sample_row(bins, w, u, plant=None):
    """One ray's samples and what they came from: (z_samples, pdf, cdf, path)."""
    bins = np.asarray(bins, F).reshape(-1)
    pdf = normalise_pdf(w, plant)
    c, path = cdf(pdf, bins.size, plant)
    return draw(c, bins, u, pdf, plant), pdf, c, path


def sample_pdf(bins, weights, ns: int, u=None, plant=None):
    """mi_sample_pdf: bins [n,nb], weights [n,nb-1]; u an injected table [ns] or None for the in-kernel linspace."""
    bins, weights = np.asarray(bins, F), np.asarray(weights, F)
    u = u_table(ns, plant) if u is None else np.asarray(u, F)
    zs = np.stack([sample_row(bins[r], weights[r], u, plant)[0] for r in range(bins.shape[0])]).reshape(bins.shape[0], ns)
    return zs, None, None


def _fine(bins, z_coarse, weights, nf, u, plant):
    z_coarse, weights = np.asarray(z_coarse, F), np.asarray(weights, F)
    n, nc = z_coarse.shape
    u = u_table(nf, plant) if u is None else np.asarray(u, F)
    zs, zf, pos = np.zeros((n, nf), F), np.zeros((n, nc + nf), F), np.zeros((n, nc + nf), np.int32)
    for r in range(n):
        zs[r] = sample_row(bins[r], weights[r, 1:-1], u, plant)[0]
        zf[r], pos[r] = merge(z_coarse[r], zs[r], plant)
    return zs, zf, pos


def sample_fine(z_coarse, weights, near, far, nf: int, z_lin=None, u=None, plant=None):
    """mi_sample_fine / mi_sample_fine_pos: the bins are the mids of the injected z_lin table [Nc], or of
    linspace_at(near, far, Nc)."""
    n, nc = np.asarray(z_coarse).shape
    lin = cref.linspace_at([near], [far], nc)[0] if z_lin is None else np.asarray(z_lin, F)
    return _fine(np.broadcast_to(mids(lin), (n, nc - 1)), z_coarse, weights, nf, u, plant)


def sample_fine_bounds(bounds, z_coarse, weights, nf: int, u=None, plant=None):
    """mi_sample_fine_bounds: the bins of ray r are the mids of linspace_at(near_r, far_r, Nc)."""
    b = np.asarray(bounds, F)
    nc = np.asarray(z_coarse).shape[1]
    return _fine(mids(cref.linspace_at(b[:, 0], b[:, 1], nc)), z_coarse, weights, nf, u, plant)


# ---- the seeded jitter -----------------------------------------------------------------------------------------------------------
def jitter(seed64: int, ray0: int, n: int, nc: int) -> np.ndarray:
    """float32 [n,Nc]: u = (word >> 8) * 2^-24, the word of sample k of ray r being word k & 3 of the Philox block with
    counter (ray_lo, ray_hi, k >> 2, 0), ray = ray0 + r (mod 2^64), under the key (seed_lo, seed_hi)."""
    out = np.zeros((n, nc), F)
    for r in range(n):
        words = lref.stream_words(int(seed64) & (2 ** 64 - 1), (ray0 + r) & (2 ** 64 - 1), nc)
        out[r] = [F(w >> 8) * F(2.0 ** -24) for w in words]
    return out


def sample_coarse_seeded(bounds, nc: int, seed64: int, ray0: int) -> np.ndarray:
    """float32 [n,Nc]: sample_coarse / sample_coarse_bounds under the in-kernel linspace and the seeded jitter."""
    b = np.asarray(bounds, F)
    return cref.sample_coarse_bounds(b, nc, jitter(seed64, ray0, b.shape[0], nc))


# ---- the accuracy measure in CDF space -----------------------------------------------------------------------------
def cdf_space_error(bins, w, z, u) -> np.ndarray:
    """float64 [n,ns]: |F64(z) - u| / scale for every sample, none left out.  F64 is the piecewise-linear cdf of
    (w + 1e-5) / sum over the ascending bins in fp64 (0 in front of the first bin, 1 behind the last);
    scale = 1e-5 + 2^-23 + slope * ulp(z): the guard's width, the fp32 roundings of pdf and cdf, and the slope of F64 (the
    largest pdf_j / width_j over the sample's bin and its two neighbours) times the spacing of fp32 at z.  A bracket or guard
    flip moves z by up to a bin but F64(z) by less than the guard's width, so the measure needs no mask."""
    bins, w, z = np.asarray(bins, F).astype(np.float64), np.asarray(w, F).astype(np.float64), np.asarray(z, F)
    u = np.broadcast_to(np.asarray(u, F).astype(np.float64), z.shape)
    out = np.zeros(z.shape)
    for r in range(z.shape[0]):
        width = np.diff(bins[r])
        assert (width > 0).all() and np.isfinite(w[r]).all(), "the measure is defined over ascending bins and finite weights"
        t = w[r] + 1e-5
        pdf = t / t.sum()
        c = np.concatenate([[0.0], np.cumsum(pdf)])
        zr = z[r].astype(np.float64)
        f = np.interp(zr, bins[r], c)
        j = np.clip(np.searchsorted(bins[r], zr, side="right") - 1, 0, pdf.size - 1)
        dens = pdf / width
        slope = np.max([dens[np.clip(j + k, 0, pdf.size - 1)] for k in (-1, 0, 1)], axis=0)
        scale = 1e-5 + 2.0 ** -23 + slope * np.spacing(np.abs(z[r])).astype(np.float64)
        out[r] = np.abs(f - u[r]) / scale
    return out


# ---- the weight rows -------------------------------------------------------------------------------------------------------------
GUARD_U = np.array([0.0, 0.25e-5, 0.5e-5, 1.2e-5, 1.7e-5, 2.5e-5, 0.5, 1.0], F)     # the injected u of the guard sweep
GUARD_STEPS = 8                                                                     # 2 * 8 + 1 rows


def _rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def _span_row(nw, d, rng):
    """Weights so large that + 1e-5f changes none (>= 2^10, half an ulp 6e-5), the smallest 2^10 and the largest 2^(10+d), both
    powers of two: they keep one mantissa through the division by the sum, so the pdf's exponent fields span exactly d."""
    e = rng.integers(10, 10 + d + 1, nw).astype(np.float64)
    row = (2.0 ** e * (1.0 + rng.random(nw))).clip(2.0 ** 10, 2.0 ** (10 + d))
    a = int(rng.integers(0, nw))
    row[a] = 2.0 ** 10
    row[(a + 1 + int(rng.integers(0, nw - 1))) % nw] = 2.0 ** (10 + d)
    return row.astype(F)


def power6(r) -> np.ndarray:
    """float32 r^6 by multiplications (each an IEEE operation: the same bits on every host, which a pow need not give)."""
    r2 = r * r
    return (r2 * r2 * r2).astype(F)


def crit_span(nb: int) -> int:
    return 28 - (nb - 1).bit_length()


def family(name: str, n: int, nw: int) -> np.ndarray:
    """float32 [n,nw]: the interior weights of family `name`."""
    rng = _rng(1234, nw, sum(map(ord, name)))
    w = power6(rng.random((n, nw)))
    if name == "random6":
        pass
    elif name == "zero":
        w[:] = 0
    elif name == "spike":                                  # first, middle, last interior bin, row after row
        w[:] = 0
        for r in range(n):
            w[r, (0, nw // 2, nw - 1)[r % 3]] = 1.0
    elif name == "two_ended":
        w[:] = 0
        w[:, 0] = w[:, -1] = 0.5
    elif name == "tiny":
        w = (w * F(1e-12)).astype(F)
    elif name in ("span40", "crit", "crit_plus1", "crit_plus2"):
        d = 40 if name == "span40" else crit_span(nw + 1) + ("crit", "crit_plus1", "crit_plus2").index(name)
        if nw >= 2:
            w = np.stack([_span_row(nw, d, rng) for _ in range(n)])
    elif name == "huge":
        w[:, nw // 2] = F(2.0 ** 127)
    elif name == "uniform":
        w[:] = 1.0
    elif name == "guard_sweep":
        # the leading bins empty, the mass M in the last one, sum = M + nw * 1e-5 stepped through 1 in units of 2^-24: the
        # empty bins' pdf 1e-5 / sum, which is their cdf step at the foot of the cdf, crosses the guard from row to row
        assert n == 2 * GUARD_STEPS + 1 and nw >= 3
        w[:] = 0
        for r in range(n):
            w[r, -1] = F(1.0 - (nw - 1) * 1e-5 - 1e-5 + (r - GUARD_STEPS) * 2.0 ** -24)
    elif name in ("inf_row", "nan_row"):
        if n > 1:
            w[1, nw // 2] = F("inf") if name == "inf_row" else F("nan")
    else:
        raise KeyError(name)
    return w


# ---- the cases of the GPU test ---------------------------------------------------------------------------------------------------
NEAR, FAR = 2.0, 6.0
NC_ALL = (3, 4, 5, 65, 66, 67, 129, 130, 258)
NF_ALL = (0, 1, 2, 63, 64, 65)
N_ALL = (1, 3, 4, 5)
FAMILIES = ("random6", "zero", "spike", "two_ended", "tiny", "span40", "crit", "crit_plus1", "crit_plus2", "huge", "inf_row",
            "nan_row")
BIG_N = 4 * 4096 + 5                          # the grid is capped at 4096 blocks of four rays: a second trip of the ray loop


def _shapes():
    """Every Nc with every Nf of NF_ALL and with the three Nf that put Nc + Nf on 255, 256, 257; n cycles through N_ALL."""
    out, k = [], 0
    for nc in NC_ALL:
        for nf in NF_ALL + tuple(s - nc for s in (255, 256, 257) if s - nc > 0):
            out.append((nc, nf, N_ALL[k % 4]))
            k += 1
    return out


def _cases():
    """name -> dict(entry, nc, nf, n, family, tables, coarse, bounds).  entry: fine | fine_pos | bounds | pdf.  tables: "injected"
    (the z_lin / u tables mirender.ops passes) or "kernel" (NULL: the in-kernel linspaces).  coarse: "stratified" (sorted) or
    "unsorted" (signed, tied: the counting merge).  bounds (entry bounds): const | varied | degenerate."""
    out = {}

    def add(entry, nc, nf, n, fam, tables="kernel", coarse="stratified", bounds=None):
        key = f"{entry}-nc{nc}-nf{nf}-n{n}-{fam}-{tables}-{coarse}" + (f"-{bounds}" if bounds else "")
        out[key] = dict(entry=entry, nc=nc, nf=nf, n=n, family=fam, tables=tables, coarse=coarse, bounds=bounds)

    entries = ("fine", "fine_pos", "bounds", "pdf")
    for i, (nc, nf, n) in enumerate(_shapes()):
        entry = entries[i % 4]
        add(entry, nc, nf, n, FAMILIES[i % len(FAMILIES)], ("kernel", "injected")[(i // 4) % 2],
            ("stratified", "unsorted")[(i // 2) % 2] if entry != "pdf" else "stratified",
            ("const", "varied", "degenerate")[(i // 4) % 3] if entry == "bounds" else None)
        if i % 3 == 0:
            add(entries[(i + 1) % 4], nc, nf, n, "random6", ("injected", "kernel")[(i // 4) % 2],
                bounds="varied" if entries[(i + 1) % 4] == "bounds" else None)
    # every family under every entry point at a small and a two-chunk shape, both merges
    for fam in FAMILIES:
        for nc, nf, n in ((5, 3, 4), (66, 65, 3), (130, 126, 5)):
            for entry in entries:
                add(entry, nc, nf, n, fam, "injected" if entry in ("fine", "pdf") else "kernel",
                    "unsorted" if entry == "fine_pos" else "stratified", "varied" if entry == "bounds" else None)
    # the criterion's two sides (and the row beyond both) at every nb of the host test's proof
    for nb in (64, 65, 129, 257):
        for fam in ("crit", "crit_plus1", "crit_plus2"):
            add("pdf", nb + 1, 65, 3, fam)
            add("fine_pos", nb + 1, 65, 3, fam)
    # uniform weights, (nb - 1) dividing (nf - 1), nb - 1 a power of two: every u is a cdf entry
    for nc, nf in ((3, 2), (4, 3), (6, 9), (66, 65), (66, 129)):
        for entry in entries:
            add(entry, nc, nf, 3, "uniform", bounds="const" if entry == "bounds" else None)
    # the guard sweep under its own u table
    for nc in (5, 66):
        for entry in entries:
            add(entry, nc, GUARD_U.size, 2 * GUARD_STEPS + 1, "guard_sweep", "guard_u", bounds="varied" if entry == "bounds" else None)
    # unsorted coarse depths across the counting merge's 256-element sweep
    for nc in (3, 66, 130):
        for total in (255, 256, 257):
            add("fine_pos", nc, total - nc, 3, "random6", coarse="unsorted")
            add("bounds", nc, total - nc, 4, "spike", coarse="unsorted", bounds="varied")
    add("fine", 1024, 0, 1, "random6")                      # 4 * (2 Nc + 2 (Nc + Nf)) * 4 = 64 KiB exactly: the largest request
    add("fine_pos", 5, 3, BIG_N, "random6", "injected")
    add("bounds", 5, 3, BIG_N, "random6", bounds="varied")
    add("pdf", 2049, 8, 4, "random6")                       # 2048 bins: the largest request that is still 64 KiB
    add("pdf", 2101, 8, 4, "random6")                       # 2100 bins: past 64 KiB of dynamic LDS
    add("pdf", 5121, 8, 4, "random6")                       # 5120 bins: 160 KiB, the largest request the launcher lets through
    return out


CASES = _cases()
BIG_DISTINCT = 64                             # the big case repeats this many distinct rays


def case_bounds(c) -> np.ndarray:
    n = min(c["n"], BIG_DISTINCT)
    rng = _rng(77, c["nc"], n)
    b = np.tile(np.array([[NEAR, FAR]], F), (n, 1))
    if c["bounds"] in ("varied", "degenerate"):
        lo = (NEAR + 3.0 * rng.random(n)).astype(F)
        b = np.stack([lo, (lo + F(0.25) + rng.random(n).astype(F)).astype(F)], 1).astype(F)
    if c["bounds"] == "degenerate":
        b[n // 2, 1] = b[n // 2, 0]
    return b


def case_inputs(name: str) -> dict:
    """The arrays of one case on the CPU: weights [n,Nc] (interior from `family`, the two ends random: nothing may read them),
    z_coarse [n,Nc], bounds [n,2] (entry bounds), bins [n,Nc-1] (entry pdf: sorted random bins), and the tables z_lin / u to
    inject (None: the in-kernel linspace).  The BIG_N case holds BIG_DISTINCT distinct rays (`tile` says how to repeat them)."""
    c = dict(CASES[name])
    nc, nf, n = c["nc"], c["nf"], min(c["n"], BIG_DISTINCT)
    rng = _rng(99, nc, nf, n, sum(map(ord, name)))
    w = rng.random((n, nc)).astype(F)
    w[:, 1:-1] = family(c["family"], n, nc - 2)
    c["weights"] = w
    c["bounds_arr"] = case_bounds(c) if c["entry"] == "bounds" else np.tile(np.array([[NEAR, FAR]], F), (n, 1))
    if c["coarse"] == "unsorted":
        zc = (np.round(rng.normal(size=(n, nc)) * 4) / 4).astype(F)               # quarters: signed, tied, both zeros
        zc[:, 0] = F(-0.0)
        if nc > 3:
            zc[:, nc // 2] = F(0.0)
            zc[:, 1] = mids(cref.linspace_at([NEAR], [FAR], nc)[0])[0]           # the sample at u = 0 (fine, fine_pos): a tie
        c["z_coarse"] = zc
    else:
        c["z_coarse"] = cref.sample_coarse_bounds(c["bounds_arr"], nc, rng.random((n, nc)).astype(F))
    bins = np.sort((NEAR + (FAR - NEAR) * rng.random((n, nc - 1))).astype(F), 1)
    if c["family"] == "uniform":
        # bins growing by an irregular factor of 3 to 5: on many of them b0 + 1 * (b1 - b0) is not b1 in fp32, so the bracket
        # below an exact hit (t = 1) and the one above it (t = 0) give different bits
        bins = np.tile(np.multiply.accumulate(np.concatenate([[1e-6], 3.0 + 2.0 * _rng(5, nc).random(nc - 2)]).astype(F)), (n, 1))
    c["bins"] = bins
    c["z_lin"] = c["u"] = None
    if c["tables"] == "guard_u":
        c["u"] = GUARD_U
    c["reps"] = c["n"] // n + 1 if c["n"] > n else 1
    return c


def tile_rows(a, c):
    """The case's distinct rows repeated up to its n."""
    return a if c["reps"] == 1 else np.tile(a, (c["reps"],) + (1,) * (a.ndim - 1))[:c["n"]]


def reference(c, plant=None, z_lin=None, u=None):
    """(z_samples, z_fine, pos) of the case from the restatement (distinct rows only); z_lin / u: the injected tables."""
    u = c["u"] if u is None else u
    if c["entry"] == "pdf":
        return sample_pdf(c["bins"], c["weights"][:, 1:-1], c["nf"], u, plant)
    if c["entry"] == "bounds":
        return sample_fine_bounds(c["bounds_arr"], c["z_coarse"], c["weights"], c["nf"], u, plant)
    return sample_fine(c["z_coarse"], c["weights"], NEAR, FAR, c["nf"], z_lin, u, plant)


def case_bins(c, z_lin=None) -> np.ndarray:
    """float32 [n,nb]: the bins each ray of the case draws from."""
    if c["entry"] == "pdf":
        return c["bins"]
    n, nc = c["z_coarse"].shape
    if c["entry"] == "bounds":
        return mids(cref.linspace_at(c["bounds_arr"][:, 0], c["bounds_arr"][:, 1], nc))
    lin = cref.linspace_at([NEAR], [FAR], nc)[0] if z_lin is None else np.asarray(z_lin, F)
    return np.broadcast_to(mids(lin), (n, nc - 1))

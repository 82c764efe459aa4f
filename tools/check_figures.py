#!/usr/bin/env python3
"""Every figure DESIGN.md / README.md quote for the headline kernel and the bench line, asserted against the tracked file
under profiles/ it is said to come from (the docs quoted 94.0 % / 994.6 ms / 22.4 B/point / 6 208 MFMAs where the
tracked profiles said 0.936 / 1 001.2 ms / 21.2 B/point / 9 280).

    python tools/check_figures.py            # prints one line per figure, exits non-zero on a mismatch or a missing sentence

A check = (document, regular expression with one group per number, the values the tracked files give, tolerance).  The
sentence must be FOUND - a figure cannot leave the check by being reworded - and every captured number must equal the
source's within the rounding the text shows (half a unit of its last printed digit, plus `slack` relative).  CPU only;
tests/test_figures.py runs it in the CPU suite."""
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND = "r04"
PEAK = 157.3


def _json_line(path):
    with open(os.path.join(ROOT, path)) as f:
        lines = [ln for ln in f if ln.startswith("{")]
    return json.loads(lines[-1])


def _num(text: str) -> float:
    return float(text.replace(" ", "").replace(" ", "").replace(",", ""))


def _digits(text: str) -> float:
    """Half a unit of the last digit the text prints ('0.930' -> 0.0005, '482 252' -> 0.5, '3.5635e10' -> 0.00005e10)."""
    t = text.replace(" ", "")
    mant, _, exp = t.lower().partition("e")
    scale = 10.0 ** int(exp) if exp else 1.0
    frac = len(mant.split(".")[1]) if "." in mant else 0
    return 0.5 * 10.0 ** (-frac) * scale


def sources():
    bench = _json_line(f"profiles/{ROUND}_bench_n1.log")
    pmc = json.load(open(os.path.join(ROOT, f"profiles/{ROUND}_pmc_nerf_fwd.json")))
    d = pmc["derived_fine_launch"]
    i = max(range(len(pmc["launch_points"])), key=lambda j: pmc["launch_points"][j])
    waves = pmc["launch_points"][i] / 32
    stats = {}
    with open(os.path.join(ROOT, f"profiles/{ROUND}_bench_c3_kernel_stats.csv")) as f:
        for r in csv.DictReader(f):
            stats[r["Name"]] = r
    fwd = next(v for k, v in stats.items() if "nerf_fwd_kernel<false, false>" in k)
    flops_fine = pmc["launch_points"][i] * 1182976
    kinds = json.load(open(os.path.join(ROOT, f"profiles/{ROUND}_pmc_kinds.json")))["kernels"]
    kb = lambda name: kinds[name]["mfma_busy_frac"]                                   # noqa: E731
    pct = {}
    with open(os.path.join(ROOT, f"profiles/{ROUND}_perf_kinds.log")) as f:
        for ln in f:
            m = re.match(r"(\w+)\s+fwd .*\(([\d.]+)% of fp32 MFMA peak\)", ln)
            if m:
                pct[m.group(1)] = float(m.group(2))
    fam = bench["psnr_vs_ref"]["families"]
    tr = bench["train"]
    return dict(
        bench=bench, pmc=d,
        fine_ms=d["ms"], fine_tflops=flops_fine / (d["ms"] * 1e-3) / 1e12, busy=d["mfma_busy_frac"], clock=d["effective_clock_GHz"],
        write_gb=d["WRITE_SIZE_bytes"] / 1e9, write_bpp=d["WRITE_SIZE_bytes"] / d["points"], fetch_gb=d["FETCH_SIZE_bytes_raw"] / 1e9,
        bpp=d["hbm_bytes_per_point_upper"], gbps=d["hbm_GBps_upper"], lds=d["lds_bank_conflict_cycles"],
        insts_mfma=pmc["counters"]["SQ_INSTS_MFMA"][i], mfma_per_wave=pmc["counters"]["SQ_INSTS_MFMA"][i] / waves,
        flops_issued=d["mfma_flops_issued"], flops_alg=flops_fine,
        stats_calls=int(fwd["Calls"]), stats_avg_ms=float(fwd["AverageNs"]) / 1e6, fam=fam, tr=tr, kb=kb, pct=pct)


def checks(s):
    b, fam, tr = s["bench"], s["fam"], s["tr"]
    r = b["roofline"]
    design = [
        # section 4.1: the PMC passes of the headline kernel
        (r"fine launch ([\d.]+) ms = ([\d.]+) TFLOP/s = ([\d.]+) % of the",
         [s["fine_ms"], s["fine_tflops"], 100 * s["fine_tflops"] / PEAK]),
        (r"`SQ_VALU_MFMA_BUSY_CYCLES` / SIMD-cycles = ([\d.]+); effective clock ([\d.]+) GHz; HBM traffic ([\d.]+) GB written",
         [s["busy"], s["clock"], s["write_gb"]]),
        (r"\(= ([\d.]+) B/point\) \+ ([\d.]+) GB x 2 read per launch = ([\d.]+) B/point against 20 algorithmic, ([\d.]+) GB/s",
         [s["write_bpp"], s["fetch_gb"], s["bpp"], s["gbps"]]),
        (r"`SQ_LDS_BANK_CONFLICT` (\d+); `SQ_INSTS_MFMA` ([\d.e]+) = ([\d ]+) MFMAs per wave-tile",
         [s["lds"], s["insts_mfma"], s["mfma_per_wave"]]),
        (r"MFMA FLOPs issued ([\d.e]+) against ([\d.e]+) algorithmic", [s["flops_issued"], s["flops_alg"]]),
        (r"`nerf_fwd_kernel<false,false>` (\d+) launches, average ([\d.]+) ms \(coarse \+ fine launch of a step = ([\d .]+) ms\)",
         [s["stats_calls"], s["stats_avg_ms"], 2 * s["stats_avg_ms"]]),
        (r"besides its ([\d ]+) MFMAs \(", [s["mfma_per_wave"]]),
        (r"`profiles/r04_perf_kinds.log`\): NeRF ([\d.]+) %, TinyNeRF ([\d.]+) %, SirenNeRF ([\d.]+) %, FilmSirenNeRF ([\d.]+) % of",
         [s["pct"]["nerf"], s["pct"]["tiny"], s["pct"]["siren"], s["pct"]["film"]]),
        (r"`profiles/r04_pmc_kinds.json`\): ([\d.]+) / ([\d.]+) / ([\d.]+) / ([\d.]+), and - a NeRF training step at 8 192 rays - saving forward ([\d.]+), chain ([\d.]+),\s+256x256 dW GEMMs ([\d.]+), the narrow tiles ([\d.]+) \(128x256\) / ([\d.]+) \(256x64\) / ([\d.]+) \(128x32\)",
         [s["kb"]("mi::nerf_fwd_kernel<false, false>"), s["kb"]("mi::nerf_fwd_kernel<true, false>"), s["kb"]("mi::siren_fwd_kernel<false>"),
          s["kb"]("mi::film_fwd_kernel<true, false>"), s["kb"]("mi::nerf_fwd_kernel<false, true>"), s["kb"]("mi::nerf_bwd_kernel<false>"),
          s["kb"]("mi::dw_gemm_kernel<4, 2, 2>"), s["kb"]("mi::dw_gemm_kernel<4, 1, 2>"), s["kb"]("mi::dw_gemm_kernel<2, 2, 1>"),
          s["kb"]("mi::dw_gemm_kernel<1, 1, 1>")]),
        # section 6: the bench line
        (r"one MI355X\): ([\d ]+) rays/s, ([\d .]+) ms per frame, `roofline.frac` ([\d.]+)\s+\(([\d.]+) TFLOP/s; average MLP launch ([\d.]+) ms",
         [b["value"], b["ms_per_step"], r["frac"], r["achieved"], r["avg_launch_ms"]]),
        (r"`frame64` \(800x800 @ 64 samples\) ([\d.]+) ms = ([\d.]+) M rays/s", [b["frame64"]["ms_per_frame"], b["frame64"]["rays_per_s"] / 1e6]),
        (r"same frame\) (\d+) rays/s, GPU/CPU (\d+)x", [b["cpu_baseline"]["value"], b["gpu_over_cpu"]]),
        (r"FETCH_SIZE doubled as the guide prescribes for\s+gfx950\): ([\d.]+) B/point against 20 algorithmic", [s["bpp"]]),
        (r"TinyNeRF ([\d.]+) vs ([\d.]+) dB \(oracle loop run live\), loss ([\d.e-]+)",
         [fam["tiny_nerf"]["hip_db"], fam["tiny_nerf"]["cpu_reference_loop_db"], fam["tiny_nerf"]["max_rel_loss_diff"]]),
        (r"round 4 - ([\d.]+) vs ([\d.]+) dB, loss ([\d.e-]+); SirenNeRF ([\d.]+) vs ([\d.]+) dB, loss ([\d.e-]+); FilmSirenNeRF \(fixed FiLM row\)\s+([\d.]+) vs ([\d.]+) dB, loss ([\d.e-]+)",
         [fam["nerf"]["hip_db"], fam["nerf"]["cpu_reference_loop_db"], fam["nerf"]["max_rel_loss_diff"],
          fam["siren_nerf"]["hip_db"], fam["siren_nerf"]["cpu_reference_loop_db"], fam["siren_nerf"]["max_rel_loss_diff"],
          fam["film_siren_nerf"]["hip_db"], fam["film_siren_nerf"]["cpu_reference_loop_db"], fam["film_siren_nerf"]["max_rel_loss_diff"]]),
        (r"nerf 1 024-ray step ([\d.]+) ms, `frac` ([\d.]+); pi_GAN C5 step \(4 images 256x256, D-step forward \+\s+G-step\) ([\d.]+) ms, `frac` ([\d.]+) \(reference-equivalent ([\d.]+)\); C4 step \(batch 32, 128x128\) ([\d.]+) ms, `frac` ([\d.]+)\s+\(reference-equivalent ([\d.]+)\)",
         [tr["nerf_train"]["ms_per_step"], tr["nerf_train"]["frac"], tr["c5"]["ms_per_step"], tr["c5"]["frac"], tr["c5"]["frac_reference_equivalent"],
          tr["c4"]["ms_per_step"], tr["c4"]["frac"], tr["c4"]["frac_reference_equivalent"]]),
    ]
    readme = [
        (r"profiles/r04_\*\): ([\d ]+) rays/s on the 64\+128 frame \(([\d.]+) s per 800×800 frame\), ([\d.]+) ms per\s+800×800 frame at 64 samples",
         [b["value"], b["ms_per_step"] / 1e3, b["frame64"]["ms_per_frame"]]),
        (r"fused NeRF MLP at ([\d.]+) TFLOP/s = ([\d.]+) % of the fp32 MFMA peak \(MFMA-busy counter ([\d.]+)\)",
         [r["achieved"], 100 * r["frac"], s["busy"]]),
        (r"(\d+)× the 16-core CPU oracle", [b["gpu_over_cpu"]]),
        (r"nerf\s+step \(1024 rays, fused Adam\) ([\d.]+) ms \(([\d.]+) of peak\)", [tr["nerf_train"]["ms_per_step"], tr["nerf_train"]["frac"]]),
        (r"generator\s+step ([\d.]+) s \(([\d.]+) of peak on the 108", [tr["c4"]["ms_per_step"] / 1e3, tr["c4"]["frac"]]),
        (r"256² training step ([\d.]+) s per GPU \(([\d.]+)\)", [tr["c5"]["ms_per_step"] / 1e3, tr["c5"]["frac"]]),
    ]
    r5 = sigma_only_sources()
    design += [
        (r"the\s+coarse launch takes ([\d.]+) ms against ([\d.]+) ms before, ([\d.]+) TFLOP/s executed = ([\d.]+) of the peak, as efficient as the\s+whole forward; the fine launch is unchanged \(([\d.]+) ms against ([\d.]+) ms\)",
         [r5["coarse"]["branch"], r5["coarse"]["main"], r5["sigma_tflops"], r5["sigma_tflops"] / PEAK, r5["fine"]["branch"], r5["fine"]["main"]]),
        (r"alternating on one MI355X\): ([\d ]+) / ([\d ]+) / ([\d ]+) rays/s before against ([\d ]+) / ([\d ]+) / ([\d ]+)\s+after, \+([\d.]+) % on every pair",
         [*r5["value"]["main"], *r5["value"]["branch"], r5["min_gain_pct"]]),
        (r"`roofline.frac` rises from ([\d.]+) to\s+([\d.]+), but only", [r5["frac"]["main"], r5["frac"]["branch"]]),
    ]
    r6 = deferred_colour_sources()
    design += [
        (r"the parent's fine launch takes ([\d.]+) ms; the branch's (\d+) trunk-and-spill launches take ([\d.]+) ms and its (\d+) colour\s+launches ([\d.]+) ms per frame, ([\d.]+) ms together",
         [r6["fine_parent"], r6["spill_calls"], r6["spill"], r6["colour_calls"], r6["colour"], r6["spill"] + r6["colour"]]),
        (r"windowed coarse pass, measured for the first time: its (\d+) field launches take ([\d.]+) ms per frame and its (\d+)\s+composite launches ([\d.]+) ms",
         [r6["window_calls"], r6["window"], r6["wcomp_calls"], r6["wcomp"]]),
        (r"deferred colour branch alternating on one MI355X\): ([\d ]+) / ([\d ]+) / ([\d ]+) rays/s before against ([\d ]+) / ([\d ]+) / ([\d ]+)\s+after, \+([\d.]+) % at least on every pair; the largest spread among runs of one build is ([\d.]+) %",
         [*r6["value"]["main"], *r6["value"]["branch"], r6["min_gain_pct"], r6["spread_pct"]]),
    ]
    st = sampler_stop_sources()
    design += [
        (r"the (\d+) coarse field launches take ([\d.]+) ms against ([\d.]+) ms before and the (\d+) window composites ([\d.]+) ms against ([\d.]+) ms;\s+the fine pass is unchanged, (\d+) trunk-and-spill launches ([\d.]+) ms against ([\d.]+) ms and (\d+) colour launches ([\d.]+) ms against ([\d.]+) ms",
         [st["window_calls"], st["window"]["branch"], st["window"]["parent"], st["wcomp_calls"], st["wcomp"]["branch"], st["wcomp"]["parent"],
          st["spill_calls"], st["spill"]["branch"], st["spill"]["parent"], st["colour_calls"], st["colour"]["branch"], st["colour"]["parent"]]),
        (r"its parent on one MI355X\): ([\d ]+) / ([\d ]+) / ([\d ]+) rays/s before against ([\d ]+) / ([\d ]+) / ([\d ]+)\s+after, \+([\d.]+) % at least on every pair; the largest spread among runs of one build is ([\d.]+) %",
         [*st["value"]["main"], *st["value"]["branch"], st["min_gain_pct"], st["spread_pct"]]),
        (r"windows of 4 give\s+([\d ]+) / ([\d ]+) / ([\d ]+) rays/s against ([\d ]+) / ([\d ]+) / ([\d ]+) with windows of 8",
         [*st["value"]["w4"], *st["value"]["w8"]]),
    ]
    return [("DESIGN.md", design), ("README.md", readme)]


def sigma_only_sources():
    """The sigma-only coarse pass: mean coarse / fine MLP launch of each build from the kernel traces (the
    launches alternate coarse, fine), and the alternating bench pairs."""
    out = {"coarse": {}, "fine": {}, "value": {"main": [], "branch": []}, "frac": {}}
    for b in ("main", "branch"):
        with open(os.path.join(ROOT, f"profiles/r05_sigma_only_c3_kernel_trace_{b}.csv")) as f:
            rows = sorted((r for r in csv.DictReader(f) if "nerf_fwd_kernel" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows]
        out["coarse"][b], out["fine"][b] = sum(d[0::2]) / len(d[0::2]), sum(d[1::2]) / len(d[1::2])
    with open(os.path.join(ROOT, "profiles/r05_sigma_only_bench_pairs.log")) as f:
        runs = [json.loads(ln) for ln in f if ln.startswith("{")]
    for r in runs:
        out["value"][r["build"]].append(r["line"]["value"])
        out["frac"].setdefault(r["build"], []).append(r["line"]["roofline"]["frac"])
    out["frac"] = {b: sum(v) / len(v) for b, v in out["frac"].items()}
    out["min_gain_pct"] = min(100 * (b / m - 1) for m, b in zip(out["value"]["main"], out["value"]["branch"]))
    out["sigma_tflops"] = 2 * 489728 * 640000 * 64 / (out["coarse"]["branch"] * 1e-3) / 1e12
    return out


def deferred_colour_sources():
    """The fine pass's deferred colour branch: per-frame kernel totals of the parent's and the branch's kernel
    statistics (rocprofv3, 4 frames each) and the alternating bench pairs."""
    frames = 4
    stats = {}
    for b in ("parent", "branch"):
        with open(os.path.join(ROOT, f"profiles/r06_deferred_colour_kernel_stats_{b}.csv")) as f:
            stats[b] = {r["Name"]: r for r in csv.DictReader(f)}

    def per_frame(b, key):
        rows = [r for k, r in stats[b].items() if key in k]
        assert len(rows) == 1, (b, key, len(rows))
        return int(rows[0]["Calls"]) // frames, float(rows[0]["TotalDurationNs"]) / 1e6 / frames

    out = {"value": {"main": [], "branch": []}}
    _, out["fine_parent"] = per_frame("parent", "nerf_fwd_kernel<false, false, false, false>")
    out["spill_calls"], out["spill"] = per_frame("branch", "nerf_fwd_kernel<false, false, true, false, true>")
    out["colour_calls"], out["colour"] = per_frame("branch", "nerf_colour_kernel<false>")
    out["window_calls"], out["window"] = per_frame("parent", "nerf_fwd_kernel<false, false, true, true>")
    out["wcomp_calls"], out["wcomp"] = per_frame("parent", "composite_weights_window_kernel")
    with open(os.path.join(ROOT, "profiles/r06_deferred_colour_bench_pairs.log")) as f:
        for r in (json.loads(ln) for ln in f if ln.startswith("{")):
            out["value"][r["build"]].append(r["line"]["value"])
    out["min_gain_pct"] = min(100 * (b / m - 1) for m, b in zip(out["value"]["main"], out["value"]["branch"]))
    out["spread_pct"] = max(100 * (max(v) / min(v) - 1) for v in out["value"].values())
    return out


def sampler_stop_sources():
    """The 2^-42 stop of the windowed coarse pass: per-frame kernel totals of the parent's and the branch's
    kernel statistics (rocprofv3, 4 frames each), the alternating bench pairs, and the window-4 against window-8 pairs."""
    frames = 4
    keys = {"window": "nerf_fwd_kernel<false, false, true, true, false>", "wcomp": "composite_weights_window_kernel",
            "spill": "nerf_fwd_kernel<false, false, true, false, true>", "colour": "nerf_colour_kernel<false>"}
    out = {k: {} for k in keys}
    out["value"] = {"main": [], "branch": [], "w4": [], "w8": []}
    for b in ("parent", "branch"):
        with open(os.path.join(ROOT, f"profiles/sampler_stop_kernel_stats_{b}.csv")) as f:
            stats = {r["Name"]: r for r in csv.DictReader(f)}
        for name, key in keys.items():
            rows = [r for k, r in stats.items() if key in k]
            assert len(rows) == 1, (b, key, len(rows))
            out[name + "_calls"] = int(rows[0]["Calls"]) // frames
            out[name][b] = float(rows[0]["TotalDurationNs"]) / 1e6 / frames
    for log in ("bench_pairs", "window_pairs"):
        with open(os.path.join(ROOT, f"profiles/sampler_stop_{log}.log")) as f:
            for r in (json.loads(ln) for ln in f if ln.startswith("{")):
                out["value"][r["build"]].append(r["line"]["value"])
    out["min_gain_pct"] = min(100 * (b / m - 1) for m, b in zip(out["value"]["main"], out["value"]["branch"]))
    out["spread_pct"] = max(100 * (max(out["value"][b]) / min(out["value"][b]) - 1) for b in ("main", "branch"))
    return out


def _format_like(text: str, value: float) -> str:
    """`value` printed the way `text` prints its number: same decimals, thin-space thousands, mantissa digits of an e-notation."""
    t = text.strip()
    if "e" in t.lower():
        mant, _, exp = t.lower().partition("e")
        frac = len(mant.split(".")[1]) if "." in mant else 0
        e = int(exp)
        out = f"{value / 10.0 ** e:.{frac}f}e{exp}"
        return out
    frac = len(t.split(".")[1]) if "." in t else 0
    out = f"{value:.{frac}f}"
    if " " in t or "\u2009" in t:                       # grouped thousands ("482 252")
        whole, dot, rest = out.partition(".")
        groups = []
        while len(whole) > 3:
            groups.insert(0, whole[-3:])
            whole = whole[:-3]
        out = " ".join([whole] + groups) + dot + rest
    return out


def fix():
    """Rewrite every checked number in DESIGN.md / README.md from the tracked files, keeping each number's printed format
    (after a new profiling round: `python tools/summarise_pmc.py rNN && python tools/check_figures.py --fix`)."""
    s = sources()
    for doc, items in checks(s):
        path = os.path.join(ROOT, doc)
        text = open(path).read()
        for pattern, want in items:
            m = re.search(pattern, text)
            if not m:
                print(f"{doc}: sentence not found: /{pattern[:90]}.../")
                continue
            piece = m.group(0)
            new, last = "", 0
            for gi, w in enumerate(want, start=1):
                a, b = m.start(gi) - m.start(0), m.end(gi) - m.start(0)
                new += piece[last:a] + _format_like(m.group(gi), w)
                last = b
            new += piece[last:]
            text = text[:m.start(0)] + new + text[m.end(0):]
        open(path, "w").write(text)


def main(verbose=True, slack=2e-4):
    s = sources()
    failures = []
    for doc, items in checks(s):
        text = open(os.path.join(ROOT, doc)).read()
        for pattern, want in items:
            m = re.search(pattern, text)
            if not m:
                failures.append(f"{doc}: sentence not found: /{pattern[:90]}.../")
                continue
            for got_text, w in zip(m.groups(), want):
                got = _num(got_text)
                tol = _digits(got_text) * 1.02 + slack * abs(w)
                ok = abs(got - w) <= tol
                if verbose:
                    print(f"{'ok ' if ok else 'BAD'} {doc:10s} quoted {got_text.strip():>12s}  tracked {w:.6g}")
                if not ok:
                    failures.append(f"{doc}: quotes {got_text.strip()} where the tracked profiles give {w:.6g} (/{pattern[:60]}.../)")
    return failures


if __name__ == "__main__":
    if "--fix" in sys.argv:
        fix()
    bad = main(verbose="--fix" not in sys.argv)
    for f in bad:
        print("MISMATCH:", f)
    sys.exit(1 if bad else 0)

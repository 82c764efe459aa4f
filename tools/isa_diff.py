#!/usr/bin/env python3
"""Build container: compare the gfx950 code of two builds of one translation unit, kernel by kernel.

    python tools/isa_diff.py old/field_mlp_nerf.o new/field_mlp_nerf.o [kernel-name-filter] [--rename PATTERN REPLACEMENT]

For every kernel in both objects: its disassembly (llvm-objdump -d --no-show-raw-insn --no-leading-addr, `//` comments
stripped) and its metadata (VGPR / AGPR / SGPR counts, spills, LDS, scratch from llvm-readelf --notes).  The 32-bit
literals of the address pairs right after s_getpc_b64 (s_add_u32 / s_addc_u32) are masked: they are pc-relative offsets
of data in the code object and move whenever anything else in the object does; the `s_nop` run behind a kernel's last
`s_endpgm` is dropped: it pads up to the next symbol's alignment and follows the kernel's place in the object.  Prints one line per kernel and exits
non-zero if any kernel in both builds differs.  The evidence that a host-side refactor left the hot kernels alone.

--rename: kernels are matched by their demangled names after re.sub(PATTERN, REPLACEMENT) on both sides, for a change that
only renames instances (a template parameter added with a default).  A new parameter `, false` at the end and a parameter
type that now depends on it:

    --rename '(nerf_fwd_kernel<\w+, \w+, \w+, \w+)(, false)?>\(.*' '\\1>'"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size")


def load(obj):
    """{kernel symbol: (instruction lines, metadata dict)} of the object's gfx950 code object."""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "k.co")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
        asm = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
        notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
    meta = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            blk = ".agpr_count:" + blk
            meta[name.group(1)] = {k: int(m.group(1)) for k in META for m in [re.search(rf"\.{k}:\s+(\d+)", blk)] if m}
    kernels, name, pcrel = {}, None, 0
    for line in asm.split("\n"):
        m = re.match(r"^<(\S+)>:$", line)
        if m:
            name = m.group(1)
            kernels[name] = []
            continue
        ins = line.split("//")[0].strip()
        if name is None or not ins or ins == "...":            # "...": zero padding up to the next kernel's alignment
            continue
        if ins.startswith("s_getpc_b64"):
            pcrel = 2
        elif pcrel and re.match(r"s_addc?_u32 ", ins):
            ins, pcrel = re.sub(r", [^,]+$", ", <pcrel>", ins), pcrel - 1
        else:
            pcrel = 0
        kernels[name].append(ins)
    # the s_nop run behind a kernel's last s_endpgm pads up to the next symbol's alignment: it depends on where the kernel lies
    # in the object (a template instance lies in a section of its own), not on its code
    for v in kernels.values():
        end = len(v)
        while end and v[end - 1] == "s_nop 0":
            end -= 1
        if end and v[end - 1] == "s_endpgm":
            del v[end:]
    return {k: (v, meta.get(k, {})) for k, v in kernels.items()}


def demangled(kernels, rename):
    """The same dict keyed by demangled name, after the --rename substitution."""
    out = {}
    for k, v in kernels.items():
        dem = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
        out[re.sub(rename[0], rename[1], dem) if rename else dem] = v
    return out


def main():
    argv, rename = sys.argv[1:], None
    if "--rename" in argv:
        i = argv.index("--rename")
        rename, argv = (argv[i + 1], argv[i + 2]), argv[:i] + argv[i + 3:]
    a, b = demangled(load(argv[0]), rename), demangled(load(argv[1]), rename)
    flt = argv[2] if len(argv) > 2 else ""
    bad = 0
    for k in sorted(set(a) | set(b)):
        if flt not in k:
            continue
        dem = k[:80]
        if k not in a or k not in b:
            print(f"{'only in ' + ('old' if k in a else 'new'):12s} {dem}")
            continue
        (ia, ma), (ib, mb) = a[k], b[k]
        same_isa, same_meta = ia == ib, ma == mb
        bad += not (same_isa and same_meta)
        n_diff = sum(x != y for x, y in zip(ia, ib)) + abs(len(ia) - len(ib))
        print(f"{'same' if same_isa and same_meta else 'DIFFERS':12s} {dem:80s} instr {len(ia):6d}/{len(ib):6d}"
              f"{'' if same_isa else f' ({n_diff} lines differ)'}{'' if same_meta else f' meta {ma} -> {mb}'}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

"""Does a hipMemsetAsync node, captured into a graph, clear its bytes on every replay?  Per size and start alignment.

DESIGN.md 4.8 "In a graph" records one captured memset (1 608 bytes) that did not.  This probe asks the runtime the same
question for the sizes of the two count clears of csrc/render_path.hip - 4 bytes per window or chunk - at every start offset
from a 16-byte boundary, with the 1 608-byte memset as the control.  It calls no library code and indexes nothing: a memset
into a torch byte buffer, two readers of that buffer, and a comparison on the host - no result of it can fault.

Per (bytes, offset) case, on one stream, captured with torch.cuda.graph:
    hipMemsetAsync(buf + LEAD + offset, 0, bytes, stream)      through ctypes, on the HIP runtime the process has loaded
    seen_copy.copy_(buf)                                        the whole buffer, guard bytes on both sides included
    torch.add(buf, 0, out=seen_kernel)                          the same through a kernel, as the library's readers are
Before each of REPLAYS replays the whole buffer is filled with 0xA5 eagerly (and both result tensors with 0x5A); after it a
reader passes when exactly the requested bytes are 0 and every other byte is 0xA5.  One line per case; exit status 0 always
(the table is the result).

    python tools/probes/graph_memset_probe.py
"""
import ctypes
import sys

import torch

SIZES = (4, 8, 12, 16, 20, 24, 28, 32, 40, 1608)
OFFSETS = (0, 4, 8, 12)
REPLAYS = 4
LEAD = 256                          # guard bytes in front; the cleared range starts LEAD + offset behind a 256-byte aligned base
TOTAL = LEAD + 16 + 1792 + 256      # the largest case and at least 256 guard bytes behind it
FILL, BLANK = 0xA5, 0x5A


def hip_runtime():
    """The libamdhip64 this process already has mapped (torch loaded it): a second copy would be another runtime."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, ("expected one HIP runtime in the process", paths)
    lib = ctypes.CDLL(paths[0])
    lib.hipMemsetAsync.restype = ctypes.c_int
    lib.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    return lib, paths[0]


def verdict(seen, start, nbytes):
    """(ok, text) for what one reader saw: the bytes of [start, start + nbytes) that are 0, the others that are not FILL."""
    inside = seen[start:start + nbytes]
    zeros = int((inside == 0).sum())
    outside = torch.cat([seen[:start], seen[start + nbytes:]])
    hit = int((outside != FILL).sum())
    ok = zeros == nbytes and hit == 0
    return ok, "ok" if ok else f"FAIL({zeros}/{nbytes} zero, {hit} guard bytes hit)"


def main():
    assert torch.cuda.is_available(), "needs a device"
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    torch.zeros(1, device=dev)
    lib, path = hip_runtime()
    buf = torch.empty(TOTAL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0, buf.data_ptr()
    seen_copy, seen_kernel = torch.empty_like(buf), torch.empty_like(buf)
    print(f"# graph_memset_probe: torch {torch.__version__}, hip {torch.version.hip}, {torch.cuda.get_device_name(0)}")
    print(f"# runtime {path}")
    print(f"# buffer of {TOTAL} bytes, base % 256 == 0, cleared range starts at {LEAD} + offset; {REPLAYS} replays per case,"
          f" buffer = 0x{FILL:02X} before each")
    print("# bytes offset | reader copy_: replay 0 1 2 3 | reader kernel: replay 0 1 2 3 | verdict")
    failed = []
    for nbytes in SIZES:
        for off in OFFSETS:
            start = LEAD + off
            assert start + nbytes + 256 <= TOTAL
            buf.fill_(FILL)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                rc = lib.hipMemsetAsync(buf.data_ptr() + start, 0, nbytes, torch.cuda.current_stream().cuda_stream)
                seen_copy.copy_(buf)
                torch.add(buf, 0, out=seen_kernel)
            assert rc == 0, ("hipMemsetAsync under capture", rc)
            words, good = {"copy": [], "kernel": []}, True
            for _ in range(REPLAYS):
                buf.fill_(FILL)
                seen_copy.fill_(BLANK)
                seen_kernel.fill_(BLANK)
                torch.cuda.synchronize()
                graph.replay()
                torch.cuda.synchronize()
                for name, seen in (("copy", seen_copy), ("kernel", seen_kernel)):
                    ok, text = verdict(seen.cpu(), start, nbytes)
                    words[name].append(text)
                    good &= ok
            if not good:
                failed.append((nbytes, off))
            print(f"bytes={nbytes:5d} offset={off:2d} | copy_: {' '.join(words['copy'])} | kernel: {' '.join(words['kernel'])} | "
                  f"{'CLEARED' if good else 'NOT CLEARED'}")
            del graph
    print(f"# cases not cleared on every replay: {failed if failed else 'none'}")
    control = [c for c in failed if c[0] == 1608]
    print(f"# control (1608 bytes): {'fails at offsets ' + str([c[1] for c in control]) if control else 'does not fail'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

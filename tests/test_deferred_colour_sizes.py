"""CPU: mi_render_deferred_colour_extra_bytes, the size of the buffer the fine pass's deferred colour branch needs behind
mi_render_workspace_bytes - one chunk's worst-case live list (a 1 KiB H8 row and an int32 index per point) and one count
per chunk.  No GPU, no compute call."""
from mirender import _lib as binding

CHUNK = 1 << 22          # kColourChunkRows of csrc/render_path.hip


def _lib():
    return binding.load()


def test_extra_bytes_hold_one_chunks_worst_case():
    lib = _lib()
    for n, nc, nf in ((1, 16, 32), (257, 16, 32), (1000, 64, 128), (640000, 64, 128), (3, 5, 1)):
        rows = min(n * (nc + nf), CHUNK)
        got = lib.mi_render_deferred_colour_extra_bytes(n, nc, nf)
        assert got >= rows * 1028, (n, nc, nf)
        assert got <= (rows + 64) * 1028 + 4 * (n + 64), (n, nc, nf)       # and not much more: rows, indices, counts
        assert got % 256 == 0


def test_extra_bytes_are_zero_without_a_fine_pass_of_its_own():
    lib = _lib()
    assert lib.mi_render_deferred_colour_extra_bytes(1000, 64, 0) == 0
    assert lib.mi_render_deferred_colour_extra_bytes(0, 64, 128) == 0


def test_extra_bytes_follow_the_chunk_hook():
    lib = _lib()
    try:
        lib.mi_render_set_colour_chunk_rows(4096)
        got = lib.mi_render_deferred_colour_extra_bytes(257, 16, 32)
        assert 4200 * 1028 > got >= 4096 * 1028               # chunks of 85 whole rays of 48 samples
        lib.mi_render_set_colour_chunk_rows(10)                # below one ray: one ray per chunk
        assert lib.mi_render_deferred_colour_extra_bytes(257, 16, 32) >= 48 * 1028
    finally:
        lib.mi_render_set_colour_chunk_rows(0)
    assert lib.mi_render_deferred_colour_extra_bytes(257, 16, 32) >= 257 * 48 * 1028


def test_kinds_with_a_deferred_colour_branch():
    lib = _lib()
    assert [lib.mi_field_has_deferred_colour(k) for k in range(5)] == [1, 0, 0, 0, 1]      # NeRF and TinyNeRF
    assert lib.mi_field_has_deferred_colour(0x100 + 2 * 6) == 0 and lib.mi_field_has_deferred_colour(99) == -1

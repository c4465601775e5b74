"""bg_bgzf_deflate[_dev] without a GPU: the argument checks that return before a device is touched (those of bg_bgzf_frame), the
sizing call (the stored bound: `bam.framed_bytes`), and `bam.virtual_offsets` on a hand-written block table."""
import ctypes as C

import numpy as np

from rust_bio_amd import _lib, bam

INVALID_ARG = -1
FAKE = np.zeros(4096, dtype=np.uint8)  # stands for a ctx or any buffer: a refused call and a sizing call dereference none of them
P = FAKE.ctypes.data


def calls():
    lib = _lib.lib()
    for dev in (False, True):
        fn = lib.bg_bgzf_deflate_dev if dev else lib.bg_bgzf_deflate
        tail = (0,) if dev else ()

        def call(ctx=P, src=P, in_bytes=100, flags=0, out=None, out_cap=0, block_off=None, n=None, fn=fn, tail=tail):
            return fn(ctx, src, in_bytes, flags, out, out_cap, block_off, n, *tail)
        yield dev, call


def test_refusals_before_a_device_is_touched():
    for dev, call in calls():
        n = C.c_uint64(77)
        ref = C.byref(n)
        assert call(ctx=None, n=ref) == INVALID_ARG, dev
        assert call(n=None) == INVALID_ARG, dev
        for flags in (2, 4, 3, 1 << 31):
            assert call(flags=flags, n=ref) == INVALID_ARG, (dev, flags)
        assert call(src=None, n=ref) == INVALID_ARG, dev
        assert call(out=None, out_cap=5, n=ref) == INVALID_ARG, dev  # a capacity without a buffer
        assert n.value == 77


def test_sizing_call_is_the_stored_bound():
    for dev, call in calls():
        for in_bytes in (0, 1, 65279, 65280, 65281, 2 * 65280 + 77, 385_000_000):
            for flags in (0, bam.BGZF_EOF):
                n = C.c_uint64(0)
                assert call(src=P if in_bytes else None, in_bytes=in_bytes, flags=flags, n=C.byref(n)) == 0
                assert n.value == bam.framed_bytes(in_bytes, flags), (dev, in_bytes, flags)

    class Ctx:  # the binding's sizing call
        h = P
    assert bam.bgzf_deflate_dev(P, 65281, 0, 0, bam.BGZF_EOF, ctx=Ctx) == 65281 + 62 + 28


def test_virtual_offsets_on_a_hand_written_table():
    block_off = np.array([0, 1000, 1500, 61000, 61030], dtype=np.uint64)  # four blocks
    offs = [0, 5, 65279, 65280, 65281, 2 * 65280, 3 * 65280 + 76]
    got = bam.virtual_offsets(offs, block_off, base=300)
    want = [(300 << 16) | 0, (300 << 16) | 5, (300 << 16) | 65279, (1300 << 16) | 0, (1300 << 16) | 1, (1800 << 16) | 0, (61300 << 16) | 76]
    assert got.dtype == np.uint64 and got.tolist() == want
    assert bam.virtual_offsets([], block_off).tolist() == []
    # a stream of stored blocks has bam.virtual_offset's closed form
    stored = np.arange(5, dtype=np.uint64) * np.uint64(65311)
    assert bam.virtual_offsets(offs, stored, base=100).tolist() == [bam.virtual_offset(o, 100) for o in offs]
    # beyond 2^32: a file offset has 48 bits
    assert bam.virtual_offsets([65280], np.array([0, 1 << 40], dtype=np.uint64), base=1 << 41).tolist() == [((1 << 41) + (1 << 40)) << 16]

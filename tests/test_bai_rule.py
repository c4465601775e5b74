"""The BAI rule of include/biogpu.h without a GPU: tests/bai_oracle.py against a hand-computed index written out as bytes,
its reader and `query` against brute force on random sorted record sets (the records inside the chunks a reader visits for a
region are a superset of those that overlap it), the case builders' own claims, and the argument checks of bg_bam_index[_dev]
that return before a device is touched."""
import ctypes as C
import struct

import numpy as np

import bai_cases as bc
import bai_oracle as ba
import bam_oracle as bo
from rust_bio_amd import _lib, bam

FAKE = np.zeros(4096, dtype=np.uint8)  # stands for a ctx or any buffer: a refused call dereferences none of them
P = FAKE.ctypes.data


def v(o):
    """the virtual offset of byte o (< 65 280) of a stored stream behind a header of 1000 bytes: 1000 << 16 | o"""
    return bytes([o & 0xFF, o >> 8, 0xE8, 0x03, 0, 0, 0, 0])


def test_known_answer():
    contigs = [(b"c0", 0, 100_000), (b"c1", 100_001, 50_000)]
    slots = [bc.rec(b"a", b"c0", 100, b"10M", contigs=contigs),      # 57 bytes at 0: [100, 110), bin 4681
             bc.rec(b"b", b"c0", 16380, b"10M", contigs=contigs),    # 57 bytes at 57: [16380, 16390) crosses 2^14, bin 585
             bc.rec(b"c", b"c1", 0, b"*", 10, flag=4, contigs=contigs)]  # 53 bytes at 114: an unmapped mate at c1:1, [0, 1), bin 4681
    assert [len(s) for s in slots] == [57, 57, 53]
    want = (b"BAI\x01" + b"\x02\0\0\0" +
            # c0: two bins and the pseudo-bin
            b"\x03\0\0\0" +
            b"\x49\x02\0\0" + b"\x01\0\0\0" + v(57) + v(114) +          # bin 585: record b
            b"\x49\x12\0\0" + b"\x01\0\0\0" + v(0) + v(57) +            # bin 4681: record a
            b"\x4a\x92\0\0" + b"\x02\0\0\0" + v(0) + v(114) + b"\x02\0\0\0\0\0\0\0" + b"\0\0\0\0\0\0\0\0" +  # 37450: all of c0; 2 mapped, 0 unmapped
            b"\x02\0\0\0" + v(0) + v(57) +                              # windows 0 and 1: the first record ending behind 0 / behind 16384
            # c1: one bin and the pseudo-bin
            b"\x02\0\0\0" +
            b"\x49\x12\0\0" + b"\x01\0\0\0" + v(114) + v(167) +
            b"\x4a\x92\0\0" + b"\x02\0\0\0" + v(114) + v(167) + b"\0\0\0\0\0\0\0\0" + b"\x01\0\0\0\0\0\0\0" +
            b"\x01\0\0\0" + v(114) +
            b"\0\0\0\0\0\0\0\0")                                        # n_no_coor
    assert ba.build(slots, contigs, ba.stored_voff(1000)) == want
    refs, n_no_coor = ba.parse(want)
    assert n_no_coor == 0 and sorted(refs[0]["bins"]) == [585, 4681] and refs[1]["meta"][2:] == (0, 1)
    assert ba.query((refs, 0), 0, 16384, 20000) == [((1000 << 16) | 57, (1000 << 16) | 114)]
    # (an index promises a superset: [120, 16380) overlaps neither record, and bins 585 and 4681 are still visited)
    assert ba.query((refs, 0), 0, 120, 16380) == [((1000 << 16) | 0, (1000 << 16) | 57), ((1000 << 16) | 57, (1000 << 16) | 114)]
    assert ba.query((refs, 0), 0, 2**17, 2**17 + 1) == [] and ba.query((refs, 0), 1, 5, 5) == []


def test_voff_forms_agree_with_the_binding():
    for o in (0, 1, 65279, 65280, 65281, 3 * 65280, 385_000_000):
        assert ba.stored_voff(77)(o) == bam.virtual_offset(o, 77)
    table = np.array([0, 1000, 1500, 61000], dtype=np.uint64)
    offs = [0, 65279, 65280, 2 * 65280 + 5, 3 * 65280]
    assert [ba.table_voff(table, 9)(o) for o in offs] == bam.virtual_offsets(offs, table, base=9).tolist()


def stream_offset(voff, base):
    block, within = divmod((voff >> 16) - base, bo.PAYLOAD + 31)
    assert within == 0
    return block * bo.PAYLOAD + (voff & 0xFFFF)


def test_query_visits_every_overlapping_record():
    rng = np.random.default_rng(11)
    contigs = [(b"c0", 0, 2**29), (b"c1", 2**29 + 1, 300_000), (b"c2", 2**29 + 300_002, 2**22)]
    for trial in range(3):
        slots = bc.random_records(rng, 700, contigs, n_unplaced=5, empty_every=50)
        base = 500 + trial
        bai = ba.build(slots, contigs, ba.stored_voff(base))
        parsed = ba.parse(bai)
        off = bo.offsets(slots)
        recs = [(int(off[i]), ba.fields(s, contigs)) for i, s in enumerate(slots) if s]
        starts = {o for o, _ in recs} | {int(off[-1])}
        assert parsed[1] == sum(1 for _, f in recs if f[0] < 0)
        for r, (_, _, ln) in enumerate(contigs):
            mine = [(o, f) for o, f in recs if f[0] == r]
            assert parsed[0][r]["meta"][2:] == (sum(1 for _, f in mine if not f[3]), sum(1 for _, f in mine if f[3]))
            picks = [int(x) for x in rng.integers(0, ln, 30)] + [f[1] for _, f in mine[::25]]
            regions = [(0, ln), (16384, 16385), (16383, 16384)] + [(p, min(p + int(w), ln)) for p in picks for w in (1, 100, 20_000, 2**21)]
            for beg, end in regions:
                chunks = [(stream_offset(b, base), stream_offset(e, base)) for b, e in ba.query(parsed, r, beg, end)]
                assert all(b in starts and e in starts for b, e in chunks)  # no chunk begins or ends inside a record
                for o, f in mine:
                    if f[1] < end and f[2] > beg:
                        assert any(b <= o < e for b, e in chunks), (trial, r, beg, end, f)


def test_cases_hold_what_they_claim():
    S = bc.shapes()
    off = bo.offsets(S["block edges, a multiple of 65 280"][0]).tolist()
    assert 0 in off and 65279 in off and 2 * 65280 in off and off[-1] == 3 * 65280
    assert any(a < 65280 < b for a, b in zip(off, off[1:]))  # a record straddles two blocks
    refs, _ = ba.parse(ba.build(*S["crossing 2^14 .. 2^26"], ba.stored_voff()))
    levels = {sum(b >= first for first in (1, 9, 73, 585, 4681)) for b in refs[0]["bins"]}
    assert levels == {0, 1, 2, 3, 4, 5}
    refs, _ = ba.parse(ba.build(*S["a bin interrupted and resumed"], ba.stored_voff()))
    assert len(refs[1]["bins"][4681]) == 4 and len(refs[1]["bins"][585]) == 3
    refs, _ = ba.parse(ba.build(*S["end exactly 16384"], ba.stored_voff()))
    assert len(refs[1]["intv"]) == 1
    refs, _ = ba.parse(ba.build(*S["a record ending at 2^29"], ba.stored_voff()))
    assert len(refs[0]["intv"]) == 2**15
    refs, _ = ba.parse(ba.build(*S["a gap of 5 windows"], ba.stored_voff()))
    assert refs[1]["intv"][1:6] == [refs[1]["intv"][6]] * 5 and refs[1]["intv"][0] != refs[1]["intv"][6]
    assert len(ba.build([], bc.CONTIGS, ba.stored_voff())) == 8 + 8 * 3 + 8


def test_refusals_before_a_device_is_touched():
    lib = _lib.lib()
    for dev in (False, True):
        fn = lib.bg_bam_index_dev if dev else lib.bg_bam_index
        tail = (0,) if dev else ()

        def call(ctx=P, n=3, recs=P, off=P, contigs=P, n_contigs=2, table=None, base=0, out=None, cap=0, total=None, bad=None):
            return fn(ctx, n, recs, off, contigs, n_contigs, table, base, out, cap, total, bad, *tail)
        total, bad = C.c_uint64(77), C.c_uint64(5)
        t, b = C.byref(total), C.byref(bad)
        assert call(ctx=None, total=t, bad=b) == -1 and bad.value == 2**64 - 1
        assert call(total=None, bad=b) == -1
        assert call(recs=None, total=t, bad=b) == -1 and call(off=None, total=t) == -1 and call(contigs=None, total=t) == -1
        assert call(out=None, cap=5, total=t, bad=b) == -1  # a capacity without a buffer
        assert total.value == 77
        assert call(n=2**32 - 1, total=t, bad=b) == -8  # TOO_LARGE

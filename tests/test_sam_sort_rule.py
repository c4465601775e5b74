"""Duplicate marking, sort keys and the sort without a GPU: hand-written known answers for every clause of the duplicate rule of
include/biogpu.h — the expected bytes are literals here, not computed — against its CPU statement (tests/sam_sort_oracle.py);
the text-only check of a sorted body on lines written by hand; every refusal of the new host entry points that is decided
before a device is touched; and bg_sam_header_so against bg_sam_header."""
import ctypes as C

import numpy as np
import pytest

import sam_oracle as so
import sam_sort_oracle as sso
from rust_bio_amd import _lib, sam
from sam_sort_cases import CONTIGS, PHRED, arrays, make_hit

INVALID_ARG, OPS_CAP = -1, -9
L = 24


def read(q, name=b"r"):
    """a read of L bases, all of quality q; q may also be the quality bytes themselves"""
    return name, b"ACGT" * (L // 4), bytes([PHRED + q]) * L if isinstance(q, int) else bytes(PHRED + v for v in q)


def fwd(start, end=None):
    return make_hit(40, 0, start, end or start + L, 0, L, L)


def rev(end, start=None):
    return make_hit(40, 1, start if start is not None else end - L, end, 0, L, L)


def rule(reads, hits, flags=0, K=1, min_qual=15):
    fq, h, strand = arrays(reads, hits)
    dup, counts = sso.markdup(CONTIGS, fq, h, strand, flags, K, PHRED, min_qual)
    return dup.tobytes(), counts


def test_two_forward_reads_with_one_start_and_different_ends():
    assert rule([read(30), read(20)], [fwd(100, 124), fwd(100, 120)]) == (b"\x00\x01", [2, 1, 0, 0])


def test_two_reverse_reads_with_one_end_and_different_starts():
    assert rule([read(20), read(30)], [rev(150, 100), rev(150, 120)]) == (b"\x01\x00", [2, 1, 0, 0])


def test_the_same_coordinate_on_opposite_strands_is_no_duplicate():
    # forward u5 = 100; reverse u5 = ref_end - 1 = 100
    assert rule([read(30), read(20)], [fwd(100), rev(101, 80)]) == (b"\x00\x00", [2, 0, 0, 0])


def test_a_score_tie_keeps_the_smaller_index():
    assert rule([read(20), read(20), read(20)], [fwd(100), fwd(100), fwd(100)]) == (b"\x00\x01\x01", [3, 2, 0, 0])


def test_min_qual_decides_the_winner():
    reads = [read([14] * 24), read([30] * 10 + [2] * 14)]  # sums 336 and 328; above 15: 0 and 300
    assert rule(reads, [fwd(100), fwd(100)], min_qual=15) == (b"\x01\x00", [2, 1, 0, 0])
    assert rule(reads, [fwd(100), fwd(100)], min_qual=0) == (b"\x00\x01", [2, 1, 0, 0])


def test_the_clip_terms_move_the_end():
    # forward, 3 bases clipped at the read's start: u5 = 103 - 3; reverse, 2 clipped at its end: u5 = 149 + 2 = 152 - 1
    clipped_f = make_hit(40, 0, 103, 124, 3, L, L)
    clipped_r = make_hit(40, 1, 120, 150, 0, L - 2, L)
    assert rule([read(30), read(20), read(30), read(20)], [fwd(100), clipped_f, rev(152), clipped_r]) == (b"\x00\x01\x00\x01", [4, 2, 0, 0])
    # ... saturating at 0
    assert rule([read(30), read(20)], [fwd(0), make_hit(40, 0, 1, 20, 3, L, L)]) == (b"\x00\x01", [2, 1, 0, 0])


def test_pairs_with_equal_ends_but_another_mate_as_lo_are_no_duplicates():
    reads = [read(30), read(30), read(30), read(30), read(20), read(20)]
    hits = [fwd(100), rev(300), rev(300), fwd(100), fwd(100), rev(300)]  # pair 1 has its mates swapped; pair 2 repeats pair 0
    assert rule(reads, hits, so.PAIRED) == (b"\x00\x00\x00\x00\x01\x01", [6, 2, 1, 0])


def test_a_pairs_score_is_the_sum_of_its_mates():
    reads = [read(40), read(16), read(30), read(30)]  # 56 L against 60 L
    assert rule(reads, [fwd(100), rev(300), fwd(100), rev(300)], so.PAIRED) == (b"\x01\x01\x00\x00", [4, 2, 1, 0])


def test_a_fragment_on_a_pairs_hi_end_is_flagged():
    reads = [read(20), read(20), read(40), read(40)]
    assert rule(reads, [fwd(100), rev(300), None, rev(300, 250)], so.PAIRED) == (b"\x00\x00\x00\x01", [3, 1, 0, 1])
    # ... also when the pair itself is a duplicate
    reads = [read(30), read(30), read(20), read(20), read(40), read(40)]
    hits = [fwd(100), rev(300), fwd(100), rev(300), fwd(100), None]
    assert rule(reads, hits, so.PAIRED) == (b"\x00\x00\x01\x01\x01\x00", [5, 3, 1, 1])


def test_a_fragment_group_without_a_pair():
    reads = [read(20), read(40), read(40), read(30)]
    assert rule(reads, [fwd(500), None, None, fwd(500)], so.PAIRED) == (b"\x01\x00\x00\x00", [2, 1, 0, 0])


def test_an_unplaced_read_between_duplicates():
    assert rule([read(30), read(40), read(20)], [fwd(100), None, fwd(100)]) == (b"\x00\x00\x01", [2, 1, 0, 0])
    reads = [read(30)] * 6
    assert rule(reads, [fwd(100), rev(300), None, None, fwd(100), rev(300)], so.PAIRED) == (b"\x00\x00\x00\x00\x01\x01", [4, 2, 1, 0])


def test_a_hit_across_a_contig_end_has_no_end():
    assert rule([read(30), read(20), read(10)], [fwd(1990, 2010), fwd(1990, 2010), fwd(1999, 2001)]) == (b"\x00\x00\x00", [0, 0, 0, 0])


def test_two_contigs_with_equal_offsets():
    assert rule([read(30), read(20), read(20)], [fwd(100), fwd(2100), fwd(4100)]) == (b"\x00\x00\x00", [3, 0, 0, 0])


def test_secondary_slots_take_no_part():
    # K = 2: read 1's secondary slot sits on read 0's end
    assert rule([read(20), read(30)], [fwd(100), None, fwd(700), fwd(100)], K=2) == (b"\x00\x00", [2, 0, 0, 0])


def test_keys_known_answers():
    fq, h, strand = arrays([read(30)] * 4, [fwd(2100), None, None, None])
    top = 2**64 - 1
    assert sso.sort_keys(CONTIGS, h, strand, so.PAIRED).tolist() == [2100, 2100, top, top]
    assert sso.sort_keys(CONTIGS, h, strand, 0).tolist() == [2100, top, top, top]
    fq, h, strand = arrays([read(30)] * 2, [fwd(100), fwd(50), fwd(1990, 2010), fwd(70)])
    assert sso.sort_keys(CONTIGS, h, strand, so.SECONDARY, 2).tolist() == [100, 50, top, top]
    assert sso.sort_keys(CONTIGS, h, strand, 0, 2).tolist() == [100, top, top, top]


def test_sort_and_the_text_only_check():
    lines = [b"a\t0\tchrA\t7\n", b"b\t4\t*\t0\n", b"c\t16\tc|3\t1\n", b"d\t0\tchrA\t7\n", b"e\t0\tchrA\t3\n", b""]
    perm, off, text = sso.sort([6, 2**64 - 1, 4000, 6, 2, 2**64 - 1], lines)
    assert perm.tolist() == [4, 0, 3, 2, 1, 5] and off.tolist() == [0, 11, 22, 33, 44, 52, 52]
    assert text == b"e\t0\tchrA\t3\na\t0\tchrA\t7\nd\t0\tchrA\t7\nc\t16\tc|3\t1\nb\t4\t*\t0\n"
    names = [c[0] for c in CONTIGS]
    sso.check_sorted_text(names, b"".join(lines), text)
    with pytest.raises(AssertionError):  # equal places out of their input order
        sso.check_sorted_text(names, b"".join(lines), text.replace(b"a\t0\tchrA\t7\nd\t0\tchrA\t7\n", b"d\t0\tchrA\t7\na\t0\tchrA\t7\n"))
    with pytest.raises(AssertionError):
        sso.check_sorted_text(names, b"".join(lines), b"".join(lines))
    assert sso.add_dup_flag(lines, [1, 1, 1, 0, 0, 1])[:3] == [b"a\t1024\tchrA\t7\n", b"b\t4\t*\t0\n", b"c\t1040\tc|3\t1\n"]


# ---- refusals that are decided before a device is touched --------------------------------------------------------------------
FAKE = np.zeros(4096, dtype=np.uint8)  # stands for a ctx, an index or any buffer: a refused call dereferences none of them
P = FAKE.ctypes.data


def md_params(flags=0, K=1):
    p = np.zeros(1, dtype=_lib.MARKDUP_PARAMS_DTYPE)
    p[0] = (flags, K, 33, 15)
    return p


def test_markdup_refusals():
    lib = _lib.lib()
    counts = np.full(4, 77, dtype=np.uint64)
    for dev in (False, True):
        fn = lib.bg_sam_markdup_dev if dev else lib.bg_sam_markdup
        tail = (0,) if dev else ()

        def call(ctx=P, mp=md_params(), n=4, contigs=P, n_contigs=3, hits=P, strand=P, recs=P, qual=P, dup=P, cnt=counts.ctypes.data):
            return fn(ctx, mp.ctypes.data if mp is not None else None, n, contigs, n_contigs, hits, strand, recs, qual, dup, cnt, *tail)
        bad = [dict(ctx=None), dict(mp=None), dict(cnt=None), dict(mp=md_params(2)), dict(mp=md_params(4)), dict(mp=md_params(0, 0)),
               dict(mp=md_params(0, 9)), dict(n_contigs=0), dict(mp=md_params(1), n=3), dict(mp=md_params(1, 2)), dict(contigs=None),
               dict(hits=None), dict(strand=None), dict(recs=None), dict(qual=None), dict(dup=None)]
        for kw in bad:
            assert call(**kw) == INVALID_ARG, (dev, kw)
        # no reads: nothing to do, the counts are zero
        assert call(n=0, contigs=None, hits=None, strand=None, recs=None, qual=None, dup=None) == 0 and (counts == 0).all()
        counts[:] = 77


def test_sort_keys_refusals():
    lib = _lib.lib()
    for dev in (False, True):
        fn = lib.bg_sam_sort_keys_dev if dev else lib.bg_sam_sort_keys
        tail = (0,) if dev else ()

        def call(ctx=P, sp=_lib.SAM_PARAMS(0, 1), n=4, contigs=P, n_contigs=3, hits=P, strand=P, key=P):
            return fn(ctx, C.byref(sp) if sp is not None else None, n, contigs, n_contigs, hits, strand, key, *tail)
        bad = [dict(ctx=None), dict(sp=None), dict(sp=_lib.SAM_PARAMS(16, 1)), dict(sp=_lib.SAM_PARAMS(0, 0)), dict(sp=_lib.SAM_PARAMS(0, 9)),
               dict(n_contigs=0), dict(sp=_lib.SAM_PARAMS(1, 1), n=3), dict(sp=_lib.SAM_PARAMS(1, 2)), dict(contigs=None), dict(hits=None),
               dict(strand=None), dict(key=None)]
        for kw in bad:
            assert call(**kw) == INVALID_ARG, (dev, kw)
        assert call(n=0, contigs=None, hits=None, strand=None, key=None) == 0


def test_sort_refusals():
    lib = _lib.lib()
    out = np.full(64, 0x7e, dtype=np.uint8)
    out_off = np.full(5, 77, dtype=np.uint64)
    for dev in (False, True):
        fn = lib.bg_sam_sort_dev if dev else lib.bg_sam_sort
        tail = (0,) if dev else ()

        def call(ctx=P, n=4, key=P, src=P, in_off=P, in_bytes=40, dst=out.ctypes.data, cap=64, o_off=out_off.ctypes.data, perm=P):
            return fn(ctx, n, key, src, in_off, in_bytes, dst, cap, o_off, perm, *tail)
        bad = [dict(ctx=None), dict(o_off=None), dict(perm=None), dict(key=None), dict(in_off=None), dict(src=None), dict(dst=None)]
        for kw in bad:
            assert call(**kw) == INVALID_ARG, (dev, kw)
        assert call(cap=39) == OPS_CAP and (out == 0x7e).all() and (out_off == 77).all()
    # no records: the host flavour has nothing to ask a device
    assert lib.bg_sam_sort(P, 0, None, None, None, 0, None, 0, out_off.ctypes.data, P) == 0 and out_off[0] == 0


def test_emit_dup_refusals():
    lib = _lib.lib()
    total = C.c_uint64(5)
    for dev in (False, True):
        fn = lib.bg_sam_emit_dup_batch_dev if dev else lib.bg_sam_emit_dup_batch
        tail = (0,) if dev else ()

        def call(fm=P, sp=_lib.SAM_PARAMS(0, 1), n=4, n_contigs=3, bufs=(P,) * 9, pairs=None, dup=P, out=None, cap=0, off=P, tot=C.byref(total)):
            return fn(fm, C.byref(sp) if sp is not None else None, n, bufs[0], n_contigs, *bufs[1:], None, pairs, dup, out, cap, off, tot, *tail)
        bad = [dict(fm=None), dict(sp=None), dict(off=None), dict(tot=None), dict(sp=_lib.SAM_PARAMS(16, 1)), dict(sp=_lib.SAM_PARAMS(0, 0)),
               dict(sp=_lib.SAM_PARAMS(0, 9)), dict(n_contigs=0), dict(sp=_lib.SAM_PARAMS(1, 1)), dict(sp=_lib.SAM_PARAMS(1, 1), n=3, pairs=P),
               dict(sp=_lib.SAM_PARAMS(1, 2), pairs=P), dict(cap=8)]
        bad += [dict(bufs=(P,) * i + (None,) + (P,) * (8 - i)) for i in range(9)]
        for kw in bad:
            assert call(**kw) == INVALID_ARG, (dev, kw)


def test_header_so_against_header():
    lib = _lib.lib()
    for entries in ([(b"chrA", 0, 1999), (b"chr_B.1", 2000, 1999)], [(b"x", 0, 5)], [(b"ctg%d" % c, 1000 * c, 999 - c) for c in range(300)]):
        table = sam.Contigs(entries)
        plain = sam.header(table)
        assert plain == so.header(entries) == sam.header(table, sam.SAM_SO_UNSORTED)
        want = plain.replace(b"SO:unsorted", b"SO:coordinate")
        assert want != plain and want.startswith(b"@HD\tVN:1.6\tSO:coordinate\n@SQ\t")
        assert sam.header(table, sam.SAM_SO_COORDINATE) == want
        # bg_sam_header itself is unchanged; an exact-fit cap writes everything, a cap one byte short nothing
        n = C.c_uint64(0)
        buf = np.full(len(want) + 1, 0x7e, dtype=np.uint8)
        args = (table.table.ctypes.data, len(table), table.names.ctypes.data)
        assert lib.bg_sam_header(*args, buf.ctypes.data, len(plain), C.byref(n)) == 0 and buf[:len(plain)].tobytes() == plain
        buf[:] = 0x7e
        assert lib.bg_sam_header_so(*args, 1, buf.ctypes.data, len(want), C.byref(n)) == 0 and n.value == len(want)
        assert buf[:len(want)].tobytes() == want and buf[len(want)] == 0x7e
        buf[:] = 0x7e
        assert lib.bg_sam_header_so(*args, 1, buf.ctypes.data, len(want) - 1, C.byref(n)) == OPS_CAP and n.value == len(want)
        assert (buf == 0x7e).all()
        for order in (2, -1, 7):
            assert lib.bg_sam_header_so(*args, order, buf.ctypes.data, len(want), C.byref(n)) == INVALID_ARG
        assert lib.bg_sam_header_so(*args, 1, buf.ctypes.data, len(want), None) == INVALID_ARG

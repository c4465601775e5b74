"""Sorted record sets for the BAI tests (tests/test_bai_rule.py, tests/test_bam_index_host_bodies.py, tests/test_gpu_bam_index.py):
BAM records synthesised with bam_oracle.record from hand-made SAM lines, so no mapper runs.  A case is (slots, contigs): slots
the record of every slot (b"": an empty slot), contigs [(name, start, len)]."""
import numpy as np

import bam_oracle as bo

PAYLOAD = bo.PAYLOAD
INVALID_ARG, UNSUPPORTED, OPS_CAP = -1, -11, -9
CONTIGS = [(b"c0", 0, 2**29), (b"c1", 2**29 + 1, 300_000), (b"c2", 2**29 + 300_002, 2**27 + 5000)]
BASES = b"ACGT"


def line(name, rname, pos0, cigar, l_seq=None, flag=0):
    """one SAM line at 0-based pos0 (None: unplaced); l_seq defaults to what the CIGAR asks for"""
    if l_seq is None:
        l_seq = sum(w >> 4 for w in bo.cigar_words(cigar) if bo.CIGAR_OPS[w & 15:(w & 15) + 1] in b"MIS=X") or 4
    seq = (BASES * (l_seq // 4 + 1))[:l_seq]
    pos1 = 0 if pos0 is None else pos0 + 1
    return b"\t".join([name, b"%d" % flag, rname, b"%d" % pos1, b"30", cigar, b"*", b"0", b"0", seq, b"*"]) + b"\n"


def rec(name, rname, pos0, cigar, l_seq=None, flag=0, contigs=CONTIGS):
    return bo.record(line(name, rname, pos0, cigar, l_seq, flag), contigs)


def unplaced(name, l_seq=8):
    return rec(name, b"*", None, b"*", l_seq, flag=4)


def sized(size, rname, pos0, contigs=CONTIGS):
    """a record of exactly `size` bytes (60 .. 6299): 8M<l - 8>S, the name as long as it takes"""
    rest = size - 36 - 8 - 2  # bases and qualities, with a name of one byte
    l_seq = min(rest * 2 // 3, 4000)
    while (l_seq + 1) // 2 + l_seq > rest:
        l_seq -= 1
    q = 1 + rest - ((l_seq + 1) // 2 + l_seq)
    assert l_seq > 8 and 1 <= q <= 254, (size, l_seq, q)
    r = rec(b"q" * q, rname, pos0, b"8M%dS" % (l_seq - 8), l_seq, contigs=contigs)
    assert len(r) == size, (len(r), size)
    return r


def fill(slots, target, rname, pos0, contigs=CONTIGS):
    """appends records on `rname` from pos0 on (one base further each) until the stream is exactly `target` bytes long;
    returns the next free position"""
    at = sum(len(s) for s in slots)
    while at < target:
        left = target - at
        size = left if left <= 5000 else 3000
        slots.append(sized(size, rname, pos0, contigs))
        at += size
        pos0 += 1
    assert at == target
    return pos0


def shapes():
    """name -> (slots, contigs)"""
    S = {}
    S["no slots"] = ([], CONTIGS)
    S["no contigs, no slots"] = ([], [])
    S["only empty slots"] = ([b"", b"", b""], CONTIGS)
    S["only unplaced"] = ([unplaced(b"u%d" % i) for i in range(5)], CONTIGS)
    S["a single record"] = ([rec(b"one", b"c1", 1234, b"20M")], CONTIGS)
    S["pos 0"] = ([rec(b"z", b"c0", 0, b"10M"), rec(b"y", b"c0", 0, b"5M"), rec(b"x", b"c1", 0, b"1M")], CONTIGS)
    S["end exactly 16384"] = ([rec(b"e", b"c1", 16384 - 50, b"50M")], CONTIGS)
    S["end 16385"] = ([rec(b"e", b"c1", 16384 - 50, b"51M")], CONTIGS)
    S["pos -1 on a contig"] = ([rec(b"m", b"c1", -1, b"*", 6, flag=4), rec(b"n", b"c1", 7, b"3M")], CONTIGS)
    cross = []
    for k in (14, 17, 20, 23, 26):  # a record across each boundary, one in front of it and one behind: bins of every level
        cross += [rec(b"f%d" % k, b"c0", 2**k - 40, b"30M"), rec(b"x%d" % k, b"c0", 2**k - 10, b"20M"), rec(b"b%d" % k, b"c0", 2**k + 1, b"20M")]
    cross.append(rec(b"top", b"c0", 2**26 * 3 - 5, b"10M"))  # 2^26 again: bin 0
    S["crossing 2^14 .. 2^26"] = (cross, CONTIGS)
    span = [rec(b"long", b"c2", 20_000, b"10M%dN10M" % (40 * 16384))]  # N over 40 windows, then short records inside them
    span += [rec(b"s%d" % i, b"c2", 20_000 + 16384 * i + 77 * i, b"25M") for i in range(1, 40, 3)]
    span += [rec(b"after", b"c2", 20_000 + 41 * 16384, b"25M")]
    S["an N over 40 windows"] = (span, CONTIGS)
    S["a gap of 5 windows"] = ([rec(b"g0", b"c1", 100, b"30M"), rec(b"g1", b"c1", 16384 * 6 + 3, b"30M"), rec(b"g2", b"c1", 16384 * 6 + 9, b"30M")], CONTIGS)
    five = [(b"e0", 0, 1000), (b"r1", 1001, 100_000), (b"e2", 101_002, 1000), (b"r3", 102_003, 50_000), (b"e4", 152_004, 1)]
    S["contigs without records first, in the middle and last"] = (
        [rec(b"a", b"r1", 5, b"10M", contigs=five), rec(b"b", b"r1", 70_000, b"10M", contigs=five), rec(b"c", b"r3", 49_990, b"10M", contigs=five)], five)
    S["a record ending at 2^29"] = ([rec(b"p", b"c0", 5, b"9M"), rec(b"q", b"c0", 2**29 - 100, b"100M"), rec(b"r", b"c0", 2**29 - 1, b"1M")], CONTIGS)
    # bin 4681 interrupted by a record of bin 585 and resumed: two chunks; then interrupted twice more
    S["a bin interrupted and resumed"] = ([rec(b"a", b"c1", 10, b"10M"), rec(b"b", b"c1", 16380, b"10M"), rec(b"c", b"c1", 16381, b"3M"),
                                           rec(b"d", b"c1", 16382, b"10M"), rec(b"e", b"c1", 16383, b"1M"), rec(b"f", b"c1", 16383, b"2M"),
                                           rec(b"g", b"c1", 16383, b"1M")], CONTIGS)
    S["empty slots in front, in the middle and behind"] = (
        [b"", b"", rec(b"a", b"c0", 3, b"5M"), b"", rec(b"b", b"c0", 9, b"5M"), b"", b"", rec(b"c", b"c2", 1, b"5M"), b"", unplaced(b"u"), b"", b""], CONTIGS)
    S["mapped and unmapped on one contig"] = ([rec(b"a", b"c2", 50, b"5M"), rec(b"a2", b"c2", 50, b"*", 5, flag=4 | 1 | 8), rec(b"b", b"c2", 60, b"5M", flag=16),
                                               rec(b"b2", b"c2", 60, b"*", 5, flag=4), unplaced(b"u0"), unplaced(b"u1")], CONTIGS)
    n_ops = 65_536 + 2  # more than n_cigar_op holds: the CG tag, the placeholder <l_seq>S<len>N in the record
    big = rec(b"cg", b"c1", 30_000, b"1M1D" * (n_ops // 2), None)
    assert b"CGBI" in big and len(big) > 4 * n_ops
    S["a CG placeholder"] = ([rec(b"pre", b"c1", 29_000, b"20M"), big, rec(b"post", b"c1", 30_001, b"20M"), rec(b"far", b"c1", 30_000 + n_ops, b"20M")], CONTIGS)
    # record starts at payload offsets 0, 65 279 and 65 280 (of the third block); one straddles two blocks; three full blocks
    blocks = []
    p = fill(blocks, PAYLOAD - 1, b"c1", 100)
    blocks.append(sized(200, b"c1", p))  # starts at 65 279
    p = fill(blocks, 2 * PAYLOAD, b"c1", p + 1)
    assert bo.offsets(blocks)[-1] == 2 * PAYLOAD
    p = fill(blocks, 3 * PAYLOAD, b"c1", p + 20_000)
    S["block edges, a multiple of 65 280"] = (blocks, CONTIGS)
    S["one block exactly"] = ((lambda b: (fill(b, PAYLOAD, b"c2", 7), b)[1])([]), CONTIGS)
    S["random"] = (random_records(np.random.default_rng(2029), 5000, CONTIGS), CONTIGS)
    return S


def random_records(rng, n, contigs, n_unplaced=37, empty_every=97):
    """n sorted records over the contigs: clustered positions, CIGARs with every operation, a few long N; unplaced ones and
    empty slots among them"""
    out = []
    per = np.sort(rng.integers(0, len(contigs), n))
    for c in range(len(contigs)):
        k = int((per == c).sum())
        ln = contigs[c][2]
        centre = rng.integers(0, max(ln - 2000, 1), max(k // 40, 1))
        pos = np.sort(np.clip(rng.choice(centre, k) + rng.integers(-30_000, 30_000, k), 0, ln - 1500))
        for i, p in enumerate(pos.tolist()):
            m = [int(x) for x in rng.integers(1, 60, 4)]
            kind = int(rng.integers(0, 12))
            cigar = (b"%dM" % m[0] if kind < 6 else b"%dS%d=%dX%dI%dM" % (m[0], m[1], m[2], m[3], m[0]) if kind < 8 else
                     b"%dM%dD%dM" % (m[0], m[1], m[2]) if kind < 10 else b"%dM%dN%dM" % (m[0], 200 * m[1] * (kind - 9), m[2]) if kind < 12 else b"*")
            span = bo.ref_length(bo.cigar_words(cigar))
            if p + span > ln:
                cigar = b"1M"
            flag = 4 if kind == 3 and i % 5 == 0 else 0
            out.append(rec(b"r%d.%d" % (c, i), contigs[c][0], p, b"*" if flag else cigar, 10 if flag else None, flag, contigs=contigs))
            if len(out) % empty_every == 0:
                out.append(b"")
    out += [unplaced(b"u%d" % i, 5 + i % 7) for i in range(n_unplaced)]
    return out


def errors():
    """(name, slots, contigs, status, first_bad)"""
    a, b, c = rec(b"a", b"c1", 100, b"10M"), rec(b"b", b"c1", 200, b"10M"), rec(b"c", b"c2", 5, b"10M")
    u = unplaced(b"u")
    three = [(b"c0", 0, 1000), (b"c1", 1001, 2**29 + 10)]
    far = rec(b"far", b"c1", 2**29 - 9, b"10M", contigs=three)  # end = 2^29 + 1

    def patched(r, at, fmt, v):
        import struct
        r = bytearray(r)
        struct.pack_into(fmt, r, at, v)
        return bytes(r)
    return [
        ("pos decreasing", [a, b"", b, a, c], CONTIGS, INVALID_ARG, 3),
        ("refID decreasing", [a, c, b""] + [b], CONTIGS, INVALID_ARG, 3),
        ("an unplaced record in front of a placed one", [a, u, b"", b], CONTIGS, INVALID_ARG, 3),
        ("a truncated slot", [a, b[:30], c], CONTIGS, INVALID_ARG, 1),
        ("a slot cut inside its bases", [a, b"", b[:-3], c], CONTIGS, INVALID_ARG, 2),
        ("block_size wrong", [a, patched(b, 0, "<I", len(b) - 5), c], CONTIGS, INVALID_ARG, 1),
        ("fields past the end", [a, patched(b, 16, "<H", 4000), c], CONTIGS, INVALID_ARG, 1),
        ("refID = n_contigs", [a, b, patched(c, 4, "<i", 3)], CONTIGS, INVALID_ARG, 2),
        ("pos -2", [patched(a, 8, "<i", -2), b], CONTIGS, INVALID_ARG, 0),
        ("end past the contig", [a, rec(b"e", b"c1", 299_995, b"6M")], CONTIGS, INVALID_ARG, 1),
        ("end = 2^29 + 1", [rec(b"p", b"c0", 3, b"4M", contigs=three), b"", far], three, UNSUPPORTED, 2),
        ("the first of two kinds decides", [rec(b"p", b"c1", 2**29 - 20, b"4M", contigs=three), far, rec(b"p", b"c1", 50, b"4M", contigs=three)], three, UNSUPPORTED, 1),
        ("out of order and beyond 2^29 at once", [rec(b"p", b"c1", 2**29 - 5, b"4M", contigs=three), far], three, INVALID_ARG, 1),
    ]

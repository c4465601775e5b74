"""Cases for the pileup (tests/test_bam_pileup_rule.py, tests/test_bam_pileup_host_bodies.py, tests/test_gpu_bam_pileup.py): the
corpus of sorted record tables with regions and parameters, the refusals with what the Python restatement
(tests/bam_pileup_oracle.py) says of each, and the stand-alone program that runs the kernels' bodies on the CPU
(tests/bam_pileup_host_bodies.cpp).  Records are built field by field with `bam_read_cases.raw`.  T is the product's tile: the
shapes sit on its borders, the expected rows know nothing of it."""
import os
import struct
import subprocess

import numpy as np

import bam_oracle
import bam_pileup_oracle as po
import bam_read_cases as rc
from rust_bio_amd import _lib

ROOT = rc.ROOT
T = _lib.PILEUP_TILE
NONE = po.NONE
DEFAULT = dict(flags=0, require=0, exclude=0x704, min_mapq=0, min_baseq=0)


def contigs_of(lens, names=None):
    out, start = [], 0
    for c, ln in enumerate(lens):
        out.append((names[c] if names else b"c%d" % c, start, ln))
        start += ln + 1
    return out


CONTIGS = contigs_of([4 * T + 37, 3 * T, 2 * T + 5, 1000])  # c2 never carries a record


def query_len(cigar):
    return sum(w >> 4 for w in bam_oracle.cigar_words(cigar) if (w & 15) in po.QUERY_OPS)


def rec(ref, pos, cigar, codes=None, qual=None, seed=0, name=None, **kw):
    """a record at (ref, pos) with the CIGAR given as text; bases (4-bit codes) by default a seeded draw of A, C, G, T, N"""
    words = bam_oracle.cigar_words(cigar) if isinstance(cigar, bytes) else list(cigar)
    if codes is None:
        n = sum(w >> 4 for w in words if (w & 15) in po.QUERY_OPS)
        codes = np.random.default_rng(seed * 7919 + pos).choice([1, 2, 4, 8, 15], n).tolist()
    return rc.raw(name or b"r%d_%d" % (ref, pos), ref=ref, pos=pos, cigar=words, codes=codes, qual=qual, **kw)


def params(**kw):
    return dict(DEFAULT, **kw)


def case(name, slots, regions, contigs=CONTIGS, **kw):
    return dict(name=name, slots=slots, contigs=contigs, regions=regions, params=params(**kw))


def by_position(recs):
    """stable, by ((uint32) refID, pos): the order the call asks for"""
    return sorted(recs, key=lambda r: (struct.unpack_from("<i", r, 4)[0] & 0xFFFFFFFF, struct.unpack_from("<i", r, 8)[0]))


def every_op():
    cigars = [b"10M", b"3S4M", b"2H5M", b"4M2D4M", b"4M5N4M", b"4M2I4M", b"3=2X3=", b"2M1P2M", b"3S2I5M", b"5M2I", b"2M1I2I2M",
              b"2H3S4M2I1P3M2D2M10N3=1X2S1H", b"1M", b"1I1M", b"1M1D1M"]
    out = [rec(0, 5 + 3 * k, c, seed=k) for k, c in enumerate(cigars)]
    out.append(rec(0, 60, [(2 << 4) | 0, (3 << 4) | 9, (2 << 4) | 0], codes=[1, 2, 4, 8]))  # code 9 consumes nothing
    out.append(rc.raw(b"noseq", ref=0, pos=70, cigar=bam_oracle.cigar_words(b"5M2D3M")))  # l_seq == 0: OTHER
    out.append(rc.raw(b"nocigar", ref=0, pos=72, codes=[1, 2, 4]))  # no operation: nothing
    return out


def every_code():
    codes = list(range(16))
    return [rec(0, 10, b"16M", codes=codes), rec(0, 12, b"16M", codes=codes, qual=bytes(range(30, 46))),
            rec(0, 20, b"1S16M", codes=[3] + codes), rec(0, 21, b"3S16M1S", codes=[3, 5, 7] + codes + [9], qual=bytes(range(20))),
            rec(0, 30, b"17M", codes=codes + [1], flag=0x10)]


def qualities():
    q = bytes([0, 1, 19, 20, 21, 254, 255, 0, 20, 255])
    return [rec(0, 100, b"10M", codes=[1, 2, 4, 8, 1, 2, 4, 8, 15, 1], qual=q), rec(0, 103, b"2S4M2I2M", codes=[1] * 10, qual=q),
            rec(0, 104, b"6M", codes=[8] * 6)]  # the last one's qualities are absent: 0xFF passes every threshold


def mapqs():
    return [rec(0, 200 + k, b"5M", mapq=m, seed=k) for k, m in enumerate((0, 59, 60, 255))]


def flagged():
    flags = [0, 0x2, 0x10, 0x12, 0x100, 0x200, 0x400, 0x800, 0x4, 0x14, 0x1 | 0x2 | 0x40, 0x1 | 0x80 | 0x10, 0x904, 0x704, 0x402]
    return [rec(0, 300 + 2 * k, b"4M1D3M1I2M", flag=f, seed=k) for k, f in enumerate(flags)]


def borders():
    out = [rec(0, T - 10, b"10M"), rec(0, T, b"10M"), rec(0, T - 10, b"20M", seed=1), rec(0, T - 10, b"5M10D5M"), rec(0, T - 4, b"4M2I4M"),
           rec(0, T - 10, b"5M%dN5M" % (T + 20)), rec(0, T - 1, b"1M1I1M"), rec(0, 2 * T - 1, b"1M"), rec(0, 2 * T, b"1M"), rec(0, 0, b"3M"),
           rec(0, T - 3, b"3M2D", flag=0x10), rec(0, 2 * T - 2, b"2M1I", flag=0x10), rec(0, T + 5, b"2S%dM" % (T - 5), seed=3)]
    return by_position(out)


def reach_back():
    """one record of span 3 T, then 200 short ones: the later tiles must reach back to slot 0"""
    long = rc.raw(b"long", ref=0, pos=5, cigar=[(3 * T) << 4])
    return [long] + [rec(0, 10 + 7 * i, b"8M", seed=i) for i in range(200)]


def gap_tile():
    return [rec(1, 10 + 9 * i, b"12M", seed=i) for i in range(20)] + [rec(1, 2 * T + 11 * i, b"6M1D6M", seed=50 + i) for i in range(20)]


def deep():
    """66 000 one-base records at one position: the smallest pile a 16-bit counter gets wrong"""
    return [rc.raw(b"d", ref=3, pos=500, cigar=[1 << 4], codes=[(1, 2, 4, 8)[k & 3]], flag=0x10 * (k % 3 == 0)) for k in range(66_000)]


def contigs_and_slots():
    len0 = CONTIGS[0][2]
    placed = [rec(0, len0 - 10, b"10M"), rec(0, len0 - 1, b"1M"), rec(1, 0, b"10M"), rec(1, 0, b"3S7M", seed=1), rec(3, 0, b"5M"), rec(3, 995, b"5M"),
              rec(3, 999, b"1M", flag=0x4), rc.raw(b"mate", ref=3, pos=999, flag=0x5, codes=[1, 2])]
    unplaced = [rc.raw(b"u1", flag=4), rc.raw(b"u2", flag=4, codes=[1, 2, 4], qual=b"\1\2\3"),
                rc.raw(b"u3", flag=4, cigar=[(3 << 4) | 4, (50 << 4) | 3], codes=[1, 2, 4])]  # a CG placeholder without a refID: let through
    return [b"", b""] + placed[:3] + [b""] + placed[3:] + [b"", b""] + unplaced + [b""]


def random_records(n=400, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ref = int(rng.choice([0, 1, 3]))
        ops = []
        for _ in range(int(rng.integers(1, 7))):
            ops.append((int(rng.integers(1, 40)), b"MIDNS=XHP"[int(rng.integers(0, 9))]))
        if not any(op in b"M=X" for _, op in ops):
            ops.append((int(rng.integers(1, 30)), ord("M")))
        if rng.integers(0, 8) == 0:
            ops.append((int(rng.integers(T, 2 * T)), ord("N")))
            ops.append((5, ord("M")))
        cigar = b"".join(b"%d%c" % o for o in ops)
        span = bam_oracle.ref_length(bam_oracle.cigar_words(cigar))
        room = CONTIGS[ref][2] - span
        if room < 0:
            continue
        n_q = query_len(cigar)
        out.append(rec(ref, int(rng.integers(0, room + 1)), cigar, codes=rng.integers(0, 16, n_q).tolist(),
                       qual=None if rng.integers(0, 4) == 0 else rng.integers(0, 60, n_q).astype(np.uint8).tobytes(),
                       flag=int(rng.choice([0, 0x10, 0x400, 0x100, 0x63, 0x93, 0x4])), mapq=int(rng.choice([0, 20, 60])), name=b"x%d" % i))
    return by_position(out)


def region_shapes():
    r = [(0, 0, 0), (0, 5, 6), (0, 3, 3 + T - 1), (0, 0, T), (0, 0, T + 1), (0, 11, 11 + 2 * T + 1), (0, 7, 2 * T + 30),
         (0, T - 20, T + 20), (0, T - 5, T + 5), (0, T - 20, T + 20), (1, 0, 3 * T), (0, 0, 4 * T + 37), (2, 0, 2 * T + 5), (2, T, T), (0, 0, 100),
         (3, 0, 1000), (3, 1000, 1000)]
    return r


def many_regions(n=1000, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ref = int(rng.choice([0, 1, 2, 3]))
        beg = int(rng.integers(0, CONTIGS[ref][2] - 3))
        out.append((ref, beg, beg + int(rng.integers(1, 4))))
    return out


def corpus(with_deep=True):
    whole0 = [(0, 0, CONTIGS[0][2])]
    head = [(0, 0, 400)]
    out = [case("every op kind", every_op(), [(0, 0, 120)], exclude=0),
           case("all 16 codes at both parities", every_code(), [(0, 0, 64)], exclude=0),
           case("all 16 codes, strands", every_code(), [(0, 0, 64)], exclude=0, flags=po.STRANDS)]
    out += [case("min_baseq %d" % q, qualities(), [(0, 90, 130)], min_baseq=q) for q in (0, 1, 20, 255)]
    out += [case("min_mapq %d" % q, mapqs(), [(0, 190, 230)], min_mapq=q) for q in (0, 1, 60, 255)]
    out += [case("flags: the default exclude", flagged(), head), case("flags: exclude 0", flagged(), head, exclude=0),
            case("flags: require 0x2", flagged(), head, require=0x2), case("flags: require 0x2, exclude 0", flagged(), head, require=0x2, exclude=0),
            case("flags: strands", flagged(), head, flags=po.STRANDS), case("flags: strands, exclude 0x10", flagged(), head, flags=po.STRANDS, exclude=0x10),
            case("flags: require and exclude overlap", flagged(), head, require=0x10, exclude=0x10)]
    out += [case("tile borders", borders(), whole0 + [(0, 7, 2 * T + 30), (0, T, 2 * T), (0, T - 1, T + 1)], exclude=0),
            case("tile borders, strands", borders(), whole0 + [(0, T - 1, T), (0, T, T + 1)], flags=po.STRANDS),
            case("a record of span 3 T in front of 200 short ones", reach_back(), whole0 + [(0, 2 * T, 3 * T + 10), (0, 3 * T + 4, 3 * T + 6)]),
            case("an empty tile between populated ones", gap_tile(), [(1, 0, 3 * T), (1, T, 2 * T)]),
            case("contig ends, an empty contig, unplaced records, empty slots", contigs_and_slots(),
                 [(0, CONTIGS[0][2] - 20, CONTIGS[0][2]), (1, 0, 30), (2, 0, CONTIGS[2][2]), (3, 0, 1000)], exclude=0),
            case("region shapes", by_position(borders() + gap_tile() + every_op()), region_shapes(), exclude=0),
            case("regions in reversed order", by_position(borders() + gap_tile()), region_shapes()[::-1], flags=po.STRANDS),
            case("1 000 regions of 1 .. 3 positions", random_records(), many_regions()),
            case("random records", random_records(), [(0, 0, CONTIGS[0][2]), (1, 0, CONTIGS[1][2]), (3, 0, 1000)], exclude=0, min_baseq=13),
            case("random records, filters and strands", random_records(seed=12), [(1, 5, CONTIGS[1][2] - 5), (0, T + 1, 3 * T - 1)], flags=po.STRANDS,
                 require=0x1, exclude=0x500, min_mapq=20, min_baseq=30),
            case("no region", every_op(), []), case("no slot", [], [(0, 0, 10), (2, 5, 5)]), case("no slot and no region", [], []),
            case("only empty slots", [b"", b"", b""], [(1, 0, 40)]), case("no contig and no region", [rc.raw(b"u", flag=4)], [], contigs=[])]
    if with_deep:
        out += [case("66 000 records at one position", deep(), [(3, 490, 510)], exclude=0),
                case("66 000 records at one position, strands", deep(), [(3, 500, 501)], flags=po.STRANDS)]
    return out


def refusals():
    """[(name, slots, contigs, regions, status, slot)]"""
    a, b, c = rec(0, 10, b"5M"), rec(0, 20, b"5M"), rec(1, 0, b"5M")
    big = contigs_of([(1 << 29) + 100], [b"big"])
    reg = [(0, 0, 50)]
    cg = rc.raw(b"cg", ref=0, pos=30, cigar=[(4 << 4) | 4, (20 << 4) | 3], codes=[1, 2, 4, 8])
    cg_early = rc.raw(b"cg", ref=0, pos=3, cigar=[(4 << 4) | 4, (20 << 4) | 3], codes=[1, 2, 4, 8])
    short_q = rc.raw(b"q", ref=0, pos=30, cigar=[5 << 4], codes=[1, 2, 4, 8])
    out = [("positions descend", [a, b, a], CONTIGS, reg, po.INVALID_ARG, 2),
           ("references descend", [a, c, b], CONTIGS, reg, po.INVALID_ARG, 2),
           ("an unplaced record in front of a placed one", [a, rc.raw(b"u", flag=4), b""] + [b], CONTIGS, reg, po.INVALID_ARG, 3),
           ("pos -1 behind pos 0", [rec(0, 0, b"1M"), rc.raw(b"m", ref=0, pos=-1)], CONTIGS, reg, po.INVALID_ARG, 1),
           ("shorter than 36 bytes", [a, b[:35]], CONTIGS, reg, po.INVALID_ARG, 1),
           ("block_size is not the slot's length", [a, rc.raw(b"x", ref=0, pos=20, block=40)], CONTIGS, reg, po.INVALID_ARG, 1),
           ("two records in one slot", [a + b], CONTIGS, reg, po.INVALID_ARG, 0),
           ("l_seq runs past the record", [b"", a, rc.raw(b"x", ref=0, pos=20, l_seq=400)], CONTIGS, reg, po.INVALID_ARG, 2),
           ("refID == n_contigs", [a, rc.raw(b"x", ref=4, pos=0)], CONTIGS, reg, po.INVALID_ARG, 1),
           ("pos -2", [rc.raw(b"x", ref=0, pos=-2), a], CONTIGS, reg, po.INVALID_ARG, 0),
           ("end past the contig", [a, rec(0, CONTIGS[0][2] - 4, b"5M")], CONTIGS, reg, po.INVALID_ARG, 1),
           ("the query lengths are not l_seq", [a, b, short_q], CONTIGS, reg, po.INVALID_ARG, 2),
           ("the query lengths are not l_seq, unplaced", [a, rc.raw(b"u", flag=4, cigar=[(3 << 4) | 4], codes=[1, 2])], CONTIGS, reg, po.INVALID_ARG, 1),
           ("an I counts into the query", [a, rc.raw(b"i", ref=0, pos=30, cigar=[2 << 4, (2 << 4) | 1, 2 << 4], codes=[1, 2, 4, 8])], CONTIGS, reg, po.INVALID_ARG, 1),
           ("operation code 10", [a, rc.raw(b"o", ref=0, pos=30, cigar=[2 << 4, (1 << 4) | 10], codes=[1, 2])], CONTIGS, reg, po.INVALID_ARG, 1),
           ("operation code 15, no bases", [rc.raw(b"o", ref=0, pos=30, cigar=[(1 << 4) | 15])], CONTIGS, reg, po.INVALID_ARG, 0),
           ("a CG placeholder", [a, b, cg, c], CONTIGS, reg, po.UNSUPPORTED, 2),
           ("a CG placeholder that also sorts early", [a, b, cg_early], CONTIGS, reg, po.INVALID_ARG, 2),
           ("a CG placeholder in front of a broken slot", [a, cg, a[:20]], CONTIGS, reg, po.UNSUPPORTED, 1),
           ("a broken slot in front of a CG placeholder", [a, short_q, cg], CONTIGS, reg, po.INVALID_ARG, 1),
           ("end beyond 2^29", [rc.raw(b"e", ref=0, pos=(1 << 29) - 5, cigar=[10 << 4])], big, [(0, 0, 10)], po.UNSUPPORTED, 0),
           ("end beyond 2^29 and a CIGAR that does not fit", [rc.raw(b"e", ref=0, pos=(1 << 29) - 5, cigar=[10 << 4], codes=[1])], big, [(0, 0, 10)],
            po.INVALID_ARG, 0),
           ("a region on refID n_contigs", [a, b], CONTIGS, [(0, 0, 5), (4, 0, 1)], po.INVALID_ARG, None),
           ("a region on refID -1", [a, b], CONTIGS, [(-1, 0, 1)], po.INVALID_ARG, None),
           ("a region with beg < 0", [a, b], CONTIGS, [(0, -1, 1)], po.INVALID_ARG, None),
           ("a region with beg > end", [a, b], CONTIGS, [(0, 6, 5)], po.INVALID_ARG, None),
           ("a region past its contig", [a, b], CONTIGS, [(3, 0, 1000), (3, 0, 1001)], po.INVALID_ARG, None),
           ("a bad region and a bad slot", [b, a], CONTIGS, [(3, 0, 1001)], po.INVALID_ARG, None),
           ("a region and no contig", [rc.raw(b"u", flag=4)], [], [(0, 0, 0)], po.INVALID_ARG, None)]
    return out


# ---- the program ------------------------------------------------------------------------------------------------------------
def build_program(source, exe, sanitize):
    """the stand-alone program of tests/<source> (the pileup's, the sites' or the indel events' host bodies), built as
    bam_read_cases.build_program builds its own"""
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + _lib.CSRC] + flags + [os.path.join(ROOT, "tests", source), "-o", exe])
    return exe


def run_program(exe, tmp, cases):
    """cases: [dict(slots, contigs, regions, params)] -> [(rc, first_bad, n_rows, rows: uint32[n_rows, W] or None, row_off or None)]"""
    inp, outp = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for c in cases:
            p, slots = c["params"], c["slots"]
            off = bam_oracle.offsets(slots)
            table = rc.contig_table(c["contigs"])
            regions = np.array([tuple(r) for r in c["regions"]], dtype=_lib.BAM_REGION_DTYPE) if c["regions"] else np.zeros(0, _lib.BAM_REGION_DTYPE)
            f.write(struct.pack("<9Q", len(slots), int(off[-1]), len(table), len(regions), p["flags"], p["require"], p["exclude"], p["min_mapq"], p["min_baseq"]))
            f.write(b"".join(slots) + off.tobytes() + table.tobytes() + regions.tobytes())
    subprocess.check_call([exe, inp, outp])
    b = open(outp, "rb").read()
    at, got = 0, []
    for c in cases:
        rcode, bad, n_rows = struct.unpack_from("<qQQ", b, at)
        at += 24
        w = 2 * po.COLS if c["params"]["flags"] & po.STRANDS else po.COLS
        rows = row_off = None
        if rcode == 0:
            rows = np.frombuffer(b, np.uint32, n_rows * w, at).reshape(n_rows, w)
            at += rows.nbytes
            row_off = np.frombuffer(b, np.uint64, len(c["regions"]) + 1, at).tolist()
            at += 8 * (len(c["regions"]) + 1)
        got.append((rcode, bad, n_rows, rows, row_off))
    assert at == len(b)
    return got


def want_of(c):
    """the oracle's (rows: uint32[n, W], row_off) of a case"""
    rows, row_off = po.pileup(c["slots"], c["contigs"], c["regions"], **c["params"])
    w = 2 * po.COLS if c["params"]["flags"] & po.STRANDS else po.COLS
    return np.array(rows, dtype=np.uint32).reshape(len(rows), w), row_off

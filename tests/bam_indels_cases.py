"""Cases for the indel events (tests/test_bam_indels_rule.py, tests/test_bam_indels_host_bodies.py, tests/test_gpu_bam_indels.py):
the pileup's corpus (tests/bam_pileup_cases.py, by import) with the thresholds rotated over it, cases of the events' own at tile
borders, at the word borders of the inserted codes and at the operations the rule drops, the pileup's refusals with what the
Python restatement (tests/bam_indels_oracle.py) says of each, and the stand-alone program that runs the kernels' bodies on the
CPU (tests/bam_indels_host_bodies.cpp, for tests/bam_indels_left_cases.py as well).  T is the product's tile; the expected events know nothing of it."""
import os
import struct
import subprocess

import numpy as np

import bam_indels_oracle as io
import bam_oracle
import bam_pileup_cases as pc
import bam_read_cases as rc
from rust_bio_amd import _lib

ROOT = pc.ROOT
T = pc.T
CONTIGS = pc.CONTIGS
M, I, D, N, S, H, P, B = 0, 1, 2, 3, 4, 5, 6, 9


def words(*ops):
    """(length, op) pairs as CIGAR words: lengths of 0 included, which text cannot say"""
    return [(n << 4) | op for n, op in ops]


def case(name, slots, regions, contigs=CONTIGS, **kw):
    return dict(name=name, slots=slots, contigs=contigs, regions=regions, params=io.params(**kw))


def ins_rec(ref, pos, codes, lead=4, tail=4, soft=0, flag=0, name=b"i"):
    """<soft>S <lead>M <len(codes)>I <tail>M at (ref, pos): the insertion starts at base soft + lead, anchored at pos + lead - 1"""
    ops = ([(soft, S)] if soft else []) + [(lead, M), (len(codes), I), (tail, M)]
    return pc.rec(ref, pos, words(*ops), codes=[1] * (soft + lead) + list(codes) + [2] * tail, flag=flag, name=name)


def tile_borders():
    """anchors at T - 1 and T of c0 (the last position of a tile and the first of the next, for a region that begins at 0), a
    deletion anchored at T - 1 whose span lies in the next tile, the same events on both strands"""
    out = [ins_rec(0, T - 4, [1, 2], flag=f, name=b"a%d" % f) for f in (0, 0x10, 0)]  # anchor T - 1
    out += [ins_rec(0, T - 3, [4, 8, 4], flag=f, name=b"b%d" % f) for f in (0, 0x10)]  # anchor T
    out += [pc.rec(0, T - 3, b"3M10D3M", flag=f, name=b"c%d" % f) for f in (0x10, 0)]  # anchor T - 1, deleted T .. T + 9
    out += [pc.rec(0, T - 3, b"4M1D3M", name=b"d")]  # anchor T
    out += [ins_rec(0, 2 * T - 8, [8], lead=8, name=b"e"), pc.rec(0, 2 * T - 1, b"1M2D1M", name=b"f")]  # anchor 2 T - 1 twice
    return pc.by_position(out)


def border_regions():
    a = T - 1
    return [(0, 0, CONTIGS[0][2]), (0, a + 1, a + 50), (0, a, a + 1), (0, a - 1, a), (0, T, T + 1), (0, T - 1, T + 1), (0, 7, 7 + 2 * T), (0, T - 1, 2 * T),
            (0, 0, T), (0, 0, T - 1), (0, 0, T + 1), (0, 5, 5), (0, T - 1, T - 1), (0, a, a + 1), (0, 0, CONTIGS[0][2])]


def word_borders(ref=1, pos=40):
    """insertions of 1, 15, 16, 17 and 33 bases at one anchor that differ only in their last base (for 17 that is base 17) and, for
    33, only in base 17; every one four times, at both parities of q and on both strands"""
    out, k = [], 0
    for n in (1, 15, 16, 17, 33):
        base = [(1, 2, 4, 8)[j % 4] for j in range(n)]
        variants = [base, base[:-1] + [15 if base[-1] != 15 else 1]]
        if n > 17:
            variants.append(base[:16] + [0] + base[17:])
        for v in variants:
            for soft, flag in ((0, 0), (1, 0x10), (1, 0), (2, 0)):  # q = 4 (even), 5 (odd), 5, 6
                out.append(ins_rec(ref, pos - (k % 3), v, lead=4 + (k % 3), soft=soft, flag=flag, name=b"w%d" % k))
                k += 1
    return pc.by_position(out)


def odd_codes():
    """N and = inside an insertion, every code once, an insertion that is all of a read's bases behind one M"""
    out = [ins_rec(0, 100, [1, 15, 0, 2], name=b"n1"), ins_rec(0, 100, [1, 15, 0, 2], soft=3, name=b"n2"), ins_rec(0, 100, [1, 15, 0, 4], name=b"n3"),
           ins_rec(0, 100, list(range(16)), name=b"all"), ins_rec(0, 100, list(range(16)), soft=1, flag=0x10, name=b"all2"),
           ins_rec(0, 100, list(range(15, -1, -1)), name=b"rev"), pc.rec(0, 103, words((1, M), (5, I)), codes=[1, 2, 2, 2, 2, 2], name=b"tail")]
    return pc.by_position(out)


def dropped():
    """I and D as the first operation or with no reference base in front, operations of length 0, code 9, H and P around events,
    I behind D and D behind I, 2I 3I and 2D 3D in a row, a record without bases"""
    out = [pc.rec(0, 200, b"2I5M", name=b"lead_i"), pc.rec(0, 200, b"2D5M", name=b"lead_d"), pc.rec(0, 200, b"3S2I5M", name=b"soft_i"),
           pc.rec(0, 200, b"2H1D4M", name=b"hard_d"), pc.rec(0, 200, b"2I2D5M", name=b"lead_id"),
           pc.rec(0, 201, words((3, M), (0, I), (2, M), (0, D), (2, M)), name=b"zero"),
           pc.rec(0, 201, words((3, M), (0, D), (2, I), (2, M)), name=b"zero_then_i"),
           pc.rec(0, 202, words((2, M), (3, B), (1, I), (1, P), (1, D), (2, M)), codes=[1, 2, 4, 8, 1], name=b"nine"),
           pc.rec(0, 203, b"4M3I2D4M", name=b"i_d"), pc.rec(0, 203, b"4M2D3I4M", name=b"d_i"), pc.rec(0, 203, b"4M3I2D4M", flag=0x10, name=b"i_d_rev"),
           pc.rec(0, 204, b"4M2I3I4M", codes=[1] * 4 + [2, 2] + [2, 2, 8] + [4] * 4, name=b"ii"), pc.rec(0, 204, b"4M2D3D4M", name=b"dd"),
           pc.rec(0, 204, b"4M2I3I4M", codes=[1] * 4 + [2, 2] + [2, 2, 8] + [4] * 4, flag=0x10, name=b"ii_rev"),
           rc.raw(b"noseq", ref=0, pos=205, cigar=bam_oracle.cigar_words(b"5M2I2D3M")), rc.raw(b"noseq2", ref=0, pos=205, cigar=bam_oracle.cigar_words(b"5M2D3M")),
           pc.rec(0, 206, b"2M5N1I2M3N1D2M", name=b"skips"), pc.rec(0, 207, b"2M1I", name=b"last_i"), pc.rec(0, 207, b"2M1D", name=b"last_d")]
    return pc.by_position(out)


def threshold_pile():
    """at c3:100 depth 20: the insertion AC 3 times forward and once reverse, AT twice forward, a deletion of two bases once on each
    strand, 12 plain reads (8 + 4)"""
    out = [ins_rec(3, 100, [1, 2], lead=1, tail=1, flag=f, name=b"ac%d" % k) for k, f in enumerate((0, 0, 0, 0x10))]
    out += [ins_rec(3, 100, [1, 8], lead=1, tail=1, name=b"at%d" % k) for k in range(2)]
    out += [pc.rec(3, 100, b"1M2D1M", flag=f, name=b"d%d" % f) for f in (0, 0x10)]
    out += [pc.rec(3, 100, b"1M", flag=0x10 * (k >= 8), name=b"p%d" % k) for k in range(12)]
    return out


def deep():
    """the pileup's 66 000 records at one position, with one insertion in every record: one event"""
    return [rc.raw(b"d", ref=3, pos=500, cigar=words((1, M), (2, I), (1, M)), codes=[(1, 2, 4, 8)[k & 3], 4, 8, 1], flag=0x10 * (k % 3 == 0)) for k in range(66_000)]


def corpus(with_deep=True):
    out = []
    for k, c in enumerate(pc.corpus(with_deep)):
        p = c["params"]
        kw = dict(require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"], min_baseq=p["min_baseq"])
        if k % 3 == 1:
            kw.update(min_depth=2)
        if k % 3 == 2:
            kw.update(min_alt=2, min_alt_permille=300)
        out.append(case(c["name"], c["slots"], c["regions"], contigs=c["contigs"], **kw))
    whole = [(r, 0, ln) for r, (_, _, ln) in enumerate(CONTIGS)]
    everything = pc.by_position(tile_borders() + word_borders() + odd_codes() + dropped() + pc.gap_tile() + pc.borders())
    out += [case("anchors at T - 1 and T, a deletion into the next tile, regions one behind and only the anchor", tile_borders(), border_regions(), exclude=0),
            case("anchors at T - 1 and T, both strands asked for", tile_borders(), border_regions()[:8], exclude=0, min_alt_strand=1),
            case("insertions that differ in the last base or in base 17", word_borders(), [(1, 0, 100), (1, 41, 44), (1, 43, 44), (1, 0, 3 * T)], exclude=0),
            case("insertions that differ in the last base, twice or more", word_borders(), [(1, 0, 100)], exclude=0, min_alt=5),
            case("N, = and every code inside an insertion", odd_codes(), [(0, 90, 120), (0, 103, 104)], exclude=0),
            case("dropped operations, shared anchors, rows of I and of D", dropped(), [(0, 190, 230), (0, 0, T), (0, 206, 208)], exclude=0),
            case("dropped operations, min_baseq 255", dropped(), [(0, 190, 230)], exclude=0, min_baseq=255),
            case("dropped operations, the default exclude and a depth", dropped(), [(0, 190, 230)], min_depth=12),
            case("records but no event", pc.mapqs(), [(0, 190, 230)]),
            case("an empty tile between populated ones, deletions", pc.gap_tile(), [(1, 0, 3 * T), (1, T, 2 * T), (1, 2 * T, 3 * T)]),
            case("everything, region shapes", everything, pc.region_shapes() + whole + pc.region_shapes()[::-1], exclude=0),
            case("everything, 1 000 regions of 1 .. 3 positions", everything, pc.many_regions(seed=5) + [(0, T - 2, T + 1)] * 3, exclude=0),
            case("random records, no threshold", pc.random_records(), whole, exclude=0),
            case("random records, strict", pc.random_records(seed=12), whole + [(0, T + 1, 3 * T - 1)], exclude=0, min_depth=3, min_alt=2, min_alt_permille=100,
                 min_alt_strand=1)]
    pile = [(3, 90, 110)]
    for kw in (dict(), dict(min_alt=3), dict(min_alt=4), dict(min_alt=5), dict(min_alt_permille=100), dict(min_alt_permille=101),
               dict(min_alt_permille=200), dict(min_alt_permille=201), dict(min_alt_permille=1000), dict(min_alt_strand=1), dict(min_alt_strand=2),
               dict(min_depth=20), dict(min_depth=21), dict(min_alt=0)):
        out.append(case("the threshold pile, %r" % (kw,), threshold_pile(), pile, exclude=0, **kw))
    if with_deep:
        out += [case("66 000 records with one insertion each", deep(), [(3, 490, 510), (3, 500, 501)], exclude=0),
                case("66 000 records with one insertion each, strict", deep(), [(3, 0, 1000)], exclude=0x10, min_alt=44_000, min_alt_permille=1000)]
    return out


def refusals():
    """[dict(name, slots, contigs, regions, params, want=(status, slot))]: the pileup's, every one"""
    return [dict(name=name, slots=slots, contigs=contigs, regions=regions, params=io.params(), want=(status, slot))
            for name, slots, contigs, regions, status, slot in pc.refusals()]


# ---- the program ------------------------------------------------------------------------------------------------------------
def build_program(exe, sanitize):
    """the program of bam_indels_host_bodies.cpp, which serves both flavours"""
    return pc.build_program("bam_indels_host_bodies.cpp", exe, sanitize)


def params_array(p):
    """bg_bam_indels_t, or bg_bam_indels_left_t where p has a max_shift"""
    shared = (0, p["require"], p["exclude"], p["min_mapq"], p["min_baseq"], 0, p["min_depth"], p["min_alt"], p["min_alt_permille"], p["min_alt_strand"])
    a = np.zeros(1, dtype=_lib.BAM_INDELS_LEFT_DTYPE if "max_shift" in p else _lib.BAM_INDELS_DTYPE)
    a[0] = shared + (p["max_shift"],) if "max_shift" in p else shared
    return a


def run_program(exe, tmp, cases):
    """cases: [dict(slots, contigs, regions, params)] -> [(rc, first_bad, n_events, n_seq, events: BAM_INDEL_DTYPE[] or None, seq: bytes or
    None, event_off or None)].  A case with a `text` runs the left-aligned flavour: the program gets the first n_text bytes of it
    and not one more (fewer where a refusal's text is only claimed)"""
    inp, outp = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for c in cases:
            slots = c["slots"]
            off = bam_oracle.offsets(slots)
            table = rc.contig_table(c["contigs"])
            regions = np.array([tuple(r) for r in c["regions"]], dtype=_lib.BAM_REGION_DTYPE) if c["regions"] else np.zeros(0, _lib.BAM_REGION_DTYPE)
            left = "text" in c
            n_text, text = (c["n_text"], c["text"][:c["n_text"]]) if left else (0, b"")
            f.write(struct.pack("<7Q", len(slots), int(off[-1]), len(table), len(regions), left, n_text, len(text)))
            f.write(params_array(c["params"]).tobytes() + b"".join(slots) + off.tobytes() + table.tobytes() + regions.tobytes() + text)
    subprocess.check_call([exe, inp, outp])
    b = open(outp, "rb").read()
    at, got = 0, []
    for c in cases:
        rcode, bad, n_events, n_seq = struct.unpack_from("<qQQQ", b, at)
        at += 32
        events = seq = event_off = None
        if rcode == 0:
            events = np.frombuffer(b, _lib.BAM_INDEL_DTYPE, n_events, at)
            at += events.nbytes
            seq = b[at:at + n_seq]
            at += n_seq
            event_off = np.frombuffer(b, np.uint64, len(c["regions"]) + 1, at).tolist()
            at += 8 * (len(c["regions"]) + 1)
        got.append((rcode, bad, n_events, n_seq, events, seq, event_off))
    assert at == len(b)
    return got


def want_of(c):
    """the oracle's (events, seq, event_off) of a case"""
    return io.indels(c["slots"], c["contigs"], c["regions"], **c["params"])

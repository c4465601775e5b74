"""Cases for the candidate sites (tests/test_bam_sites_rule.py, tests/test_bam_sites_host_bodies.py, tests/test_gpu_bam_sites.py):
the pileup's corpus (tests/bam_pileup_cases.py, by import) held against a reference text with lower-case, N and IUPAC bytes,
cases of the sites' own at tile borders and thresholds, the refusals with what the Python restatement
(tests/bam_sites_oracle.py) says of each, and the stand-alone program that runs the kernels' bodies on the CPU
(tests/bam_sites_host_bodies.cpp).  T is the product's tile; the expected sites know nothing of it."""
import os
import struct
import subprocess

import numpy as np

import bam_oracle
import bam_pileup_cases as pc
import bam_pileup_oracle as po
import bam_read_cases as rc
import bam_sites_oracle as so
from rust_bio_amd import _lib

ROOT = pc.ROOT
T = pc.T
CONTIGS = pc.CONTIGS
CODE = {65: 1, 67: 2, 71: 4, 84: 8}  # the 4-bit code of an ASCII base


def text_of(contigs, seed=1, plain=()):
    """the index text of a contig table: S0 $ S1 $ ...; mostly ACGT, one byte in 16 lower-case, one in 32 from "NRYKMnry-";
    `plain`: (contig, beg, end) spans that hold upper-case ACGT only"""
    rng = np.random.default_rng(seed)
    n = max([start + ln + 1 for _, start, ln in contigs] + [0])
    t = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    lower = rng.integers(0, 16, n) == 0
    odd = rng.integers(0, 32, n) == 0
    keep = np.zeros(n, bool)
    for c, beg, end in plain:
        keep[contigs[c][1] + beg:contigs[c][1] + end] = True
    t = np.where(lower & ~keep, t + 32, t)
    t = np.where(odd & ~keep, rng.choice(np.frombuffer(b"NRYKMnry-", np.uint8), n), t).astype(np.uint8)
    for _, start, ln in contigs:
        t[start + ln] = ord("$")
    return t.tobytes()


TEXT = text_of(CONTIGS, plain=[(0, T, 2 * T)])


def case(name, slots, regions, contigs=CONTIGS, text=TEXT, **kw):
    return dict(name=name, slots=slots, contigs=contigs, text=text, regions=regions, params=so.params(**kw))


def other_than(ref_byte, k=0):
    """the code of the k-th base that is not the (folded) reference byte"""
    return [CODE[b] for b in b"ACGT" if b != so.fold(ref_byte)][k]


def ref_codes(contig, pos, n, text=TEXT, contigs=CONTIGS):
    return [CODE.get(so.fold(b), 15) for b in text[contigs[contig][1] + pos:contigs[contig][1] + pos + n]]


def full_tile():
    """every position of [T, 2 T) of c0 gives 5 sites: the three other bases, a deletion, an insertion"""
    ref = TEXT[T:2 * T]
    out = [pc.rec(0, T - 1, b"1M%dD1M" % T, codes=[1, 1])]
    out += [pc.rec(0, T, b"%dM" % T, codes=[other_than(b, k) for b in ref], flag=0x10 * (k == 1), name=b"alt%d" % k) for k in range(3)]
    ins = [w for _ in range(T) for w in ((1 << 4) | 0, (1 << 4) | 1)]
    out.append(pc.rec(0, T, ins, codes=[c for b in ref for c in (CODE[b], 1)], name=b"ins"))
    return pc.by_position(out)


def across_a_border():
    """a mismatch on the last position of a tile and one on the first of the next, matches around them"""
    ref = ref_codes(0, 2 * T - 3, 6)
    text = TEXT[2 * T - 3:2 * T + 3]
    codes = ref[:2] + [other_than(text[2]), other_than(text[3], 2)] + ref[4:]
    return [pc.rec(0, 2 * T - 3, b"6M", codes=codes), pc.rec(0, 2 * T - 3, b"6M", codes=codes, flag=0x10, name=b"rev")]


def threshold_pile():
    """at c3:100 the reference base 8 times forward and 4 reverse, one other base 3 times forward and once reverse, another
    twice forward only; a deletion once on each strand: depth 20"""
    base = so.fold(TEXT[CONTIGS[3][1] + 100])
    a, b = other_than(base, 0), other_than(base, 1)
    recs = [(CODE[base], 0)] * 8 + [(CODE[base], 0x10)] * 4 + [(a, 0)] * 3 + [(a, 0x10)] + [(b, 0)] * 2
    out = [rc.raw(b"t%d" % k, ref=3, pos=100, cigar=[1 << 4], codes=[code], flag=flag) for k, (code, flag) in enumerate(recs)]
    out += [pc.rec(3, 99, b"1M1D1M", codes=ref_codes(3, 99, 1) + ref_codes(3, 101, 1), flag=f, name=b"d%d" % f) for f in (0, 0x10)]
    return pc.by_position(out)


def corpus(with_deep=True):
    out = []
    for k, c in enumerate(pc.corpus(with_deep)):
        p = c["params"]
        text = TEXT if c["contigs"] is CONTIGS else text_of(c["contigs"])
        kw = dict(require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"], min_baseq=p["min_baseq"])
        if k % 3 == 1:
            kw.update(min_depth=2, cover=(0, 1, 2, 3))
        if k % 3 == 2:
            kw.update(min_alt=2, min_alt_permille=300, cover=(2, 2, 5, 2**32 - 1))
        out.append(case(c["name"], c["slots"], c["regions"], contigs=c["contigs"], text=text, **kw))
    whole0 = [(0, 0, CONTIGS[0][2])]
    out += [case("a tile whose 512 positions all give 5 sites", full_tile(), [(0, T, 2 * T)], exclude=0),
            case("the full tile in the middle of a region, and cut", full_tile(), whole0 + [(0, T + 1, 2 * T - 1), (0, 2 * T - 1, 2 * T + 1)], exclude=0),
            case("sites across a tile border", across_a_border(), whole0 + [(0, 2 * T - 1, 2 * T), (0, 2 * T, 2 * T + 1), (0, 2 * T, 2 * T)], exclude=0),
            case("sites across a tile border, both strands asked for", across_a_border(), whole0, exclude=0, min_alt_strand=1)]
    pile = [(3, 90, 110)]
    for kw in (dict(), dict(min_alt=3), dict(min_alt=4), dict(min_alt=5), dict(min_alt_permille=200), dict(min_alt_permille=201),
               dict(min_alt_permille=1000), dict(min_alt_strand=1), dict(min_alt_strand=2), dict(min_depth=20), dict(min_depth=21),
               dict(min_alt=0), dict(cover=(20, 21, 0, 2))):
        out.append(case("the threshold pile, %r" % (kw,), threshold_pile(), pile, exclude=0, **kw))
    out.append(case("random records, strict", pc.random_records(), [(0, 0, CONTIGS[0][2]), (1, 0, CONTIGS[1][2]), (3, 0, 1000)], exclude=0, min_depth=3,
                    min_alt=2, min_alt_permille=250, min_alt_strand=1))
    return out


def refusals():
    """[dict(name, slots, contigs, text, n_text, regions, params, want=(status, slot))]: the pileup's, every one, and the text's.
    n_text is what the call is told: a refusal reads no byte of the text, so the one contig of 2^29 bases has none behind it"""
    out = []
    for name, slots, contigs, regions, status, slot in pc.refusals():
        big = max([start + ln + 1 for _, start, ln in contigs] + [0]) > 1 << 20
        text = TEXT if contigs is CONTIGS else b"ACGT" if big else text_of(contigs)
        out.append(dict(name=name, slots=slots, contigs=contigs, text=text, n_text=contigs[-1][1] + contigs[-1][2] + 1 if big else len(text),
                        regions=regions, params=so.params(), want=(status, slot)))
    a, b = pc.rec(0, 10, b"5M"), pc.rec(0, 20, b"5M")
    end3 = CONTIGS[3][1] + CONTIGS[3][2]
    for name, slots, n_text, regions in (("the last contig runs one byte past the text", [a, b], end3 - 1, [(0, 0, 5), (3, 0, 1)]),
                                         ("an empty region on a contig past the text", [a, b], CONTIGS[1][1], [(0, 0, 5), (2, 7, 7)]),
                                         ("a contig past the text and a bad slot", [b, a], 100, [(0, 0, 5)]),
                                         ("no text at all", [a, b], 0, [(0, 0, 5)])):
        out.append(dict(name=name, slots=slots, contigs=CONTIGS, text=TEXT[:n_text], n_text=n_text, regions=regions, params=so.params(),
                        want=(so.INVALID_ARG, None)))
    return out


def synthetic():
    """[(16 counters, reference byte, params, what flips in 32 bits)]: counts of millions, which records cannot reach cheaply"""
    row1, row2 = [0] * 16, [0] * 16
    row1[po.A], row1[po.C], row1[po.COLS + po.C] = 3_580_000, 2_500_000, 2_500_000  # 5e9 >= 500 * 8 580 000 = 4.29e9, below 2^32
    row2[po.A], row2[po.COLS + po.A], row2[po.C], row2[po.COLS + po.C] = 1_900_000, 1_900_000, 2_100_000, 2_100_000  # 4.2e9 < 600 * 8e6 = 4.8e9
    return [(row1, ord("A"), so.params(min_alt_permille=500)), (row2, ord("a"), so.params(min_alt_permille=600)),
            (row1, ord("N"), so.params(min_alt_permille=500))]


# ---- the program ------------------------------------------------------------------------------------------------------------
def build_program(exe, sanitize):
    """the program of bam_sites_host_bodies.cpp"""
    return pc.build_program("bam_sites_host_bodies.cpp", exe, sanitize)


def params_array(p):
    a = np.zeros(1, dtype=_lib.BAM_SITES_DTYPE)
    a[0] = (0, p["require"], p["exclude"], p["min_mapq"], p["min_baseq"], 0, p["min_depth"], p["min_alt"], p["min_alt_permille"], p["min_alt_strand"],
            tuple(p["cover"]))
    return a


def run_program(exe, tmp, cases, synth=()):
    """cases: [dict(slots, contigs, text, regions, params)] -> [(rc, first_bad, n_sites, sites: BAM_SITE_DTYPE[] or None, site_off
    or None, summary: BAM_REGION_SUMMARY_DTYPE[] or None)], and for every synthetic tile the sites of its positions 0 and T - 1"""
    inp, outp = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for c in cases:
            slots = c["slots"]
            off = bam_oracle.offsets(slots)
            table = rc.contig_table(c["contigs"])
            regions = np.array([tuple(r) for r in c["regions"]], dtype=_lib.BAM_REGION_DTYPE) if c["regions"] else np.zeros(0, _lib.BAM_REGION_DTYPE)
            f.write(struct.pack("<6Q", len(slots), int(off[-1]), len(table), len(regions), len(c["text"]), c.get("n_text", len(c["text"]))))
            f.write(params_array(c["params"]).tobytes() + b"".join(slots) + off.tobytes() + table.tobytes() + regions.tobytes() + bytes(c["text"]))
        f.write(struct.pack("<Q", len(synth)))
        for row, ref_byte, p in synth:
            f.write(params_array(p).tobytes() + struct.pack("<16IB", *row, ref_byte))
    subprocess.check_call([exe, inp, outp])
    b = open(outp, "rb").read()
    at, got = 0, []
    for c in cases:
        rcode, bad, n_sites = struct.unpack_from("<qQQ", b, at)
        at += 24
        sites = site_off = summary = None
        if rcode == 0:
            sites = np.frombuffer(b, _lib.BAM_SITE_DTYPE, n_sites, at)
            at += sites.nbytes
            site_off = np.frombuffer(b, np.uint64, len(c["regions"]) + 1, at).tolist()
            at += 8 * (len(c["regions"]) + 1)
            summary = np.frombuffer(b, _lib.BAM_REGION_SUMMARY_DTYPE, len(c["regions"]), at)
            at += summary.nbytes
        got.append((rcode, bad, n_sites, sites, site_off, summary))
    tiles = []
    for _ in synth:
        n, = struct.unpack_from("<Q", b, at)
        tiles.append(np.frombuffer(b, _lib.BAM_SITE_DTYPE, n, at + 8))
        at += 8 + 32 * n
    assert at == len(b)
    return got, tiles


def want_of(c):
    """the oracle's (sites, site_off, summaries) of a case"""
    return so.sites(c["slots"], c["contigs"], c["text"], c["regions"], n_text=c.get("n_text"), **c["params"])

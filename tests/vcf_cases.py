"""Cases for the VCF writer (tests/test_vcf_rule.py, tests/test_vcf_host_bodies.py, tests/test_gpu_vcf.py): the smallest shapes at
which its kernels can go wrong — digit boundaries of POS and of the counters, contig names around the 16-byte store, every kind
at one position, the ends of the merge's binary searches, regions in any order, reference and inserted bytes that fold, deletions
at a contig's end, around the stage size (STAGE, the product's 256 bytes; the expected lines know nothing of it) and far beyond
it — every refusal of the rule with what the Python restatement (tests/vcf_oracle.py) says of it, and the stand-alone program
that runs the kernels' bodies on the CPU (tests/vcf_host_bodies.cpp)."""
import os
import struct
import subprocess

import numpy as np

import vcf_oracle as vo
from rust_bio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SITE, EVENT = _lib.BAM_SITE_DTYPE, _lib.BAM_INDEL_DTYPE
SNV, DEL, INS = vo.SNV, vo.DEL, vo.INS
STAGE = 256
U32 = 2**32 - 1


def contigs_of(lens, names):
    out, start = [], 0
    for name, ln in zip(names, lens):
        out.append((name, start, ln))
        start += ln + 1
    return out


def text_of(contigs, seed=1, plain=False):
    """the index text S0 $ S1 $ ...: mostly ACGT, one byte in 16 lower-case, one in 24 from "NRYKMSWBDHVnry-*" (plain: neither)"""
    rng = np.random.default_rng(seed)
    n = max([start + ln + 1 for _, start, ln in contigs] + [0])
    t = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    if not plain:
        t = np.where(rng.integers(0, 16, n) == 0, t + 32, t)
        t = np.where(rng.integers(0, 24, n) == 0, rng.choice(np.frombuffer(b"NRYKMSWBDHVnry-*", np.uint8), n), t)
    t = t.astype(np.uint8)
    for _, start, ln in contigs:
        t[start + ln] = ord("$")
    return t.tobytes()


NAMES = [b"1", b"chr_of_15_bytes", b"chr_of_16_bytes_", b"chr_of_17_bytes__", b"n" * 255]
CONTIGS = contigs_of([400, 300, 1200, 80, 50], NAMES)
TEXT = text_of(CONTIGS)
BIG = contigs_of([1_000_100, 64], [b"big", b"behind"])
BIG_TEXT = text_of(BIG, seed=2)


class Lists:
    """the two lists and the inserted bases, appended to in the order the caller wants them"""

    def __init__(self, contigs=CONTIGS, text=TEXT):
        self.contigs, self.text, self.sites, self.events, self.seq = contigs, text, [], [], b""

    def base(self, ref, pos):
        return vo.fold(self.text[self.contigs[ref][1] + pos])

    def snv(self, ref, pos, alt=None, region=0, depth=30, ro=20, fwd=6, rev=4):
        base = self.base(ref, pos)
        alt = alt if alt is not None else next(b for b in b"ACGT" if b != base)
        self.sites.append((ref, pos, region, SNV, base, alt, 0, depth, ro, fwd, rev))
        return self

    def other(self, ref, pos, kind, region=0):
        """a site of kind DEL or INS: it gives no line"""
        self.sites.append((ref, pos, region, kind, self.base(ref, pos), 0, 0, 12, 7, 3, 2))
        return self

    def dele(self, ref, pos, n, region=0, depth=30, fwd=6, rev=4):
        self.events.append((ref, pos, region, DEL, (0, 0, 0), n, depth, fwd, rev, len(self.seq)))
        return self

    def ins(self, ref, pos, s, region=0, depth=30, fwd=6, rev=4):
        self.events.append((ref, pos, region, INS, (0, 0, 0), len(s), depth, fwd, rev, len(self.seq)))
        self.seq += s
        return self

    def case(self, name):
        return dict(name=name, sites=np.array(self.sites, dtype=SITE) if self.sites else np.zeros(0, SITE),
                    events=np.array(self.events, dtype=EVENT) if self.events else np.zeros(0, EVENT), seq=self.seq, contigs=self.contigs,
                    text=self.text, n_text=len(self.text))


def digits():
    v = Lists(BIG, BIG_TEXT)
    counters = [(9, 9, 4, 5), (10, 10, 9, 1), (99, 0, 10, 89), (100, 100, 99, 1), (U32, U32, U32, U32), (U32, 0, U32, 1), (0, 0, 0, 0), (1_000_000, 999_999, 1, 0)]
    for k, pos in enumerate((8, 9, 98, 99, 999, 9_999, 99_999, 999_998, 999_999, 1_000_098)):
        depth, ro, fwd, rev = counters[k % len(counters)]
        v.snv(0, pos, depth=depth, ro=ro, fwd=fwd, rev=rev)
        d2, _, f2, r2 = counters[(k + 3) % len(counters)]
        v.dele(0, pos, 1 + k % 3, depth=d2, fwd=f2, rev=r2).ins(0, pos, b"ACGTA"[:1 + k % 5], depth=depth, fwd=rev, rev=fwd)
    return v.case("POS 9 / 10 .. 999 999 / 1 000 000, counters at 9 / 10, 99 / 100 and 2^32 - 1, AO beyond 2^32")


def names():
    v = Lists()
    for ref in range(len(CONTIGS)):
        v.snv(ref, 7, region=ref).dele(ref, 7, 3, region=ref).ins(ref, 9, b"GT", region=ref)
    return v.case("contig names of 1, 15, 16, 17 and 255 bytes")


def one_position():
    v = Lists()
    base = v.base(2, 500)
    for alt in [b for b in b"ACGT" if b != base]:
        v.snv(2, 500, alt=alt)
    v.other(2, 500, DEL).other(2, 500, INS)
    v.dele(2, 500, 2).ins(2, 500, b"A").ins(2, 500, b"AC")
    v.snv(2, 501).ins(2, 501, b"T")
    return v.case("three SNV alleles, a DEL and two INS at one position")


def merges():
    out = []
    v = Lists()
    for pos in (3, 3, 5, 90, 399):
        v.snv(0, pos)
    out.append(v.case("sites only"))
    v = Lists()
    v.dele(0, 3, 1).ins(0, 3, b"C").dele(0, 90, 5).ins(0, 399, b"ACGT")
    out.append(v.case("events only"))
    out.append(Lists().case("neither"))
    v = Lists()
    v.other(0, 1, DEL).other(0, 2, INS)
    out.append(v.case("sites of kind DEL and INS only: no line"))
    v = Lists()
    v.other(0, 1, DEL).snv(0, 1).other(0, 1, INS).other(0, 2, DEL).other(0, 3, DEL).snv(0, 4).other(0, 4, DEL).other(0, 9, INS).snv(0, 9).other(0, 10, INS)
    v.dele(0, 1, 2).dele(0, 2, 1).ins(0, 4, b"G").ins(0, 9, b"TT").dele(0, 10, 1).ins(0, 11, b"A")
    out.append(v.case("sites of kind DEL and INS interleaved and skipped"))
    v = Lists(contigs=CONTIGS)
    v.dele(2, 10, 1)
    for k in range(300):
        v.snv(2, 11 + k // 2) if k % 7 else v.other(2, 11 + k // 2, DEL)
    v.dele(2, 11 + 150, 1)
    out.append(v.case("a run of 300 sites between two events"))
    v = Lists()
    v.snv(2, 10)
    for k in range(100):
        v.dele(2, 10 + k, 1 + k % 3).ins(2, 10 + k, b"ACGTACGTA"[:1 + k % 9]).ins(2, 10 + k, b"TTGCA"[:1 + k % 5])
    v.snv(2, 10 + 100)
    out.append(v.case("a run of 300 events between two sites"))
    v = Lists()  # regions: 0 = c2[100, 200), 1 = c2[150, 250) overlaps it, 2 = empty, 3 = c2[100, 200) again, 4 = c0: descends, 5 = c2 again
    for region, ref, places in ((0, 2, (100, 150, 199)), (1, 2, (150, 199, 249)), (3, 2, (100, 150, 199)), (4, 0, (0, 399)), (5, 2, (5, 1199))):
        for pos in places:
            v.snv(ref, pos, region=region)
            if pos % 2:
                v.ins(ref, pos, b"CA", region=region)
            elif pos + 2 < CONTIGS[ref][2]:
                v.dele(ref, pos, 1, region=region)
    out.append(v.case("regions that overlap, repeat and descend, an empty region between populated ones"))
    return out


def planted():
    """a contig whose bytes 100 .. 100 + len(ODD) are every byte that folds, an SNV, an insertion and deletions over them"""
    odd = b"acgtnryNRYKMSWBDHVkmswbdhv-*Xx.="
    start = CONTIGS[2][1]
    text = TEXT[:start + 100] + odd + TEXT[start + 100 + len(odd):]
    v = Lists(text=text)
    for k in range(len(odd)):
        v.snv(2, 100 + k).dele(2, 100 + k, 1 + k % 4).ins(2, 100 + k, b"ACGT"[k % 4:k % 4 + 1])
    v.dele(2, 99, len(odd) + 1).dele(2, 100 + len(odd), 3)
    v.events.sort(key=lambda e: (e[2], e[1]))  # (stable: the list stays in (region, pos) order)
    return v.case("lower-case, N, R, Y and every other byte at an anchor and inside a deleted span")


def inserted():
    v = Lists()
    for k, s in enumerate((b"=", b"N", b"M", b"A=C", b"acgt", b"ACGTN=MRWSYKVHDB", b"\0\xff$")):
        v.ins(1, 20 + k, s)
    for k, n in enumerate((1, 15, 16, 17, 33)):
        v.ins(1, 40 + k, (b"ACGT" * 9)[k:k + n])
    return v.case("inserted bytes =, N, M and more; insertions of 1, 15, 16, 17 and 33 bases")


def line_len_of_deletion(v, ref, pos, n):
    w = Lists(v.contigs, v.text).dele(ref, pos, n).case("")
    return len(vo.lines(w["sites"], w["events"], b"", w["contigs"], w["text"])[0])


def deletions():
    out = []
    v = Lists()
    for ref in (0, 1, 3):
        ln = CONTIGS[ref][2]
        assert TEXT[CONTIGS[ref][1] + ln] == ord("$") and TEXT[CONTIGS[ref + 1][1]] != ord("$")
        v.dele(ref, ln - 6, 5, region=ref).dele(ref, ln - 2, 1, region=ref)
    out.append(v.case("deletions that end on their contig's last base"))
    v = Lists()
    n0 = next(n for n in range(1, 400) if line_len_of_deletion(v, 2, 300, n) == STAGE)
    for k, n in enumerate((n0 - 1, n0, n0 + 1)):
        v.snv(2, 300 + k).dele(2, 300 + k, n)
    assert [line_len_of_deletion(v, 2, 300, n) for n in (n0 - 1, n0, n0 + 1)] == [STAGE - 1, STAGE, STAGE + 1]
    for k, n in enumerate((n0 - 1, n0, n0 + 1)):  # and insertions whose lines have these lengths
        v.ins(2, 310 + k, (b"ACGT" * 80)[:n])
    out.append(v.case("deletions whose line is one under, at and one over the stage size"))
    v = Lists(BIG, BIG_TEXT)
    v.snv(0, 1000).dele(0, 1000, 70_000).ins(0, 1000, b"A").snv(0, 50_000).dele(0, 1_000_100 - 70_001, 70_000).dele(1, 0, 63, region=1)
    out.append(v.case("a deletion of 70 000 bases, one more that ends on the contig's last base"))
    return out


def corpus():
    return [digits(), names(), one_position()] + merges() + [planted(), inserted()] + deletions()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def base_case():
    v = Lists()
    for k, pos in enumerate((5, 5, 17, 40, 41, 77)):
        v.snv(1, pos, alt=[b for b in b"ACGT" if b != v.base(1, pos)][k % 3])
    v.other(1, 78, DEL)
    v.snv(3, 10, region=1)
    v.ins(1, 5, b"AC").dele(1, 17, 4).ins(1, 17, b"G").dele(1, 60, 2).ins(3, 10, b"TTT", region=1).dele(3, 70, 9, region=1)
    return v.case("the base of the refusals")


def mutated(c, what, sites=(), events=(), **kw):
    """c with fields of some sites and events set: sites / events are (index, {field: value})"""
    d = dict(c, name=what, sites=c["sites"].copy(), events=c["events"].copy(), **kw)
    for i, fields in sites:
        for f, v in fields.items():
            d["sites"][i][f] = v
    for j, fields in events:
        for f, v in fields.items():
            d["events"][j][f] = v
    return d


def refusals():
    """[case with want = the first refused index]: every check of the rule in the first and in the last element of each list,
    and in both lists at once (the site wins: it has the smaller index)"""
    c = base_case()
    ns, ne, n_seq = len(c["sites"]), len(c["events"]), len(c["seq"])
    len3 = CONTIGS[3][2]
    last_base = vo.fold(TEXT[CONTIGS[3][1] + 10])
    site_faults = [("ref -1", dict(ref=-1)), ("ref n_contigs", dict(ref=len(CONTIGS))), ("pos -1", dict(pos=-1)), ("pos at the contig's length", dict(pos=1200)),
                   ("kind 3", dict(kind=3)), ("kind 255", dict(kind=255)), ("a reserved byte", dict(reserved=1)), ("ref_base is not the text's", dict(ref_base=ord("n"))),
                   ("alt N", dict(alt=ord("N"))), ("alt lower-case", dict(alt=ord("a"))), ("alt 0", dict(alt=0))]
    event_faults = [("ref -1", dict(ref=-1)), ("ref n_contigs", dict(ref=len(CONTIGS))), ("pos -1", dict(pos=-1)), ("pos at the contig's length", dict(pos=1200)),
                    ("kind SNV", dict(kind=SNV)), ("kind 3", dict(kind=3)), ("a reserved byte", dict(reserved=(0, 0, 7))), ("len 0", dict(len=0))]
    out = []
    for what, f in site_faults:
        out += [dict(mutated(c, "first site: " + what, sites=[(0, f)]), want=0), dict(mutated(c, "last site: " + what, sites=[(ns - 1, f)]), want=ns - 1)]
    for what, f in event_faults:
        out += [dict(mutated(c, "first event: " + what, events=[(0, f)]), want=ns), dict(mutated(c, "last event: " + what, events=[(ne - 1, f)]), want=ns + ne - 1)]
    out += [dict(mutated(c, "first site: alt is ref_base", sites=[(0, dict(alt=int(c["sites"][0]["ref_base"])))]), want=0),
            dict(mutated(c, "last site: alt is ref_base", sites=[(ns - 1, dict(alt=last_base))]), want=ns - 1),
            dict(mutated(c, "first event: an insertion one byte past the bases", events=[(0, dict(seq_off=n_seq - 1))]), want=ns),
            dict(mutated(c, "an insertion whose seq_off + len wraps", events=[(0, dict(seq_off=2**64 - 1))]), want=ns),
            dict(mutated(c, "last event: a deletion up to the contig's end", events=[(ne - 1, dict(len=len3 - 70))]), want=ns + ne - 1),
            dict(mutated(c, "a deletion of 2^32 - 1", events=[(1, dict(len=U32))]), want=ns + 1),
            dict(mutated(c, "second site: behind its predecessor", sites=[(1, dict(pos=4))]), want=1),
            dict(mutated(c, "last site: a region below its predecessor's", sites=[(ns - 2, dict(region=2))]), want=ns - 1),
            dict(mutated(c, "second event: behind its predecessor", events=[(1, dict(pos=4))]), want=ns + 1),
            dict(mutated(c, "last event: behind its predecessor", events=[(ne - 1, dict(pos=9))]), want=ns + ne - 1),
            dict(mutated(c, "both lists: the site wins", sites=[(ns - 1, dict(kind=9))], events=[(0, dict(len=0))]), want=ns - 1),
            dict(mutated(c, "both lists, first elements", sites=[(0, dict(pos=-5))], events=[(0, dict(ref=99))]), want=0),
            dict(mutated(c, "the last contig the lists use runs past the text", n_text=CONTIGS[3][1] + len3 - 1), want=ns - 1),
            dict(mutated(c, "no text at all", n_text=0), want=0),
            dict(mutated(c, "no contig at all", contigs=[]), want=0)]
    return out


# ---- the program ------------------------------------------------------------------------------------------------------------
def build_program(exe, sanitize):
    """the program of vcf_host_bodies.cpp, built as bam_indels_cases.build_program builds its own"""
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + _lib.CSRC] + flags + [os.path.join(ROOT, "tests", "vcf_host_bodies.cpp"), "-o", exe])
    return exe


def contig_arrays(contigs):
    """(bg_sam_contig_t[], the names' bytes)"""
    table, names = np.zeros(len(contigs), dtype=_lib.SAM_CONTIG_DTYPE), b""
    for k, (name, start, ln) in enumerate(contigs):
        table[k] = (start, ln, len(names), len(name), 0)
        names += bytes(name)
    return table, names


def run_program(exe, tmp, cases):
    """cases -> [(rc, first_bad, n_lines, out_bytes, text or None, line_off or None)]; a case's text is cut to the n_text it tells"""
    inp, outp = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for c in cases:
            table, names = contig_arrays(c["contigs"])
            text = c["text"][:c["n_text"]]
            f.write(struct.pack("<6Q", len(c["sites"]), len(c["events"]), len(c["seq"]), len(table), len(names), len(text)))
            f.write(c["sites"].tobytes() + c["events"].tobytes() + c["seq"] + table.tobytes() + names + text)
    subprocess.check_call([exe, inp, outp])
    b = open(outp, "rb").read()
    at, got = 0, []
    for c in cases:
        rcode, bad, n_lines, out_bytes = struct.unpack_from("<qQQQ", b, at)
        at += 32
        text = line_off = None
        if rcode == 0:
            text = b[at:at + out_bytes]
            at += out_bytes
            line_off = np.frombuffer(b, np.uint64, n_lines + 1, at).tolist()
            at += 8 * (n_lines + 1)
        got.append((rcode, bad, n_lines, out_bytes, text, line_off))
    assert at == len(b)
    return got


def want_of(c):
    """the oracle's (text, line_off) of a case"""
    return vo.emit(c["sites"], c["events"], c["seq"], c["contigs"], c["text"], c["n_text"])

"""Cases for the left-aligned indel events (tests/test_bam_indels_left_rule.py, tests/test_bam_indels_left_host_bodies.py,
tests/test_gpu_bam_indels_left.py): texts with runs and tandem copies planted where the product's tile (T = 512) ends, events
that land one and two tiles in front of their raw anchor, regions that hold only the raw or only the shifted anchor, insertions
at the word borders of the packed bases with k below, at and above their length, spellings that meet only behind the shift, more
records than four strides of a workgroup on one event, and the whole corpus of tests/bam_indels_cases.py with max_shift 0, where
the expected result is the older oracle's.  The refusals with what the Python restatement (tests/bam_indels_left_oracle.py) says
of each, and the stand-alone program that runs the kernels' bodies on the CPU (tests/bam_indels_host_bodies.cpp, its left
flavour).  The expected events know nothing of tiles."""
import numpy as np

import bam_indels_cases as ic
import bam_indels_left_oracle as lo
import bam_pileup_cases as pc
import bam_sites_cases as sc

ROOT = pc.ROOT
T = pc.T
CONTIGS = pc.CONTIGS
NO_LIMIT = lo.NO_LIMIT
CODE = {65: 1, 67: 2, 71: 4, 84: 8}
M, I, D, S = 0, 1, 2, 4


def text_for(contigs, planted=()):
    """S0 $ S1 $ ...: ACGT over and over (no two adjacent bytes equal, so nothing shifts by itself), then `planted`: (contig, beg,
    bytes) written over it"""
    n = max(start + ln + 1 for _, start, ln in contigs)
    t = bytearray(n)
    for _, start, ln in contigs:
        t[start:start + ln] = (b"ACGT" * (ln // 4 + 1))[:ln]
        t[start + ln] = ord("$")
    for c, beg, what in planted:
        assert 0 <= beg and beg + len(what) <= contigs[c][2]
        t[contigs[c][1] + beg:contigs[c][1] + beg + len(what)] = what
    return bytes(t)


def run_of(beg, n):
    """n equal bytes at beg that differ from the pattern's bytes on both sides"""
    around = {b"ACGT"[(beg - 1) % 4], b"ACGT"[(beg + n) % 4]}
    return bytes([next(b for b in b"ACGT" if b not in around)]) * n


def case(name, slots, regions, text, contigs=CONTIGS, n_text=None, **kw):
    return dict(name=name, slots=slots, contigs=contigs, text=text, n_text=len(text) if n_text is None else n_text, regions=regions, params=lo.params(**kw))


def del_rec(ref, pos, anchor, n=1, tail=6, flag=0, name=b"d"):
    """<anchor - pos + 1>M <n>D <tail>M at (ref, pos)"""
    lead = anchor - pos + 1
    return pc.rec(ref, pos, ic.words((lead, M), (n, D), (tail, M)), codes=[1] * (lead + tail), flag=flag, name=name)


# ---- the tile's edge --------------------------------------------------------------------------------------------------------
def edge_text():
    """runs of two equal bytes at T - 1, 2 T and 3 T + 1 of c0: a one-base deletion anchored on a run's first byte shifts by one"""
    return text_for(CONTIGS, [(0, b, run_of(b, 2)) for b in (T - 1, 2 * T, 3 * T + 1)])


def edge_records():
    """raw anchors T - 1, 2 T and 3 T + 1 (relative to a tile's edge: T - 1, T, T + 1), each on both strands, each shifting by one;
    beside every one a deletion two positions behind that does not shift"""
    out = []
    for a in (T - 1, 2 * T, 3 * T + 1):
        out += [del_rec(0, a - 9, a, flag=f, name=b"e%d_%d" % (a, f)) for f in (0, 0x10)]
        out += [del_rec(0, a - 9, a + 2, name=b"s%d" % a)]
    return pc.by_position(out)


def edge_regions():
    whole = CONTIGS[0][2]
    return [(0, 0, whole), (0, 1, whole), (0, 2, whole), (0, T - 2, T - 1), (0, T - 1, T), (0, 2 * T - 1, 2 * T), (0, 2 * T, 2 * T + 1), (0, 3 * T, 3 * T + 1),
            (0, T - 2, 3 * T + 2), (0, 3 * T + 1, 3 * T + 2)]


# ---- two tiles in front -----------------------------------------------------------------------------------------------------
RUN = (50, 1150)  # of c1: 1 100 equal bytes


def long_text():
    return text_for(CONTIGS, [(1, RUN[0], run_of(RUN[0], RUN[1] - RUN[0]))])


def long_records():
    """one record of 1 200 aligned bases at c1:40 whose deletion of the run's last byte (raw anchor 1148, the third tile of a region
    that begins at 0) lands at 49 (the first tile); plain reads in front and behind"""
    return pc.by_position([pc.rec(1, 40, b"1109M1D90M", codes=[2] * 1199, name=b"long"), pc.rec(1, 30, b"40M", name=b"front"), pc.rec(1, 1100, b"80M", name=b"back")])


def long_regions():
    """the whole contig; one that holds the raw anchor only (no event); one that holds the shifted one only; one position,
    overlapping, repeated, descending"""
    return [(1, 0, 3 * T), (1, 1100, 1200), (1, 40, 60), (1, 49, 50), (1, 49, 50), (1, 0, 100), (1, 30, 70), (1, 1000, 3 * T), (1, 500, 800), (1, 0, 50),
            (1, 48, 49), (1, 1148, 1149)]


# ---- insertions at the word borders -----------------------------------------------------------------------------------------
def _spans():
    """of c3: where three copies of a unit of n bytes begin, one place for each of k = n - 1 (0 for n = 1), n and n + 2, so that
    no raw event is carried by records of different pos"""
    out, at = {}, 20
    for n in (1, 15, 16, 17, 33):
        for k in (max(n - 1, 0), n, n + 2):
            out[(n, k)] = at
            at += 3 * n + 5
    assert at < CONTIGS[3][2]
    return out


SPANS = _spans()


def unit(n):
    rng = np.random.default_rng(100 + n)
    u = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist())
    return u if n > 1 else b"G"


def word_text():
    """three copies of unit(n) at every place of SPANS, a byte in front that is not the unit's last"""
    planted = []
    for (n, _), b in SPANS.items():
        u = unit(n)
        planted += [(3, b - 1, bytes([next(x for x in b"ACGT" if x != u[-1])])), (3, b, u * 3)]
    return text_for(CONTIGS, planted)


def ins_at(ref, pos, anchor, seq, soft=0, flag=0, tail=3, name=b"i"):
    return ic.ins_rec(ref, pos, [CODE[b] for b in seq], lead=anchor - pos + 1, tail=tail, soft=soft, flag=flag, name=name)


def word_records():
    """the unit inserted behind its third copy, by records whose pos stops the shift after n - 1 (or 0), n and n + 2 steps, each at
    q even and odd and on both strands; beside the k = n + 2 ones the unit one copy earlier from the same pos (equal only behind
    the shift, another record and another k) and the unit rotated by one behind the anchor in front (another spelling); beside
    the k = n - 1 ones a unit that differs in its FIRST byte, which n - 1 steps carry to the LAST byte of the shifted sequence"""
    out = []
    for (n, k), b in SPANS.items():
        u, a = unit(n), b + 3 * n - 1
        for soft, flag in ((0, 0), (1, 0x10)):
            out.append(ins_at(3, a - k, a, u, soft=soft, flag=flag, name=b"w%d_%d_%d" % (n, k, soft)))
        if k == n + 2:
            out.append(ins_at(3, a - k, a - n, u, soft=1, name=b"copy%d" % n))
            out.append(ins_at(3, a - k, a - 1, u[-1:] + u[:-1], name=b"rot%d" % n))
        if k == n - 1 and n > 1:
            v = bytes([next(x for x in b"ACGT" if x != u[0])]) + u[1:]
            out.append(ins_at(3, a - k, a, v, soft=1, name=b"last%d" % n))
    return pc.by_position(out)


def split_records():
    """ONE raw event (the unit of 15 behind its third copy) carried by records of three different pos: each stops at its own pos,
    so the one event of bg_bam_indels leaves as three.  The rule says so (`a record that begins inside a repeat stops at its own
    pos`); it is the one case where the shifted events are more than the unshifted ones"""
    b = SPANS[(15, 17)]
    a = b + 3 * 15 - 1
    return pc.by_position([ins_at(3, a - k, a, unit(15), name=b"split%d" % k) for k in (14, 15, 17)])


# ---- one event of many records ----------------------------------------------------------------------------------------------
def pile_text():
    return text_for(CONTIGS, [(0, 300, run_of(300, 8))])


def pile_records(n=1100):
    """1 100 records at c0:295 whose one-base deletions cycle over the seven anchors 299 .. 305 of a run of eight, both strands"""
    return [del_rec(0, 295, 299 + k % 7, tail=10, flag=0x10 * (k % 3 == 0), name=b"p") for k in range(n)]


def corpus(with_deep=True):
    edge, long_, word, pile = edge_text(), long_text(), word_text(), pile_text()
    out = [case("raw anchors at T - 1, T and T + 1 of a tile that shift by one", edge_records(), edge_regions(), edge, exclude=0),
           case("the same, both strands asked for and one step allowed", edge_records(), edge_regions(), edge, exclude=0, min_alt_strand=1, max_shift=1),
           case("the same, no step allowed", edge_records(), edge_regions(), edge, exclude=0, max_shift=0),
           case("a deletion that lands two tiles in front of its raw anchor", long_records(), long_regions(), long_, exclude=0),
           case("the same, max_shift ends it inside the middle tile", long_records(), long_regions() + [(1, 648, 649), (1, 600, 700)], long_, exclude=0, max_shift=500),
           case("the same, max_shift ends it on the middle tile's first position", long_records(), long_regions(), long_, exclude=0, max_shift=1148 - T),
           case("the same, max_shift ends it on the middle tile's last position", long_records(), long_regions(), long_, exclude=0, max_shift=1148 - 2 * T + 1),
           case("insertions of 1, 15, 16, 17 and 33 bases with k below, at and above their length", word_records(), [(3, 0, 1000), (3, 45, 60), (3, 400, 500)], word,
                exclude=0),
           case("the same insertions, three steps at most", word_records(), [(3, 0, 1000)], word, exclude=0, max_shift=3),
           case("the same insertions, at least two records an event", word_records(), [(3, 0, 1000)], word, exclude=0, min_alt=2),
           dict(case("one raw event from three pos: three events", split_records(), [(3, 0, 1000)], word, exclude=0), splits=True),
           case("1 100 records, seven spellings, one event", pile_records(), [(0, 0, T), (0, 298, 300), (0, 299, 306)], pile, exclude=0),
           case("1 100 records, seven spellings, two steps", pile_records(), [(0, 0, T)], pile, exclude=0, max_shift=2, min_alt=150)]
    for c in ic.corpus(with_deep):
        out.append(dict(name=c["name"] + ", max_shift 0", slots=c["slots"], contigs=c["contigs"], text=None, n_text=None, regions=c["regions"],
                        params=dict(c["params"], max_shift=0), plain=True))
    by = {c["name"]: c for c in ic.corpus(False)}
    for name in ("everything, region shapes", "random records, no threshold", "random records, strict"):
        c = by[name]
        out.append(dict(name=name + ", against a random text", slots=c["slots"], contigs=c["contigs"], text=None, n_text=None, regions=c["regions"],
                        params=dict(c["params"], max_shift=NO_LIMIT)))
    texts = {}
    for c in out:
        if c["text"] is None:
            key = tuple(c["contigs"])
            if key not in texts:
                texts[key] = sc.text_of(c["contigs"])
            c["text"], c["n_text"] = texts[key], len(texts[key])
    return out


def refusals():
    """[dict(..., want=(status, slot))]: those of tests/bam_indels_cases.py (held against a text that fits), a region whose contig
    lies outside the text by one byte, and a text of no byte.  n_text is what the call is told: a refusal reads no byte of the
    text, so the one contig of 2^29 bases has none behind it"""
    out = []
    for c in ic.refusals():
        contigs = c["contigs"]
        big = max([start + ln + 1 for _, start, ln in contigs] + [0]) > 1 << 20
        text = sc.TEXT if contigs is CONTIGS else b"ACGT" if big else sc.text_of(contigs)
        out.append(dict(c, text=text, n_text=contigs[-1][1] + contigs[-1][2] + 1 if big else len(text), params=lo.params(**c["params"])))
    text = edge_text()
    end = CONTIGS[1][1] + CONTIGS[1][2]
    out += [dict(name="a contig that ends one byte behind the text", slots=edge_records(), contigs=CONTIGS, text=text, n_text=end - 1, regions=[(0, 0, 10), (1, 0, 0)],
                 params=lo.params(), want=(lo.INVALID_ARG, None)),
            dict(name="a text of no byte", slots=edge_records(), contigs=CONTIGS, text=text, n_text=0, regions=[(0, 0, 10)], params=lo.params(),
                 want=(lo.INVALID_ARG, None)),
            dict(name="min_alt_permille above 1000", slots=edge_records(), contigs=CONTIGS, text=text, n_text=len(text), regions=[(0, 0, 10)],
                 params=lo.params(min_alt_permille=1001), want=(lo.INVALID_ARG, None))]
    return out


def want_of(c):
    """the oracle's (events, seq, event_off) of a case"""
    return lo.indels(c["slots"], c["contigs"], c["text"], c["regions"], n_text=c["n_text"], **c["params"])


# ---- the program: bam_indels_cases' own, which takes a case's text -----------------------------------------------------------
build_program = ic.build_program
run_program = ic.run_program

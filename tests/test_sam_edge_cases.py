"""The cases of tests/sam_edge_cases.py hold what they are for — derived from the oracles alone (tests/sam_oracle.py,
tests/sam_sort_oracle.py), without a GPU.  Nothing else is asserted here: the GPU tests that import the same generators
(test_gpu_sam_emit_edges.py, test_gpu_sam_keys.py, test_gpu_sam_sort.py, test_gpu_sam_markdup.py) compare bytes, and this file
is the proof that they cannot pass vacuously."""
import re

import pytest

import sam_edge_cases as ec
import sam_oracle as so
import sam_sort_oracle as sso
from sam_edge_cases import fields, tag


def digits(values):
    return {len(b"%d" % abs(v)) for v in values}


def by_kind(case, value, want_kinds=("forward", "reverse")):
    """{kind: set of value(line)} over the case's lines; kind: forward, reverse, unplaced, secondary"""
    out = {"forward": set(), "reverse": set(), "unplaced": set(), "secondary": set()}
    for line in case.want():
        if not line:
            continue
        flag = int(fields(line)[1])
        kind = "secondary" if flag & 0x100 else "unplaced" if flag & 0x4 else "reverse" if flag & 0x10 else "forward"
        v = value(line)
        if v is not None:
            out[kind].add(v)
    return out


def test_pos_and_pnext():
    case = ec.emit_case("pos_pnext")
    pos, pnext = by_kind(case, lambda l: int(fields(l)[3])), by_kind(case, lambda l: int(fields(l)[7]))
    for kind in ("forward", "reverse", "unplaced"):
        assert pos[kind] >= set(ec.POS_VALUES) and digits(pos[kind]) == set(range(1, 11)), kind
        assert pnext[kind] >= set(ec.POS_VALUES), kind
    assert all(int(h["ref_start"]) >= 2**40 for h in case.hits if int(h["aln"]["score"]) != so.MIN_SCORE) and max(pos["forward"]) < 2**32


def test_tlen():
    case = ec.emit_case("tlen")
    t = by_kind(case, lambda l: int(fields(l)[8]))
    both = {s for v in ec.SPANS for s in (v, -v)}
    assert t["forward"] == both and t["reverse"] == both and t["unplaced"] == {0}
    assert digits(both) == set(range(1, 11))
    # equal starts: mate 1 positive, mate 2 negative
    want = case.want()
    ties = [(int(fields(want[s])[8]), int(fields(want[s + 1])[8])) for s in range(0, case.n, 2)
            if fields(want[s])[3] == fields(want[s + 1])[3] and fields(want[s])[2] == fields(want[s + 1])[2] and int(fields(want[s])[8])]
    assert len(ties) >= len(ec.POS_VALUES) and all(a > 0 and b == -a for a, b in ties)


def test_as_and_xs():
    case = ec.emit_case("as_xs")
    a, x = by_kind(case, lambda l: int(tag(l, b"AS:i:") or 0)), by_kind(case, lambda l: None if tag(l, b"XS:i:") is None else int(tag(l, b"XS:i:")))
    for kind in ("forward", "reverse", "secondary"):
        assert a[kind] >= set(ec.SCORES), kind
    assert x["forward"] >= set(ec.SCORES) and x["reverse"] >= set(ec.SCORES) and not x["secondary"] and not x["unplaced"]
    assert so.MIN_SCORE + 1 == -858993458 in a["forward"]
    assert sum(tag(l, b"XS:i:") is None and int(tag(l, b"AS:i:")) < 0 and not int(fields(l)[1]) & 0x100 for l in case.want() if l and tag(l, b"AS:i:")) >= 2


def test_mapq():
    m = by_kind(ec.emit_case("mapq"), lambda l: int(fields(l)[4]))
    assert m["forward"] == m["reverse"] == set(ec.MAPQS) and m["secondary"] == m["unplaced"] == {0}
    m = by_kind(ec.emit_case("mapq_255"), lambda l: int(fields(l)[4]))
    assert m["forward"] == m["reverse"] == {255} and m["secondary"] == m["unplaced"] == {0}


def test_nm():
    n = by_kind(ec.emit_case("nm"), lambda l: None if tag(l, b"NM:i:") is None else int(tag(l, b"NM:i:")))
    assert n["forward"] == n["reverse"] == n["secondary"] == set(ec.NMS) and not n["unplaced"]


def test_cigar():
    case = ec.emit_case("cigar")

    def runs(line):
        c = fields(line)[5]
        return None if c == b"*" else frozenset((int(n), op) for n, op in re.findall(rb"([0-9]+)([=XDIS])", c))
    r = by_kind(case, runs)
    for kind in ("forward", "reverse", "secondary"):
        seen = set().union(*r[kind])
        assert seen >= {(n, op) for n in ec.RUNS for op in (b"=", b"D", b"I", b"X", b"S")}, kind
    # clips at either end
    cig = [fields(l)[5] for l in case.want() if l]
    for n in ec.RUNS:
        assert any(c.startswith(b"%dS" % n) and c.endswith(b"%dS" % n) for c in cig), n
    assert b"65535=" in cig and max(len(l) for l in case.want()) > 130_000


def test_md():
    case = ec.emit_case("md")
    m = by_kind(case, lambda l: tag(l, b"MD:Z:"))
    for kind in ("forward", "reverse", "secondary"):
        mds = m[kind]
        assert all(any(re.fullmatch(rb"0[ACGT]%d[ACGT]0" % r, s) for s in mds) for r in ec.RUNS), kind
        assert any(re.fullmatch(rb"0[ACGT]0[ACGT]0", s) for s in mds), kind                 # adjacent mismatches
        assert {len(x) for s in mds for x in re.findall(rb"\^([ACGT]+)", s)} == {1, 100}, kind
        assert any(re.fullmatch(rb"1[ACGT]0\^[ACGT]1", s) for s in mds), kind               # a deletion directly behind a mismatch
        assert any(re.fullmatch(rb"1\^[ACGT]0[ACGT]1", s) for s in mds), kind               # a mismatch directly behind a deletion
    assert not m["unplaced"]


@pytest.mark.parametrize("paired", [True, False])
def test_flag(paired):
    case = ec.emit_case("flag_paired" if paired else "flag_secondary")
    want = case.want()
    flags = {int(fields(l)[1]) for l in want if l}
    assert flags == ec.expected_flags(paired), (sorted(flags - ec.expected_flags(paired)), sorted(ec.expected_flags(paired) - flags))
    assert set(case.dup.tolist()) == set(ec.DUPS)
    # never on an unplaced line, although reads with a dup byte have unplaced lines; on every placed line of a flagged read
    for s, l in enumerate(want):
        if l:
            f = int(fields(l)[1])
            assert bool(f & 0x400) == (not f & 0x4 and case.dup[s // case.K] != 0)
    assert sum(bool(l) and int(fields(l)[1]) & 0x4 and case.dup[s // case.K] != 0 for s, l in enumerate(want)) >= 6
    if not paired:
        assert {int(case.dup[s // 2]) for s, l in enumerate(want) if l and int(fields(l)[1]) & 0x500 == 0x500} == {1, 0x7e, 255}


def test_qname():
    q = by_kind(ec.emit_case("qname_single"), lambda l: fields(l)[0])
    for kind in ("forward", "reverse", "unplaced"):
        assert q[kind] == {b"*", b"x", b"/1", b"a/1", ec.LONG_ID + b"/1", b"z" * 255}, kind
    case = ec.emit_case("qname_paired")
    want = case.want()
    for first, kept, cut in ((True, b"/2", b"/1"), (False, b"/1", b"/2")):
        names = [(bytes(case.fq.text[int(r["id_off"]):int(r["id_off"]) + int(r["id_len"])]), fields(want[i])[0], int(fields(want[i])[1]))
                 for i, r in enumerate(case.fq.recs) if (i % 2 == 0) == first]
        for kind in (0x0, 0x10, 0x4):
            got = {(a, b) for a, b, f in names if f & 0x14 == kind}
            assert got == {(b"", b"*"), (b"x", b"x"), (kept, kept), (cut, cut), (b"a" + kept, b"a" + kept), (b"a" + cut, b"a"),
                           (ec.LONG_ID + kept, ec.LONG_ID + kept), (ec.LONG_ID + cut, ec.LONG_ID), (b"z" * 255, b"z" * 255)}, (first, kind)


def test_rname():
    case = ec.emit_case("rname")
    names = {c[0] for c in ec.NAME_CONTIGS}
    assert {len(n) for n in names} >= {1, 200}
    r, nx = by_kind(case, lambda l: fields(l)[2]), by_kind(case, lambda l: fields(l)[6])
    assert r["forward"] == r["reverse"] == names and r["unplaced"] == names | {b"*"}
    for kind in ("forward", "reverse"):
        assert nx[kind] == names | {b"="}, kind
    assert nx["unplaced"] == {b"=", b"*"}


def test_staging_limit():
    case = ec.emit_case("staging_limit")
    pairs = ec.staged_pairs(case)
    assert pairs == {(res, total, placed) for res in range(16) for total in (ec.STAGE, ec.STAGE + 1) for placed in (False, True)}
    want = case.want()
    for s in case.targets:  # the placed ones: reverse strand, all tags
        if not int(fields(want[s])[1]) & 0x4:
            assert int(fields(want[s])[1]) & 0x10 and all(tag(want[s], t) for t in (b"AS:i:", b"NM:i:", b"MD:Z:"))
    case = ec.emit_case("stage_1024")
    assert ec.staged_pairs(case) == {(0, length, placed) for length in (1023, 1024, 1025, 1026) for placed in (False, True)}


def test_grid():
    for n in ec.GRID_SLOTS:
        case = ec.emit_case("grid_%d_K1" % n)
        assert len(case.want()) == n and all(case.want())
        assert n < 3 or {bool(int(fields(l)[1]) & 0x4) for l in case.want()} == {False, True}
    assert {n for n in ec.GRID_SLOTS} == {1, 15, 16, 17, 255, 256, 257, 2047, 2048, 2049}
    slots = set()
    for n in ec.GRID_READS_K8:
        want = ec.emit_case("grid_%d_K8" % n).want()
        slots.add(len(want))
        assert not want[-1], "the very last slot writes no line"
        if n >= 33:  # the first slot of every 256-slot block follows an empty one
            assert all(want[s] and not want[s - 1] for s in range(256, len(want), 256))
        if n >= 96:  # whole groups of slots, and all but every eighth slot of three 256-slot blocks, write nothing
            assert all(bool(want[s]) == (s % 8 == 0) for s in range(512, 768))
        if n >= 3:
            kinds = {sum(bool(x) for x in want[8 * r:8 * r + 8]) for r in range(n)}
            assert kinds >= {1, 8}
    assert slots == {8, 16, 24, 248, 256, 264, 2040, 2048, 2056}
    want = ec.emit_case("nothing_placed").want()
    assert all(int(fields(l)[1]) & 0x4 for l in want if l) and sum(bool(l) for l in want) == 40 and not any(want[1::2])
    want = ec.emit_case("one_empty_read").want()
    assert len(want) == 1 and fields(want[0])[9:11] == [b"*", b"*"]


def test_key_batches():
    total = {}
    seen = {}
    names = set()
    for b in ec.key_batches():
        names.add((bool(b.flags & so.PAIRED), b.K, bool(b.flags & so.SECONDARY)))
        key = sso.sort_keys(b.contigs, b.hits, b.strand, b.flags, b.K, events=seen)
        for k, v in b.counts().items():
            total[k] = total.get(k, 0) + v
        if b.name.endswith("unmapped"):
            assert (key == ec.TOP).all()
    print("key batches:", total, seen)
    assert all(v >= 20 for v in total.values()) and len(total) == 4, total
    assert seen["key UINT64_MAX"] >= 1000
    assert names == {(False, 1, False), (True, 1, False), (False, 4, False), (False, 4, True)}
    assert {b.n * b.K for b in ec.key_batches()} >= {1, 255, 256, 257, 2800}
    assert {b.flags & (so.TAG_NM | so.TAG_MD) for b in ec.key_batches()} == {0, so.TAG_NM, so.TAG_MD, so.TAG_NM | so.TAG_MD}
    big = [b for b in ec.key_batches() if b.contigs is ec.BIG_CONTIGS]
    key = sso.sort_keys(big[0].contigs, big[0].hits, big[0].strand, big[0].flags, big[0].K)
    real = key[key != ec.TOP]
    assert len(big) == 1 and len({int(k) >> 32 for k in real}) >= 3 and len({int(k) & 0xFFFFFFFF for k in real} & {int(k) & 0xFFFFFFFF for k in real if k >> 32}) > 0


def test_sort_batches():
    b = ec.sort_switch()
    placed = [p for p in b.placed() if p[0] >= 16383]
    assert {(ln, res) for ln, res, _ in placed} == {(ln, res) for ln in ec.SWITCH_LENGTHS for res in ec.RESIDUES}
    assert len({d for _, _, d in placed}) >= 3
    b = ec.sort_chunk()
    placed = b.placed()
    assert {ln for ln, _, _ in placed} == {base + d for base in ec.CHUNK_BASES for d in ec.CHUNK_DELTAS}
    assert {res for _, res, _ in placed} == set(ec.RESIDUES) and len({d for _, _, d in placed}) >= 3
    # chunks of a line as the long-line kernel counts them: c with c * 256 <= len >> 4
    assert {(ln >> 4) // 256 + 1 for ln, _, _ in placed} == {5, 6, 32, 33, 34}
    for n in (255, 256, 257):
        b = ec.sort_rows(n)
        lens = [len(r) for r in b.recs]
        longs = [ln for ln in lens if ln > ec.LONG_LINE]
        assert len(longs) == n and all(16_385 <= ln <= 16_500 for ln in longs) and 0 in lens and ec.TOP in b.key.tolist()
        perm, _, _ = sso.sort(b.key, b.recs)
        order = [int(i) for i in perm if lens[int(i)] > ec.LONG_LINE]
        assert order != sorted(order)
        assert sum(len(r) for r in b.recs) < 4_600_000
    for which in ("first", "last"):
        b = ec.sort_ends(which)
        perm, _, _ = sso.sort(b.key, b.recs)
        assert len(b.recs[int(perm[0 if which == "first" else -1])]) == 20_000
    # the keys come back from the hit records the stand-alone host program is fed
    fq, hits, strand = ec.sort_switch().hits()
    assert (sso.sort_keys(ec.CONTIGS, hits, strand) == ec.sort_switch().key).all()


def test_quality_lengths():
    fq, hits, strand = ec.qual_lengths()
    assert tuple(int(r["qual_len"]) for r in fq.recs[::3]) == ec.QUAL_LENGTHS
    quals = bytes(fq.qual)
    assert {q < ec.PHRED for q in quals} == {False, True} and set(ec.LEVELS) <= set(quals)
    for mq in ec.MIN_QUALS:
        dup, counts = sso.markdup(ec.CONTIGS, fq, hits, strand, 0, 1, ec.PHRED, mq)
        assert dup.tolist() == [0, 1, 1] + [1, 1, 0] * (len(ec.QUAL_LENGTHS) - 1) and counts == [len(dup), 2 * len(ec.QUAL_LENGTHS), 0, 0]
        # the winner is decided by the last byte: without it the members of a group tie and the first would win
        for g in range(1, len(ec.QUAL_LENGTHS)):
            recs = fq.recs[3 * g:3 * g + 3]
            body = {quals[int(r["qual_off"]):int(r["qual_off"]) + int(r["qual_len"]) - 1] for r in recs}
            score = [sso.score_of(quals[int(r["qual_off"]):int(r["qual_off"]) + int(r["qual_len"])], ec.PHRED, mq) for r in recs]
            assert len(body) == 1 and score[2] > max(score[:2])
    fq, hits, strand = ec.fragments_only()
    seen = {}
    dup, counts = sso.markdup(ec.CONTIGS, fq, hits, strand, so.PAIRED, 1, ec.PHRED, 15, events=seen)
    assert counts[0] == len(fq.recs) // 2 and counts[2] == counts[3] == 0 and seen["pair group"] == 0 and seen["fragment group"] >= 10 and counts[1] >= 20

"""The Python restatement of the left-aligned indel events (tests/bam_indels_left_oracle.py) pinned to known answers written by
hand from the rule (tests/golden/bam_indels_left_kats.json: a homopolymer, a tandem repeat walked further than the insertion is
long, a deleted unit, a record that begins inside the run, max_shift 0, 1, 2 and beyond the run, soft-masked, N, IUPAC and `=`
bytes, the contig's last base, one record twice, min_baseq, thresholds that only the joined event passes) at both levels, the
tally and the events, and through tests/vcf_oracle.py to REF and ALT; a verifier that shares nothing with that restatement
(string surgery on the contig: the edited contig is the same before and behind the shift, and no further step would keep it the
same unless pos, max_shift, a non-base or the contig's end forbids it) over every case of tests/bam_indels_left_cases.py; the
binding's struct against the header; and, through ctypes without a GPU, the argument checks of bg_bam_indels_left[_dev]."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import bam_indels_left_cases as lc
import bam_indels_left_oracle as lo
import bam_indels_oracle as io
import bam_pileup_cases as pc
import bam_pileup_oracle as po
import vcf_oracle as vo
from rust_bio_amd import _lib, bam

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KATS = json.load(open(os.path.join(GOLDEN, "bam_indels_left_kats.json")))["kats"]
INVALID_ARG, TOO_LARGE = -1, -8
CODES = {b: c for c, b in enumerate(io.ASCII)}


def events_of(listed):
    """the JSON's events as the oracle's tuples and their strings: seq_off is the running sum of the insertions in front"""
    out, at = [], 0
    for pos, kind, n, seq, depth, fwd, rev in listed:
        assert len(seq) == (n if kind == io.INS else 0)
        out.append((0, pos, 0, kind, n, depth, fwd, rev, at))
        at += len(seq)
    return out, "".join(e[3] for e in listed).encode()


def kat_inputs(k):
    text = k["contig"].encode() + b"$"
    contigs = [(b"k", 0, len(k["contig"]))]
    slots = []
    for flag, pos, cigar, seq, qual in k["records"]:
        n = pc.query_len(cigar.encode())
        q = b"*" if qual is None else bytes(v + 33 for v in qual)
        slots.append(po.record(b"r", flag, b"k", pos + 1, 60, cigar.encode(), (seq or "A" * n).encode(), contigs, q))
    return slots, contigs, text, [(0, 0, len(k["contig"]))]


def test_hand_made_known_answers_at_both_levels():
    seen = lines = plains = 0
    for k in KATS:
        slots, contigs, text, regions = kat_inputs(k)
        for v in k["variants"]:
            p = lo.params(exclude=0, **v["params"])
            tally = lo.tally(slots, contigs, text, p)
            want = {(0, a, kind, n, tuple(CODES[b] for b in s.encode())): [fwd, rev] for a, kind, n, s, fwd, rev in v["tally"]}
            assert tally == want, (k["name"], v["params"])
            events, seq, event_off = lo.indels(slots, contigs, text, regions, **p)
            assert (events, seq) == events_of(v["events"]), (k["name"], v["params"])
            assert event_off == [0, len(events)], (k["name"], v["params"])
            if "plain" in v:
                plain = {f: p[f] for f in io.DEFAULT}
                assert io.indels(slots, contigs, regions, **plain)[:2] == events_of(v["plain"]), (k["name"], v["params"])
                plains += 1
            if "vcf" in v:
                arr = np.zeros(len(events), dtype=_lib.BAM_INDEL_DTYPE)
                for f, col in zip(io.EVENT_FIELDS, zip(*events)):
                    arr[f] = col
                got = [ln.split(b"\t") for ln in vo.lines(np.zeros(0, _lib.BAM_SITE_DTYPE), arr, seq, contigs, text)]
                assert [(int(g[1]), g[3].decode(), g[4].decode()) for g in got] == [tuple(w) for w in v["vcf"]], k["name"]
                lines += 1
            seen += 1
    assert seen == 23 and lines >= 4 and plains >= 6


def test_the_homopolymer_is_one_line_and_was_four():
    k = KATS[0]
    slots, contigs, text, regions = kat_inputs(k)
    assert k["contig"] == "GCAAAATG" and [r[2] for r in k["records"]] == ["2M1D5M", "3M1D4M", "4M1D3M", "5M1D2M", "3M1D4M"]
    events, seq, _ = lo.indels(slots, contigs, text, regions, exclude=0)
    assert events == [(0, 1, 0, io.DEL, 1, 5, 4, 1, 0)] and seq == b""
    assert len(io.indels(slots, contigs, regions, exclude=0)[0]) == 4


# ---- the verifier -----------------------------------------------------------------------------------------------------------
def folded(text, start, ln):
    return bytes(text[start:start + ln]).upper()


def edited(contig, anchor, kind, n, seq):
    """the contig with the event applied, as a string"""
    return contig[:anchor + 1] + contig[anchor + 1 + n:] if kind == io.DEL else contig[:anchor + 1] + seq + contig[anchor + 1:]


def verify(c):
    """every raw event of a case and its shifted form; returns (events seen, events that moved)"""
    p, seen, moved = c["params"], 0, 0
    refs = {r[0] for r in c["regions"]}
    slots = [rec if rec and po.fields(rec)["ref"] in refs else b"" for rec in c["slots"]]
    for ref, strand, (a, kind, n, codes), (a2, kind2, n2, codes2), k, pos in lo.shifted_events(slots, c["contigs"], c["text"], p):
        contig = folded(c["text"], c["contigs"][ref][1], c["contigs"][ref][2])
        s, s2 = bytes(io.ASCII[x] for x in codes), bytes(io.ASCII[x] for x in codes2)
        assert (kind2, n2, a2) == (kind, n, a - k) and pos <= a2 and 0 <= k <= p["max_shift"], c["name"]
        assert edited(contig, a, kind, n, s) == edited(contig, a2, kind, n, s2), (c["name"], a, k)
        if k < p["max_shift"] and a2 > pos:  # one more step: the byte at a2 enters the event, the event's last byte leaves it
            last = s2[-1:] if kind == io.INS else contig[a2 + n:a2 + n + 1]
            further = edited(contig, a2 - 1, kind, n, contig[a2:a2 + 1] + s2[:-1] if kind == io.INS else b"")
            same = further == edited(contig, a2, kind, n, s2)
            assert same == (last == contig[a2:a2 + 1]), c["name"]
            assert not same or contig[a2] not in b"ACGT", (c["name"], a, k)
        seen += 1
        moved += k > 0
    return seen, moved


def test_a_shift_keeps_the_edited_contig_and_ends_only_where_the_rule_ends_it():
    seen = moved = 0
    for k in KATS:
        slots, contigs, text, regions = kat_inputs(k)
        for v in k["variants"]:
            a, b = verify(dict(name=k["name"], slots=slots, contigs=contigs, text=text, regions=regions, params=lo.params(exclude=0, **v["params"])))
            seen, moved = seen + a, moved + b
    for c in lc.corpus(with_deep=False):
        a, b = verify(c)
        seen, moved = seen + a, moved + b
    assert seen > 3_000 and moved > 1_000


def test_with_no_threshold_nothing_is_lost_and_events_only_merge():
    """one whole-contig region at a time: the sum of alt is bg_bam_indels' and there are no more events than it has"""
    merged = 0
    for c in lc.corpus(with_deep=False):
        lax = dict(c["params"], min_depth=0, min_alt=1, min_alt_permille=0, min_alt_strand=0)
        for r, (_, start, ln) in enumerate(c["contigs"]):
            if start + ln > c["n_text"]:
                continue
            events, _, _ = lo.indels(c["slots"], c["contigs"], c["text"], [(r, 0, ln)], **lax)
            plain, _, _ = io.indels(c["slots"], c["contigs"], [(r, 0, ln)], **{f: lax[f] for f in io.DEFAULT})
            assert sum(e[6] + e[7] for e in events) == sum(e[6] + e[7] for e in plain), c["name"]
            if c.get("splits"):  # the rule's own exception: records that begin inside the repeat stop at their own pos
                assert (len(plain), len(events)) == (1, 3) if r == 3 else not plain, c["name"]
                continue
            assert len(events) <= len(plain), c["name"]
            assert events == sorted(events, key=lambda e: (e[2], e[1], e[3], e[4])), c["name"]
            if lax["max_shift"] == 0:
                assert events == plain, c["name"]
            merged += len(plain) - len(events)
    assert merged >= 26  # by design: the copy and the rotated spelling of five units in two cases, six of seven spellings of the pile


def test_the_corpus_holds_what_it_says():
    by = {c["name"]: c for c in lc.corpus(with_deep=False)}
    T = lc.T
    c = by["a deletion that lands two tiles in front of its raw anchor"]
    events, _, event_off = lc.want_of(c)
    assert [e[:5] for e in events if e[2] == 0] == [(1, 49, 0, io.DEL, 1)] and event_off[1:4] == [1, 1, 2]  # raw anchor only: none; shifted only: one
    assert 49 // T == 0 and 1148 // T == 2
    mid = lc.want_of(by["the same, max_shift ends it inside the middle tile"])[0]
    assert [e[1] for e in mid if e[2] == 0] == [648] and 648 // T == 1
    assert [e[1] for e in lc.want_of(by["the same, max_shift ends it on the middle tile's first position"])[0] if e[2] == 0] == [T]
    assert [e[1] for e in lc.want_of(by["the same, max_shift ends it on the middle tile's last position"])[0] if e[2] == 0] == [2 * T - 1]
    c = by["raw anchors at T - 1, T and T + 1 of a tile that shift by one"]
    first = [e for e in lc.want_of(c)[0] if e[2] == 0]
    assert [(e[1], e[6], e[7]) for e in first] == [(T - 2, 1, 1), (T + 1, 1, 0), (2 * T - 1, 1, 1), (2 * T + 2, 1, 0), (3 * T, 1, 1), (3 * T + 3, 1, 0)]
    c = by["insertions of 1, 15, 16, 17 and 33 bases with k below, at and above their length"]
    shifted = lo.shifted_events(c["slots"], c["contigs"], c["text"], c["params"])
    rel = {(raw[2], (k > raw[2]) - (k < raw[2])) for _, _, raw, _, k, _ in shifted}
    assert rel == {(n, s) for n in (1, 15, 16, 17, 33) for s in (-1, 0, 1)}
    events, seq, _ = lc.want_of(c)
    first = [(e, s) for e, s in zip(events, io.strings(events, seq)) if e[2] == 0]
    for (n, k), b in lc.SPANS.items():
        a = b + 3 * n - 1
        at = [(e, s) for e, s in first if e[4] == n and e[1] == a - k]
        if k == n + 2:  # two records of k = n + 2, the copy (k = 2), the rotated spelling (k = n + 1)
            assert len(at) == 1 and at[0][0][6] + at[0][0][7] == 4, n
        elif k == n - 1 and n > 1:  # the unit and the one that differs in its first byte
            assert len(at) == 2 and at[0][1][:-1] == at[1][1][:-1] and at[0][1][-1] != at[1][1][-1], n
        else:
            assert len(at) == 1 and at[0][0][6:8] == (1, 1), n
    c = by["1 100 records, seven spellings, one event"]
    assert [e[1:8] for e in lc.want_of(c)[0] if e[2] == 0] == [(299, 0, io.DEL, 1, 1100, 733, 367)]
    assert sum(1 for c in lc.corpus(with_deep=False) if c.get("plain")) == len(lc.ic.corpus(with_deep=False))


def test_every_refusal_of_the_corpus_is_the_oracles():
    kinds = set()
    for c in lc.refusals():
        with pytest.raises(lo.Refused) as e:
            lc.want_of(c)
        assert (e.value.status, e.value.slot) == c["want"], c["name"]
        kinds.add(c["name"])
    assert {"a contig that ends one byte behind the text", "a text of no byte"} <= kinds and len(kinds) == len(pc.refusals()) + 3


def test_structs_and_symbols_are_the_headers():
    head = open(os.path.join(pc.ROOT, "include", "biogpu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} bg_bam_indels_left_t;", head).group(1)
    fields = [f.strip().split("[")[0] for decl in re.findall(r"u?int\d+_t ([^;]*);", body) for f in decl.split(",")]
    left, plain = _lib.BAM_INDELS_LEFT_DTYPE, _lib.BAM_INDELS_DTYPE
    assert fields == list(left.names) and left.itemsize == 32 and plain.itemsize == 28
    assert list(left.names)[:-1] == list(plain.names) and all(left.fields[f][:2] == plain.fields[f][:2] for f in plain.names)
    assert left.fields["max_shift"][1] == 28
    assert "static_assert(sizeof(bg_bam_indels_left_t) == 32" in open(os.path.join(_lib.CSRC, "bam_indels_left_rule.h")).read()
    kw = dict(require=1, exclude=2, min_mapq=3, min_baseq=4, min_depth=5, min_alt=6, min_alt_permille=7, min_alt_strand=8)
    assert bam.indels_left_params(max_shift=9, **kw).tobytes() == bam.indels_params(**kw).tobytes() + np.uint32(9).tobytes()
    assert int(bam.indels_left_params()["max_shift"][0]) == 0xFFFFFFFF == lo.NO_LIMIT
    for s in ("bg_bam_indels_left", "bg_bam_indels_left_dev"):
        assert s in _lib.SYMBOLS and getattr(_lib.lib(), s) and re.search(r"\bint %s\(" % s, head)
    assert head.index("int bg_bam_indels(") < head.index("int bg_bam_indels_left_dev(") < head.index("int bg_vcf_header(")


FAKE = np.zeros(4096, dtype=np.uint8)  # stands for any buffer: a refused call dereferences none of them
P = FAKE.ctypes.data


def calls():
    lib = _lib.lib()
    for dev in (False, True):
        fn = lib.bg_bam_indels_left_dev if dev else lib.bg_bam_indels_left
        tail = (None,) if dev else ()

        def call(ctx=P, prm=None, n_slots=1, recs=P, off=P, contigs=P, n_contigs=1, text=P, n_text=1, regions=P, n_regions=1, events=None, cap=0, seq=None,
                 seq_cap=0, event_off=None, n=None, n_seq=None, bad=None, fn=fn, tail=tail, **kw):
            prm = bam.indels_left_params(**kw) if prm is None else prm
            return fn(ctx, prm.ctypes.data if prm is not False else None, n_slots, recs, off, contigs, n_contigs, text, n_text, regions, n_regions, events, cap,
                      seq, seq_cap, event_off, n, n_seq, bad, *tail)
        yield dev, call


def test_arguments_are_checked_before_a_device_is_touched():
    for dev, call in calls():
        n, n_seq, bad = C.c_uint64(77), C.c_uint64(78), C.c_uint64(5)
        ref = dict(n=C.byref(n), n_seq=C.byref(n_seq), bad=C.byref(bad))
        assert call(ctx=None, **ref) == INVALID_ARG and bad.value == io.NONE, dev
        assert call(prm=False, **ref) == INVALID_ARG, dev
        assert call(n=None, n_seq=C.byref(n_seq)) == INVALID_ARG and call(n=C.byref(n), n_seq=None) == INVALID_ARG, dev
        assert call(recs=None, **ref) == INVALID_ARG and call(off=None, **ref) == INVALID_ARG, dev
        assert call(contigs=None, **ref) == INVALID_ARG and call(regions=None, **ref) == INVALID_ARG, dev
        assert call(text=None, **ref) == INVALID_ARG, dev  # a null text with n_text > 0
        assert call(events=None, cap=1, **ref) == INVALID_ARG, dev  # a capacity without a buffer
        assert call(events=P, cap=1, seq=None, seq_cap=1, **ref) == INVALID_ARG, dev
        assert call(events=None, cap=0, seq=P, seq_cap=0, **ref) == INVALID_ARG, dev  # a sizing call takes no d_seq ...
        assert call(events=None, cap=0, seq=None, seq_cap=1, **ref) == INVALID_ARG, dev  # ... and no seq_cap
        assert (n.value, n_seq.value) == (77, 78)
        assert call(min_alt_permille=1001, **ref) == INVALID_ARG and (n.value, n_seq.value) == (0, 0) and _lib.lib().bg_last_error(), dev
        for field in ("flags", "reserved"):
            prm = bam.indels_left_params()
            prm[field] = 1
            assert call(prm=prm, **ref) == INVALID_ARG, (dev, field)
        assert call(n_slots=2**32 - 1, **ref) == TOO_LARGE and call(n_regions=2**24, **ref) == TOO_LARGE, dev
    n, n_seq = C.c_uint64(0), C.c_uint64(0)
    misaligned = P + 4 if P % 8 == 0 else P + (8 - P % 8) + 4
    args = (P, bam.indels_left_params().ctypes.data, 0, None, None, None, 0, None, 0, None, 0)
    assert _lib.lib().bg_bam_indels_left_dev(*args, misaligned, 4, None, 0, None, C.byref(n), C.byref(n_seq), None, None) == INVALID_ARG
    assert _lib.lib().bg_bam_indels_left_dev(*args, P + (8 - P % 8) % 8, 4, None, 0, misaligned, C.byref(n), C.byref(n_seq), None, None) == INVALID_ARG

"""The Python restatement of the indel events (tests/bam_indels_oracle.py) pinned to known answers written by hand from the rule
(tests/golden/bam_indels_kats.json: the alignment example of SAM v1.6 section 1.1, whose anchor 13 holds two different
insertions; a pile of depth 20 with every threshold one below and at its value; the same insertion on one strand only; adjacent
and leading operations) and to identities over the corpus of tests/bam_indels_cases.py; the binding's structs against the
header; and, through ctypes without a GPU, the argument checks of bg_bam_indels[_dev]."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import bam_indels_cases as ic
import bam_indels_oracle as io
import bam_pileup_cases as pc
import bam_pileup_oracle as po
import bam_sites_cases as sc
import bam_sites_oracle as so
from rust_bio_amd import _lib, bam

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KATS = json.load(open(os.path.join(GOLDEN, "bam_indels_kats.json")))
PILEUP_KATS = json.load(open(os.path.join(GOLDEN, "bam_pileup_kats.json")))
INVALID_ARG, TOO_LARGE = -1, -8


def events_of(listed, region=0, ref=0):
    """the JSON's events as the oracle's tuples and their strings: seq_off is the running sum of the insertions in front"""
    out, at = [], 0
    for pos, kind, n, seq, depth, fwd, rev in listed:
        assert len(seq) == (n if kind == io.INS else 0)
        out.append((ref, pos, region, kind, n, depth, fwd, rev, at))
        at += len(seq)
    return out, "".join(e[3] for e in listed).encode()


def test_the_specifications_example():
    ex, mine = PILEUP_KATS["sam_example"], KATS["sam_example"]
    contigs = [(ex["contig"][0].encode(), 0, ex["contig"][1])]
    slots = [po.record(n.encode(), flag, contigs[0][0], pos1, mapq, cigar.encode(), seq.encode(), contigs) for n, flag, pos1, mapq, cigar, seq in ex["records"]]
    events, seq, event_off = io.indels(slots, contigs, [(0, 0, 45)], **mine["params"])
    assert (events, seq) == events_of(mine["events"]) and event_off == [0, 3]
    assert io.strings(events, seq) == [b"G", b"AG", b""]  # two different insertions behind 0-based 13
    # a region of its own holds what the whole contig holds there; one that begins behind the anchor holds nothing
    part, part_seq, part_off = io.indels(slots, contigs, [(0, 13, 14), (0, 14, 17), (0, 0, 0), (0, 17, 45)], **mine["params"])
    assert [e[:2] + e[3:8] for e in part] == [e[:2] + e[3:8] for e in events] and [e[2] for e in part] == [0, 0, 3]
    assert part_seq == seq and part_off == [0, 2, 2, 2, 3]


def kat_slots(k, contigs):
    out = []
    for flag, pos, mapq, cigar, seq, qual in k["records"]:
        q = b"*" if qual is None else bytes((v + 33) & 0xFF for v in qual)
        out.append(po.record(b"k", flag, contigs[0][0], pos + 1, mapq, cigar.encode(), seq.encode(), contigs, q))
    return out


def test_hand_made_known_answers():
    seen = 0
    for k in KATS["kats"]:
        contigs = [(b"k", 0, k["contig"])]
        slots = kat_slots(k, contigs)
        for v in k["variants"]:
            events, seq, event_off = io.indels(slots, contigs, [tuple(k["region"])], exclude=0, **v["params"])
            assert (events, seq) == events_of(v["events"]), (k["name"], v["params"])
            assert event_off == [0, len(events)], (k["name"], v["params"])
            seen += 1
    assert seen >= 22


def test_identities_over_the_corpus():
    """with no threshold, the INS counts of an anchor's events sum to the pileup's INS column there, wherever no record holds a
    zero-length I or an I without bases; every event's depth is the sites oracle's; every deleted position lies in a DEL column"""
    seen = summed = 0
    for c in ic.corpus(with_deep=False):
        p, contigs = c["params"], c["contigs"]
        whole = [(r, 0, ln) for r, (_, _, ln) in enumerate(contigs)]
        lax = dict(p, min_depth=0, min_alt=1, min_alt_permille=0, min_alt_strand=0)
        events, seq, event_off = io.indels(c["slots"], contigs, whole, **lax)
        assert len(seq) == sum(e[4] for e in events if e[3] == io.INS) and io.strings(events, seq) == [bytes(s) for s in io.strings(events, seq)]
        assert events == sorted(events, key=lambda e: (e[2], e[1], e[3], e[4])) and event_off[-1] == len(events), c["name"]
        rows, row_off = po.pileup(c["slots"], contigs, whole, flags=po.STRANDS, require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"],
                                  min_baseq=p["min_baseq"])
        text = sc.text_of(contigs)
        sites, _, _ = so.sites(c["slots"], contigs, text, whole, **so.params(require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"],
                                                                              min_baseq=p["min_baseq"]))
        site_depth = {(s[0], s[1]): s[6] for s in sites}
        plain = True
        for rec in c["slots"]:
            if rec:
                f = po.fields(rec)
                plain &= not any(op == 1 and (n == 0 or not f["l_seq"]) for op, n in f["cigar"])
        ins = {}
        for ref, pos, region, kind, n, depth, fwd, rev, _ in events:
            row = rows[row_off[region] + pos]
            assert depth == io.depth_of(row), c["name"]
            if (ref, pos) in site_depth:
                assert depth == site_depth[(ref, pos)], c["name"]
                seen += 1
            if kind == io.INS:
                cell = ins.setdefault((region, pos), [0, 0])
                cell[0], cell[1] = cell[0] + fwd, cell[1] + rev
            else:
                for k in range(1, n + 1):
                    assert rows[row_off[region] + pos + k][po.DEL] >= fwd and rows[row_off[region] + pos + k][po.COLS + po.DEL] >= rev, c["name"]
        if plain:
            for r, (_, _, ln) in enumerate(contigs):
                for pos in range(ln):
                    row = rows[row_off[r] + pos]
                    assert ins.get((r, pos), [0, 0]) == [row[po.INS], row[po.COLS + po.INS]], (c["name"], r, pos)
                    summed += row[po.INS] + row[po.COLS + po.INS]
    assert seen > 200 and summed > 300


def test_every_refusal_of_the_corpus_is_the_oracles():
    for c in ic.refusals():
        with pytest.raises(io.Refused) as e:
            ic.want_of(c)
        assert (e.value.status, e.value.slot) == c["want"], c["name"]
    assert len(ic.refusals()) == len(pc.refusals())
    with pytest.raises(io.Refused):
        io.indels([], ic.CONTIGS, [], min_alt_permille=1001)


def test_structs_and_constants_are_the_headers():
    head = open(os.path.join(pc.ROOT, "include", "biogpu.h")).read()
    assert (bam.SITE_DEL, bam.SITE_INS) == (io.DEL, io.INS) == (1, 2) and bam.SEQ_CODES == io.ASCII == b"=ACMGRSVTWYHKDBN"
    for name, dtype, size in (("bg_bam_indels_t", _lib.BAM_INDELS_DTYPE, 28), ("bg_bam_indel_t", _lib.BAM_INDEL_DTYPE, 40)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, head).group(1)
        fields = [f.strip().split("[")[0] for decl in re.findall(r"u?int\d+_t ([^;]*);", body) for f in decl.split(",")]
        assert fields == list(dtype.names) and dtype.itemsize == size, name
    assert bam.INDEL_DTYPE.fields["seq_off"][1] == 32 and bam.INDEL_DTYPE.fields["len"][1] == 16
    p = bam.indels_params(require=1, exclude=2, min_mapq=3, min_baseq=4, min_depth=5, min_alt=6, min_alt_permille=7, min_alt_strand=8)
    assert p.tobytes() == bytes([0, 0, 0, 0, 1, 0, 2, 0, 3, 4, 0, 0]) + np.arange(5, 9, dtype="<u4").tobytes()
    assert bam.indels_params().tobytes()[4:8] == bytes([0, 0, 4, 7]) and int(bam.indels_params()["min_alt"][0]) == 1
    for s in ("bg_bam_indels", "bg_bam_indels_dev"):
        assert s in _lib.SYMBOLS and getattr(_lib.lib(), s)
    events = np.zeros(3, dtype=bam.INDEL_DTYPE)
    events["kind"], events["len"], events["seq_off"] = [io.INS, io.DEL, io.INS], [2, 5, 1], [0, 2, 2]
    assert bam.indel_sequences(events, b"AGT") == [b"AG", b"", b"T"]


FAKE = np.zeros(4096, dtype=np.uint8)  # stands for any buffer: a refused call dereferences none of them
P = FAKE.ctypes.data


def calls():
    lib = _lib.lib()
    for dev in (False, True):
        fn = lib.bg_bam_indels_dev if dev else lib.bg_bam_indels
        tail = (None,) if dev else ()

        def call(ctx=P, prm=None, n_slots=1, recs=P, off=P, contigs=P, n_contigs=1, regions=P, n_regions=1, events=None, cap=0, seq=None, seq_cap=0,
                 event_off=None, n=None, n_seq=None, bad=None, fn=fn, tail=tail, **kw):
            prm = bam.indels_params(**kw) if prm is None else prm
            return fn(ctx, prm.ctypes.data if prm is not False else None, n_slots, recs, off, contigs, n_contigs, regions, n_regions, events, cap, seq, seq_cap,
                      event_off, n, n_seq, bad, *tail)
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
        assert call(events=None, cap=1, **ref) == INVALID_ARG, dev  # a capacity without a buffer
        assert call(events=P, cap=1, seq=None, seq_cap=1, **ref) == INVALID_ARG, dev
        assert call(events=None, cap=0, seq=P, seq_cap=0, **ref) == INVALID_ARG, dev  # a sizing call takes no d_seq ...
        assert call(events=None, cap=0, seq=None, seq_cap=1, **ref) == INVALID_ARG, dev  # ... and no seq_cap
        assert (n.value, n_seq.value) == (77, 78)
        assert call(min_alt_permille=1001, **ref) == INVALID_ARG and (n.value, n_seq.value) == (0, 0) and _lib.lib().bg_last_error(), dev
        for field in ("flags", "reserved"):
            prm = bam.indels_params()
            prm[field] = 1
            assert call(prm=prm, **ref) == INVALID_ARG, (dev, field)
        assert call(n_slots=2**32 - 1, **ref) == TOO_LARGE and call(n_regions=2**24, **ref) == TOO_LARGE, dev
    n, n_seq = C.c_uint64(0), C.c_uint64(0)
    misaligned = P + 4 if P % 8 == 0 else P + (8 - P % 8) + 4
    args = (P, bam.indels_params().ctypes.data, 0, None, None, None, 0, None, 0)
    assert _lib.lib().bg_bam_indels_dev(*args, misaligned, 4, None, 0, None, C.byref(n), C.byref(n_seq), None, None) == INVALID_ARG
    assert _lib.lib().bg_bam_indels_dev(*args, P + (8 - P % 8) % 8, 4, None, 0, misaligned, C.byref(n), C.byref(n_seq), None, None) == INVALID_ARG

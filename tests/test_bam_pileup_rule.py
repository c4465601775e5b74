"""The Python restatement of the pileup (tests/bam_pileup_oracle.py) pinned to known answers (tests/golden/bam_pileup_kats.json:
the alignment example of SAM v1.6 section 1.1 with its rows and the column sums of four parameter variants; hand-made records
for what the example lacks) and to identities over the corpus of tests/bam_pileup_cases.py; the binding's constants against the
headers; and, through ctypes without a GPU, the argument checks of bg_bam_pileup[_dev], the sizing path (which fails loudly
where there is no device) and `bam.pileup_bam`'s ValueError for a region the file's header does not carry."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import bam_oracle
import bam_pileup_cases as pc
import bam_pileup_oracle as po
from rust_bio_amd import _lib, bam

KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bam_pileup_kats.json")))
INVALID_ARG, TOO_LARGE = -1, -8


def example():
    ex = KATS["sam_example"]
    contigs = [(ex["contig"][0].encode(), 0, ex["contig"][1])]
    slots = [po.record(n.encode(), flag, contigs[0][0], pos1, mapq, cigar.encode(), seq.encode(), contigs) for n, flag, pos1, mapq, cigar, seq in ex["records"]]
    return ex, contigs, slots


def test_the_specifications_example():
    ex, contigs, slots = example()
    rows, row_off = po.pileup(slots, contigs, [(0, 0, 45)], exclude=0)
    assert row_off == [0, 45] and po.sparse(rows) == ex["rows"]
    for v in ex["sums"]:
        p = dict(pc.DEFAULT, **v["params"])
        rows, _ = po.pileup(slots, contigs, [(0, 0, 45)], **p)
        assert np.array(rows).sum(axis=0).tolist() == v["sums"], v["params"]
        for pos in v.get("skip_only", []):
            assert po.sparse(rows)[str(pos)] == {"SKIP": 1}, (v["params"], pos)
    # a region of its own holds what the whole contig holds there
    part, _ = po.pileup(slots, contigs, [(0, 13, 22), (0, 0, 0), (0, 13, 14)], exclude=0)
    whole, _ = po.pileup(slots, contigs, [(0, 0, 45)], exclude=0)
    assert part == whole[13:22] + whole[13:14]


def kat_slots(k, contigs):
    out = []
    for flag, pos, mapq, cigar, seq, qual in k["records"]:
        q = b"*" if qual is None else bytes((v + 33) & 0xFF for v in qual)  # (the encoder takes 33 off again, modulo 256)
        out.append(po.record(b"k", flag, contigs[0][0], pos + 1, mapq, cigar.encode(), seq.encode(), contigs, q))
    return out


def test_hand_made_known_answers():
    contigs = [(b"k", 0, 100)]
    for k in KATS["kats"]:
        p = dict(pc.DEFAULT, exclude=0, **k.get("params", {}))
        rows, _ = po.pileup(kat_slots(k, contigs), contigs, [(0, 0, 100)], **p)
        assert po.sparse(rows) == k["rows"], k["name"]


def test_identities_over_the_corpus():
    seen = 0
    for c in pc.corpus():
        p = c["params"]
        whole = [(r, 0, ln) for r, (_, _, ln) in enumerate(c["contigs"])]
        rows, _ = po.pileup(c["slots"], c["contigs"], whole, **p)
        rows = np.array(rows, dtype=np.int64).reshape(len(rows), 2 * po.COLS if p["flags"] & po.STRANDS else po.COLS)
        bases = dels = skips = 0
        for s in c["slots"]:
            if not s:
                continue
            f = po.fields(s)
            if not po.kept(f, p["require"], p["exclude"], p["min_mapq"]):
                continue
            q = 0
            for op, n in f["cigar"]:
                if op in po.M_OPS:
                    bases += sum(1 for k in range(n) if not f["l_seq"] or f["qual"][q + k] >= p["min_baseq"])
                dels += n if op == 2 else 0
                skips += n if op == 3 else 0
                q += n if op in po.QUERY_OPS else 0
        both = rows[:, :po.COLS] + (rows[:, po.COLS:] if rows.shape[1] == 2 * po.COLS else 0)
        assert both[:, :po.OTHER + 1].sum() == bases and both[:, po.DEL].sum() == dels and both[:, po.SKIP].sum() == skips, c["name"]
        seen += bases + dels + skips
    assert seen > 100_000


def test_every_refusal_of_the_corpus_is_the_oracles():
    for name, slots, contigs, regions, status, slot in pc.refusals():
        with pytest.raises(po.Refused) as e:
            po.pileup(slots, contigs, regions)
        assert (e.value.status, e.value.slot) == (status, slot), name


def test_constants_are_the_headers():
    rule = open(os.path.join(_lib.CSRC, "bam_pileup_rule.h")).read()
    assert int(re.search(r"#define BG_PILEUP_TILE (\d+)u", rule).group(1)) == bam.PILEUP_TILE == pc.T
    assert 2 * 2 * po.COLS * bam.PILEUP_TILE * 4 <= 160 * 1024  # two workgroups of the 16-column form in a CU's LDS
    head = open(os.path.join(pc.ROOT, "include", "biogpu.h")).read()
    names = re.search(r"enum \{ (BG_PILEUP_A,.*?)BG_PILEUP_COLS", head, flags=re.S).group(1).replace("\n", " ")
    assert [n.strip()[len("BG_PILEUP_"):] for n in names.split(",") if n.strip()] == po.NAMES
    assert [bam.PILEUP_A, bam.PILEUP_C, bam.PILEUP_G, bam.PILEUP_T, bam.PILEUP_OTHER, bam.PILEUP_DEL, bam.PILEUP_SKIP, bam.PILEUP_INS,
            bam.PILEUP_COLS] == list(range(9)) and bam.PILEUP_STRANDS == 1
    assert bam.pileup_params().tobytes() == bytes([0, 0, 0, 0, 0, 0, 4, 7, 0, 0, 0, 0])
    rows = np.arange(32, dtype=np.uint32).reshape(2, 16)
    assert bam.depth(rows[:, :8]).tolist() == [10, 90] and bam.depth(rows[:, :8], deletions=True).tolist() == [15, 111]
    assert bam.depth(rows).tolist() == [10 + 50, 90 + 130] and bam.depth(rows, deletions=True).tolist() == [60 + 5 + 13, 220 + 21 + 29]


FAKE = np.zeros(4096, dtype=np.uint8)  # stands for any buffer: a refused call dereferences none of them
P = FAKE.ctypes.data


def calls():
    lib = _lib.lib()
    for dev in (False, True):
        fn = lib.bg_bam_pileup_dev if dev else lib.bg_bam_pileup
        tail = (None,) if dev else ()

        def call(ctx=P, prm=None, n_slots=1, recs=P, off=P, contigs=P, n_contigs=1, regions=P, n_regions=1, rows=None, cap=0, row_off=None, n=None, bad=None,
                 fn=fn, tail=tail, **kw):
            prm = bam.pileup_params(**kw) if prm is None else prm
            return fn(ctx, prm.ctypes.data if prm is not False else None, n_slots, recs, off, contigs, n_contigs, regions, n_regions, rows, cap, row_off, n, bad,
                      *tail)
        yield dev, call


def test_arguments_are_checked_before_a_device_is_touched():
    for dev, call in calls():
        n, bad = C.c_uint64(77), C.c_uint64(5)
        ref = dict(n=C.byref(n), bad=C.byref(bad))
        assert call(ctx=None, **ref) == INVALID_ARG and bad.value == po.NONE, dev
        assert call(prm=False, **ref) == INVALID_ARG, dev
        assert call(n=None) == INVALID_ARG, dev
        assert call(recs=None, **ref) == INVALID_ARG and call(off=None, **ref) == INVALID_ARG, dev
        assert call(contigs=None, **ref) == INVALID_ARG and call(regions=None, **ref) == INVALID_ARG, dev
        assert call(rows=None, cap=1, **ref) == INVALID_ARG, dev  # a capacity without a buffer
        assert n.value == 77
        for flags in (2, 3, 1 << 31):
            assert call(flags=flags, **ref) == INVALID_ARG and n.value == 0, (dev, flags)
        prm = bam.pileup_params()
        prm["reserved"] = 1
        assert call(prm=prm, **ref) == INVALID_ARG, dev
        assert call(n_slots=2**32 - 1, **ref) == TOO_LARGE and call(n_regions=2**24, **ref) == TOO_LARGE, dev
    n = C.c_uint64(0)
    misaligned = P + 2 if P % 4 == 0 else P + (4 - P % 4) + 2
    assert _lib.lib().bg_bam_pileup_dev(P, bam.pileup_params().ctypes.data, 0, None, None, None, 0, None, 0, misaligned, 4, None, C.byref(n), None, None) == INVALID_ARG


def test_the_sizing_path_needs_a_device():
    contigs = pc.CONTIGS
    slots = pc.every_op()
    if _lib.lib().bg_device_count() > 0:
        rows, row_off = bam.pileup_arrays(b"".join(slots), bam_oracle.offsets(slots), bam.sam.Contigs(contigs), [(0, 0, 100)])
        assert rows.shape == (100, 8) and row_off.tolist() == [0, 100]
        return
    body = np.frombuffer(b"".join(slots), dtype=np.uint8)
    off, table = bam_oracle.offsets(slots), bam.sam.Contigs(contigs).table
    reg = bam.pileup_regions([(0, 0, 100)])
    n = C.c_uint64(0)
    for dev, call in calls():  # a zeroed ctx names device 0: the call gets as far as asking for it
        rc = call(n_slots=len(slots), recs=body.ctypes.data, off=off.ctypes.data, contigs=table.ctypes.data, n_contigs=len(table), regions=reg.ctypes.data,
                  n=C.byref(n))
        assert rc in (-2, -3) and n.value == 0 and _lib.lib().bg_last_error(), dev
    with pytest.raises((_lib.BiogpuError, RuntimeError)):
        bam.pileup_arrays(body, off, bam.sam.Contigs(contigs), [(0, 0, 100)])


def test_pileup_bam_names_a_bad_region_before_any_device_work():
    ex, contigs, slots = example()
    two = contigs + [(b"other", 46, 30)]
    data = bam_oracle.frame(bam_oracle.header(b"@HD\tVN:1.6\tSO:coordinate\n", two)) + bam_oracle.frame(b"".join(slots), eof=True)
    for region, word in ((("chrX", 0, 5), "chrX"), ((b"nope", 0, 5), "nope"), (("ref", 7, 3), "7"), (("ref", 0, 46), "46"), (("other", 0, 31), "31"),
                         ((2, 0, 1), "2"), ((-1, 0, 1), "-1"), (("ref", -1, 4), "-1")):
        with pytest.raises(ValueError) as e:
            bam.pileup_bam(data, [("ref", 0, 45), region])
        assert "region" in str(e.value) and word in str(e.value), region
    reg = bam.resolve_regions(bam.sam.Contigs(two), [("other", 0, 30), (b"ref", 5, 5), (1, 2, 3)])
    assert reg.tolist() == [(1, 0, 30), (0, 5, 5), (1, 2, 3)]

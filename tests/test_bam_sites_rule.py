"""The Python restatement of the candidate sites (tests/bam_sites_oracle.py) pinned to known answers written by hand from the rule
(tests/golden/bam_sites_kats.json: the alignment example of SAM v1.6 section 1.1 against its own reference line; a pile with
every threshold one below and at its value, permille equality, all alternative reads on one strand; unjudged and soft-masked
reference bytes; a deletion of three positions) and to identities over the corpus of tests/bam_sites_cases.py; the binding's
structs and constants against the header; and, through ctypes without a GPU, the argument checks of bg_bam_sites[_dev]."""
import ctypes as C
import json
import os
import re

import numpy as np

import bam_pileup_cases as pc
import bam_pileup_oracle as po
import bam_sites_cases as sc
import bam_sites_oracle as so
from rust_bio_amd import _lib, bam

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KATS = json.load(open(os.path.join(GOLDEN, "bam_sites_kats.json")))
PILEUP_KATS = json.load(open(os.path.join(GOLDEN, "bam_pileup_kats.json")))
INVALID_ARG, TOO_LARGE = -1, -8


def site_of(s, region=0, ref=0):
    pos, kind, ref_base, alt, depth, ref_count, fwd, rev = s
    return (ref, pos, region, kind, ord(ref_base), ord(alt) if alt else 0, depth, ref_count, fwd, rev)


def test_the_specifications_example():
    ex, mine = PILEUP_KATS["sam_example"], KATS["sam_example"]
    contigs = [(ex["contig"][0].encode(), 0, ex["contig"][1])]
    assert len(mine["reference"]) == ex["contig"][1]
    slots = [po.record(n.encode(), flag, contigs[0][0], pos1, mapq, cigar.encode(), seq.encode(), contigs) for n, flag, pos1, mapq, cigar, seq in ex["records"]]
    text = mine["reference"].encode() + b"$"
    sites, site_off, summary = so.sites(slots, contigs, text, [(0, 0, 45)], **mine["params"])
    assert sites == [site_of(s) for s in mine["sites"]] and site_off == [0, 4] and summary == [mine["summary"]]
    # a region of its own holds what the whole contig holds there; lower case changes nothing but nothing
    part, part_off, _ = so.sites(slots, contigs, text.lower(), [(0, 13, 19), (0, 0, 0), (0, 41, 42)], **mine["params"])
    assert [s[:2] + s[3:] for s in part] == [s[:2] + s[3:] for s in sites[1:]] and [s[2] for s in part] == [0, 0, 2] and part_off == [0, 2, 2, 3]


def kat_slots(k, contigs):
    out = []
    for flag, pos, mapq, cigar, seq, qual in k["records"]:
        q = b"*" if qual is None else bytes((v + 33) & 0xFF for v in qual)
        out.append(po.record(b"k", flag, contigs[0][0], pos + 1, mapq, cigar.encode(), seq.encode(), contigs, q))
    return out


def test_hand_made_known_answers():
    seen = 0
    for k in KATS["kats"]:
        text = k["text"].encode() + b"$"
        contigs = [(b"k", 0, len(k["text"]))]
        slots = kat_slots(k, contigs)
        for v in k["variants"]:
            sites, site_off, summary = so.sites(slots, contigs, text, [tuple(k["region"])], exclude=0, **v["params"])
            assert sites == [site_of(s) for s in v["sites"]], (k["name"], v["params"])
            assert site_off == [0, len(sites)] and summary == [k["summary"]], (k["name"], v["params"])  # (no threshold touches a summary)
            seen += 1
    assert seen >= 17


def test_identities_over_the_corpus():
    seen = 0
    for c in sc.corpus(with_deep=False):
        p, contigs, text = c["params"], c["contigs"], c["text"]
        whole = [(r, 0, ln) for r, (_, _, ln) in enumerate(contigs)]
        lax = dict(p, min_depth=0, min_alt=1, min_alt_permille=0, min_alt_strand=0, cover=(0, 1, 2**32 - 1, 0))
        sites, site_off, summary = so.sites(c["slots"], contigs, text, whole, **lax)
        rows, row_off = po.pileup(c["slots"], contigs, whole, flags=po.STRANDS, require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"],
                                  min_baseq=p["min_baseq"])
        rows = np.array(rows, dtype=np.int64).reshape(len(rows), 16)
        both = rows[:, :8] + rows[:, 8:]
        for r, (name, start, ln) in enumerate(contigs):
            ref = np.frombuffer(text[start:start + ln], np.uint8)
            judged = np.isin(ref & 0xDF, np.frombuffer(b"ACGT", np.uint8)) & (((ref & 0xDF) == ref) | ((ref >= 97) & (ref <= 122)))
            mine = both[int(row_off[r]):int(row_off[r + 1])]
            s = summary[r]
            assert s["match"] + s["mismatch"] == mine[judged][:, :4].sum(), c["name"]
            assert s["covered"][0] == s["covered"][3] == ln and s["covered"][2] == 0 and s["n_ref_other"] == ln - judged.sum(), c["name"]
            assert s["covered"][1] == (mine[:, :6].sum(axis=1) > 0).sum() and s["sum_depth"] == mine[:, :6].sum(), c["name"]
            col = np.array([b"ACGT".find(bytes([b & 0xDF])) for b in ref[judged]], dtype=np.int64)
            cells = mine[judged][:, :4].copy()
            cells[np.arange(len(col)), col] = 0
            snvs = [x for x in sites[site_off[r]:site_off[r + 1]] if x[3] == so.SNV]
            assert len(snvs) == (cells > 0).sum() and s["mismatch"] == cells.sum(), c["name"]
            seen += len(snvs)
    assert seen > 5_000


def test_every_refusal_of_the_corpus_is_the_oracles():
    import pytest
    for c in sc.refusals():
        with pytest.raises(so.Refused) as e:
            sc.want_of(c)
        assert (e.value.status, e.value.slot) == c["want"], c["name"]
    assert len(sc.refusals()) == len(pc.refusals()) + 4


def test_structs_and_constants_are_the_headers():
    head = open(os.path.join(pc.ROOT, "include", "biogpu.h")).read()
    assert re.search(r"enum \{ BG_SITE_SNV = 0, BG_SITE_DEL = 1, BG_SITE_INS = 2 \}", head)
    assert (bam.SITE_SNV, bam.SITE_DEL, bam.SITE_INS) == (so.SNV, so.DEL, so.INS) == (0, 1, 2)
    for name, dtype, size in (("bg_bam_sites_t", _lib.BAM_SITES_DTYPE, 44), ("bg_bam_site_t", _lib.BAM_SITE_DTYPE, 32),
                              ("bg_bam_region_summary_t", _lib.BAM_REGION_SUMMARY_DTYPE, 48)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, head).group(1)
        fields = [f.strip().split("[")[0] for decl in re.findall(r"u?int\d+_t ([^;]*);", body) for f in decl.split(",")]
        assert fields == list(dtype.names) and dtype.itemsize == size, name
    p = bam.sites_params(require=1, exclude=2, min_mapq=3, min_baseq=4, min_depth=5, min_alt=6, min_alt_permille=7, min_alt_strand=8, cover=(9, 10, 11, 12))
    assert p.tobytes() == bytes([0, 0, 0, 0, 1, 0, 2, 0, 3, 4, 0, 0]) + np.arange(5, 13, dtype="<u4").tobytes()
    assert bam.sites_params().tobytes()[4:8] == bytes([0, 0, 4, 7]) and int(bam.sites_params()["min_alt"][0]) == 1
    rule = open(os.path.join(_lib.CSRC, "bam_sites_rule.h")).read()
    assert "SIT_PACK_BITS 10u" in rule and bam.PILEUP_TILE < 2**10 and 5 * bam.PILEUP_TILE < 2**12  # the packed word cannot overflow


FAKE = np.zeros(4096, dtype=np.uint8)  # stands for any buffer: a refused call dereferences none of them
P = FAKE.ctypes.data


def calls():
    lib = _lib.lib()
    for dev in (False, True):
        fn = lib.bg_bam_sites_dev if dev else lib.bg_bam_sites
        tail = (None,) if dev else ()

        def call(ctx=P, prm=None, n_slots=1, recs=P, off=P, contigs=P, n_contigs=1, text=P, n_text=8, regions=P, n_regions=1, sites=None, cap=0, site_off=None,
                 summary=None, n=None, bad=None, fn=fn, tail=tail, **kw):
            prm = bam.sites_params(**kw) if prm is None else prm
            return fn(ctx, prm.ctypes.data if prm is not False else None, n_slots, recs, off, contigs, n_contigs, text, n_text, regions, n_regions, sites, cap,
                      site_off, summary, n, bad, *tail)
        yield dev, call


def test_arguments_are_checked_before_a_device_is_touched():
    for dev, call in calls():
        n, bad = C.c_uint64(77), C.c_uint64(5)
        ref = dict(n=C.byref(n), bad=C.byref(bad))
        assert call(ctx=None, **ref) == INVALID_ARG and bad.value == so.NONE, dev
        assert call(prm=False, **ref) == INVALID_ARG, dev
        assert call(n=None) == INVALID_ARG, dev
        assert call(recs=None, **ref) == INVALID_ARG and call(off=None, **ref) == INVALID_ARG, dev
        assert call(contigs=None, **ref) == INVALID_ARG and call(regions=None, **ref) == INVALID_ARG, dev
        assert call(text=None, **ref) == INVALID_ARG, dev
        assert call(sites=None, cap=1, **ref) == INVALID_ARG, dev  # a capacity without a buffer
        assert n.value == 77
        assert call(min_alt_permille=1001, **ref) == INVALID_ARG and n.value == 0 and _lib.lib().bg_last_error(), dev
        for field in ("flags", "reserved"):
            prm = bam.sites_params()
            prm[field] = 1
            assert call(prm=prm, **ref) == INVALID_ARG, (dev, field)
        assert call(n_slots=2**32 - 1, **ref) == TOO_LARGE and call(n_regions=2**24, **ref) == TOO_LARGE, dev
    n = C.c_uint64(0)
    misaligned = P + 2 if P % 4 == 0 else P + (4 - P % 4) + 2
    args = (P, bam.sites_params().ctypes.data, 0, None, None, None, 0, None, 0, None, 0)
    assert _lib.lib().bg_bam_sites_dev(*args, misaligned, 4, None, None, C.byref(n), None, None) == INVALID_ARG
    assert _lib.lib().bg_bam_sites_dev(*args, P, 4, None, misaligned, C.byref(n), None, None) == INVALID_ARG


def test_sites_bam_needs_a_reference_that_fits_the_header():
    import pytest
    contigs = bam.sam.Contigs([(b"one", 0, 4), (b"two", 5, 3)])
    assert bytes(bam._reference_text(b"ACGT$NNN$", contigs, None)) == b"ACGT$NNN$"
    for text, word in ((b"ACGT$NN$", "two"), (b"ACG$NNN$", "one"), (b"ACGT$", "two"), (b"ACGT$NNN$A$", "#2")):
        with pytest.raises(ValueError) as e:
            bam._reference_text(text, contigs, None)
        assert word in str(e.value), text

"""The Python restatement of the VCF writer (tests/vcf_oracle.py) pinned to answers written by hand from the rule
(tests/golden/vcf_kats.json: the alignment example of SAM v1.6 section 1.1 carried from its records through the sites and the
indel events to literal VCF lines; one line of each type on a text with soft-masked and IUPAC bytes; the header for two
contigs, byte for byte, which bg_vcf_header must give as well: it needs no GPU).  A strict parser of a line, written here and
sharing nothing with the oracle's formatter, re-derives the fields of every line of the corpus of tests/vcf_cases.py and holds
REF against the text by a table of its own.  The binding's struct and symbols against the header; through ctypes without a
GPU, the argument checks that come before any device work."""
import ctypes as C
import json
import os
import re

import numpy as np

import bam_indels_oracle as io
import bam_pileup_oracle as po
import bam_sites_oracle as so
import vcf_cases as vc
import vcf_oracle as vo
from rust_bio_amd import _lib, sam, vcf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KATS = json.load(open(os.path.join(GOLDEN, "vcf_kats.json")))
PILEUP_KATS = json.load(open(os.path.join(GOLDEN, "bam_pileup_kats.json")))
SITES_KATS = json.load(open(os.path.join(GOLDEN, "bam_sites_kats.json")))
INDELS_KATS = json.load(open(os.path.join(GOLDEN, "bam_indels_kats.json")))

NUM = r"(0|[1-9][0-9]*)"
LINE = re.compile((r"([^\t\n]+)\t([1-9][0-9]*)\t\.\t([ACGTN]+)\t([ACGTN]+)\t\.\t\.\tDP=%s(?:;RO=%s)?;AO=%s;SAF=%s;SAR=%s;TYPE=(snp|del|ins)\n" % ((NUM,) * 5)).encode())
# R of the rule, written as a translation of all 256 bytes: the 15 letters that stand for bases, both cases, N for the rest
TABLE = bytearray(b"N" * 256)
for letters, base in ((b"AMRWDHV", b"A"), (b"CYSB", b"C"), (b"GK", b"G"), (b"T", b"T")):
    for b in letters:
        TABLE[b] = TABLE[b + 32] = base[0]


def sites_array(listed):
    out = np.zeros(len(listed), dtype=vc.SITE)
    for k, (ref, pos, region, kind, base, alt, depth, ro, fwd, rev) in enumerate(listed):
        out[k] = (ref, pos, region, kind, base if isinstance(base, int) else ord(base), alt if isinstance(alt, int) else ord(alt) if alt else 0, 0, depth, ro, fwd, rev)
    return out


def events_array(listed):
    """(events, seq) from [ref, pos, region, kind, len, seq, depth, fwd, rev]"""
    out, seq = np.zeros(len(listed), dtype=vc.EVENT), b""
    for k, (ref, pos, region, kind, n, s, depth, fwd, rev) in enumerate(listed):
        s = s.encode() if isinstance(s, str) else s
        out[k] = (ref, pos, region, kind, (0, 0, 0), n, depth, fwd, rev, len(seq))
        seq += s
    return out, seq


def test_the_specifications_example_as_vcf_lines():
    ex = PILEUP_KATS["sam_example"]
    contigs = [(ex["contig"][0].encode(), 0, ex["contig"][1])]
    text = SITES_KATS["sam_example"]["reference"].encode() + b"$"
    slots = [po.record(n.encode(), flag, contigs[0][0], pos1, mapq, cigar.encode(), seq.encode(), contigs) for n, flag, pos1, mapq, cigar, seq in ex["records"]]
    sites, _, _ = so.sites(slots, contigs, text, [(0, 0, 45)], **SITES_KATS["sam_example"]["params"])
    events, seq, _ = io.indels(slots, contigs, [(0, 0, 45)], **INDELS_KATS["sam_example"]["params"])
    assert [e[1] for e in events] == [13, 13, 17] and io.strings(events, seq)[:2] == [b"G", b"AG"]  # anchor 13 with G and AG
    s = sites_array([(ref, pos, region, kind, base, alt, depth, ro, fwd, rev) for ref, pos, region, kind, base, alt, depth, ro, fwd, rev in sites])
    e, e_seq = events_array([(ref, pos, region, kind, n, seq[at:at + n] if kind == io.INS else b"", depth, fwd, rev)
                             for ref, pos, region, kind, n, depth, fwd, rev, at in events])
    assert e_seq == seq
    assert vo.lines(s, e, seq, contigs, text) == [ln.encode() for ln in KATS["sam_example"]["lines"]]


def test_one_line_of_each_type_written_by_hand():
    k = KATS["kats"]
    contigs = [(n.encode(), start, ln) for n, start, ln in k["contigs"]]
    events, seq = events_array(k["events"])
    got, off = vo.emit(sites_array(k["sites"]), events, seq, contigs, k["text"].encode())
    assert got == "".join(k["lines"]).encode() and off == [0] + list(np.cumsum([len(ln) for ln in k["lines"]]))
    assert {ln.rsplit("=", 1)[1] for ln in k["lines"]} == {"snp\n", "del\n", "ins\n"}


def test_the_header_byte_for_byte_from_the_oracle_and_from_the_library():
    h = KATS["header"]
    entries, start = [], 0
    for name, ln in h["contigs"]:
        entries.append((name.encode(), start, ln))
        start += ln + 1
    assert vo.header(entries) == h["text"].encode()
    assert vcf.header(sam.Contigs(entries)) == h["text"].encode()
    assert vcf.header(sam.Contigs([])) == vo.header([]) and b"##contig" not in vo.header([])
    table, n = sam.Contigs(entries), C.c_uint64(0)
    out = np.full(len(h["text"]) + 8, 0xC3, dtype=np.uint8)
    args = (table.table.ctypes.data, 2, table.names.ctypes.data)
    assert _lib.lib().bg_vcf_header(*args, out.ctypes.data, len(h["text"]) - 1, C.byref(n)) == vo.OPS_CAP and n.value == len(h["text"])
    assert (out == 0xC3).all()  # one byte short: nothing written
    assert _lib.lib().bg_vcf_header(*args, out.ctypes.data, len(h["text"]), C.byref(n)) == 0 and (out[len(h["text"]):] == 0xC3).all()
    assert _lib.lib().bg_vcf_header(*args, None, 5, C.byref(n)) == vo.INVALID_ARG and _lib.lib().bg_vcf_header(*args, None, 0, None) == vo.INVALID_ARG


def parse(line):
    m = LINE.fullmatch(line)
    assert m, line
    chrom, pos, ref, alt, dp, ro, ao, saf, sar, kind = m.groups()
    return dict(chrom=chrom, pos=int(pos) - 1, ref=ref, alt=alt, dp=int(dp), ro=None if ro is None else int(ro), ao=int(ao), saf=int(saf), sar=int(sar),
                kind=kind)


def test_a_strict_parser_finds_every_field_and_ref_is_the_folded_text():
    kinds, folded = set(), 0
    for c in vc.corpus():
        text, line_off = vc.want_of(c)
        assert text.count(b"\n") == len(line_off) - 1 == int((c["sites"]["kind"] == vc.SNV).sum()) + len(c["events"]), c["name"]
        by_name = {bytes(name): (start, ln) for name, start, ln in c["contigs"]}
        for a, b in zip(line_off, line_off[1:]):
            f = parse(text[a:b])
            start, ln = by_name[f["chrom"]]
            at = start + f["pos"]
            assert 0 <= f["pos"] < ln and f["ref"][0] == TABLE[c["text"][at]], c["name"]
            assert f["ao"] == f["saf"] + f["sar"] and (f["ro"] is not None) == (f["kind"] == b"snp"), c["name"]
            if f["kind"] == b"snp":
                assert len(f["ref"]) == len(f["alt"]) == 1 and f["alt"] != f["ref"] or c["text"][at] not in b"ACGTacgt", c["name"]
            elif f["kind"] == b"del":
                n = len(f["ref"]) - 1
                assert n >= 1 and f["alt"] == f["ref"][:1] and f["pos"] + n < ln, c["name"]
                assert f["ref"][1:] == bytes(c["text"][at + 1:at + 1 + n]).translate(bytes(TABLE)), c["name"]
                folded += f["ref"][1:] != bytes(c["text"][at + 1:at + 1 + n])
            else:
                assert len(f["ref"]) == 1 and len(f["alt"]) >= 2 and f["alt"][:1] == f["ref"], c["name"]
            kinds.add(f["kind"])
    assert kinds == {b"snp", b"del", b"ins"} and folded > 10


def test_the_lines_and_counters_are_the_lists_in_merged_order():
    """the parsed fields against the elements, taken in the order a stable sort by (region, pos, events behind SNVs) gives"""
    for c in vc.corpus():
        text, line_off = vc.want_of(c)
        elems = [(int(s["region"]), int(s["pos"]), 0, k, s) for k, s in enumerate(c["sites"]) if s["kind"] == vc.SNV]
        elems += [(int(e["region"]), int(e["pos"]), 1, k, e) for k, e in enumerate(c["events"])]
        elems.sort(key=lambda t: t[:4])
        assert len(elems) == len(line_off) - 1
        for (region, pos, is_event, _, rec), a, b in zip(elems, line_off, line_off[1:]):
            f = parse(text[a:b])
            assert (f["chrom"], f["pos"], f["dp"], f["saf"], f["sar"]) == (bytes(c["contigs"][int(rec["ref"])][0]), pos, int(rec["depth"]), int(rec["alt_fwd"]),
                                                                            int(rec["alt_rev"])), c["name"]
            assert f["kind"] == (b"snp", b"del", b"ins")[int(rec["kind"])], c["name"]
            if is_event and rec["kind"] == vc.INS:
                raw = c["seq"][int(rec["seq_off"]):int(rec["seq_off"]) + int(rec["len"])]
                assert f["alt"][1:] == bytes(b if b in b"ACGT" else ord("N") for b in raw), c["name"]
            if not is_event:
                assert f["ro"] == int(rec["ref_count"]) and f["alt"] == bytes([int(rec["alt"])]), c["name"]


def test_the_corpus_holds_what_it_promises():
    by = {c["name"]: c for c in vc.corpus()}
    text, off = vc.want_of(by["deletions whose line is one under, at and one over the stage size"])
    lens = [b - a for a, b in zip(off, off[1:])]
    assert lens.count(vc.STAGE - 1) == lens.count(vc.STAGE) == lens.count(vc.STAGE + 1) == 2  # a deletion and an insertion each
    text, off = vc.want_of(by["POS 9 / 10 .. 999 999 / 1 000 000, counters at 9 / 10, 99 / 100 and 2^32 - 1, AO beyond 2^32"])
    for needle in (b"\t9\t", b"\t10\t", b"\t99\t", b"\t100\t", b"\t999999\t", b"\t1000000\t", b"DP=9;", b"DP=10;", b"AO=8589934590;", b"SAF=4294967295;", b"DP=0;"):
        assert needle in text, needle
    text, off = vc.want_of(by["a deletion of 70 000 bases, one more that ends on the contig's last base"])
    assert max(b - a for a, b in zip(off, off[1:])) > 70_000
    assert len(vc.want_of(by["neither"])[0]) == 0 and vc.want_of(by["neither"])[1] == [0]
    assert vc.want_of(by["sites of kind DEL and INS only: no line"]) == (b"", [0])


def test_every_refusal_is_refused_with_its_index_and_the_base_is_not():
    vc.want_of(vc.base_case())
    for c in vc.refusals():
        try:
            vc.want_of(c)
            raise AssertionError(c["name"])
        except vo.Refused as e:
            assert (e.status, e.first_bad) == (vo.INVALID_ARG, c["want"]), c["name"]


def test_the_binding_agrees_with_the_header():
    hdr = open(os.path.join(vc.ROOT, "include", "biogpu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} bg_vcf_params_t;", hdr).group(1)
    assert re.findall(r"uint32_t (\w+);", body) == list(_lib.VCF_PARAMS_DTYPE.names) and _lib.VCF_PARAMS_DTYPE.itemsize == 8
    for name in ("bg_vcf_header", "bg_vcf_emit", "bg_vcf_emit_dev"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    decl = re.search(r"int bg_vcf_emit_dev\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(_lib.lib().bg_vcf_emit_dev.argtypes) == len(_lib.lib().bg_vcf_emit.argtypes) + 1


def test_a_null_ctx_is_refused_before_any_device_work():
    prm = vcf.params()
    n = [C.c_uint64(7) for _ in range(3)]
    rc = _lib.lib().bg_vcf_emit_dev(None, prm.ctypes.data, None, 0, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, C.byref(n[0]), C.byref(n[1]),
                                    C.byref(n[2]), None)
    assert rc == vo.INVALID_ARG
    assert _lib.lib().bg_vcf_emit(None, prm.ctypes.data, None, 0, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, C.byref(n[0]), C.byref(n[1]),
                                  C.byref(n[2])) == vo.INVALID_ARG

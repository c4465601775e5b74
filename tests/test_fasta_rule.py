"""The FASTA reader's rules (include/biogpu.h, io/fasta.rs:334-359, 982-1009, 1090-1111) on the CPU: the Python restatement
against the reference's own cases, each rule pinned by one input, and the host reference builder (no GPU) against the numpy
statement, through bg_sam_header."""
import json
import os

import numpy as np
import pytest

import fasta_oracle as fo
from rust_bio_amd import _lib, fasta, sam

KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fasta_kats.json")))


def _b(s):
    return None if s is None else s.encode("latin-1")


@pytest.mark.parametrize("case", KATS["read"], ids=lambda c: c["name"])
def test_oracle_reads_the_reference_cases(case):
    recs, status, err_pos = fo.parse(_b(case["text"]))
    assert (status, err_pos) == (case["status"], case["err_pos"])
    assert [(r["id"], r["desc"], r["seq"], r["check"]) for r in recs] == [(_b(w["id"]), _b(w["desc"]), _b(w["seq"]), w["check"])
                                                                          for w in case["records"]]


@pytest.mark.parametrize("case", KATS["check"], ids=lambda c: c["check"] + "@" + c["source"])
def test_oracle_check_cases(case):
    assert fo.check({"id": _b(case["id"]), "desc": _b(case["desc"]), "seq": _b(case["seq"])}) == case["check"]


def _parse(text):
    recs, status, err_pos = fo.parse(text)
    return [(r["id"], r["desc"], r["seq"]) for r in recs], status, err_pos


def test_a_bad_header_line_loses_the_record_before_it():
    # the header of record 1 is read by record 0's loop: its failure is record 0's
    text = b">a\nAC\n>b\xff\nGT\n"
    assert _parse(text) == ([], "Io", 6)
    text = b">a\nAC\n>b\nG\xffT\n>c\nA\n"
    assert _parse(text) == ([(b"a", None, b"AC")], "Io", 9)
    assert _parse(b"\xff>a\nAC\n") == ([], "Io", 0)


def test_the_empty_record_ends_the_stream():
    assert _parse(b">\n\n>x\nAC\n") == ([], "ok", 0)
    assert _parse(b">a\nAC\n>  \n \n>x\nAC\n") == ([(b"a", None, b"AC")], "ok", 0)
    assert _parse(b">a\nAC\n>\n>x\xff\n") == ([(b"a", None, b"AC")], "Io", 8)  # the empty record's own read fails first
    assert _parse(b">a\nAC\n>\n\n>x\xff\n") == ([(b"a", None, b"AC")], "Io", 9)  # ... also on the line that would end it
    assert _parse(b">a\nAC\n>\n\n>y\nA\n>x\xff\n") == ([(b"a", None, b"AC")], "ok", 0)


def test_a_leading_blank_line_is_missing_gt():
    assert _parse(b"\n>a\nAC\n") == ([], "MissingGt", 0)
    assert _parse(b"") == ([], "ok", 0)
    assert _parse(b"\n") == ([], "MissingGt", 0)
    assert _parse(b">") == ([], "ok", 0)


def test_header_fields():
    assert _parse(b"> desc\nA\n")[0] == [(b"", b"desc", b"A")]
    assert _parse(b">id  two  words \t\nA\n")[0] == [(b"id", b" two  words", b"A")]
    assert _parse(">id\u2003d\u00a0\nA\n".encode())[0] == [(b"id", b"d", b"A")]
    assert _parse(b">id \nA\n")[0] == [(b"id", None, b"A")]
    assert _parse(b">id\x1cx\nA\n")[0] == [(b"id\x1cx", None, b"A")]  # U+001C is no White_Space (str.isspace says it is)


def test_sequence_lines_keep_interior_white_space_and_check_rejects_it():
    recs, status, _ = fo.parse(b">a\nAC GT \r\n\x0b\nA\n")
    assert status == "ok" and [(r["seq"], r["check"]) for r in recs] == [(b"AC GTA", "InvalidSequence")]
    recs, _, _ = fo.parse(">a\nAC\u2003\u0085\nG\u3000T\n".encode())
    assert [(r["seq"], r["check"]) for r in recs] == [("ACG\u3000T".encode(), "NonAsciiSequence")]


def _parsed_of(records):
    """a fasta.Parsed holding the oracle's records, as the parse would lay them out"""
    text = b"".join(b">" + r["id"] + b"\n" for r in records)
    recs = np.zeros(len(records), dtype=_lib.FAREC_DTYPE)
    so = np.zeros(len(records) + 1, dtype=np.uint64)
    pos = 0
    for k, r in enumerate(records):
        recs[k] = (pos + 1, 0, so[k], len(r["seq"]), len(r["id"]), 0, 0, fasta.CHECK.index(r["check"]))
        so[k + 1] = so[k] + len(r["seq"])
        pos += len(r["id"]) + 2
    return fasta.Parsed(np.frombuffer(text, dtype=np.uint8), recs, np.frombuffer(b"".join(r["seq"] for r in records), dtype=np.uint8), so, 0, 0)


@pytest.mark.parametrize("flags", [0, fasta.REF_FMD, fasta.REF_UPPER, fasta.REF_FMD | fasta.REF_UPPER])
def test_host_reference_statement_and_sam_header(flags):
    records, status, _ = fo.parse(b">chr1 first\nACGTacgtNN\nRYKM\n>empty\n>chrM\nggatcc\n")
    assert status == "ok" and len(records) == 3
    want, contigs = fo.reference(records, fmd=bool(flags & fasta.REF_FMD), upper=bool(flags & fasta.REF_UPPER))
    text, got = fasta.reference_arrays(_parsed_of(records), flags)
    assert text.tobytes() == want.tobytes()
    assert [(got.name(c), int(got.table["start"][c]), int(got.table["len"][c])) for c in range(len(got))] == contigs
    assert sam.header(got) == sam.header(sam.Contigs(contigs))
    assert b"@SQ\tSN:empty\tLN:0\n" in sam.header(got)


def test_host_reference_refusals():
    records, _, _ = fo.parse(b">a\nAC\n>\nGT\n>c\nA$\n")
    p = _parsed_of(records)
    with pytest.raises(fasta.BadRecord) as e:
        fasta.reference_arrays(p)
    assert e.value.index == 1
    ok = _parsed_of(records[:1])
    nt, nb, bad = (_lib.C.c_uint64(0) for _ in range(3))
    args = (None, 1, ok.recs.ctypes.data, ok.text.ctypes.data, ok.seq.ctypes.data)
    out, table, names = np.full(8, 7, np.uint8), np.zeros(1, _lib.SAM_CONTIG_DTYPE), np.zeros(8, np.uint8)
    tail = (_lib.C.byref(nt), _lib.C.byref(nb), _lib.C.byref(bad))
    L = _lib.lib()
    assert L.bg_fasta_reference(*args, 4, None, 0, None, None, 0, *tail) == -1  # unknown flag bits
    assert L.bg_fasta_reference(None, 0, *args[2:], 0, None, 0, None, None, 0, *tail) == -1  # no records
    assert L.bg_fasta_reference(*args, 0, out.ctypes.data, 2, table.ctypes.data, names.ctypes.data, 8, *tail) == -9
    assert (nt.value, nb.value) == (3, 1) and (out == 7).all()  # sized, nothing written
    assert L.bg_fasta_reference(*args, 0, out.ctypes.data, 8, table.ctypes.data, names.ctypes.data, 0, *tail) == -9
    assert L.bg_fasta_reference(*args, 0, out.ctypes.data, 3, table.ctypes.data, names.ctypes.data, 1, *tail) == 0
    assert out[:3].tobytes() == b"AC$"

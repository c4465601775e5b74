"""bg_bam_header_parse (host only, through ctypes): the inverse of bg_bam_header — contigs, names and `start` come back, every
prefix that ends inside the header says how long it must at least be, the SAM text comes back as a range, and each refusal of
the rule is given.  Held to tests/bam_read_oracle.py."""
import ctypes as C
import struct

import numpy as np
import pytest

import bam_oracle
import bam_read_oracle as ro
from rust_bio_amd import _lib, bam, sam

OPS_CAP, INVALID_ARG = -9, -1


def parse(b, cap=None):
    """-> (rc, n_contigs, names_bytes, text_off, text_len, body_off, need, table, names)"""
    out = [C.c_uint64(0) for _ in range(6)]
    refs = [C.byref(x) for x in out]
    buf = np.frombuffer(bytes(b) + b"\0", np.uint8)
    rc = _lib.lib().bg_bam_header_parse(buf.ctypes.data, len(b), None, 0, None, 0, *refs)
    if rc or cap is False:
        return (rc,) + tuple(x.value for x in out) + (None, None)
    n, nb = (out[0].value, out[1].value) if cap is None else cap
    table, names = np.zeros(max(n, 1), _lib.SAM_CONTIG_DTYPE), np.full(max(nb, 1), 0x7E, np.uint8)
    rc = _lib.lib().bg_bam_header_parse(buf.ctypes.data, len(b), table.ctypes.data, n, names.ctypes.data, nb, *refs)
    return (rc,) + tuple(x.value for x in out) + (table[:n], names[:nb].tobytes())


def entries(n, name_len=None, big=False):
    out, start = [], 0
    for i in range(n):
        name = (b"c%d" % i) if name_len is None else (b"%d" % i).rjust(name_len, b"x")[-name_len:]
        ln = 2**31 - 1 if big and i == n - 1 else 100 + 7 * i
        out.append((name, start, ln))
        start += ln + 1
    return out


@pytest.mark.parametrize("n, name_len, big", [(0, None, False), (1, 1, False), (1, 254, False), (300, None, False), (3, 254, True), (2, 1, True)])
def test_the_header_written_comes_back(n, name_len, big):
    ent = entries(n, name_len, big)
    b = bam.header(sam.Contigs(ent))
    text, want, body = ro.parse_header(b)
    assert want == ent and body == len(b)
    rc, k, nb, text_off, text_len, body_off, need, table, names = parse(b)
    assert (rc, k, body_off, need) == (0, n, len(b), 0)
    assert b[text_off:text_off + text_len] == text
    assert names == b"".join(e[0] for e in ent) and nb == len(names)
    got = [(names[int(t["name_off"]):int(t["name_off"]) + int(t["name_len"])], int(t["start"]), int(t["len"])) for t in table]
    assert got == ent
    text2, contigs, body2 = bam.read_header(b + b"trailing records")
    assert (text2, body2) == (text, len(b)) and [(contigs.name(c), int(contigs.table["start"][c]), int(contigs.table["len"][c])) for c in range(n)] == ent


def test_every_prefix_says_how_much_it_needs():
    b = bam_oracle.header(b"@HD\tVN:1.6\n@SQ\tSN:a\tLN:5\n", [(b"a", 0, 5), (b"second", 6, 70), (b"c", 77, 1)])
    for n in range(len(b)):
        rc, *_, need, _, _ = parse(b[:n], cap=False)
        with pytest.raises(ro.Short) as e:
            ro.parse_header(b[:n])
        assert rc == OPS_CAP and n < need <= len(b) and need == e.value.need, (n, need)
    assert parse(b)[0] == 0 and parse(b + b"more")[5] == len(b)


def test_read_header_fetches_a_logarithmic_number_of_prefixes():
    ent = entries(3000)
    b = bam.header(sam.Contigs(ent)) + b"\0" * 100
    asked = []

    def fetch(n):
        asked.append(n)
        return b[:n]
    _, contigs, body = bam.read_header(fetch, first=16)
    assert len(contigs) == 3000 and body == len(b) - 100
    assert len(asked) <= 16 and all(y >= 2 * x for x, y in zip(asked, asked[1:]))
    with pytest.raises(bam.BamReadError):
        bam.read_header(b[:body - 1])  # the stream itself ends inside the header


def test_a_text_with_read_groups_comes_back_as_a_range():
    text = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:x\tLN:9\n@RG\tID:g1\tSM:s\n@RG\tID:g2\tSM:t\n@PG\tID:p\n"
    b = bam_oracle.header(text, [(b"x", 0, 9)])
    rc, _, _, text_off, text_len, body_off, *_ = parse(b)
    assert rc == 0 and b[text_off:text_off + text_len] == text and body_off == len(b)


def test_caps_too_small_leave_the_tables_unwritten():
    b = bam.header(sam.Contigs(entries(4)))
    for cap in ((3, 100), (4, 7)):
        rc, k, nb, _, _, _, need, table, names = parse(b, cap=cap)
        assert (rc, k, nb, need) == (OPS_CAP, 4, 8, 0)
        assert not table["len"].any() and names == b"\x7e" * cap[1]


def test_each_refusal():
    good = bam_oracle.header(b"@HD\tVN:1.6\n", [(b"ab", 0, 5), (b"c", 6, 7)])
    at_nref = 8 + 11
    at_lname = at_nref + 4
    edits = {"magic": (0, b"BAM\2"), "a gzip magic": (0, b"\x1f\x8b\x08\x04"), "l_text -1": (4, struct.pack("<i", -1)),
             "n_ref -1": (at_nref, struct.pack("<i", -1)), "l_name 0": (at_lname, struct.pack("<i", 0)), "l_name -5": (at_lname, struct.pack("<i", -5)),
             "a name without NUL": (at_lname + 4 + 2, b"x"), "l_ref -1": (at_lname + 4 + 3, struct.pack("<i", -1))}
    assert parse(good)[0] == 0
    for name, (at, new) in edits.items():
        b = bytearray(good)
        b[at:at + len(new)] = new
        with pytest.raises(ro.Refused):
            ro.parse_header(bytes(b))
        assert parse(bytes(b))[0] == INVALID_ARG, name
        with pytest.raises(bam.BamReadError):
            bam.read_header(bytes(b))

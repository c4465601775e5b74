"""tests/bam_oracle.py against constants written out by hand (the bins of the specification's examples, three records and a
block in tests/golden/bam_kats.json), against itself (record -> fields gives back the line, over every case of
tests/sam_edge_cases.py) and against gzip (the framed stream decompresses to the input).  No GPU."""
import gzip
import json
import os
import struct

import pytest

import bam_oracle as bo
import sam_edge_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "bam_kats.json")))
KAT_CONTIGS = [(n.encode(), s, ln) for n, s, ln in KATS["contigs"]]
# the cases with a line on (or beside) the 3 Gbp contig of WIDE_CONTIGS, and those with an id of 255 bytes
UNREPRESENTABLE = {"pos_pnext", "tlen", "cigar", "flag_paired", "qname_single", "qname_paired"}


def test_bins():
    assert bo.reg2bin(-1, 0) == 4680
    assert bo.reg2bin(0, 1) == 4681
    assert bo.reg2bin(16383, 16385) == 585
    assert bo.reg2bin(0, 2**29) == 0
    assert bo.reg2bin(2**29 - 1, 2**29) == 4681 + 32767


def test_integer_tag_types():
    want = {-2**31: b"i", -32769: b"i", -32768: b"s", -129: b"s", -128: b"c", -1: b"c", 0: b"C", 255: b"C", 256: b"S", 65535: b"S", 65536: b"I",
            2**31 - 1: b"I", 2**32 - 1: b"I"}
    assert {v: bo.int_tag(v)[0] for v in want} == want


def test_base_codes():
    assert bo.pack_seq(b"=ACMGRSVTWYHKDBN") == bytes.fromhex("0123456789abcdef")
    assert bo.pack_seq(b"acgtn") == bytes.fromhex("1248f0")
    assert bo.pack_seq(b"U.*") == bytes.fromhex("fff0")


@pytest.mark.parametrize("k", range(len(KATS["records"])))
def test_written_out_records(k):
    kat = KATS["records"][k]
    want = bytes.fromhex("".join(h for _, h in kat["parts"]))
    line = kat["line"].encode()
    assert bo.record(line, KAT_CONTIGS) == want
    assert bo.decode(want, KAT_CONTIGS) == [f.upper() if i == 9 else f for i, f in enumerate(ec.fields(line))]


def test_header():
    text = b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n"
    want = b"BAM\1" + bytes([len(text), 0, 0, 0]) + text + bytes.fromhex("02000000" "05000000") + b"chr1\0" + bytes.fromhex("e8030000" "05000000") + \
        b"chr2\0" + bytes.fromhex("f4010000")
    assert bo.header(text, KAT_CONTIGS) == want
    with pytest.raises(bo.Unrepresentable):
        bo.header(text, [(b"big", 0, 2**31)])
    assert bo.header(text, [(b"big", 0, 2**31 - 1)])[-4:] == bytes.fromhex("ffffff7f")


def test_written_out_blocks():
    for b in KATS["blocks"]:
        assert bo.block(bytes.fromhex(b["payload"])).hex() == b["block"]
    assert bo.EOF_BLOCK.hex() == KATS["eof"] and gzip.decompress(bo.EOF_BLOCK) == b""
    assert bo.frame(b"") == b"" and bo.frame(b"", True) == bo.EOF_BLOCK


@pytest.mark.parametrize("n", [0, 1, 3, 4, 65279, 65280, 65281, 2 * 65280, 2 * 65280 + 1])
def test_framed_stream_decompresses(n):
    x = bytes((i * 131 + (i >> 8)) & 0xFF for i in range(n))
    framed = bo.frame(x, True)
    assert len(framed) == n + 31 * ((n + 65279) // 65280) + 28
    assert gzip.decompress(framed) == x


@pytest.mark.parametrize("name", sorted(ec.EMIT_CASES))
def test_decode_gives_back_the_line(name):
    case = ec.emit_case(name)
    want = case.want()
    recs, refused = [], 0
    for ln in want:  # line by line: a case with lines BAM cannot hold still has its other lines looked at
        try:
            recs.append(bo.record(ln, case.contigs) if ln else b"")
        except bo.Unrepresentable:
            refused += 1
            continue
        if ln:
            assert bo.decode(recs[-1], case.contigs) == ec.fields(ln), name
    assert (refused > 0) == (name in UNREPRESENTABLE)
    assert bo.split_records(b"".join(recs)) == [r for r in recs if r]
    if refused:
        with pytest.raises(bo.Unrepresentable):
            bo.records(want, case.contigs)


def test_more_than_65535_operations():
    line = b"long\t0\tchr1\t1\t9\t" + b"1=1D" * 40000 + b"\t*\t0\t0\t" + b"A" * 40000 + b"\t*\tAS:i:1\n"
    contigs = [(b"chr1", 0, 100000)]
    rec = bo.record(line, contigs)
    n_cigar, = struct.unpack_from("<H", rec, 16)
    assert n_cigar == 2 and rec[36 + 5:36 + 13] == bytes.fromhex("04c40900" "03881300")  # 40000S 80000N
    assert rec[-(8 + 4 * 80000):][:8] == b"CGBI" + struct.pack("<I", 80000)
    assert bo.decode(rec, contigs) == ec.fields(line)

"""The SAM record without a GPU: the CPU statement of the record (tests/sam_oracle.py) against hand-written lines
(tests/golden/sam_kats.json), `bg_sam_header` (host code) against the same statement, and every line the statement produces for
a synthetic batch against the regular expressions the SAM specification gives for the eleven mandatory fields (SAM v1.6,
section 1.4) and for tags (section 1.5)."""
import ctypes as C
import json
import os
import re

import numpy as np

import sam_oracle as so
from rust_bio_amd import _lib, sam

KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_kats.json")))
DTYPES = (_lib.SEED_HIT_DTYPE, _lib.MULTI_HIT_DTYPE, _lib.PAIR_HIT_DTYPE, _lib.FQREC_DTYPE)
OPS_CAP = -9


def contig_list(entries):
    return [(name.encode(), start, ln) for name, start, ln in entries]


def test_kats_cover_what_they_must():
    recs = KATS["records"]
    assert len(recs) + len(KATS["header"]) >= 12 and all(k["spec"] for k in recs + KATS["header"])
    md = [line.split("MD:Z:")[1].strip() for k in recs for line in k["expect"] if "MD:Z:" in line]
    assert "0A0" in md and any("^AC0T" in m for m in md) and any(re.search(r"[ACGT]0\^", m) for m in md)
    flags = [int(line.split("\t")[1]) for k in recs for line in k["expect"] if line]
    assert any(f & 0x10 and f & 0x1 for f in flags) and any(f & 0x4 and f & 0x1 and not f & 0x8 for f in flags)
    assert any(line.startswith("*\t") for k in recs for line in k["expect"])


def test_oracle_reproduces_every_kat():
    text, contigs = KATS["text"].encode(), contig_list(KATS["contigs"])
    for kat in KATS["records"]:
        flags, K, fq, hits, strand, ops, multi, pairs = so.kat_arrays(kat, *DTYPES)
        got = so.lines(contigs, fq, hits, strand, ops, flags, K, multi, pairs, text)
        assert got == [e.encode() for e in kat["expect"]], kat["name"]


def test_header_matches_the_oracle():
    cases = [contig_list(h["contigs"]) for h in KATS["header"]]
    cases.append([(b"ctg%d" % c, 1000 * c, 999 - c) for c in range(300)])
    for want, entries in zip([h["expect"].encode() for h in KATS["header"]] + [None], cases):
        assert so.header(entries) == (want or so.header(entries))
        table = sam.Contigs(entries)
        assert [table.name(c) for c in range(len(table))] == [e[0] for e in entries]
        assert sam.header(table) == so.header(entries)
        # an exact-fit cap writes everything, a cap one byte short nothing
        need, n = len(so.header(entries)), C.c_uint64(0)
        buf = np.full(need + 1, 0x7e, dtype=np.uint8)
        args = (table.table.ctypes.data, len(table), table.names.ctypes.data, buf.ctypes.data)
        assert _lib.lib().bg_sam_header(*args, need, C.byref(n)) == 0 and n.value == need
        assert buf[:need].tobytes() == so.header(entries) and buf[need] == 0x7e
        buf[:] = 0x7e
        assert _lib.lib().bg_sam_header(*args, need - 1, C.byref(n)) == OPS_CAP and n.value == need
        assert (buf == 0x7e).all()


RNAME = rb"[0-9A-Za-z!#$%&+./:;?@^_|~-][0-9A-Za-z!#$%&*+./:;=?@^_|~-]*"
FIELDS = [rb"[!-?A-~]{1,254}", rb"[0-9]+", rb"\*|" + RNAME, rb"[0-9]+", rb"[0-9]+", rb"\*|([0-9]+[MIDNSHPX=])+", rb"\*|=|" + RNAME,
          rb"[0-9]+", rb"-?[0-9]+", rb"\*|[A-Za-z=.]+", rb"[!-~]+"]
TAG = rb"[A-Za-z][A-Za-z0-9]:(i:[-+]?[0-9]+|Z:[ !-~]*)"
MD = rb"MD:Z:[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*"


def synthetic_batch(n=400, seed=3):
    """hits made up on the CPU: three contigs in a random text, random operation lists at random places on either strand, some
    across a boundary, some unmapped; interleaved pairs"""
    rng = np.random.default_rng(seed)
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=6001)
    text[[1999, 3999, 6000]] = ord("$")
    contigs = [(b"chrA", 0, 1999), (b"chr_B.1", 2000, 1999), (b"c|3", 4000, 2000)]
    reads, hits = [], []
    for r in range(n):
        L = int(rng.integers(1, 120))
        ops = "".join(rng.choice(list("=====XDI"), size=L))
        ops = re.sub(r"^[DI]+|[DI]+$", "", ops) or "="
        clip = [int(rng.integers(0, 4)), int(rng.integers(0, 4))]
        qlen = sum(c in "=XI" for c in ops)
        rlen = sum(c in "=XD" for c in ops)
        seq = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=clip[0] + qlen + clip[1]))
        qual = bytes(rng.integers(33, 127, size=len(seq)).astype(np.uint8))
        start = int(rng.integers(0, 6000 - rlen))
        reads.append({"id": "read%d/%d" % (r // 2, r % 2 + 1), "seq": seq.decode(), "qual": qual.decode()})
        hits.append(None if r % 11 == 0 else {"score": int(rng.integers(-50, 150)), "strand": int(rng.integers(0, 2)), "ref_start": start,
                                              "ref_end": start + rlen, "xstart": clip[0], "xend": clip[0] + qlen, "xlen": len(seq),
                                              "ops": ops})
    pairs = [{"proper": int(rng.integers(0, 2)), "span": 0} for _ in range(n // 2)]
    kat = {"flags": ["PAIRED", "NM", "MD"], "K": 1, "reads": reads, "hits": hits, "pairs": pairs}
    return text.tobytes(), contigs, kat


def test_every_line_satisfies_the_specification():
    text, contigs, kat = synthetic_batch()
    flags, K, fq, hits, strand, ops, multi, pairs = so.kat_arrays(kat, *DTYPES)
    seen = {"placed": 0, "unplaced": 0, "md_del": 0}
    for paired in (so.PAIRED, 0):
        ls = so.lines(contigs, fq, hits, strand, ops, (flags & ~so.PAIRED) | paired, K, None, pairs if paired else None, text)
        assert len(ls) == len(hits)
        for line in ls:
            assert line.endswith(b"\n") and line.count(b"\n") == 1
            f = line[:-1].split(b"\t")
            assert len(f) >= 11
            for rx, v in zip(FIELDS, f):
                assert re.fullmatch(rx, v), (rx, line)
            for t in f[11:]:
                assert re.fullmatch(TAG, t), line
            flag = int(f[1])
            assert flag < 65536 and int(f[4]) < 256 and int(f[3]) < 2**31 and abs(int(f[8])) < 2**31
            if flag & 0x4:
                assert f[5] == b"*" and len(f) == 11
                seen["unplaced"] += 1
            else:
                seen["placed"] += 1
                query = sum(int(n) for n, c in re.findall(rb"([0-9]+)([MIDNSHPX=])", f[5]) if c in b"MIS=X")
                assert query == len(f[9]) == len(f[10]), line
                md = [t for t in f[11:] if t.startswith(b"MD:Z:")]
                assert len(md) == 1 and re.fullmatch(MD, md[0]), line
                seen["md_del"] += b"^" in md[0]
                name = {c[0]: c for c in contigs}[f[2]]
                ref = sum(int(n) for n, c in re.findall(rb"([0-9]+)([MIDNSHPX=])", f[5]) if c in b"MDN=X")
                assert 1 <= int(f[3]) and int(f[3]) + ref - 1 <= name[2], line
    assert seen["placed"] >= 300 and seen["unplaced"] >= 60 and seen["md_del"] >= 100, seen

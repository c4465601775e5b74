"""Cases for reading BAM (tests/test_bam_read_host_bodies.py, tests/test_gpu_bam_records.py, tests/test_gpu_bam_reads.py): a raw
record builder for what no SAM line encodes, the corpus of streams with what the Python restatement (tests/bam_read_oracle.py)
says of each, and the stand-alone program that runs the kernels' bodies on the CPU (tests/bam_read_host_bodies.cpp)."""
import os
import struct
import subprocess

import numpy as np

import bam_oracle
import bam_read_oracle as ro
from rust_bio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REF = 64  # (the close pair needs a refID >= 33 to be legal)
CONTIGS = [(b"chr%d" % i, 1001 * i, 1000) for i in range(N_REF)]
TEXT = b"@HD\tVN:1.6\tSO:unsorted\n@RG\tID:a\tSM:s\n"
HEADER = bam_oracle.header(TEXT, CONTIGS)
BODY = len(HEADER)
NONE = ro.NONE
FQREC = _lib.FQREC_DTYPE


def raw(name=b"r1", flag=0, ref=-1, pos=-1, cigar=(), codes=(), qual=None, next_ref=-1, next_pos=-1, tlen=0, tags=b"", mapq=0, l_name=None,
        l_seq=None, block=None):
    """a BAM record field by field; codes: 4-bit base codes; qual: raw quality bytes (None: 0xFF); the overrides lie on purpose"""
    nm = name + b"\0"
    codes = list(codes)
    packed = bytes((a << 4) | b for a, b in zip(codes[::2], codes[1::2] + [0] * (len(codes) & 1)))
    q = b"\xff" * len(codes) if qual is None else bytes(qual)
    assert len(q) == len(codes)
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(nm) if l_name is None else l_name, mapq, 4680, len(cigar), flag,
                       len(codes) if l_seq is None else l_seq, next_ref, next_pos, tlen)
    body += nm + struct.pack("<%dI" % len(cigar), *cigar) + packed + q + tags
    return struct.pack("<I", len(body) if block is None else block) + body


def seq_rec(i, n, flag=0, **kw):
    rng = np.random.default_rng(1000 + i)
    return raw(b"read%d" % i, flag=flag, codes=rng.choice([1, 2, 4, 8, 15], n).tolist(), qual=rng.integers(0, 42, n).astype(np.uint8).tobytes(), **kw)


def pad_tag(n):
    """n >= 4 bytes of a Z tag"""
    assert n >= 4
    return b"XPZ" + b"p" * (n - 4) + b"\0"


def close_pair(seed=7, tries=20000):
    """record A such that an accepted record also stands 4 bytes behind its start: that one's block_size is A's refID.  Found by a
    seeded random search against the Python verdict; returns A, followed by bytes that let the second one end inside the stream"""
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        name = bytes(rng.integers(65, 91, int(rng.integers(1, 9))).astype(np.uint8))
        a = raw(name, ref=int(rng.integers(0, N_REF)), pos=int(rng.integers(-1, N_REF)), cigar=[int(rng.integers(1, 50)) << 4] * int(rng.integers(1, 4)),
                next_ref=int(rng.integers(-1, 4)), next_pos=int(rng.integers(-1, N_REF)), tlen=int(rng.integers(-1, 100)), tags=pad_tag(40))
        if ro.verdict(a, 0, N_REF) == len(a) and ro.verdict(a, 4, N_REF) is not None:
            return a
    return None


def fakes_in_quals():
    inner = raw(b"in", ref=2, pos=5, codes=[1, 2], qual=b"\x05\x06")
    q = b"\x01" * 3 + inner + b"\x02" * 4
    return raw(b"outer", codes=[1] * len(q), qual=q), 36 + 6 + (len(q) + 1) // 2 + 3


def fakes_in_b_tag():
    f = [raw(b"f%d" % i, ref=i, pos=i) for i in range(3)]
    data = b"".join(f)
    return raw(b"withB", codes=[1, 2, 4], qual=b"\x10\x11\x12", tags=b"XBBC" + struct.pack("<I", len(data)) + data), len(data)


def corpus():
    """[(name, stream, n_ref)] — good and refused streams alike; the oracle's walk says which"""
    out = []

    def add(name, recs, tail=b"", n_ref=N_REF):
        out.append((name, HEADER + b"".join(recs) + tail, n_ref))
    plain = [seq_rec(i, 20 + i, ref=i % 3, pos=10 * i, cigar=[(20 + i) << 4]) for i in range(5)]
    add("no record", [])
    add("one record", plain[:1])
    add("the minimal record", [raw(b"")])
    assert len(raw(b"")) == 37
    add("no cigar / no bases / neither", [seq_rec(1, 9), raw(b"c", ref=1, pos=3, cigar=[5 << 4]), raw(b"n")])
    add("odd and even l_seq", [seq_rec(2, 7), seq_rec(3, 8), seq_rec(4, 1)])
    add("0xFF qualities", [raw(b"q", codes=[1, 2, 4, 8, 15]), seq_rec(5, 5)])
    add("star names", [raw(b"*", codes=[1, 2], qual=b"\x01\x02"), raw(b"*")])
    add("unplaced", [raw(b"u", flag=4, ref=-1, pos=-1, codes=[1], qual=b"\x09")])
    rec, at = fakes_in_quals()
    assert ro.verdict(rec, at, N_REF) is not None
    add("a record inside the qualities", plain[:2] + [rec] + plain[2:])
    rec, n = fakes_in_b_tag()
    assert ro.verdict(rec, len(rec) - n, N_REF) is not None
    add("three linked fakes in a B:C tag", plain[:1] + [rec] + plain[1:])
    pair = close_pair()
    if pair is not None:
        add("two accepted positions 4 bytes apart", plain[:1] + [pair] + plain[1:])
    good = HEADER + b"".join(plain)
    out.append(("one byte short", good[:-1], N_REF))
    out.append(("one byte long", good + b"\0", N_REF))
    jump = bytearray(good)
    o = BODY + len(plain[0])
    struct.pack_into("<I", jump, o, len(plain[1]) - 4 + 11)
    out.append(("block_size into the middle of the next record", bytes(jump), N_REF))
    add("refID == n_ref", plain[:2] + [raw(b"x", ref=N_REF, pos=1)] + plain[2:])
    add("refID == n_ref - 1", plain[:2] + [raw(b"x", ref=N_REF - 1, pos=1)] + plain[2:])
    add("refID -2", plain[:1] + [raw(b"x", ref=-2)])
    add("next_refID == n_ref", plain[:3] + [raw(b"x", next_ref=N_REF)])
    add("pos -2", plain[:1] + [raw(b"x", ref=0, pos=-2)] + plain[1:])
    add("next_pos -2", [raw(b"x", next_pos=-2)] + plain)
    add("l_read_name 0", plain[:2] + [raw(b"x", l_name=0)])
    add("a name without its NUL", plain[:2] + [raw(b"x", l_name=1)])
    add("l_seq -1", plain[:4] + [raw(b"x", l_seq=-1)])
    add("block_size below what the fields need", plain[:1] + [raw(b"x", codes=[1, 2], qual=b"\1\2", block=36)] + plain[1:])
    add("fewer than 36 bytes left", plain, tail=raw(b"")[:35])
    add("n_ref 0, unplaced only", [raw(b"u1"), raw(b"u2", codes=[8], qual=b"\x03")], n_ref=0)
    return out


def mixed_flags():
    flags = [0, 0x4, 0x10, 0x100, 0x800, 0x904, 0x14, 0x40 | 0x1, 0x80 | 0x1 | 0x10]
    return HEADER + b"".join(seq_rec(100 + i, 5 + 3 * i, flag=fl) for i, fl in enumerate(flags))


def all_codes():
    """reversed records over all 16 base codes, both parities of l_seq, beside forward ones"""
    recs = []
    for n in (16, 17, 1, 2):
        codes = [(k * 7 + 3) % 16 for k in range(n)] if n < 16 else list(range(16)) + [5] * (n - 16)
        q = bytes(range(1, n + 1))
        recs += [raw(b"rev%d" % n, flag=0x10, codes=codes, qual=q), raw(b"fwd%d" % n, flag=0, codes=codes, qual=q)]
    recs.append(raw(b"revstar", flag=0x10, codes=[1, 2, 4]))
    recs.append(raw(b"hi", codes=[1], qual=b"\x60"))
    return HEADER + b"".join(recs)


def reads_cases():
    """[(name, stream, flags, require, exclude)]"""
    m, a = mixed_flags(), all_codes()
    return [("all", m, 0, 0, 0), ("exclude 0x900", m, 0, 0, 0x900), ("require 0x4", m, 0, 0x4, 0), ("exclude 0x4", m, 0, 0, 0x4),
            ("original", a, ro.ORIGINAL, 0, 0), ("as stored", a, 0, 0, 0), ("original, require 0x10", m, ro.ORIGINAL, 0x10, 0)]


def voff_cases():
    """[(name, block_off, out_off, [stream offsets])]: payloads of 100 and 50 bytes among empty members"""
    def table(sizes):
        block_off, out_off = [0], [0]
        for isize in sizes:
            block_off.append(block_off[-1] + 28 + isize // 2)
            out_off.append(out_off[-1] + isize)
        return block_off, out_off
    ask = [0, 1, 99, 100, 101, 149, 150]
    return [("an end-of-file member", *table([100, 50, 0]), ask), ("no end-of-file member", *table([100, 50]), ask),
            ("one empty member between", *table([100, 0, 50, 0]), ask), ("two empty members between", *table([100, 0, 0, 50]), ask),
            ("empty members in front", *table([0, 0, 100, 50, 0, 0]), ask), ("no member", [0], [0], [0])]


# ---- the program ------------------------------------------------------------------------------------------------------------
def build_program(exe, sanitize):
    """the program of bam_read_host_bodies.cpp, built as bgzf_inflate_cases.build_program builds its own"""
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + _lib.CSRC] + flags + [os.path.join(ROOT, "tests", "bam_read_host_bodies.cpp"), "-o", exe])
    return exe


def contig_table(contigs):
    t = np.zeros(len(contigs), dtype=_lib.SAM_CONTIG_DTYPE)
    at = 0
    for c, (name, start, ln) in enumerate(contigs):
        t[c] = (start, ln, at, len(name), 0)
        at += len(name)
    return t


def run_program(exe, tmp, cases):
    """cases: [dict(stream, body_off, n_ref, flags, require, exclude, contigs, off, tables, ask)] -> [dict] of what the program
    printed: table (rc, n, n_cand, first_bad, off), reads (rc, first_bad, recs, seq, seq_off, qual, qual_off, src), keys (rc,
    first_bad, key), voff"""
    inp, outp = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for c in cases:
            off, tables, ask = c.get("off") or [], c.get("tables"), c.get("ask") or []
            contigs = contig_table(c.get("contigs") or [])
            f.write(struct.pack("<10Q", len(c["stream"]), c["body_off"], c["n_ref"], c.get("flags", 0), c.get("require", 0), c.get("exclude", 0),
                                len(contigs), len(off), NONE if tables is None else len(tables[0]) - 1, len(ask)))
            f.write(c["stream"] + contigs.tobytes() + struct.pack("<%dQ" % len(off), *off))
            if tables is not None:
                f.write(struct.pack("<%dQ" % len(tables[0]), *tables[0]) + struct.pack("<%dQ" % len(tables[1]), *tables[1]))
            f.write(struct.pack("<%dQ" % len(ask), *ask))
    subprocess.check_call([exe, inp, outp])
    b = open(outp, "rb").read()
    at, got = 0, []

    def take(fmt):
        nonlocal at
        v = struct.unpack_from(fmt, b, at)
        at += struct.calcsize(fmt)
        return v

    def arr(dtype, n):
        nonlocal at
        v = np.frombuffer(b, dtype, n, at)
        at += v.nbytes
        return v
    for c in cases:
        g = {}
        rc, n, n_cand, bad = take("<q3Q")
        g["table"] = (rc, n, n_cand, bad, arr(np.uint64, n + 1).tolist() if rc == 0 else None)
        if c.get("off") or rc == 0:
            rc2, bad2, k, sb, qb = take("<q4Q")
            g["reads"] = (rc2, bad2) + ((arr(FQREC, k), arr(np.uint8, sb).tobytes(), arr(np.uint64, k + 1).tolist(), arr(np.uint8, qb).tobytes(),
                                        arr(np.uint64, k + 1).tolist(), arr(np.uint64, k).tolist()) if rc2 == 0 else ())
            rc3, bad3 = take("<qQ")
            m = (len(c["off"]) if c.get("off") else n + 1) - 1
            g["keys"] = (rc3, bad3, arr(np.uint64, m).tolist() if rc3 == 0 else None)
        g["voff"] = arr(np.uint64, len(c.get("ask") or [])).tolist()
        got.append(g)
    assert at == len(b)
    return got


def same_records(got, want):
    """a FQREC array against the oracle's list of dicts"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k, v in w.items():
            assert int(g[k]) == v, (k, int(g[k]), v)
    return True

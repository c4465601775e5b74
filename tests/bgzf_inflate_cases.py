"""Cases for the BGZF reader (tests/test_bgzf_inflate_host_bodies.py, tests/test_gpu_bgzf_inflate.py): a small BGZF writer
on top of zlib, a bit writer for hand-made deflate streams, the Python walk over BSIZE that the block table must equal, zlib's
verdict on a member, and the stand-alone program that runs the kernel's bodies on the CPU (tests/bgzf_inflate_host_bodies.cpp).

The expected payload of a good member is always the bytes that went in.  The expected verdict on a hand-made or corrupted
member is asked of zlib at test time (`verdict`): accept means `zlib.decompressobj(-15)` raises nothing, reaches `eof`, leaves no
unused byte, and the trailer holds the CRC-32 and the length of what came out."""
import os
import struct
import subprocess
import zlib

import numpy as np

import bgzf_deflate_cases as dc
from rust_bio_amd import _lib

ROOT = dc.ROOT
P = dc.P
HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")
EOF_BLOCK = HEAD + struct.pack("<H", 27) + b"\x03\x00" + bytes(8)
OK, BAD_TYPE, BAD_STORED, BAD_LENGTHS, BAD_SYMBOL, BAD_DISTANCE, TRUNCATED, TRAILING, SIZE, CRC = range(10)
INVALID_ARG, OPS_CAP, UNSUPPORTED = -1, -9, -11
NONE = 2**64 - 1
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ---- the writer -------------------------------------------------------------------------------------------------------------
def member_of(raw, data, isize=None, crc=None):
    """a BGZF member around the raw deflate stream `raw`, with the trailer of `data` (or the given fields)"""
    n = 18 + len(raw) + 8
    assert 28 <= n <= 65536
    return HEAD + struct.pack("<H", n - 1) + raw + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)


def stored(data):
    assert len(data) <= 65535
    return b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data


def deflate(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return z.compress(data) + z.flush()


def member(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    """one payload as one member; the stored form where the compressed one would not fit BSIZE"""
    raw = deflate(data, level, mem, strategy)
    return member_of(raw if len(raw) + 26 <= 65536 else stored(data), data)


def bgzf(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, eof=True):
    """`data` cut at 65 280 as a BGZF file"""
    return b"".join(member(data[a:a + P], level, mem, strategy) for a in range(0, len(data), P)) + (EOF_BLOCK if eof else b"")


# ---- the walk and zlib's verdict --------------------------------------------------------------------------------------------
def walk(f):
    """-> (status, block_off, out_off, first_bad): the rule of bg_bgzf_blocks in include/biogpu.h, member by member"""
    at, block_off, out_off = 0, [0], [0]

    def bad(rc):
        return rc, block_off[:-1], out_off[:-1], len(block_off) - 1
    while at < len(f):
        left = len(f) - at
        if left < 2 or f[at:at + 2] != b"\x1f\x8b" or left < 12:
            return bad(INVALID_ARG)
        if f[at + 2] != 8 or f[at + 3] != 4 or f[at + 10:at + 12] != b"\x06\x00":
            return bad(UNSUPPORTED)
        if left < 18:
            return bad(INVALID_ARG)
        if f[at + 12:at + 16] != b"BC\x02\x00":
            return bad(UNSUPPORTED)
        n = struct.unpack_from("<H", f, at + 16)[0] + 1
        if n < 28 or n > left:
            return bad(INVALID_ARG)
        isize = struct.unpack_from("<I", f, at + n - 4)[0]
        if isize > 65536:
            return bad(INVALID_ARG)
        at += n
        block_off.append(at)
        out_off.append(out_off[-1] + isize)
    return 0, block_off, out_off, NONE


def verdict(m):
    """zlib plus the trailer on one member -> its payload, or None"""
    z = zlib.decompressobj(-15)
    try:
        out = z.decompress(m[18:-8])
    except zlib.error:
        return None
    crc, isize = struct.unpack("<II", m[-8:])
    return out if z.eof and not z.unused_data and len(out) == isize and zlib.crc32(out) == crc else None


# ---- hand-made streams ------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, k):
        """k bits of v, lowest first (header fields, extra bits)"""
        for i in range(k):
            self.acc |= ((v >> i) & 1) << self.n
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                self.acc = self.n = 0
        return self

    def code(self, c, k):
        """a Huffman code: highest bit first"""
        for i in reversed(range(k)):
            self.bits((c >> i) & 1, 1)
        return self

    def done(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]


def len_sym(n):
    s = max(i for i in range(29) if LEN_BASE[i] <= n) if n < 258 else 28
    return 257 + s, LEN_EXTRA[s], n - LEN_BASE[s]


def dist_sym(d):
    s = max(i for i in range(30) if DIST_BASE[i] <= d)
    return s, DIST_EXTRA[s], d - DIST_BASE[s]


def canon(lens):
    """symbol -> code of the canonical Huffman code with these lengths (RFC 1951, 3.2.2)"""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = nxt[n]
            nxt[n] += 1
    return out


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


class Block:
    """one deflate block written symbol by symbol into a Bits"""

    def __init__(self, w, ll, dl):
        self.w, self.ll, self.dl, self.lc, self.dcodes = w, ll, dl, canon(ll), canon(dl)

    def sym(self, s):
        self.w.code(self.lc[s], self.ll[s])
        return self

    def lits(self, data):
        for b in data:
            self.sym(b)
        return self

    def dsym(self, s):
        self.w.code(self.dcodes[s], self.dl[s])
        return self

    def match(self, n, d):
        s, k, v = len_sym(n)
        self.sym(s).w.bits(v, k)
        s, k, v = dist_sym(d)
        self.dsym(s).w.bits(v, k)
        return self

    def end(self):
        return self.sym(256)


def fixed(w, final=1):
    w.bits(final, 1).bits(1, 2)
    return Block(w, FIXED_LL, FIXED_D)


def lens_of(n, given):
    out = [0] * n
    for s, k in given.items():
        out[s] = k
    return out


CL_PLAIN = [4] * 16 + [0, 0, 0]  # the lengths 0 .. 15 as four bits each, no repeats


def dynamic(w, ll, dl, cl=CL_PLAIN, items=None, hlit=None, hdist=None, final=1):
    """the header of a dynamic block: ll / dl are the code lengths (as many as HLIT / HDIST say), items the symbols of the
    code-length alphabet to write for them, (symbol, extra value); the default writes every length as itself"""
    w.bits(final, 1).bits(2, 2).bits(len(ll) - 257 if hlit is None else hlit, 5).bits(len(dl) - 1 if hdist is None else hdist, 5).bits(15, 4)
    for s in ORDER:
        w.bits(cl[s], 3)
    cc = canon(cl)
    for s, extra in (items if items is not None else [(n, 0) for n in ll + dl]):
        w.code(cc[s], cl[s])
        if s >= 16:
            w.bits(extra, (2, 3, 7)[s - 16])
    return Block(w, ll, dl)


def hand_made():
    """[(name, member, status the rule gives it)]; the trailer is that of `data` where the stream is good"""
    out = []

    def add(name, w, data=b"abcd", status=OK, **kw):
        out.append((name, member_of(w if isinstance(w, bytes) else w.done(), data, **kw), status))
    A = ord("a")
    ll3 = lens_of(258, {A: 2, 256: 2, 257: 1})  # a, end of block, length 3: complete
    w = Bits(); fixed(w).lits(b"a").match(3, 2).end(); add("distance 2 after one byte", w, status=BAD_DISTANCE)
    w = Bits(); fixed(w).lits(b"a").match(3, 1).end(); add("distance 1 / length 3 after one byte", w, b"aaaa")
    w = Bits(); fixed(w).lits(b"a").sym(286).end(); add("symbol 286", w, status=BAD_SYMBOL)
    w = Bits(); b = fixed(w).lits(b"abcd"); b.sym(257).dsym(30).end(); add("distance code 30", w, status=BAD_SYMBOL)
    add("block type 3", Bits().bits(1, 1).bits(3, 2).bits(0, 13), status=BAD_TYPE)
    add("bad NLEN", b"\x01\x04\x00\xfa\xff" + b"abcd", status=BAD_STORED)
    w = Bits(); fixed(w).lits(b"abcd" * 5).end(); add("a fixed stream cut short", w.done()[:-1], b"abcd" * 5, status=TRUNCATED)
    add("a stored block cut short", stored(b"abcdefgh")[:-1], b"abcdefgh", status=TRUNCATED)
    w = Bits(); fixed(w).lits(b"x" * 300).match(258, 301).end(); add("distance too far by exactly one", w, status=BAD_DISTANCE)
    w = Bits(); fixed(w).lits(b"x" * 300).match(258, 300).end(); add("distance exactly as far as the block reaches", w, b"x" * 558)
    w = Bits(); fixed(w, 0).lits(b"ab").end(); w.bits(0, 3); w.bits(0, (8 - w.n) % 8).bits(0, 16).bits(0xFFFF, 16)
    fixed(w).lits(b"cd").end(); add("fixed, an empty stored block, fixed", w)
    # dynamic headers: each of the three alphabets over-subscribed and incomplete
    w = Bits(); dynamic(w, lens_of(257, {A: 1, A + 1: 1, 256: 1}), [1]); add("literal/length set over-subscribed", w, status=BAD_LENGTHS)
    w = Bits(); dynamic(w, lens_of(257, {A: 2, 256: 2}), [1]); add("literal/length set incomplete", w, status=BAD_LENGTHS)
    w = Bits(); dynamic(w, lens_of(257, {A: 1, 256: 1}), [1, 1, 1]); add("distance set over-subscribed", w, status=BAD_LENGTHS)
    w = Bits(); dynamic(w, lens_of(257, {A: 1, 256: 1}), [2, 2]); add("distance set incomplete", w, status=BAD_LENGTHS)
    w = Bits(); dynamic(w, lens_of(257, {A: 1, 256: 1}), [1], cl=[4] * 19, items=[]); add("code-length set over-subscribed", w, status=BAD_LENGTHS)
    w = Bits(); dynamic(w, lens_of(257, {A: 1, 256: 1}), [1], cl=[1] + [0] * 18, items=[]); add("code-length set incomplete", w, status=BAD_LENGTHS)
    w = Bits(); dynamic(w, lens_of(257, {A: 1, 256: 1}), [1], cl=[0] * 19, items=[]); add("code-length set empty", w, status=BAD_LENGTHS)
    w = Bits(); dynamic(w, lens_of(257, {A: 1, A + 1: 1}), [1]).lits(b"ab"); add("no code for 256", w, status=BAD_LENGTHS)
    w = Bits(); dynamic(w, lens_of(257, {A: 1, 256: 1}), [1], hlit=30, items=[]); w.bits(0, 64); add("HLIT 287", w, status=BAD_LENGTHS)
    w = Bits(); dynamic(w, lens_of(257, {A: 1, 256: 1}), [1], hdist=30, items=[]); w.bits(0, 64); add("HDIST 31", w, status=BAD_LENGTHS)
    rep = [4] * 14 + [0, 0, 4, 0, 4]  # 0 .. 13, 16 and 18 as four bits each: complete
    w = Bits(); dynamic(w, lens_of(257, {A: 1, 256: 1}), [1], cl=rep, items=[(16, 0)]); w.bits(0, 64); add("a repeat with nothing before it", w, status=BAD_LENGTHS)
    w = Bits(); dynamic(w, lens_of(257, {A: 1, 256: 1}), [1], cl=rep, items=[(18, 127), (18, 127 - 11)]); w.bits(0, 64)
    add("a repeat across the end", w, status=BAD_LENGTHS)  # 138 + 127 = 265 > 257 + 1
    items = [(18, 97 - 11), (1, 0), (18, 138 - 11), (18, 256 - 98 - 138 - 11), (1, 0), (1, 0)]  # 97 zeros, a, 158 zeros, 256, one distance code
    w = Bits(); dynamic(w, lens_of(257, {A: 1, 256: 1}), [1], cl=rep, items=items).lits(b"aaaa").end(); add("lengths written with repeats", w, b"aaaa")
    # one distance code (an incomplete set that is legal) and none at all
    w = Bits(); dynamic(w, ll3, [1]).lits(b"a").sym(257).dsym(0).end(); add("a single-code distance set", w, b"aaaa")
    w = Bits(); b = dynamic(w, ll3, [1]).lits(b"a").sym(257); w.bits(1, 1); b.end(); add("the unassigned code of a one-code distance set", w, status=BAD_SYMBOL)
    w = Bits(); dynamic(w, ll3, [0]).lits(b"aaaa").end(); add("no distance code, literals only", w, b"aaaa")
    w = Bits(); b = dynamic(w, ll3, [0]).lits(b"a").sym(257); w.bits(0, 1); b.end(); add("a length symbol with no distance codes", w, status=BAD_SYMBOL)
    w = Bits(); dynamic(w, lens_of(257, {256: 1}), [0]).end(); add("a single-code literal/length set", w, b"")
    w = Bits(); dynamic(w, lens_of(257, {256: 1}), [0]); w.bits(1, 1); add("the unassigned code of a one-code literal/length set", w, b"", status=BAD_SYMBOL)
    # long codes: the second level of both tables (15-bit literal codes, 12-bit distance codes)
    ll = [15] * 256 + [0] * 30
    for s, k in ((256, 1), (257, 2), (285, 3), (258, 4), (259, 5), (260, 6), (261, 7)):
        ll[s] = k  # 1/2 + 1/4 + 1/8 + 1/16 + 1/32 + 1/64 + 1/128 + 256 / 32768 = 1
    dl = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 12] + [0] * 17
    data = bytes(range(256)) + bytes(range(255, -1, -1))
    w = Bits(); b = dynamic(w, ll, dl).lits(data).match(258, 96).match(3, 1).match(4, 65).match(5, 49).end()
    want = bytearray(data)
    for n, d in ((258, 96), (3, 1), (4, 65), (5, 49)):
        for _ in range(n):
            want.append(want[-d])
    add("15-bit literal codes and 12-bit distance codes", w, bytes(want))
    # the trailer and the stream's end
    good = deflate(dc.TEXT * 3)
    add("one byte short", good[:-1], dc.TEXT * 3, status=TRUNCATED)
    add("one spare byte", good + b"\x00", dc.TEXT * 3, status=TRAILING)
    add("ISIZE one too large", good, dc.TEXT * 3, status=SIZE, isize=3 * len(dc.TEXT) + 1)
    add("ISIZE one too small", good, dc.TEXT * 3, status=SIZE, isize=3 * len(dc.TEXT) - 1)
    add("ISIZE 0 for one byte", deflate(b"a"), b"a", status=SIZE, isize=0)
    add("one flipped CRC bit", good, dc.TEXT * 3, status=CRC, crc=zlib.crc32(dc.TEXT * 3) ^ 0x00100000)
    return out


# ---- good files -------------------------------------------------------------------------------------------------------------
def fake_header(bsize1):
    return HEAD + struct.pack("<H", bsize1 - 1)


def good_members():
    """[(name, member, payload)]"""
    rng = np.random.default_rng(412)
    body = dc.bam_like()
    named = dc.payloads() + [("BAM-like %d" % i, body[a:a + P]) for i, a in enumerate(range(0, len(body), P))]
    out = []
    for level in (0, 1, 6, 9):
        out += [("%s, level %d" % (name, level), member(d, level), d) for name, d in named]
    pick = [d for name, d in named if name in ("text 65280", "random 259", "period 258", "period 32768", "zeros 65280", "BAM-like 1", "fibonacci counts")]
    for mem in (1, 8):
        for sname, strategy in (("default", zlib.Z_DEFAULT_STRATEGY), ("fixed", zlib.Z_FIXED), ("huffman only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
            out += [("memLevel %d, %s, %d bytes" % (mem, sname, len(d)), member(d, 6, mem, strategy), d) for d in pick]
    text = dc.text_of(rng, 5000)
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = z.compress(text[:1234]) + z.flush(zlib.Z_SYNC_FLUSH) + z.compress(text[1234:3000]) + z.flush(zlib.Z_SYNC_FLUSH) + z.compress(text[3000:]) + z.flush()
    assert raw.count(b"\x00\x00\xff\xff") >= 2
    out.append(("Z_SYNC_FLUSH in the middle", member_of(raw, text), text))
    big = dc.text_of(rng, 65536)
    out.append(("65 536 bytes in one member", member(big, 6), big))
    out.append(("an empty payload, zlib", member(b"", 6), b""))
    out.append(("the end-of-file block", EOF_BLOCK, b""))
    # fake headers inside stored payloads: one alone; one whose BSIZE leads to a second, whose BSIZE leads to the member's end
    # with the member's own ISIZE (<= 65 536) in front of it: a chain of candidates that joins the real one
    lone = dc.rand(rng, 700) + fake_header(5000) + dc.rand(rng, 9000)
    out.append(("a fake header in a stored payload", member_of(stored(lone), lone), lone))
    tail = dc.rand(rng, 300)
    second = fake_header(18 + len(tail) + 8) + tail  # ends with the payload; CRC-32 and ISIZE follow: it runs to the member's end
    gap = dc.rand(rng, 1000) + bytes(4)  # four zero bytes: an ISIZE of 0 for the first fake
    first = fake_header(18 + len(gap))
    linked = dc.rand(rng, 333) + first + gap + second
    out.append(("two linked fake headers in a stored payload", member_of(stored(linked), linked), linked))
    for name, m, d in out:
        assert len(m) <= 65536 and struct.unpack_from("<H", m, 16)[0] + 1 == len(m), name
    return out


def empty_member_file():
    """[(name, member, payload)] of ONE file with ISIZE 0 members in front, in the middle and at the end: candidate 0 is empty with
    real blocks behind it, and every zero-length output range shares its address with a neighbour's"""
    rng = np.random.default_rng(28)
    text, stored_empty = dc.text_of(rng, 7000), member_of(stored(b""), b"")  # (zlib's own empty member is the end-of-file block)
    real = [("text %d, level %d" % (n, level), member(text[:n], level), text[:n]) for n, level in ((1, 0), (300, 6), (7000, 9), (259, 1), (4000, 6))]
    eof, empty = ("the end-of-file block", EOF_BLOCK, b""), ("an empty payload, stored", stored_empty, b"")
    return [eof, empty] + real[:2] + [empty, eof, empty] + real[2:] + [empty, eof]


def bad_files():
    """[(name, file, status of bg_bgzf_blocks, first_bad)] for the walk, each behind two good members"""
    a, b = member(dc.TEXT * 20, 6), member(dc.TEXT * 7, 1)
    two = HEAD[:10] + struct.pack("<H", 12) + b"BC\x02\x00" + struct.pack("<H", 18 + 6 + 2 + 8 - 1) + b"XY\x02\x00\x00\x00" + b"\x03\x00" + bytes(8)
    short = HEAD + struct.pack("<H", 26) + b"\x03" + bytes(8)
    big = member_of(deflate(b"abc"), b"abc", isize=65537)
    return [("trailing garbage", a + b + b"garbage", INVALID_ARG, 2), ("a last member cut short", a + b + a[:-1], INVALID_ARG, 2),
            ("a last member cut inside its header", a + b + a[:11], INVALID_ARG, 2), ("BSIZE + 1 = 27", a + b + short + a, INVALID_ARG, 2),
            ("XLEN = 12 with a second subfield", a + b + two + a, UNSUPPORTED, 2), ("ISIZE 65 537", a + b + big + a, INVALID_ARG, 2),
            ("FLG 0: plain gzip", a + b + b"\x1f\x8b\x08\x00" + a[4:], UNSUPPORTED, 2), ("no member at byte 0", b"\x00" + a + b, INVALID_ARG, 0),
            ("an empty file", b"", 0, NONE), ("the end-of-file block alone", EOF_BLOCK, 0, NONE)]


def corruptions(n=2000, seed=2026):
    """n members, each a good member with one byte behind its header changed at a seeded random place"""
    rng = np.random.default_rng(seed)
    text, body = dc.text_of(rng, 3000), dc.bam_like(12)
    base = [member(text, 1), member(text, 6), member(text, 9), member(text, 6, 1), member(text, 6, 8, zlib.Z_FIXED), member(text, 6, 8, zlib.Z_HUFFMAN_ONLY),
            member(text, 6, 8, zlib.Z_RLE), member(text[:900], 0), member(body, 6), member(body, 9, 1), member(bytes(2000), 9), member(b"ACGT" * 700, 6)]
    out = []
    for k in range(n):
        m = bytearray(base[k % len(base)])
        at = int(rng.integers(18, len(m)))
        m[at] ^= int(rng.integers(1, 256))
        out.append(bytes(m))
    return out


def range_of(m):
    """the output range a table gives a (possibly corrupted) member: its ISIZE, as far as the call admits one"""
    return min(struct.unpack("<I", m[-4:])[0], 65536)


# ---- the program ------------------------------------------------------------------------------------------------------------
def build_program(exe, sanitize):
    """the program of bgzf_inflate_host_bodies.cpp, built as bgzf_deflate_cases.build_program builds its own"""
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + _lib.CSRC] + flags + [os.path.join(ROOT, "tests", "bgzf_inflate_host_bodies.cpp"), "-o", exe])
    return exe


def run_program(exe, tmp, files, members):
    """files: [bytes]; members: [(bytes, output range)] -> ([(status, n_blocks, out_bytes, first_bad, block_off, out_off, statuses,
    lowest bad block, payload)], [(status, bytes of the range)]); a file the walk refuses has None from block_off on"""
    inp, outp = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<2Q", len(files), len(members)))
        for d in files:
            f.write(struct.pack("<Q", len(d)) + d)
        for m, isize in members:
            f.write(struct.pack("<2Q", len(m), isize) + m)
    subprocess.check_call([exe, inp, outp])
    raw = open(outp, "rb").read()
    at, got_files, got_members = 0, [], []
    for _ in files:
        rc, n, total, bad = struct.unpack_from("<q3Q", raw, at)
        at += 32
        if rc:
            got_files.append((rc, n, total, bad, None, None, None, None, None))
            continue
        rows = np.frombuffer(raw, np.uint64, 2 * (n + 1), at).reshape(-1, 2)
        at += 16 * (n + 1)
        statuses = list(raw[at:at + n])
        first_bad = struct.unpack_from("<Q", raw, at + n)[0]
        at += n + 8
        got_files.append((rc, n, total, bad, rows[:, 0].tolist(), rows[:, 1].tolist(), statuses, first_bad, raw[at:at + total]))
        at += total
    for _, isize in members:
        got_members.append((struct.unpack_from("<I", raw, at)[0], raw[at + 4:at + 4 + isize]))
        at += 4 + isize
    assert at == len(raw)
    return got_files, got_members

"""Payloads for the deflate tests (tests/test_bgzf_deflate_host_bodies.py, tests/test_gpu_bgzf_deflate.py), the stand-alone
program that runs the kernel's bodies on the CPU (tests/bgzf_deflate_host_bodies.cpp), and the checks every block must pass."""
import os
import struct
import subprocess
import zlib

import numpy as np

from rust_bio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 65280
LENGTHS = (1, 2, 3, 4, 257, 258, 259, P - 1, P)
PERIODS = (1, 2, 3, 4, 258, 32768, 32769)
FIB = (1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946, 17711)
TEXT = (b"It was the best of times, it was the worst of times, it was the age of wisdom, it was the age of foolishness, it was the "
        b"epoch of belief, it was the epoch of incredulity, it was the season of Light, it was the season of Darkness.\n")


def rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def text_of(rng, n):
    """ASCII text: the sentence above from changing starts, so that matches have every length and distance"""
    out = bytearray()
    while len(out) < n:
        a = int(rng.integers(0, len(TEXT) - 1))
        out += TEXT[a:a + int(rng.integers(1, len(TEXT)))] + b"%d " % int(rng.integers(0, 10**6))
    return bytes(out[:n])


def payloads():
    """[(name, bytes)], each 1 .. 65 280 bytes: one block"""
    rng = np.random.default_rng(20260)
    out = []
    for n in LENGTHS:
        out += [("zeros %d" % n, bytes(n)), ("random %d" % n, rand(rng, n)), ("text %d" % n, text_of(rng, n))]
    for period in PERIODS:  # 32 769: every candidate lies one byte beyond the window
        unit = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), period))
        out.append(("period %d" % period, (unit * (P // period + 1))[:P]))
    seg = text_of(rng, 3000)
    for gap in (31000, 40000):
        out.append(("segment, %d random, segment" % gap, seg + rand(rng, gap) + seg))
    out.append(("last match ends on the last byte", rand(rng, 700) + seg[:100] + rand(rng, 50) + seg[:100]))
    out.append(("one 258-run ending on the last byte", rand(rng, 300) + b"Q" * 259))
    out += [("one symbol, length 1", b"a"), ("one symbol, length 2", b"aa"), ("two symbols", b"ab" * 40 + b"a")]
    # every match length: an L-gram, a separator, the L-gram again (in two payloads: together they exceed one)
    for name, ls in (("match lengths 3 .. 180", range(3, 181)), ("match lengths 181 .. 258", range(181, 259))):
        buf = bytearray()
        for L in ls:
            gram = rand(rng, L)
            buf += gram + b"|" + gram
        assert len(buf) <= P
        out.append((name, bytes(buf)))
    out.append(("fibonacci counts", fibonacci_payload()))
    assert all(1 <= len(d) <= P for _, d in out)
    return out


def fibonacci_payload():
    """22 symbols with the counts 1, 1, 2, 3, .., 17 711 (46 367 bytes), shuffled: an unlimited Huffman tree is 21 deep"""
    data = np.concatenate([np.full(c, 65 + i, np.uint8) for i, c in enumerate(FIB)])
    np.random.default_rng(7).shuffle(data)
    assert len(data) == 46367
    return data.tobytes()


def limiter_cases():
    """[(counts, limit)] for dfl_huff_lengths called directly"""
    return [(list(FIB), 15), ([1, 1, 2, 3, 5, 8, 13, 21, 34], 7), ([0, 0, 9, 0], 15), ([0, 0, 9, 0], 7), ([5] * 19, 7), ([1] * 286, 15),
            ([3, 0, 3], 7), ([1, 1, 2, 3, 5, 8, 13, 21, 34, 0, 0, 55, 89, 144, 233, 377, 610, 987, 1597], 7)]


def bam_like(n_records=700, seed=11):
    """Records like a coordinate-sorted BAM body: the 36 fixed bytes with ascending positions, names that share a prefix, 150
    random bases 4 bits each, qualities from a skewed distribution capped at 40, AS / XS / NM / MD tags."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    pos = 10_000
    codes = np.array([1, 2, 4, 8], np.uint8)
    for r in range(n_records):
        pos += int(rng.integers(1, 400))
        name = b"HWI-ST1234:77:C0ABCACXX:3:%d:%d:%d\0" % (1101 + r // 97, int(rng.integers(1000, 20000)), int(rng.integers(1000, 99999)))
        cigar = struct.pack("<I", 150 << 4)
        b = rng.choice(codes, 150)
        seq = ((b[0::2] << 4) | b[1::2]).astype(np.uint8).tobytes()
        qual = np.minimum(40, 41 - np.minimum(rng.geometric(0.25, 150), 39)).astype(np.uint8).tobytes()
        nm = int(rng.integers(0, 4))
        md = b"%d%s%d" % (int(rng.integers(0, 75)), b"ACGT"[nm:nm + 1], int(rng.integers(0, 75))) if nm else b"150"
        tags = b"ASC" + bytes([150 - 5 * nm]) + b"XSC" + bytes([int(rng.integers(0, 100))]) + b"NMC" + bytes([nm]) + b"MDZ" + md + b"\0"
        flag = (99, 147, 83, 163)[int(rng.integers(0, 4))]
        body = struct.pack("<iiBBHHHIiii", 0, pos, len(name), int(rng.integers(0, 61)), 4681 + (pos >> 14), 1, flag, 150, 0,
                           pos + int(rng.integers(-300, 300)), int(rng.integers(-500, 500))) + name + cigar + seq + qual + tags
        out += struct.pack("<I", len(body)) + body
    return bytes(out)


def build_program(exe, sanitize):
    """the program of bgzf_deflate_host_bodies.cpp, built as tests/test_bam_host_bodies.py builds its own"""
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + _lib.CSRC] + flags + [os.path.join(ROOT, "tests", "bgzf_deflate_host_bodies.cpp"), "-o", exe])
    return exe


def run_program(exe, tmp, cases, datas):
    """-> ([code lengths of a case], [(block, encoding, (stored, fixed, dynamic) bits) of a payload])"""
    inp, outp = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<2Q", len(cases), len(datas)))
        for counts, limit in cases:
            f.write(struct.pack("<2Q", len(counts), limit) + struct.pack("<%dI" % len(counts), *counts))
        for d in datas:
            f.write(struct.pack("<Q", len(d)) + d)
    subprocess.check_call([exe, inp, outp])
    raw = open(outp, "rb").read()
    at = 0
    lens, blocks = [], []
    for counts, _ in cases:
        lens.append(list(raw[at:at + len(counts)]))
        at += len(counts)
    for _ in datas:
        total, mode, c0, c1, c2 = struct.unpack_from("<5I", raw, at)
        blocks.append((raw[at + 20:at + 20 + total], mode, (c0, c1, c2)))
        at += 20 + total
    assert at == len(raw)
    return lens, blocks


def check_block(block, data, name=""):
    """header bytes and BSIZE, a raw deflate stream that inflates to exactly the payload and ends, the trailer, the size bound"""
    assert len(block) <= len(data) + 31, name
    assert block[:16] == bytes.fromhex("1f8b08040000000000ff060042430200"), name
    assert struct.unpack_from("<H", block, 16)[0] == len(block) - 1, name
    z = zlib.decompressobj(-15)
    assert z.decompress(block[18:]) == data and z.eof, name
    assert z.unused_data == struct.pack("<II", zlib.crc32(data), len(data)), name


def split_blocks(stream):
    """the blocks of a BGZF stream, found by walking BSIZE"""
    out, at = [], 0
    while at < len(stream):
        n = struct.unpack_from("<H", stream, at + 16)[0] + 1
        out.append(stream[at:at + n])
        at += n
    assert at == len(stream)
    return out

"""The `__host__ __device__` bodies behind bg_bam_emit_batch and bg_bgzf_frame (csrc/bam_rule.h: the bin, the base codes, integer
tags in their smallest type — the size the length pass counts against the bytes the writer puts —, and a BGZF block as the 256
lanes of the kernel make it: the table, every lane's destination-aligned copy with its CRC share, the combination) run on the
CPU by a stand-alone program (tests/bam_host_bodies.cpp) built with AddressSanitizer and UBSan, against tests/bam_oracle.py byte
for byte.  Payloads of 0, 1, 3, 4, 5, 255, 256, 65 279 and 65 280 bytes (and a few between), each an exact-size buffer at
several residues of source and destination, so a byte loaded or stored outside one stops the program.  Nothing is loaded into
Python."""
import os
import struct
import subprocess

import numpy as np

import bam_oracle as bo
from rust_bio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 33, 255, 256, 257, 4095, 4112, 65279, 65280)
RESIDUES = ((0, 0), (7, 7), (7, 0), (0, 9), (15, 1), (1, 15), (8, 12))  # (destination, source): 23 mod 16 is 7
EDGES = (0, 1, 2**14 - 1, 2**14, 2**17 - 1, 2**17, 2**20, 2**23, 2**26 - 1, 2**26, 2**29 - 1, 2**29, 2**31 - 2)
INTS = (-2**31, -32769, -32768, -129, -128, -1, 0, 1, 127, 128, 255, 256, 65535, 65536, 2**31 - 1, 2**32 - 1)


def test_bam_bodies_on_the_host_under_sanitizers(tmp_path):
    exe, inp, outp = str(tmp_path / "bodies"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + _lib.CSRC, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "bam_host_bodies.cpp"), "-o", exe])
    rng = np.random.default_rng(77)
    bins = [(-1, 0), (-1, 5)] + [(p, r) for p in EDGES for r in (0, 1, 2, 150, 2**14, 2**26 + 1) if p + r <= 2**31 - 1]
    bases = bytes(range(256))
    payloads = []
    for n in LENGTHS:
        for j, (r_dst, r_src) in enumerate(RESIDUES):
            data = bytes(n) if (n + j) % 5 == 0 else rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            payloads.append((n, r_dst, r_src, data))
    with open(inp, "wb") as f:
        f.write(struct.pack("<4Q", len(bins), len(bases), len(INTS), len(payloads)))
        for pos, ref_len in bins:
            f.write(struct.pack("<qQ", pos, ref_len))
        f.write(bases + struct.pack("<%dq" % len(INTS), *INTS))
        for n, r_dst, r_src, data in payloads:
            f.write(struct.pack("<3Q", n, r_dst, r_src) + data)
    subprocess.check_call([exe, inp, outp])
    raw = open(outp, "rb").read()
    at = 0

    def take(n):
        nonlocal at
        at += n
        return raw[at - n:at]
    for pos, ref_len in bins:
        assert struct.unpack("<H", take(2))[0] == bo.reg2bin(pos, pos + (ref_len or 1)) & 0xFFFF, (pos, ref_len)
    want = bytes(bo.BASES.index(bytes([b]).upper()) if bytes([b]).upper() in bo.BASES else 15 for b in bases)
    assert take(256) == want
    for v in INTS:
        code, fmt = bo.int_tag(v)
        w = b"XY" + code + struct.pack(fmt, v)
        assert take(len(w)) == w, v
    for n, r_dst, r_src, data in payloads:
        w = bo.block(data)
        assert take(len(w)) == w, (n, r_dst, r_src)
    assert take(28) == bo.EOF_BLOCK and at == len(raw)

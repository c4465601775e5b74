"""The `__host__ __device__` bodies behind bg_bam_index (csrc/bam_index_rule.h: a record's fields decoded byte by byte, the
CIGAR walk, the checks, the virtual offset with a block table and in closed form, the sizes and places of a reference's pieces,
the stores, the window search) run on the CPU by a stand-alone program (tests/bam_index_host_bodies.cpp) built with
AddressSanitizer and UBSan, in the order of the kernels' passes, against tests/bai_oracle.py byte for byte.  Every shape and
every error of tests/bai_cases.py, the records at odd addresses in exact-size allocations, the index in an allocation of the size
the sizing pass gives.  Nothing is loaded into Python."""
import os
import struct
import subprocess

import numpy as np

import bai_cases as bc
import bai_oracle as ba
import bam_oracle as bo
from rust_bio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATUS = {0: 0, 1: bc.INVALID_ARG, 2: bc.UNSUPPORTED}


def fake_table(total, rng):
    """a block table as bg_bgzf_deflate could give it: blocks of 100 .. 65 311 bytes"""
    sizes = rng.integers(100, bo.PAYLOAD + 32, (total + bo.PAYLOAD - 1) // bo.PAYLOAD)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def test_bam_index_bodies_on_the_host_under_sanitizers(tmp_path):
    exe, inp, outp = str(tmp_path / "bodies"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + _lib.CSRC, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "bam_index_host_bodies.cpp"), "-o", exe])
    rng = np.random.default_rng(5)
    cases = []  # (name, slots, contigs, block table or None, base, residue, status, first_bad)
    for k, (name, (slots, contigs)) in enumerate(bc.shapes().items()):
        total = sum(len(s) for s in slots)
        cases.append((name, slots, contigs, None, 0, 1, 0, None))
        cases.append((name, slots, contigs, None, 4321 + k, 7, 0, None))
        cases.append((name, slots, contigs, fake_table(total, rng), (1 << 40) + k, 2 * k % 16 + 1, 0, None))
    for name, slots, contigs, status, first_bad in bc.errors():
        cases.append((name, slots, contigs, None, 0, 3, status, first_bad))
    with open(inp, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for name, slots, contigs, table, base, res, _, _ in cases:
            f.write(struct.pack("<Q", len(contigs)) + b"".join(struct.pack("<QQQII", start, ln, 0, len(nm), 0) for nm, start, ln in contigs))
            f.write(struct.pack("<Q", len(slots)) + bo.offsets(slots).tobytes())
            f.write(struct.pack("<Q", 0 if table is None else len(table)) + (b"" if table is None else table.tobytes()))
            f.write(struct.pack("<QQ", base, res) + b"".join(slots))
    subprocess.check_call([exe, inp, outp])
    raw = open(outp, "rb").read()
    at = 0
    for name, slots, contigs, table, base, res, status, first_bad in cases:
        got_status, got_bad, n = struct.unpack_from("<qQQ", raw, at)
        got = raw[at + 24:at + 24 + n]
        at += 24 + n
        assert STATUS[got_status] == status, name
        if status:
            assert (got_bad, n) == (first_bad, 0), name
            continue
        assert got_bad == 2**64 - 1
        want = ba.build(slots, contigs, ba.stored_voff(base) if table is None else ba.table_voff(table, base))
        assert got == want, (name, base, res)
    assert at == len(raw)

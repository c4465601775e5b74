"""The carver behind every `*_dev` entry point's device scratch (csrc/bg_carve.h) run on the CPU by a stand-alone program
(tests/scratch_carve_host.cpp) built by the host compiler with AddressSanitizer and UBSan.  The program includes the carver's
header alone (no HIP).  Lists of pieces of 0, 1, 255, 256 and 257 elements of 1-, 4-, 8- and 40-byte types, with empty pieces
first, last and next to each other: the measured total is where the bound run ends, every piece starts a multiple of 256 bytes
from the base, the pieces are disjoint and inside the reservation, an empty piece has an address inside it, measuring returns
null only, and every piece of a list bound to an allocation of exactly the measured bytes is filled to its last byte.  Nothing is
loaded into Python."""
import os
import subprocess

from rust_bio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scratch_carve_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "carve")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I" + _lib.CSRC,
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "scratch_carve_host.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("scratch carve ok"), out.stdout[-4000:]

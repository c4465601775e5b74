"""The per-record bodies of the demultiplexing kernels (csrc/fastq_demux_rule.h: the per-lane share of the assign reduction,
the state merge, the verdict, the pair rule, the in-tile stable rank, and the record copy of csrc/fastq_emit_rule.h;
`__host__ __device__`) run on the CPU by a stand-alone program (tests/fastq_demux_host_bodies.cpp) built with AddressSanitizer
and UBSan, on seeded random batches against the restatement (tests/fastq_demux_oracle.py), byte for byte.  Every buffer has
exactly its size: a byte loaded or stored outside one stops the program.  n_pat 1, 3, 16, 17, 40; n_bins 1, 2, 5; group widths 1
and 16; every legal flag combination; two batches span more than one tile of the split."""
import os
import random
import subprocess

import numpy as np

import fastq_demux_oracle as dm
from fastq_demux_cases import LEGAL_FLAGS, random_hits, random_pat_bin
from fastq_write_cases import Batch, random_records
from rust_bio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_demux_bodies_on_the_host_under_sanitizers(tmp_path):
    exe, inp, outp = str(tmp_path / "bodies"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"),
                           "-I" + _lib.CSRC, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "fastq_demux_host_bodies.cpp"), "-o", exe])
    rng = random.Random(11)
    seen = {"assigned": 0, "unassigned": 0, "ambiguous": 0}
    rounds = [(n_pat, n_bins, G) for n_pat in (1, 3, 16, 17, 40) for n_bins in (1, 2, 5) for G in (1, 16)]
    for rnd, (n_pat, n_bins, G) in enumerate(rounds):
        flags = LEGAL_FLAGS[rnd % len(LEGAL_FLAGS)]  # 30 rounds: each of the 15 twice, once per group width
        n = 2 * rng.randint(1, 30) if rnd not in (7, 20) else 2 * rng.randint(1100, 2200)  # ... two of them over several tiles
        a_seq, a_qual = (rnd * 7 + 3) % 16, (rnd * 5 + 1) % 16
        b = Batch(random_records(rng, n, 0, 12 if n > 100 else 40), a_seq=a_seq, a_qual=a_qual)
        hits = random_hits(rng, n, n_pat, p_hit=min(0.5, 1.5 / n_pat))
        pat_bin = random_pat_bin(rng, n_pat, n_bins)
        prm = dict(flags=flags, min_margin=rng.choice([0, 1, 2]), max_offset=rng.choice([0, 2, 3]))
        w_bin, w_hit, w_pat = dm.assign(hits, n_pat, pat_bin, n_bins, **prm)
        # the split gets assign's bins with a few values above n_bins + 1 thrown in
        split_bin = w_bin.copy()
        for r in rng.sample(range(n), max(1, n // 10)):
            split_bin[r] = rng.choice([n_bins + 2, 0xFFFFFFFF, rng.randrange(n_bins + 2)])
        with open(inp, "wb") as f:
            f.write(np.array([n, n_pat, n_bins, G, prm["flags"], prm["min_margin"], prm["max_offset"], a_seq, a_qual, len(b.seq) - a_seq,
                              len(b.qual) - a_qual], dtype=np.uint32).tobytes())
            f.write(pat_bin.tobytes() + hits.tobytes() + split_bin.tobytes() + b.recs.tobytes() + b.seq + b.qual + b.seq_off.tobytes() +
                    b.qual_off.tobytes())
        subprocess.check_call([exe, inp, outp])
        raw = open(outp, "rb").read()
        o = 0

        def take(dtype, count):
            nonlocal o
            a = np.frombuffer(raw, dtype, count, o)
            o += a.nbytes
            return a

        assert (take(np.uint32, n) == w_bin).all(), (rnd, "bin")
        assert take(_lib.ALN_DTYPE, n).tobytes() == w_hit.tobytes(), (rnd, "hit_out")
        assert (take(np.uint32, n) == w_pat).all(), (rnd, "pat_out")
        s_recs, s_seq, s_so, s_qual, s_qo, s_hit, s_perm, s_boff = dm.split(split_bin, n_bins, *b.columns(), hit=w_hit)
        assert take(_lib.FQREC_DTYPE, n).tobytes() == s_recs.tobytes(), (rnd, "recs")
        assert (take(np.uint64, n + 1) == s_so).all() and (take(np.uint64, n + 1) == s_qo).all(), rnd
        assert take(np.uint8, len(s_seq)).tobytes() == s_seq and take(np.uint8, len(s_qual)).tobytes() == s_qual, rnd
        assert take(_lib.ALN_DTYPE, n).tobytes() == s_hit.tobytes(), (rnd, "split hit_out")
        assert (take(np.uint64, n) == s_perm).all(), (rnd, "perm")
        assert (take(np.uint64, n_bins + 3) == s_boff).all() and o == len(raw), rnd
        seen["assigned"] += int((w_bin < n_bins).sum())
        seen["unassigned"] += int((w_bin == n_bins).sum())
        seen["ambiguous"] += int((w_bin == n_bins + 1).sum())
    assert min(seen.values()) > 50, seen

"""bg_bam_records[_dev] on the GPU: the corpus of tests/bam_read_cases.py (what tests/test_bam_read_host_bodies.py holds the CPU
run of the same bodies to) against the Python walk of tests/bam_read_oracle.py, plus what only the kernels have: record starts at
every residue of the 2 048-position chunks, the 36 fixed bytes across a chunk boundary, a record longer than two chunks, two
accepted positions 4 bytes apart inside one thread's 8 positions, across two threads and across two chunks, d_bam at every
offset 0 .. 15 between intact guards, refusals and too small a cap that leave the table unwritten, the sizing call."""
import numpy as np
import pytest
import torch

import bam_read_cases as rc
import bam_read_oracle as ro
from dev_shift import guards_intact, shifted_from
from rust_bio_amd import _lib, bam

pytestmark = pytest.mark.gpu
CHUNK = 2048


def stream():
    return torch.cuda.current_stream().cuda_stream


def table_dev(s, n_ref, residue=0, body=rc.BODY):
    """-> (off, n_candidates) of bg_bam_records_dev: the sizing call, then the table between two untouched entries"""
    d = shifted_from(s, residue)
    n, cand = bam.records_dev(d.data_ptr(), len(s), body, n_ref, stream=stream())
    d_off = torch.full((n + 3,), -1, dtype=torch.int64, device="cuda")
    assert bam.records_dev(d.data_ptr(), len(s), body, n_ref, d_off[1:].data_ptr(), n, stream=stream()) == (n, cand)
    assert int(d_off[0]) == -1 and int(d_off[n + 2]) == -1 and guards_intact(d)
    return d_off[1:n + 2].cpu().numpy().astype(np.uint64).tolist(), cand


def refused_dev(s, n_ref):
    d = shifted_from(s, 3)
    d_off = torch.full((1000,), -1, dtype=torch.int64, device="cuda")
    with pytest.raises(bam.BamReadError) as e:
        bam.records_dev(d.data_ptr(), len(s), rc.BODY, n_ref, d_off.data_ptr(), 999, stream=stream())
    assert bool((d_off == -1).all()) and guards_intact(d) and e.value.status == ro.INVALID_ARG
    return e.value.record


def test_the_corpus():
    n_refused = 0
    for name, s, n_ref in rc.corpus():
        try:
            want = ro.walk(s, rc.BODY, n_ref)
        except ro.Refused as e:
            assert refused_dev(s, n_ref) == e.first_bad, name
            n_refused += 1
            continue
        off, cand = table_dev(s, n_ref, residue=len(name) % 16)
        assert off == want and cand == len(ro.candidates(s, rc.BODY, n_ref)), name
    assert n_refused == 13


def pad_to(stream_len, target):
    """records that bring a stream of stream_len bytes to exactly `target`"""
    gap = target - stream_len
    assert gap >= 41
    if gap < 82 + 37:
        return [rc.raw(b"", tags=rc.pad_tag(gap - 37))]
    return [rc.raw(b"", tags=rc.pad_tag(4))] + pad_to(stream_len + 41, target)


def test_every_residue_of_a_chunk_and_records_across_chunks():
    recs = [rc.raw(b"", tags=rc.pad_tag(8)) for _ in range(2100)]  # 45 bytes each: coprime with 2 048
    recs += [rc.seq_rec(i, 1 + i % 90, ref=i % rc.N_REF, pos=i) for i in range(2900)]
    s = rc.HEADER + b"".join(recs)
    edge = rc.BODY + ((len(s) - rc.BODY) // CHUNK + 2) * CHUNK - 20
    s += b"".join(pad_to(len(s), edge)) + rc.seq_rec(7, 30)  # its fixed bytes straddle a chunk boundary
    s += rc.seq_rec(8, 5000) + rc.seq_rec(9, 3)  # longer than two chunks
    want = ro.walk(s, rc.BODY, rc.N_REF)
    assert {(o - rc.BODY) % CHUNK for o in want} == set(range(CHUNK)) and edge in want
    off, cand = table_dev(s, rc.N_REF, residue=5)
    assert off == want and len(off) > 5000
    assert cand == len(ro.candidates(s, rc.BODY, rc.N_REF)) >= len(off) - 1


@pytest.mark.parametrize("at", [8 * 40, 8 * 40 + 6, 3 * CHUNK - 2, 3 * CHUNK - 4, 3 * CHUNK + 1])
def test_the_close_pair_inside_a_thread_across_threads_and_across_chunks(at):
    pair = rc.close_pair()
    assert pair is not None
    s = rc.HEADER + rc.seq_rec(1, 40)
    s += b"".join(pad_to(len(s), rc.BODY + at)) + pair + rc.seq_rec(2, 11)
    assert ro.verdict(s, rc.BODY + at, rc.N_REF) and ro.verdict(s, rc.BODY + at + 4, rc.N_REF)
    want = ro.walk(s, rc.BODY, rc.N_REF)
    assert rc.BODY + at in want and rc.BODY + at + 4 not in want
    off, cand = table_dev(s, rc.N_REF)
    assert off == want and cand == len(ro.candidates(s, rc.BODY, rc.N_REF)) > len(off) - 1


def test_every_alignment_of_the_stream():
    name, s, n_ref = next(c for c in rc.corpus() if c[0] == "three linked fakes in a B:C tag")
    want = ro.walk(s, rc.BODY, n_ref)
    for r in range(16):
        assert table_dev(s, n_ref, residue=r)[0] == want


def test_sizing_caps_and_arguments():
    s = rc.HEADER + b"".join(rc.seq_rec(i, 12) for i in range(6))
    d = shifted_from(s, 1)
    assert bam.records_dev(d.data_ptr(), len(s), rc.BODY, rc.N_REF, stream=stream())[0] == 6
    d_off = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.BiogpuError) as e:
        bam.records_dev(d.data_ptr(), len(s), rc.BODY, rc.N_REF, d_off.data_ptr(), 5, stream=stream())
    assert e.value.status == -9 and bool((d_off == -1).all())
    # no record: the closing row alone; a body_off beyond the stream and a cap without a table are refused
    assert bam.records_dev(d.data_ptr(), rc.BODY, rc.BODY, rc.N_REF, d_off.data_ptr(), 0, stream=stream()) == (0, 0)
    torch.cuda.synchronize()
    assert int(d_off[0]) == rc.BODY and int(d_off[1]) == -1
    for args in ((len(s), len(s) + 1, 0, 0), (len(s), rc.BODY, 0, 4)):
        with pytest.raises(_lib.BiogpuError) as e:
            bam.records_dev(d.data_ptr(), args[0], args[1], rc.N_REF, args[2], args[3], stream=stream())
        assert e.value.status == -1
    with pytest.raises(_lib.BiogpuError) as e:
        bam.records_dev(d.data_ptr(), 1 << 35, rc.BODY, rc.N_REF, stream=stream())
    assert e.value.status == -8
    # the host flavour, and the error that names the record and its offset
    off, cand = bam.records_arrays(s, rc.BODY, rc.N_REF, candidates=True)
    assert off.tolist() == ro.walk(s, rc.BODY, rc.N_REF) and cand >= 6
    with pytest.raises(bam.BamReadError) as e:
        bam.records_arrays(s + b"x", rc.BODY, rc.N_REF)
    assert e.value.record == 6

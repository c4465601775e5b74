"""bg_bam_reads[_dev] and bg_bam_sort_keys[_dev] on the GPU against tests/bam_read_oracle.py: the columns of the cases of
tests/bam_read_cases.py with the stream, the bases and the qualities at every offset 0 .. 15 between intact guards; reads of 1,
2, 63, 64, 65, 255, 256 and 257 bases side by side (the lanes' shares and the 16-byte stores at every length class); the FASTQ
text bg_fastq_emit_dev writes from the columns with the stream in the text's place; `src` under a filter; sizing, caps, a table
from elsewhere."""
import numpy as np
import pytest
import torch

import bam_read_cases as rc
import bam_read_oracle as ro
from dev_shift import guards_intact, shifted, shifted_from
from rust_bio_amd import _lib, bam, fastq

pytestmark = pytest.mark.gpu
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257)


def stream():
    return torch.cuda.current_stream().cuda_stream


def table(values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint64).view(np.int64).copy()).cuda()


def reads_dev(s, off, n_ref, flags=0, require=0, exclude=0, r_in=0, r_seq=0, r_qual=0):
    """-> (recs, seq, seq_off, qual, qual_off, src, the device tensors) of bg_bam_reads_dev: the sizing call, then the columns"""
    d, d_off, n = shifted_from(s, r_in), table(off), len(off) - 1
    kw = dict(flags=flags, require=require, exclude=exclude, stream=stream())
    k, sb, qb = bam.reads_dev(n, d.data_ptr(), d_off.data_ptr(), n_ref, **kw)
    d_recs = torch.zeros((k + 1) * 56, dtype=torch.uint8, device="cuda")
    d_seq, d_qual = shifted(max(sb, 1), r_seq), shifted(max(qb, 1), r_qual)  # (a view of no bytes has no address of its own)
    d_so, d_qo, d_src = (torch.full((k + 2,), -1, dtype=torch.int64, device="cuda") for _ in range(3))
    assert bam.reads_dev(n, d.data_ptr(), d_off.data_ptr(), n_ref, d_recs.data_ptr(), k, d_seq.data_ptr(), sb, d_so.data_ptr(), d_qual.data_ptr(), qb,
                         d_qo.data_ptr(), d_src.data_ptr(), **kw) == (k, sb, qb)
    assert guards_intact(d) and guards_intact(d_seq) and guards_intact(d_qual)
    assert int(d_so[k + 1]) == -1 and int(d_qo[k + 1]) == -1 and int(d_src[k]) == -1 and not bool(d_recs[k * 56:].any())
    recs = np.frombuffer(d_recs[:k * 56].cpu().numpy().tobytes(), dtype=_lib.FQREC_DTYPE)
    u = lambda t, m: t[:m].cpu().numpy().astype(np.uint64).tolist()  # noqa: E731
    assert sb or int(d_seq[0]) == 0xA5
    assert qb or int(d_qual[0]) == 0xA5
    return (recs, d_seq[:sb].cpu().numpy().tobytes(), u(d_so, k + 1), d_qual[:qb].cpu().numpy().tobytes(), u(d_qo, k + 1), u(d_src, k)), (d, d_recs, d_seq, d_qual, k)


def same(got, want):
    recs, seq, seq_off, qual, qual_off, src = want
    return rc.same_records(got[0], recs) and tuple(got[1:]) == (seq, seq_off, qual, qual_off, src)


def test_the_cases_at_every_alignment():
    for k, (name, s, fl, rq, ex) in enumerate(rc.reads_cases()):
        off = ro.walk(s, rc.BODY, rc.N_REF)
        want = ro.reads(s, off, rc.N_REF, fl, rq, ex)
        for r in range(16):
            got, _ = reads_dev(s, off, rc.N_REF, fl, rq, ex, r_in=r, r_seq=(5 * r + k) % 16, r_qual=(11 * r + 3 * k) % 16)
            assert same(got, want), (name, r)


def test_the_corpus_and_its_keys():
    contigs = bam.sam.Contigs(rc.CONTIGS)
    for name, s, n_ref in rc.corpus():
        try:
            off = ro.walk(s, rc.BODY, n_ref)
        except ro.Refused:
            continue
        got, _ = reads_dev(s, off, n_ref, r_in=7, r_seq=9, r_qual=2)
        assert same(got, ro.reads(s, off, n_ref)), name
        if n_ref:
            assert bam.sort_keys_records_arrays(s, off, contigs).tolist() == ro.keys(s, off, rc.CONTIGS), name


def test_lengths_side_by_side_and_the_fastq_text():
    recs = []
    for i, n in enumerate(LENGTHS + LENGTHS[::-1]):
        recs.append(rc.seq_rec(i, n, flag=0x10 if i & 1 else 0))
        recs.append(rc.raw(b"star%d" % i, flag=0x10 if i & 2 else 0, codes=[1 + (k % 15) for k in range(n)]))
    s = rc.HEADER + b"".join(recs)
    off = ro.walk(s, rc.BODY, rc.N_REF)
    for fl in (0, ro.ORIGINAL):
        want = ro.reads(s, off, rc.N_REF, fl)
        got, (d, d_recs, d_seq, d_qual, k) = reads_dev(s, off, rc.N_REF, fl, r_in=13, r_seq=1, r_qual=6)
        assert same(got, want) and k == len(recs)
        d_text, _, total = fastq.emit_dev(k, d, d_recs, d_seq, d_qual, stream=stream())
        assert d_text.cpu().numpy().tobytes() == ro.fastq_text(s, want[0], want[1], want[3]) and total == len(d_text)
    # the host flavour gives the same columns
    h = bam.reads_arrays(s, off, rc.N_REF, flags=ro.ORIGINAL)
    assert same((h[0], h[1].tobytes(), h[2].tolist(), h[3].tobytes(), h[4].tolist(), h[5].tolist()), ro.reads(s, off, rc.N_REF, ro.ORIGINAL))


def test_src_under_a_filter():
    s = rc.mixed_flags()
    off = ro.walk(s, rc.BODY, rc.N_REF)
    got, _ = reads_dev(s, off, rc.N_REF, exclude=0x900)
    assert got[5] == ro.reads(s, off, rc.N_REF, exclude=0x900)[5] == [0, 1, 2, 6, 7, 8]
    got, _ = reads_dev(s, off, rc.N_REF, require=0x1, exclude=0x80)
    assert got[5] == [7]
    got, _ = reads_dev(s, off, rc.N_REF, require=0x200)
    assert got[5] == [] and got[2] == [0] and got[4] == [0]


def test_caps_and_a_table_from_elsewhere():
    s = rc.HEADER + b"".join(rc.seq_rec(i, 10 + i, ref=1, pos=i) for i in range(4))
    off = ro.walk(s, rc.BODY, rc.N_REF)
    d, n = shifted_from(s, 2), len(off) - 1
    k, sb, qb = bam.reads_dev(n, d.data_ptr(), table(off).data_ptr(), rc.N_REF, stream=stream())
    assert (k, sb, qb) == (4, 46, 46)
    bufs = [torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(6)]
    for caps in ((3, sb, qb), (k, sb - 1, qb), (k, sb, qb - 1)):
        with pytest.raises(_lib.BiogpuError) as e:
            bam.reads_dev(n, d.data_ptr(), table(off).data_ptr(), rc.N_REF, bufs[0].data_ptr(), caps[0], bufs[1].data_ptr(), caps[1], bufs[2].data_ptr(),
                          bufs[3].data_ptr(), caps[2], bufs[4].data_ptr(), bufs[5].data_ptr(), stream=stream())
        assert e.value.status == -9 and all(bool((b == 0x5A).all()) for b in bufs)
    for bad_table in (off[:2] + off[3:], off[:1] + [off[1] - 1] + off[2:], [off[0] + 1] + off[1:]):
        with pytest.raises(ro.Refused) as want:
            ro.reads(s, bad_table, rc.N_REF)
        with pytest.raises(bam.BamReadError) as e:
            bam.reads_dev(len(bad_table) - 1, d.data_ptr(), table(bad_table).data_ptr(), rc.N_REF, bufs[0].data_ptr(), 4, bufs[1].data_ptr(), 64,
                          bufs[2].data_ptr(), bufs[3].data_ptr(), 64, bufs[4].data_ptr(), bufs[5].data_ptr(), stream=stream())
        assert e.value.record == want.value.first_bad and all(bool((b == 0x5A).all()) for b in bufs)
        with pytest.raises(bam.BamReadError) as e:
            bam.sort_keys_records_arrays(s, bad_table, bam.sam.Contigs(rc.CONTIGS))
        assert e.value.record == want.value.first_bad
    # an empty slot is skipped, and its key is the largest
    with_empty = off[:3] + [off[3]] + off[3:]
    got, _ = reads_dev(s, with_empty, rc.N_REF)
    assert same(got, ro.reads(s, with_empty, rc.N_REF)) and got[5] == [0, 1, 2, 4]
    assert bam.sort_keys_records_arrays(s, with_empty, bam.sam.Contigs(rc.CONTIGS)).tolist() == ro.keys(s, with_empty, rc.CONTIGS)

"""`bg_fastq_emit[_dev]` (csrc/fastq_emit.hip) byte for byte against `fastq::Writer::write` restated in Python
(tests/fastq_write_oracle.py): record counts at the lane-group, block and scan-block edges, every combination of field
lengths around the 16- and 32-byte marks, sources and output at every byte alignment, lines around the staging area, `first`
and `step`, the sizing call, BG_ERR_OPS_CAP, the host flavour, and a round trip through bg_fastq_parse_dev.  The output is
always a slice of a larger tensor filled with 0xA5: the bytes before and behind the text must stay as they were."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest
import torch

import fastq_write_oracle as fw
from fastq_write_cases import Batch, random_records
from rust_bio_amd import _lib, fastq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGE = [0, 1, 15, 16, 17, 31, 32, 33]
MODES = [1, 2]  # fq_emit_mode: byte stores, lines staged in LDS and stored 16 bytes wide


def emit_checked(batch, first=0, step=1, shift=0, dev=None):
    """sizing call, then the writing call into big[shift : shift + total]; everything compared with the restatement"""
    d_text, d_recs, d_seq, _, d_qual, _ = dev or batch.to_dev(DEV)
    n = len(batch)
    want, want_off = fw.emit(batch.text, batch.recs, batch.seq, batch.qual, first, step)
    m = fastq.n_lines(n, first, step)
    assert len(want_off) == m + 1
    d_off = torch.full((m + 1,), -1, dtype=torch.int64, device=DEV)
    total = C.c_uint64(99)
    args = (_lib.default_context().h, n, first, step, d_text.data_ptr(), d_recs.data_ptr(), d_seq.data_ptr(), d_qual.data_ptr())
    assert _lib.lib().bg_fastq_emit_dev(*args, None, 0, d_off.data_ptr(), C.byref(total), 0) == 0
    assert total.value == len(want)
    assert (d_off.cpu().numpy().astype(np.uint64) == want_off).all()
    big = torch.full((shift + len(want) + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    d_out = big[shift:shift + len(want)]
    d_off.fill_(-1)
    got, d_off2, total2 = fastq.emit_dev(n, d_text, d_recs, d_seq, d_qual, first, step, out=(d_out, d_off))
    torch.cuda.synchronize()
    host = big.cpu().numpy()
    assert total2 == len(want)
    assert (host[:shift] == 0xA5).all() and (host[shift + len(want):] == 0xA5).all()
    assert host[shift:shift + len(want)].tobytes() == want
    assert (d_off2.cpu().numpy().astype(np.uint64) == want_off).all()
    return want


@pytest.fixture
def mode(request):
    ctx = _lib.default_context()
    ctx.set_option("fq_emit_mode", request.param)
    yield request.param
    ctx.set_option("fq_emit_mode", 0)


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 2047, 2048, 2049])
def test_record_counts(n):
    rng = random.Random(n)
    hi = 3 if n > 100 else 40
    emit_checked(Batch(random_records(rng, n, 1, hi)), shift=5)


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_every_combination_of_field_lengths(mode):
    rng = random.Random(2)

    def run(k):
        return bytes(rng.randint(48, 122) for _ in range(k))

    records = [(run(i), run(d), run(s), run(q)) for i, d, s, q in itertools.product(EDGE, EDGE, EDGE, EDGE)]
    records += [(run(i), None, run(s), run(q)) for i, s, q in itertools.product(EDGE, EDGE, EDGE)]
    rng.shuffle(records)
    b = Batch(records)
    assert (b.recs["desc_len"][b.recs["has_desc"] == 1] == 0).any() and (b.recs["id_len"] == 0).any()
    emit_checked(b, shift=3)


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_sources_and_output_at_every_alignment(mode):
    rng = random.Random(4)
    records = random_records(rng, 37, 0, 40) + random_records(rng, 6, 140, 152, tag=b"long")
    for a in range(16):
        b = Batch(records, a_text=a, a_seq=(a * 7 + 3) % 16, a_qual=(a * 5 + 1) % 16)
        dev = b.to_dev(DEV)
        for shift in (1, 7, 16):
            emit_checked(b, shift=shift, dev=dev)


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_lines_around_the_staging_area(mode):
    """a line is staged when its bytes and its offset inside a 16-byte granule fit 1040 bytes: line lengths 1010 .. 1045 at
    whatever offsets they fall on, and one line of 40 006 bytes"""
    rng = random.Random(6)
    s = bytes(rng.choice(b"ACGT") for _ in range(500))
    records = [(b"i" * (ln - 1006), None, s, s[::-1]) for ln in range(1010, 1046)]
    records.append((b"big", b"read", s * 40, s[::-1] * 40))
    records += random_records(rng, 5, 1, 30)
    b = Batch(records)
    dev = b.to_dev(DEV)
    for shift in (0, 9):
        emit_checked(b, shift=shift, dev=dev)


@pytest.mark.parametrize("n", [7, 8])
def test_first_and_step(n):
    b = Batch(random_records(random.Random(n), n, 1, 40))
    dev = b.to_dev(DEV)
    r1 = emit_checked(b, 0, 2, shift=1, dev=dev)
    r2 = emit_checked(b, 1, 2, shift=1, dev=dev)
    assert r1.count(b"\n+\n") == (n + 1) // 2 and r2.count(b"\n+\n") == n // 2
    assert emit_checked(b, n, 1, dev=dev) == b"" and emit_checked(b, n + 5, 2, dev=dev) == b""
    emit_checked(b, 2, 3, dev=dev)
    emit_checked(b, n - 1, 1 << 40, dev=dev)


def test_ops_cap_leaves_the_buffer_untouched():
    b = Batch(random_records(random.Random(8), 50, 1, 40))
    d_text, d_recs, d_seq, _, d_qual, _ = b.to_dev(DEV)
    want, want_off = fw.emit(b.text, b.recs, b.seq, b.qual)
    big = torch.full((len(want) + 32,), 0xA5, dtype=torch.uint8, device=DEV)
    d_off = torch.zeros(51, dtype=torch.int64, device=DEV)
    total = C.c_uint64(0)
    rc = _lib.lib().bg_fastq_emit_dev(_lib.default_context().h, 50, 0, 1, d_text.data_ptr(), d_recs.data_ptr(), d_seq.data_ptr(), d_qual.data_ptr(),
                                      big.data_ptr(), len(want) - 1, d_off.data_ptr(), C.byref(total), 0)
    torch.cuda.synchronize()
    assert rc == -9 and total.value == len(want)
    assert (big.cpu().numpy() == 0xA5).all()
    assert (d_off.cpu().numpy().astype(np.uint64) == want_off).all()
    with pytest.raises(_lib.BiogpuError, match="OPS_CAP"):
        fastq.emit_dev(50, d_text, d_recs, d_seq, d_qual, out=(big[:len(want) - 1], d_off))


def test_unequal_lengths_and_empty_records_are_written_as_they_are():
    records = [(b"a", None, b"ACGT", b"I"), (b"b", b"x", b"A", b"IIII"), (b"c", None, b"", b""), (b"", b"", b"", b"II"), (b"d", b"", b"AC", b"")]
    assert emit_checked(Batch(records), shift=2) == b"@a\nACGT\n+\nI\n@b x\nA\n+\nIIII\n@c\n\n+\n\n@ \n\n+\nII\n@d \nAC\n+\n\n"


def test_a_wrapped_record_comes_back_on_one_line():
    fq = b"@id description\nACGT\nGGGG\nC\n+\n@@@@\n!!!!\n$\n@id2\nAC\nG\n+\nII\nI\n"
    d_fq = torch.frombuffer(bytearray(fq), dtype=torch.uint8).to(DEV)
    k, status, _, d_recs, d_seq, _, d_qual, _ = fastq.parse_dev(d_fq)
    assert (k, status) == (2, "ok")
    d_out, d_off, total = fastq.emit_dev(k, d_fq, d_recs, d_seq, d_qual)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == b"@id description\nACGTGGGGC\n+\n@@@@!!!!$\n@id2\nACG\n+\nIII\n"
    assert d_off.cpu().tolist() == [0, 38, total] and total == 53


def test_host_flavour_and_the_writer():
    rng = random.Random(10)
    b = Batch(random_records(rng, 300, 0, 60), a_text=3, a_seq=5, a_qual=9)
    for first, step in [(0, 1), (0, 2), (1, 2), (300, 1)]:
        want, want_off = fw.emit(b.text, b.recs, b.seq, b.qual, first, step)
        got, off = fastq.emit_arrays(b.host(), first, step)
        assert got == want and (off == want_off).all()
    d_text, d_recs, d_seq, _, d_qual, _ = b.to_dev(DEV)
    d_out, _, _ = fastq.emit_dev(300, d_text, d_recs, d_seq, d_qual)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == fastq.emit_arrays(b.host())[0]
    w = fastq.Writer(batch=128)  # several batches
    for id_, desc, seq, qual in b.records:
        w.write(id_.decode(), None if desc is None else desc.decode(), seq, qual)
    w.write_record(fastq.Record(b"last", b"one", b"ACGT", b"!!!!"))
    assert w.getvalue() == fw.emit(b.text, b.recs, b.seq, b.qual)[0] + b"@last one\nACGT\n+\n!!!!\n"
    assert fastq.Writer().getvalue() == b""


def test_round_trip_through_the_device_reader():
    rng = random.Random(12)
    records = []
    for r in range(5000):
        ln = rng.randint(1, 150)
        desc = None if r % 3 == 0 else b"%d:N:0 x" % r
        records.append((b"read%d" % r, desc, bytes(rng.choice(b"ACGTN") for _ in range(ln)), bytes(rng.randint(33, 73) for _ in range(ln))))
    b = Batch(records, a_text=1)
    d_text, d_recs, d_seq, _, d_qual, _ = b.to_dev(DEV)
    d_out, _, total = fastq.emit_dev(5000, d_text, d_recs, d_seq, d_qual)
    assert total == len(fw.emit(b.text, b.recs, b.seq, b.qual)[0])
    k, status, _, p_recs, p_seq, p_so, p_qual, p_qo = fastq.parse_dev(d_out)
    torch.cuda.synchronize()
    assert (k, status) == (5000, "ok")
    recs = p_recs.cpu().numpy().view(_lib.FQREC_DTYPE)
    assert (recs["check"] == 0).all()
    for f in ("id_len", "desc_len", "has_desc", "seq_len", "qual_len"):
        assert (recs[f] == b.recs[f]).all(), f
    assert (p_so.cpu().numpy().astype(np.uint64) == b.seq_off).all() and (p_qo.cpu().numpy().astype(np.uint64) == b.qual_off).all()
    assert p_seq.cpu().numpy()[:len(b.seq)].tobytes() == b.seq and p_qual.cpu().numpy()[:len(b.qual)].tobytes() == b.qual
    out = d_out.cpu().numpy().tobytes()
    for r in (0, 1, 2, 2499, 4999):
        c = recs[r]
        assert out[int(c["id_off"]):int(c["id_off"] + c["id_len"])] == records[r][0]
        assert (out[int(c["desc_off"]):int(c["desc_off"] + c["desc_len"])] if c["has_desc"] else None) == records[r][1]

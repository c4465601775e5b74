"""The BAM record writer (`bg_bam_emit_batch[_dev]`) on the hand-made records of tests/sam_edge_cases.py: records and `out_off`
byte for byte against `bam_oracle.records(case.want())`, i.e. against the encoding of the SAM writer's own lines — field
widths, the staging limit, slots per group / block / tile, `dup`, MD.  Both flavours; the device flavour with a sizing call,
then an exact-fit cap into a poisoned buffer with 64 bytes behind the total, with 16 and 32 lanes a record.  The cases with a
line on the 3 Gbp contig of WIDE_CONTIGS or with an id of 255 bytes must come back BG_ERR_UNSUPPORTED with nothing written
(tests/test_bam_rule.py names them from the oracle alone).  Then: an id of 254 bytes, more than 65 535 CIGAR operations (the CG
tag), BG_ERR_OPS_CAP one byte short, caller pointers off 16-byte alignment, and no reads at all."""
import struct
import types

import numpy as np
import pytest
import torch

import bam_oracle as bo
import dev_align_cases as dc
import sam_edge_cases as ec
from dev_shift import guards_intact, shifted, shifted_from
from rust_bio_amd import _lib, bam, sam
from test_bam_rule import UNREPRESENTABLE
from test_gpu_sam_emit_edges import DEV, POISON, dev, index

pytestmark = pytest.mark.gpu
UNSUPPORTED, OPS_CAP = -11, -9
BIG_CONTIGS = [(b"big", 0, 200_000), (b"edge", 200_001, 2**31 - 1)]


def same(want, data, off, what):
    assert (np.asarray(off) == bo.offsets(want)).all(), what
    if data != b"".join(want):
        for s, w in enumerate(want):
            assert data[int(off[s]):int(off[s + 1])] == w, (what, s)
    assert data == b"".join(want), what


def dev_args(fm, case):
    table = sam.Contigs(case.contigs)
    d = [dev(x) for x in (table.table, table.names, case.fq.text, case.fq.recs, case.fq.seq, case.fq.qual, case.hits, case.strand, case.ops)]
    opt = {k: dev(v) for k, v in (("d_multi", case.multi), ("d_pairs", case.pairs), ("d_dup", case.dup)) if v is not None}
    kw = {k: v.data_ptr() for k, v in opt.items()}
    kw["stream"] = torch.cuda.current_stream().cuda_stream
    args = (fm, sam.SamParams(case.flags, case.K), case.n, d[0].data_ptr(), len(table), d[1].data_ptr(), *(x.data_ptr() for x in d[2:]))
    return args, kw, (d, opt)  # the last keeps the buffers alive


def emit_dev(fm, case):
    args, kw, _keep = dev_args(fm, case)
    n_slots = case.n * case.K
    d_off = torch.full((n_slots + 1,), -1, dtype=torch.int64, device=DEV)
    total = bam.emit_dev(*args, 0, 0, d_off.data_ptr(), **kw)
    torch.cuda.synchronize()
    sized = d_off.cpu().numpy().astype(np.uint64)
    assert int(sized[-1]) == total
    d_out = torch.full((total + 64,), POISON, dtype=torch.uint8, device=DEV)
    d_off.fill_(-1)
    assert bam.emit_dev(*args, d_out.data_ptr(), total, d_off.data_ptr(), **kw) == total
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[total:] == POISON).all(), "bytes behind the total were touched"
    off = d_off.cpu().numpy().astype(np.uint64)
    assert (off == sized).all()
    return out[:total].tobytes(), off


def refused_dev(fm, case):
    """BG_ERR_UNSUPPORTED from the sizing call and from a call with room to spare, which writes nothing"""
    args, kw, _keep = dev_args(fm, case)
    d_off = torch.zeros((case.n * case.K + 1,), dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.BiogpuError) as e:
        bam.emit_dev(*args, 0, 0, d_off.data_ptr(), **kw)
    assert e.value.status == UNSUPPORTED
    d_out = torch.full((1 << 20,), POISON, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.BiogpuError) as e:
        bam.emit_dev(*args, d_out.data_ptr(), 1 << 20, d_off.data_ptr(), **kw)
    torch.cuda.synchronize()
    assert e.value.status == UNSUPPORTED and bool((d_out == POISON).all())


def host_call(fm, case):
    return bam.emit_arrays(fm, sam.SamParams(case.flags, case.K), sam.Contigs(case.contigs), case.fq, case.hits, case.strand, case.ops,
                           multi=case.multi, pairs=case.pairs, dup=case.dup)


def run(case, lanes=(16, 32)):
    fm = index()
    try:
        want = bo.records(case.want(), case.contigs)
    except bo.Unrepresentable:
        want = None
    if want is None:
        with pytest.raises(_lib.BiogpuError) as e:
            host_call(fm, case)
        assert e.value.status == UNSUPPORTED
        refused_dev(fm, case)
        return None
    same(want, *host_call(fm, case), (case.name, "host"))
    for g in lanes:
        fm.ctx.set_option("sam_lanes", g)
        try:
            same(want, *emit_dev(fm, case), (case.name, "device", g))
        finally:
            fm.ctx.set_option("sam_lanes", 0)
    return want


@pytest.mark.parametrize("name", sorted(ec.EMIT_CASES))
def test_every_emit_case(name):
    want = run(ec.emit_case(name))
    assert (want is None) == (name in UNREPRESENTABLE)


def qname_case(id_len):
    lo = ec.WIDE_CONTIGS[0][1]
    reads = [ec.read(b"a", 5), ec.read(b"n" * id_len, 5, 1), ec.read(b"u" * id_len, 4, 2)]
    hits = [ec.hit(lo + 10, "=====", 0), ec.hit(lo + 20, "==X==", 1), None]
    return ec.EmitCase("qname_%d" % id_len, "an id of %d bytes on a placed and an unplaced line" % id_len, ec.WIDE_CONTIGS,
                       {"flags": ["NM"], "K": 1, "reads": reads, "hits": hits})


def test_qname_of_254_bytes_passes_and_255_does_not():
    want = run(qname_case(254))
    assert want is not None and want[1][12] == 255 and want[2][12] == 255  # l_read_name
    assert run(qname_case(255)) is None


def test_contig_of_2_31_minus_1_passes():
    at = BIG_CONTIGS[1][1]
    reads = [ec.read(b"last", 3), ec.read(b"first", 3, 1)]
    hits = [ec.hit(at + 2**31 - 4, "===", 1), ec.hit(at, "=X=", 0)]
    want = run(ec.EmitCase("edge", "POS 1 and POS 2^31 - 3 on a contig of 2^31 - 1 bases", BIG_CONTIGS, {"flags": ["NM"], "K": 1, "reads": reads, "hits": hits}))
    assert struct.unpack_from("<i", want[0], 8)[0] == 2**31 - 4


def test_more_than_65535_operations_go_into_the_cg_tag():
    n = 65_535
    ops = "=D" * (n - 1) + "="
    reads = [ec.read(b"short", 4), ec.read(b"cg", n, 3), ec.read(b"after", 4, 1)]
    hits = [ec.hit(7, "====", 0), ec.hit(100, ops, 1, score=-70_000), ec.hit(9, "=X==", 1)]
    case = ec.EmitCase("cg", "65 535 bases, 131 069 operations", BIG_CONTIGS, {"flags": ["NM"], "K": 1, "reads": reads, "hits": hits})
    want = run(case, lanes=(16,))
    n_cigar, = struct.unpack_from("<H", want[1], 16)
    assert n_cigar == 2 and want[1][-(8 + 4 * 131_069):][:8] == b"CGBI" + struct.pack("<I", 131_069)
    assert bo.decode(want[1], BIG_CONTIGS) == ec.fields(case.want()[1])


def test_ops_cap_one_byte_short_writes_nothing():
    fm, case = index(), ec.emit_case("md")
    total = sum(len(r) for r in bo.records(case.want(), case.contigs))
    args, kw, _keep = dev_args(fm, case)
    d_off = torch.zeros((case.n * case.K + 1,), dtype=torch.int64, device=DEV)
    d_out = torch.full((total + 64,), POISON, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.BiogpuError) as e:
        bam.emit_dev(*args, d_out.data_ptr(), total - 1, d_off.data_ptr(), **kw)
    torch.cuda.synchronize()
    assert e.value.status == OPS_CAP and bool((d_out == POISON).all())
    assert int(d_off[-1]) == total  # out_off is still filled


def test_pointers_off_16_byte_alignment():
    from test_gpu_dev_pointer_alignment import host, stream, typed
    fm, case = index(), dc.sam_case()
    want = bo.records(case.want(), case.contigs)
    total = sum(len(w) for w in want)
    table = sam.Contigs(case.contigs)
    n = case.n
    fixed = [typed(a) for a in (table.table, table.names, case.fq.recs, case.hits, case.strand, case.ops)]
    d_table, d_names, d_recs, d_hits, d_strand, d_ops = (a.data_ptr() for a in fixed)
    for r_in in range(16):
        d_fq, d_seq, d_qual = (shifted_from(np.ascontiguousarray(a), r_in) for a in (case.fq.text, case.fq.seq, case.fq.qual))
        r_out = (5 * r_in + 1) % 16  # every residue of the output once
        d_out, d_off = shifted(total, r_out), shifted((n + 1) * 8, 0)
        got = bam.emit_dev(fm, sam.SamParams(case.flags, 1), n, d_table, len(table), d_names, d_fq.data_ptr(), d_recs, d_seq.data_ptr(),
                           d_qual.data_ptr(), d_hits, d_strand, d_ops, d_out.data_ptr(), total, d_off.data_ptr(), stream=stream())
        assert got == total and guards_intact(d_out) and guards_intact(d_off), (r_in, r_out)
        same(want, host(d_out).tobytes(), host(d_off, np.uint64), (r_in, r_out))


def test_no_reads():
    fm = index()
    table = sam.Contigs(ec.MD_CONTIGS)
    none = np.zeros(0, np.uint8)
    parsed = types.SimpleNamespace(text=none, recs=np.zeros(0, _lib.FQREC_DTYPE), seq=none, qual=none)
    data, off = bam.emit_arrays(fm, sam.SamParams(0, 1), table, parsed, np.zeros(0, _lib.SEED_HIT_DTYPE), np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    assert data == b"" and off.tolist() == [0]
    d_off = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    assert bam.emit_dev(fm, sam.SamParams(0, 1), 0, 0, len(table), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, d_off.data_ptr()) == 0
    torch.cuda.synchronize()
    assert int(d_off[0]) == 0

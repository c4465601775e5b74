"""The SAM writer (`bg_sam_emit[_dup]_batch[_dev]`) on the hand-made records of tests/sam_edge_cases.py, byte for byte against
tests/sam_oracle.py: every decimal width of every numeric field, every FLAG, ids and names at their length limits, lines on
both sides of the staging limit at every residue of the output offset, and slot counts around a group, a block and a scan
tile.  Both flavours; the device flavour as `test_gpu_sam_emit.Batch.emit_dev` runs it — a sizing call, then an exact-fit cap
into a poisoned buffer with 64 bytes behind the total — with 16 and 32 lanes a line.  tests/test_sam_edge_cases.py shows,
without a GPU, that the cases hold what they claim."""
import functools

import numpy as np
import pytest
import torch

import sam_edge_cases as ec
import sam_oracle as so
from rust_bio_amd import sam
from rust_bio_amd.pipeline import attach_text
from test_gpu_pipeline import build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0xAA


@functools.lru_cache(maxsize=None)
def index():
    """an index of the small text of the MD cases; the cases without MD only borrow its context"""
    text = ec.md_text()
    sa, b, ls, fm = build(text, 0)
    attach_text(fm, text)
    return fm


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(DEV) if a.size else torch.zeros(16, dtype=torch.uint8, device=DEV)


def same(want, text, off, what):
    """the oracle's lines against (text, out_off) of a call; names the first line that differs"""
    assert (np.asarray(off) == so.offsets(want)).all(), what
    if text != b"".join(want):
        for s, w in enumerate(want):
            assert text[int(off[s]):int(off[s + 1])] == w, (what, s)
    assert text == b"".join(want), what


def emit_dev(fm, case):
    table = sam.Contigs(case.contigs)
    n, K = case.n, case.K
    d = [dev(x) for x in (table.table, table.names, case.fq.text, case.fq.recs, case.fq.seq, case.fq.qual, case.hits, case.strand, case.ops)]
    opt = {k: dev(v) for k, v in (("d_multi", case.multi), ("d_pairs", case.pairs), ("d_dup", case.dup)) if v is not None}
    kw = {k: v.data_ptr() for k, v in opt.items()}
    kw["stream"] = torch.cuda.current_stream().cuda_stream
    args = (fm, sam.SamParams(case.flags, K), n, d[0].data_ptr(), len(table), d[1].data_ptr(), *(x.data_ptr() for x in d[2:]))
    d_off = torch.full((n * K + 1,), -1, dtype=torch.int64, device=DEV)
    total = sam.emit_dev(*args, 0, 0, d_off.data_ptr(), **kw)
    torch.cuda.synchronize()
    sized = d_off.cpu().numpy().astype(np.uint64)
    assert int(sized[-1]) == total
    d_out = torch.full((total + 64,), POISON, dtype=torch.uint8, device=DEV)
    d_off.fill_(-1)
    assert sam.emit_dev(*args, d_out.data_ptr(), total, d_off.data_ptr(), **kw) == total
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[total:] == POISON).all(), "bytes behind the total were touched"
    off = d_off.cpu().numpy().astype(np.uint64)
    assert (off == sized).all()
    return out[:total].tobytes(), off


def run(name):
    fm, case = index(), ec.emit_case(name)
    want = case.want()
    text, off = sam.emit_arrays(fm, sam.SamParams(case.flags, case.K), sam.Contigs(case.contigs), case.fq, case.hits, case.strand, case.ops,
                                multi=case.multi, pairs=case.pairs, dup=case.dup)
    same(want, text, off, (name, "host"))
    for lanes in (16, 32):
        fm.ctx.set_option("sam_lanes", lanes)
        try:
            same(want, *emit_dev(fm, case), (name, "device", lanes))
        finally:
            fm.ctx.set_option("sam_lanes", 0)
    return case, want


@pytest.mark.parametrize("name", sorted(ec.FIELD_CASES))
def test_field_widths(name):
    case, want = run(name)
    assert sum(bool(w) for w in want) >= 10


def test_the_staging_limit():
    case, want = run("staging_limit")
    assert len(ec.staged_pairs(case)) == 64  # 16 residues x (1040, 1041) x (unplaced, placed reverse with all tags)
    case, want = run("stage_1024")
    assert {total for _, total, _ in ec.staged_pairs(case)} == {1023, 1024, 1025, 1026}


@pytest.mark.parametrize("name", sorted(ec.GRID_CASES))
def test_grid_and_group_edges(name):
    case, want = run(name)
    assert len(want) == case.n * case.K and (case.K == 1 or name == "nothing_placed" or not want[-1])

"""bg_sam_sort_keys[_dev] against `sam_sort_oracle.sort_keys` on the synthetic batches of `sam_edge_cases.key_batches`: unpaired
and paired with K = 1, K = 4 with and without secondary lines, every combination of the NM / MD bits (they must not matter),
from nothing to everything unmapped, slot counts around a block of the key kernel, and contigs whose starts differ only above
bit 32.  tests/test_sam_edge_cases.py requires of the batches together, from the placement rule alone, at least 20 keys
borrowed from a placed mate, 20 secondary slots with a key, 20 without one because slot 0 is unplaced, and 20 hits across a
contig's end.  The device flavour writes into a poisoned buffer with 16 bytes behind it.  Then the consistency property: the
lines the writer emits for a batch, sorted by the device's keys, pass the check that reads only SAM text."""
import numpy as np
import pytest
import torch

import sam_edge_cases as ec
import sam_oracle as so
import sam_sort_oracle as sso
from rust_bio_amd import sam
from test_gpu_sam_emit_edges import DEV, dev, index

pytestmark = pytest.mark.gpu
BATCHES = {b.name: b for b in ec.key_batches()}


def test_the_batches_hold_what_they_are_for():
    assert all(sum(b.counts()[k] for b in BATCHES.values()) >= 20 for k in next(iter(BATCHES.values())).counts())


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_keys_and_sorted_text(name):
    b = BATCHES[name]
    fm = index()
    want = sso.sort_keys(b.contigs, b.hits, b.strand, b.flags, b.K)
    table, sp = sam.Contigs(b.contigs), sam.SamParams(b.flags, b.K)
    got = sam.sort_keys_arrays(sp, table, b.n, b.hits, b.strand, ctx=fm.ctx)
    assert (got == want).all(), np.nonzero(got != want)[0][:5]
    n_slots = b.n * b.K
    d_table, d_hits, d_strand = dev(table.table), dev(b.hits), dev(b.strand)
    d_key = torch.full((8 * n_slots + 16,), 0x7e, dtype=torch.uint8, device=DEV)
    sam.sort_keys_dev(sp, b.n, d_table.data_ptr(), len(table), d_hits.data_ptr(), d_strand.data_ptr(), d_key.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream, ctx=fm.ctx)
    torch.cuda.synchronize()
    raw = d_key.cpu().numpy()
    key = raw[:8 * n_slots].view(np.uint64)
    assert (raw[8 * n_slots:] == 0x7e).all(), "bytes behind the keys were touched"
    assert (key == want).all(), np.nonzero(key != want)[0][:5]
    # consistency: the writer's lines (without MD: these hits lie on no text) in the order of the device's keys
    flags = b.flags & ~so.TAG_MD
    pairs = np.zeros(b.n // 2, dtype=ec.DTYPES[2]) if flags & so.PAIRED else None
    ops = np.zeros(0, dtype=np.uint8)
    text, off = sam.emit_arrays(fm, sam.SamParams(flags, b.K), table, b.fq, b.hits, b.strand, ops, pairs=pairs)
    lines = so.lines(b.contigs, b.fq, b.hits, b.strand, ops, flags, b.K, None, pairs, None)
    assert text == b"".join(lines)
    body, _, _ = sam.sort_arrays(key, text, off, ctx=fm.ctx)
    sso.check_sorted_text([c[0] for c in b.contigs], text, body)

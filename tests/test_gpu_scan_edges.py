"""`bg_scan_u32` (csrc/scan.hip) at its edges, through the one public path that scans an exact item count: the FASTQ
reader's general kernels (`fq_no_fused`), whose F5 scans exactly n_records sequence lengths and n_records quality
lengths, and whose F1 scans one newline count per 4096-byte chunk of the text.

The scan works in blocks of 2048 items (sums per block, one block scanning the sums, every block scanning its items);
when n is a multiple of 2048 one more block exists only to write the closing offset.  The single-block stage takes
4096 block sums a trip: its second trip needs more than 2048 * 4096 = 8.39 M scanned items, out of reach of a quick
test, and is not covered here."""
import numpy as np
import pytest

import oracle_py as orc
from rust_bio_amd import _lib
from test_gpu_fastq import same_as_oracle

pytestmark = pytest.mark.gpu
ALPHA = np.frombuffer(b"ACGTN", dtype=np.uint8)


@pytest.fixture(scope="module")
def general_ctx():
    ctx = _lib.Context(0)
    ctx.set_option("fq_no_fused", 1)
    yield ctx
    ctx.close()


def columns_like_the_oracle(text, ctx):
    """records like same_as_oracle, and the four columns the scans place — seq_off, qual_off, seq, qual — byte for byte"""
    p = same_as_oracle(text, ctx=ctx)
    want, _, _ = orc.fastq_parse(text)
    assert p.status == "ok"
    for off, col, key in ((p.seq_off, p.seq, "seq"), (p.qual_off, p.qual, "qual")):
        lens = np.array([len(w[key]) for w in want], dtype=np.uint64)
        assert (off == np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(lens, dtype=np.uint64)])).all(), key
        assert col.tobytes() == b"".join(w[key] for w in want), key
    return p


@pytest.mark.parametrize("n_records", [1, 2047, 2048, 2049, 4096, 4097])
def test_record_counts_around_the_scan_blocks(general_ctx, n_records):
    """reads of 1 - 40 bases of pseudo-random length: every offset differs from its neighbours'"""
    rng = np.random.default_rng(1000 + n_records)
    out = []
    for k in range(n_records):
        ln = int(rng.integers(1, 41))
        out.append(b"@r%d\n" % k + ALPHA[rng.integers(0, 5, size=ln)].tobytes() + b"\n+\n"
                   + rng.integers(33, 75, size=ln).astype(np.uint8).tobytes() + b"\n")
    p = columns_like_the_oracle(b"".join(out), general_ctx)
    assert len(p) == n_records


def test_chunk_counts_past_one_scan_block(general_ctx):
    """a text of more than 2048 chunks of 4096 bytes: F1's scan of the newline counts crosses a block boundary (and F5's
    two scans thirteen of them)"""
    n, L = 26_720, 150
    rng = np.random.default_rng(7)
    rec = np.empty((n, 2 * L + 14), dtype=np.uint8)  # "@r0000000\n" seq "\n+\n" qual "\n"
    ids = np.char.zfill(np.arange(n).astype("S7"), 7)
    rec[:, 0:2] = np.frombuffer(b"@r", dtype=np.uint8)
    rec[:, 2:9] = np.frombuffer(ids.tobytes(), dtype=np.uint8).reshape(n, 7)
    rec[:, 9] = 10
    rec[:, 10:10 + L] = ALPHA[rng.integers(0, 5, size=(n, L))]
    rec[:, 10 + L:13 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 13 + L:13 + 2 * L] = rng.integers(33, 75, size=(n, L)).astype(np.uint8)
    rec[:, 13 + 2 * L] = 10
    text = rec.tobytes()
    assert len(text) > 2048 * 4096
    p = columns_like_the_oracle(text, general_ctx)
    assert len(p) == n

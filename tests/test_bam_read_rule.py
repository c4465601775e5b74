"""The Python restatement of reading BAM (tests/bam_read_oracle.py) pinned by the restatements of writing it: its walk over
`bam_oracle.records` output gives `bam_oracle.offsets`; its header parser inverts `bam_oracle.header`; its index through
`bai_oracle.build` with the virtual offsets of any framing, on a stream framed by `bam_oracle.frame`, is the one with
`bai_oracle.stored_voff` — except for the stream's end, which the rule for any framing puts at the end-of-file block."""
import numpy as np

import bai_oracle
import bam_oracle
import bam_read_oracle as ro
import bgzf_inflate_cases as ic

CONTIGS = [(b"chr1", 0, 200000), (b"chr2", 200001, 90000)]


def lines(n=400, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ref = int(rng.integers(0, 2))
        pos = int(rng.integers(1, 80000))
        ln = int(rng.integers(20, 300))
        seq = bytes(rng.choice(list(b"ACGTN"), ln).astype(np.uint8))
        qual = bytes(rng.integers(33, 74, ln).astype(np.uint8))
        out.append((ref, pos, b"r%d\t%d\t%s\t%d\t30\t%dM\t*\t0\t0\t%s\t%s\tAS:i:%d\n" % (i, 16 * (i & 1), CONTIGS[ref][0], pos, ln, seq, qual, ln)))
    out.sort(key=lambda t: t[:2])
    return [ln for _, _, ln in out] + [b"u\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n"]


def test_the_walk_gives_the_offsets_that_were_written():
    recs = bam_oracle.records(lines() + [b""], CONTIGS)
    head = bam_oracle.header(b"@HD\tVN:1.6\n", CONTIGS)
    s = head + b"".join(recs)
    text, contigs, body = ro.parse_header(s)
    assert (text, contigs, body) == (b"@HD\tVN:1.6\n", CONTIGS, len(head))
    assert ro.walk(s, body, 2) == [int(o) + body for o in sorted(set(bam_oracle.offsets(recs).tolist()))]
    assert [s[a:b] for a, b in zip(ro.walk(s, body, 2), ro.walk(s, body, 2)[1:])] == bam_oracle.split_records(s[body:])


def test_reads_give_the_lines_bases_and_qualities_back():
    ls = lines(50)
    recs = bam_oracle.records(ls, CONTIGS)
    s = b"".join(recs)
    off = ro.walk(s, 0, 2)
    got, seq, seq_off, qual, qual_off, src = ro.reads(s, off, 2, flags=0)
    assert src == list(range(len(ls)))
    for r, ln in zip(got, ls):
        f = ln[:-1].split(b"\t")
        assert seq[r["seq_off"]:r["seq_off"] + r["seq_len"]] == f[9] and s[r["id_off"]:r["id_off"] + r["id_len"]] == f[0]
        assert qual[r["qual_off"]:r["qual_off"] + r["qual_len"]] == (b"" if f[10] == b"*" else f[10])
    assert ro.keys(s, off, CONTIGS)[:-1] == [CONTIGS[[c[0] for c in CONTIGS].index(ln.split(b"\t")[2])][1] + int(ln.split(b"\t")[3]) - 1 for ln in ls[:-1]]
    assert ro.keys(s, off, CONTIGS)[-1] == ro.NONE


def test_the_index_in_any_framing_is_the_stored_one_but_for_the_streams_end():
    recs = bam_oracle.records(lines(3000, seed=9), CONTIGS)  # (the last record is unplaced: the index never names the stream's end)
    body = b"".join(recs)
    assert len(body) > 3 * bam_oracle.PAYLOAD
    framed = bam_oracle.frame(body, eof=True)
    rc, block_off, out_off, _ = ic.walk(framed)
    assert rc == 0
    voff = ro.blocks_voff(block_off, out_off)
    assert bai_oracle.build(recs, CONTIGS, voff) == bai_oracle.build(recs, CONTIGS, bai_oracle.stored_voff())
    stored = bai_oracle.stored_voff()
    assert all(voff(o) == stored(o) for o in range(0, len(body), 997))
    k = bam_oracle.PAYLOAD
    assert voff(k) == stored(k) == block_off[1] << 16  # a byte on a block boundary belongs to the block it starts
    assert voff(len(body)) == block_off[-2] << 16  # the end-of-file block ...
    assert stored(len(body)) == (block_off[-3] << 16) | (len(body) % k)  # ... where the closed form stays in the last payload

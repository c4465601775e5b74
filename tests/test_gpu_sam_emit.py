"""SAM records written on the device (`bg_sam_emit_batch[_dev]`) against the CPU statement of the record (tests/sam_oracle.py),
byte for byte and offset for offset: the host flavour on the numpy outputs of the host seed-extend calls, the device flavour on
what `bg_fastq_parse_dev` and the device seed-extend calls left in HBM.  The genomes are those of the neighbouring tests
(`test_gpu_seed_extend_multi.make_case`, `test_gpu_seed_extend_pairs.make_case`) cut into three contigs by two '$', with
reads planted across the first cut.

What the cases hold, counted from the oracle's lines alone before anything is compared (the floors asserted are the ones the
feature was specified with):
  multi case (K = 4, 700 reads)   504 reverse-strand lines, 517 lines whose MD has a '^', 552 lines with an 'I' in CIGAR, 109
                                  lines with 0 < MAPQ < cap, 415 secondary lines (floors 200, 100, 100, 20, 30); all 20 reads
                                  across the cut unplaced
  pairs case (1054 reads)         466 proper pairs, 51 pairs with exactly one mate placed, 12 unplaced boundary hits
                                  (floors 50, 10, 5)"""
import functools

import numpy as np
import pytest
import torch

import sam_oracle as so
from rust_bio_amd import _lib, fastq, sam, synth
from rust_bio_amd.alphabets import dna
from rust_bio_amd.pairwise import Scoring
from rust_bio_amd.pipeline import (MultiParams, PairParams, SeedParams, attach_text, seed_extend_multi_arrays, seed_extend_multi_dev,
                                   seed_extend_pairs_arrays, seed_extend_pairs_dev, seed_extend_strands_arrays, seed_extend_strands_dev)
from test_gpu_pipeline import build
from test_gpu_seed_extend_multi import make_case
from test_gpu_seed_extend_pairs import make_case as make_pairs_case
from test_gpu_seed_extend_pairs import mates_at
from test_sam_host import DTYPES, KATS, contig_list

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID_ARG, OPS_CAP = -1, -9
SC = Scoring.from_scores(-5, -1, 1, -1)
L = 150
POISON = 0xAA
ALL_TAGS = sam.SAM_TAG_NM | sam.SAM_TAG_MD


def cut(g, cuts, names=("chr1", "chr2", "chr3")):
    """the genome as three contigs: a '$' at each cut, the final sentinel behind.  Returns (text, contig entries)."""
    text = np.append(g, np.uint8(ord("$")))
    text[list(cuts)] = ord("$")
    edges = [-1] + list(cuts) + [len(g)]
    return text, [(names[c].encode(), edges[c] + 1, edges[c + 1] - edges[c] - 1) for c in range(3)]


def fastq_text(seqs, ids, seed=1, quals=None):
    """a four-line FASTQ of the reads with random qualities (or the given ones)"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (s, id_) in enumerate(zip(seqs, ids)):
        q = quals[k] if quals and quals[k] is not None else bytes(rng.integers(33, 127, size=len(s)).astype(np.uint8))
        out.append(b"@" + id_ + b"\n" + bytes(s) + b"\n+\n" + q + b"\n")
    return b"".join(out)


def split(flat, off):
    return [flat[int(off[r]):int(off[r + 1])].tobytes() for r in range(len(off) - 1)]


class Batch:
    """one FASTQ text on both sides: parsed by the host call (numpy) and by bg_fastq_parse_dev (left in HBM)"""

    def __init__(self, fm, entries, text, fq_bytes, n_expected):
        self.fm, self.entries, self.text = fm, entries, text.tobytes()
        self.contigs = sam.Contigs(entries)
        self.parsed = fastq.parse_arrays(fq_bytes, ctx=fm.ctx)
        assert self.parsed.status == "ok" and len(self.parsed) == n_expected
        self.n = n_expected
        self.max_len = max(int(self.parsed.recs["seq_len"].max()), 1)
        self.d_fq = torch.frombuffer(bytearray(fq_bytes), dtype=torch.uint8).to(DEV)
        k, status, _, self.d_recs, self.d_seq, self.d_seq_off, self.d_qual, _ = fastq.parse_dev(self.d_fq, ctx=fm.ctx)
        assert (k, status) == (n_expected, "ok")
        self.d_contigs = torch.from_numpy(self.contigs.table.view(np.uint8).copy()).to(DEV)
        self.d_names = torch.from_numpy(self.contigs.names).to(DEV)

    def device_slots(self, K, prm=None):
        """hits, strand and operation slots for a device seed-extend call"""
        stride = 2 * self.max_len + 2 * (prm or SeedParams()).pad + 4
        return (torch.zeros(self.n * K * 96, dtype=torch.uint8, device=DEV), torch.full((self.n * K,), 77, dtype=torch.uint8, device=DEV),
                torch.zeros(self.n * K * stride, dtype=torch.uint8, device=DEV), stride)

    def oracle(self, flags, K, hits, strand, ops, multi=None, pairs=None):
        return so.lines(self.entries, self.parsed, hits, strand, ops, flags, K, multi, pairs, self.text)

    def emit_dev(self, flags, K, d_hits, d_strand, d_ops, d_multi=None, d_pairs=None, cap_delta=0, sizing=False):
        """the device flavour: a sizing call, then the call with an exact-fit cap (+ cap_delta) into a poisoned buffer.
        Returns (text, out_off); checks that nothing behind the total was touched."""
        stream = torch.cuda.current_stream().cuda_stream
        d_off = torch.full((self.n * K + 1,), -1, dtype=torch.int64, device=DEV)
        args = (self.fm, sam.SamParams(flags, K), self.n, self.d_contigs.data_ptr(), len(self.contigs), self.d_names.data_ptr(),
                self.d_fq.data_ptr(), self.d_recs.data_ptr(), self.d_seq.data_ptr(), self.d_qual.data_ptr(), d_hits.data_ptr(),
                d_strand.data_ptr(), d_ops.data_ptr())
        kw = dict(d_multi=d_multi.data_ptr() if d_multi is not None else 0, d_pairs=d_pairs.data_ptr() if d_pairs is not None else 0,
                  stream=stream)
        total = sam.emit_dev(*args, 0, 0, d_off.data_ptr(), **kw)
        torch.cuda.synchronize()
        sized_off = d_off.cpu().numpy().astype(np.uint64)
        assert int(sized_off[-1]) == total
        if sizing:
            return total, sized_off
        d_out = torch.full((total + 64,), POISON, dtype=torch.uint8, device=DEV)
        d_off.fill_(-1)
        if cap_delta < 0:
            with pytest.raises(_lib.BiogpuError) as e:
                sam.emit_dev(*args, d_out.data_ptr(), total + cap_delta, d_off.data_ptr(), **kw)
            torch.cuda.synchronize()
            assert e.value.status == OPS_CAP and (d_out == POISON).all()
            return None, None
        assert sam.emit_dev(*args, d_out.data_ptr(), total + cap_delta, d_off.data_ptr(), **kw) == total
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert (out[total:] == POISON).all()
        off = d_off.cpu().numpy().astype(np.uint64)
        assert (off == sized_off).all()
        return out[:total].tobytes(), off

    def same(self, want, got):
        """the oracle's lines against (text, out_off) of a call"""
        text, off = got
        assert (np.asarray(off) == so.offsets(want)).all()
        if text != b"".join(want):  # name the first line that differs
            for s, w in enumerate(want):
                assert text[int(off[s]):int(off[s + 1])] == w, s
        assert text == b"".join(want)


def fields(line):
    return line[:-1].split(b"\t")


def tag(line, name):
    for t in fields(line)[11:]:
        if t.startswith(name):
            return t[5:]
    return None


@functools.lru_cache(maxsize=None)
def multi_case():
    """make_case's genome cut at 90 000 and 190 000, its 680 reads and 20 reads taken across the first cut"""
    g, _, reads, off, kind = make_case(False)
    text, entries = cut(g, (90_000, 190_000))
    rng = np.random.default_rng(23)
    across = [g[s:s + L].tobytes() for s in 90_000 - rng.integers(20, 130, size=20)]
    seqs = split(reads, off) + across
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    return Batch(fm, entries, text, fastq_text(seqs, [b"r%d" % r for r in range(len(seqs))]), len(seqs))


def test_after_the_strands_call():
    """K = 1, MAPQ 255, every subset of the two tag flags; host and device flavours"""
    B = multi_case()
    p = B.parsed
    hits, strand, ops = seed_extend_strands_arrays(B.fm, SC, p.seq, p.seq_off)
    d_hits, d_strand, d_ops, stride = B.device_slots(1)
    seed_extend_strands_dev(B.fm, SC, B.n, B.d_seq.data_ptr(), B.d_seq_off.data_ptr(), B.max_len, d_hits.data_ptr(), d_strand.data_ptr(),
                            d_ops.data_ptr(), stride, stream=torch.cuda.current_stream().cuda_stream)
    for flags in (0, sam.SAM_TAG_NM, sam.SAM_TAG_MD, ALL_TAGS):
        want = B.oracle(flags, 1, hits, strand, ops)
        assert all(w for w in want) and sum(fields(w)[4] == b"255" for w in want) >= 500
        assert all((tag(w, b"NM:i:") is not None) == bool(flags & sam.SAM_TAG_NM) and
                   (tag(w, b"MD:Z:") is not None) == bool(flags & sam.SAM_TAG_MD) for w in want if tag(w, b"AS:i:") is not None)
        B.same(want, sam.emit_arrays(B.fm, sam.SamParams(flags, 1), B.contigs, p, hits, strand, ops))
        B.same(want, B.emit_dev(flags, 1, d_hits, d_strand, d_ops))


def test_after_the_multi_call():
    """K = 4 with and without secondary lines; XS and MAPQ from the multi records; 16 and 32 lanes per line write the same"""
    B = multi_case()
    p, K, cap = B.parsed, 4, 60
    mp = MultiParams(K, -2**31, cap)
    hits, strand, multi, ops = seed_extend_multi_arrays(B.fm, SC, p.seq, p.seq_off, multi_params=mp)
    want = B.oracle(ALL_TAGS | sam.SAM_SECONDARY, K, hits, strand, ops, multi)
    # the case holds the hard lines (counts in the module docstring)
    ls = [w for w in want if w]
    counts = (sum(int(fields(w)[1]) & 0x10 > 0 for w in ls), sum(b"^" in (tag(w, b"MD:Z:") or b"") for w in ls),
              sum(b"I" in fields(w)[5] for w in ls), sum(0 < int(fields(w)[4]) < cap for w in ls),
              sum(int(fields(w)[1]) & 0x100 > 0 for w in ls))
    print("multi case: reverse, MD with ^, CIGAR with I, 0 < MAPQ < cap, secondary:", counts)
    assert counts[0] >= 200 and counts[1] >= 100 and counts[2] >= 100 and counts[3] >= 20 and counts[4] >= 30, counts
    across = want[4 * 680::4]
    print("multi case: unplaced reads across the cut:", sum(int(fields(w)[1]) & 0x4 > 0 for w in across), "of", len(across))
    assert sum(tag(w, b"XS:i:") is not None for w in ls) >= 100
    d_hits, d_strand, d_ops, stride = B.device_slots(K)
    d_multi = torch.zeros(B.n * 16, dtype=torch.uint8, device=DEV)
    seed_extend_multi_dev(B.fm, SC, B.n, B.d_seq.data_ptr(), B.d_seq_off.data_ptr(), B.max_len, d_hits.data_ptr(), d_multi.data_ptr(),
                          d_strand.data_ptr(), d_ops.data_ptr(), stride, multi_params=mp, stream=torch.cuda.current_stream().cuda_stream)
    for flags in (ALL_TAGS | sam.SAM_SECONDARY, ALL_TAGS, sam.SAM_SECONDARY):
        want = B.oracle(flags, K, hits, strand, ops, multi)
        if not flags & sam.SAM_SECONDARY:
            assert all(not w for s, w in enumerate(want) if s % K) and all(w for w in want[::K])
        B.same(want, sam.emit_arrays(B.fm, sam.SamParams(flags, K), B.contigs, p, hits, strand, ops, multi=multi))
        for lanes in (16, 32):
            B.fm.ctx.set_option("sam_lanes", lanes)
            try:
                B.same(want, B.emit_dev(flags, K, d_hits, d_strand, d_ops, d_multi=d_multi))
            finally:
                B.fm.ctx.set_option("sam_lanes", 0)
    # without the multi records: MAPQ 255 on slot 0, no XS
    want = B.oracle(sam.SAM_SECONDARY, K, hits, strand, ops)
    assert not any(tag(w, b"XS:i:") for w in want if w)
    B.same(want, B.emit_dev(sam.SAM_SECONDARY, K, d_hits, d_strand, d_ops))


@functools.lru_cache(maxsize=None)
def pairs_case():
    """the pairs generator's 500 pairs on its genome cut at 70 000 and 140 000, 15 more pairs with an unmappable mate 2 and 12
    whose mate 1 lies across the first cut"""
    g, _, reads, off, org, rev = make_pairs_case()
    text, entries = cut(g, (70_000, 140_000))
    rng = np.random.default_rng(29)
    lone, _, _ = mates_at(g, rng.integers(1_000, 60_000, size=15), np.full(15, 400), L, 93, np.zeros(15, bool))
    lone[1::2] = synth.random_dna(15 * L, seed=8).reshape(15, L)
    across, _, _ = mates_at(g, 70_000 - rng.integers(30, 120, size=12), np.full(12, 400), L, 94, np.zeros(12, bool), sub=0.01)
    seqs = split(reads, off) + [x.tobytes() for x in lone] + [x.tobytes() for x in across]
    ids = [b"frag%d/%d" % (r // 2, r % 2 + 1) for r in range(len(seqs))]
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    return Batch(fm, entries, text, fastq_text(seqs, ids, seed=2), len(seqs))


def test_after_the_pairs_call():
    B = pairs_case()
    p, pp = B.parsed, PairParams(0, 1000, 17)
    hits, strand, pairs, ops = seed_extend_pairs_arrays(B.fm, SC, p.seq, p.seq_off, pair_params=pp)
    flags = sam.SAM_PAIRED | ALL_TAGS
    want = B.oracle(flags, 1, hits, strand, ops, pairs=pairs)
    f = [fields(w) for w in want]
    flag = np.array([int(x[1]) for x in f])
    proper = int(((flag[0::2] & 0x2) > 0).sum())
    one = int((((flag[0::2] & 0x4) > 0) != ((flag[1::2] & 0x4) > 0)).sum())
    boundary = int(((flag[-24::2] & 0x4) > 0).sum())
    print("pairs case: proper pairs, pairs with one mate placed, unplaced boundary hits:", (proper, one, boundary))
    assert proper >= 50 and one >= 10 and boundary >= 5, (proper, one, boundary)
    assert all(x[0].startswith(b"frag") and b"/" not in x[0] for x in f)
    # |TLEN| is the span of every proper pair, and the mates' TLEN sum to 0
    tlen = np.array([int(x[8]) for x in f])
    assert (tlen[0::2] + tlen[1::2] == 0).all()
    is_proper = (flag[0::2] & 0x2) > 0
    assert (np.abs(tlen[0::2])[is_proper] == pairs["span"][is_proper].astype(np.int64)).all() and (tlen[0::2][is_proper] != 0).all()
    B.same(want, sam.emit_arrays(B.fm, sam.SamParams(flags, 1), B.contigs, p, hits, strand, ops, pairs=pairs))
    d_hits, d_strand, d_ops, stride = B.device_slots(1)
    d_pairs = torch.zeros(B.n // 2 * 16, dtype=torch.uint8, device=DEV)
    seed_extend_pairs_dev(B.fm, SC, B.n // 2, B.d_seq.data_ptr(), B.d_seq_off.data_ptr(), B.max_len, d_hits.data_ptr(), d_pairs.data_ptr(),
                          d_strand.data_ptr(), d_ops.data_ptr(), stride, pair_params=pp, stream=torch.cuda.current_stream().cuda_stream)
    B.same(want, B.emit_dev(flags, 1, d_hits, d_strand, d_ops, d_pairs=d_pairs))
    text, off = B.emit_dev(flags, 1, d_hits, d_strand, d_ops, d_pairs=d_pairs)
    assert (tlen == [int(fields(text[int(off[s]):int(off[s + 1])])[8]) for s in range(B.n)]).all()
    # the same hits read as single reads: no pair fields, /1 and /2 stay
    want = B.oracle(ALL_TAGS, 1, hits, strand, ops)
    assert all(fields(w)[0].endswith((b"/1", b"/2")) and fields(w)[6] == b"*" for w in want)
    B.same(want, B.emit_dev(ALL_TAGS, 1, d_hits, d_strand, d_ops))


def test_ragged_fastq_with_a_long_read():
    """FASTQ in through bg_fastq_parse_dev: ragged reads of 15 - 150 bases, a read of 20 000 bases on the reverse strand (its line
    is longer than the staging area of the write pass: the path straight to global memory), an empty read (the reader takes no record without qualities, so it has two) and a
    record whose qualities are shorter than its sequence.  One seed per 400 bases keeps the long read inside the seed limits."""
    g, _, reads, off, kind = make_case(True)
    text, entries = cut(g, (90_000, 190_000))
    seqs = split(reads, off)[300:560]
    long_read = g[100_000:120_000].copy()
    long_read[np.arange(50, 20_000, 97)] = ord("A")
    long_read = np.delete(long_read, [7_000, 7_001])
    long_read = np.insert(long_read, 12_000, [ord("C"), ord("C"), ord("G")])
    long_read = dna.revcomp(long_read.tobytes())[:20_000]
    seqs = seqs[:100] + [long_read] + seqs[100:200] + [b""] + seqs[200:] + [g[5_000:5_100].tobytes()]
    quals = [None] * len(seqs)
    quals[-1] = b"I" * 60
    quals[201] = b"II"  # (the reader takes no record without qualities: fastq.rs:298-300)
    sa, b, ls, fm = build(text, 8)
    attach_text(fm, text)
    B = Batch(fm, entries, text, fastq_text(seqs, [b"q%d" % r for r in range(len(seqs))], quals=quals), len(seqs))
    assert B.max_len == 20_000 and int(B.parsed.recs["check"][-1]) == 5
    prm = SeedParams(20, 400, 16, 25)
    hits, strand, ops = seed_extend_strands_arrays(B.fm, SC, B.parsed.seq, B.parsed.seq_off, params=prm)
    want = B.oracle(ALL_TAGS, 1, hits, strand, ops)
    long_line, empty_line, short_qual = fields(want[100]), fields(want[201]), fields(want[-1])
    print("ragged case: the long read's FLAG, POS, line bytes:", long_line[1], long_line[3], len(want[100]),
          "placed lines:", sum(tag(w, b"AS:i:") is not None for w in want))
    assert len(want[100]) > 40_000 and empty_line[9:11] == [b"*", b"*"] and short_qual[10] == b"*" and len(short_qual[9]) == 100
    # (a read maps when its one seed, the first 20 bases, carries no mutation: about a third of the 245 reads of 20 bases or more)
    assert sum(tag(w, b"AS:i:") is not None for w in want) >= 40
    B.same(want, sam.emit_arrays(B.fm, sam.SamParams(ALL_TAGS, 1), B.contigs, B.parsed, hits, strand, ops))
    d_hits, d_strand, d_ops, stride = B.device_slots(1, prm)
    seed_extend_strands_dev(B.fm, SC, B.n, B.d_seq.data_ptr(), B.d_seq_off.data_ptr(), B.max_len, d_hits.data_ptr(), d_strand.data_ptr(),
                            d_ops.data_ptr(), stride, prm, stream=torch.cuda.current_stream().cuda_stream)
    for lanes in (16, 32):
        B.fm.ctx.set_option("sam_lanes", lanes)
        try:
            B.same(want, B.emit_dev(ALL_TAGS, 1, d_hits, d_strand, d_ops))
        finally:
            B.fm.ctx.set_option("sam_lanes", 0)
    fm.close()


def test_long_placed_lines():
    """hand-made hits: a placed read of 30 000 bases whose CIGAR and MD alone exceed the staging area of the write pass, and
    lines of every length around the staging size (1024 bytes), on both strands"""
    B = multi_case()
    reads, hits = [], []
    for n, at in [(30_000, 100_000)] + [(n, 1_000 + 600 * (n - 300)) for n in range(300, 380)]:
        ops = np.zeros(n, dtype=np.uint8)
        ops[np.arange(3, n, 7)] = 1
        ops[np.arange(40, n - 40, 211)] = 2
        ops[np.arange(41, n - 40, 211)] = 2
        ops[np.arange(90, n - 40, 333)] = 3
        s = "".join("=XDI"[o] for o in ops)
        qlen, rlen = int(np.isin(ops, (0, 1, 3)).sum()), int(np.isin(ops, (0, 1, 2)).sum())
        seq = bytes(np.random.default_rng(n).choice(np.frombuffer(b"ACGTN", np.uint8), size=qlen + 5))
        reads.append({"id": "long%d" % n, "seq": seq.decode(), "qual": "".join(chr(33 + k % 90) for k in range(len(seq)))})
        hits.append({"score": -n, "strand": n % 2, "ref_start": at, "ref_end": at + rlen, "xstart": 2, "xend": 2 + qlen, "xlen": qlen + 5,
                     "ops": s})
    kat = {"flags": ["NM", "MD"], "K": 1, "reads": reads, "hits": hits}
    flags, K, fq, h, strand, ops, _, _ = so.kat_arrays(kat, *DTYPES)
    want = so.lines(B.entries, fq, h, strand, ops, flags, K, None, None, B.text)
    sizes = sorted(len(w) for w in want)
    assert sizes[-1] > 60_000 and all(tag(w, b"MD:Z:") for w in want) and sizes[0] < 1000 and sizes[-2] > 1100, sizes
    for lanes in (16, 32):
        B.fm.ctx.set_option("sam_lanes", lanes)
        try:
            B.same(want, sam.emit_arrays(B.fm, sam.SamParams(flags, K), B.contigs, fq, h, strand, ops))
        finally:
            B.fm.ctx.set_option("sam_lanes", 0)


def test_hand_written_records():
    """the records of tests/golden/sam_kats.json on an index of their own 42-byte text"""
    text = np.frombuffer(KATS["text"].encode(), np.uint8)
    sa, b, ls, fm = build(text, 0)
    attach_text(fm, text)
    contigs = sam.Contigs(contig_list(KATS["contigs"]))
    done = 0
    for kat in KATS["records"]:
        flags, K, fq, h, strand, ops, multi, pairs = so.kat_arrays(kat, *DTYPES)
        want = [e.encode() for e in kat["expect"]]
        text_out, off = sam.emit_arrays(fm, sam.SamParams(flags, K), contigs, fq, h, strand, ops, multi=multi, pairs=pairs)
        assert text_out == b"".join(want) and (off == so.offsets(want)).all(), kat["name"]
        done += bool(flags & sam.SAM_TAG_MD)
    assert done >= 4
    fm.close()


def test_sizing_caps_and_arguments():
    B = multi_case()
    p = B.parsed
    hits, strand, ops = seed_extend_strands_arrays(B.fm, SC, p.seq, p.seq_off)
    d_hits, d_strand, d_ops, stride = B.device_slots(1)
    seed_extend_strands_dev(B.fm, SC, B.n, B.d_seq.data_ptr(), B.d_seq_off.data_ptr(), B.max_len, d_hits.data_ptr(), d_strand.data_ptr(),
                            d_ops.data_ptr(), stride, stream=torch.cuda.current_stream().cuda_stream)
    want = B.oracle(ALL_TAGS, 1, hits, strand, ops)
    # the sizing call reports the later call's total; a larger cap is fine; one byte short writes nothing
    total, off = B.emit_dev(ALL_TAGS, 1, d_hits, d_strand, d_ops, sizing=True)
    assert total == sum(len(w) for w in want) and (off == so.offsets(want)).all()
    B.same(want, B.emit_dev(ALL_TAGS, 1, d_hits, d_strand, d_ops, cap_delta=17))
    B.emit_dev(ALL_TAGS, 1, d_hits, d_strand, d_ops, cap_delta=-1)
    d_off = torch.zeros(8 * B.n + 1, dtype=torch.int64, device=DEV)
    d_out = torch.full((total,), POISON, dtype=torch.uint8, device=DEV)
    d_pairs = torch.zeros(B.n * 16, dtype=torch.uint8, device=DEV)

    def call(flags, K, n=B.n, n_contigs=len(B.contigs), pairs=0, fm=B.fm):
        return sam.emit_dev(fm, sam.SamParams(flags, K), n, B.d_contigs.data_ptr(), n_contigs, B.d_names.data_ptr(), B.d_fq.data_ptr(),
                            B.d_recs.data_ptr(), B.d_seq.data_ptr(), B.d_qual.data_ptr(), d_hits.data_ptr(), d_strand.data_ptr(),
                            d_ops.data_ptr(), d_out.data_ptr(), total, d_off.data_ptr(), d_pairs=pairs)
    assert call(ALL_TAGS, 1) == total
    bad = [dict(flags=0, K=0), dict(flags=0, K=9), dict(flags=0, K=1, n_contigs=0), dict(flags=16, K=1),
           dict(flags=sam.SAM_PAIRED, K=1, n=B.n - 1, pairs=d_pairs.data_ptr()), dict(flags=sam.SAM_PAIRED, K=2, pairs=d_pairs.data_ptr()),
           dict(flags=sam.SAM_PAIRED, K=1)]
    assert B.n % 2 == 0
    for kw in bad:
        with pytest.raises(_lib.BiogpuError) as e:
            call(**kw)
        assert e.value.status == INVALID_ARG, kw
    # MD needs the text
    sa, b, ls, bare = build(np.frombuffer(KATS["text"].encode(), np.uint8), 0)
    with pytest.raises(_lib.BiogpuError) as e:
        call(sam.SAM_TAG_MD, 1, fm=bare)
    assert e.value.status == INVALID_ARG
    bare.close()
    torch.cuda.synchronize()

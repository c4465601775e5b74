"""Seed-and-extend seeded with the SMEMs of an FMD index (`bg_seed_extend_smem_batch[_dev]`) against its CPU statement
(tests/smem_seed_oracle.py: all_smems, the suffix array of T$R$ and Aligner::semiglobal of the oracle): every hit field, the
strand and the winner's operations, read by read.  Genomes of 30 kbp, `full_text` as in tests/fmd_cases.py."""
import functools

import numpy as np
import pytest
import torch

import fmd_cases as fc
import oracle_py as orc
import sam_oracle as so
import smem_seed_oracle as sso
from rust_bio_amd import _lib, sam
from rust_bio_amd.bwt import Occ, bwt, less
from rust_bio_amd.fmindex import FMIndex
from rust_bio_amd.pairwise import MIN_SCORE, Scoring
from rust_bio_amd.pipeline import (SeedParams, SmemSeedParams, attach_text, seed_extend_smem_arrays, seed_extend_smem_dev,
                                   seed_extend_strands_arrays)
from rust_bio_amd.suffix_array import RawSuffixArray, SampledSuffixArray, suffix_array

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID_ARG, OUT_OF_ALPHABET, OPS_CAP, UNSUPPORTED = -1, -7, -9, -11
F, R, NONE = sso.HIT_FORWARD, sso.HIT_REVERSE, sso.HIT_NONE
SCORES = (-5, -1, 1, -1)
SC = Scoring.from_scores(*SCORES)
PRM = dict(min_seed_len=19, max_smems=16, max_occ=16, pad=25)
GENOME = fc.random_dna(30_000, 41)


@functools.lru_cache(maxsize=None)
def tables(fwd):
    """T$R$ and the oracle's index over it: (text array, suffix array, BWT, less, oracle FMDIndex)"""
    text = np.frombuffer(fc.full_text(fwd), np.uint8)
    sa = np.asarray(orc.suffix_array(text), np.uint64)
    b = np.frombuffer(bytes(orc.bwt(text, sa)), np.uint8)
    ls = np.asarray(orc.less(b, fc.ALPHA), np.uint64)
    return text, sa, b, ls, orc.FMDIndex(b, ls, orc.Occ(b, 3, fc.ALPHA))


def device_index(fwd, sampled=0, ctx=None, with_text=True, with_sa=True):
    text, sa, b, ls, _ = tables(fwd)
    fm = FMIndex(b, ls, Occ(b, 3, fc.ALPHA), ctx=ctx)
    if with_sa and sampled:
        SampledSuffixArray(sa, text, b, sampled, fmindex=fm)
    elif with_sa:
        RawSuffixArray(sa, fm)
    if with_text:
        attach_text(fm, text)
    return fm


def oracle(fwd, buf, off, **kw):
    text, sa, _, _, ofmd = tables(fwd)
    prm = dict(PRM)
    prm.update(kw)
    return sso.candidates(orc, ofmd, sa, np.frombuffer(fwd, np.uint8), orc.make_scoring(*SCORES), buf, off, **prm)


def mixed_reads(n, seed, lo=100, hi=150):
    """reads of lo ..= hi bases from GENOME: exact, with substitutions, with one indel, with both; every odd one reverse
    complemented; every 20th a chimera; the first ones at the ends of T, the last ones random.  Returns (reads, truth starts)"""
    rng = np.random.default_rng(seed)
    reads, starts = [], []
    for r in range(n):
        L = int(rng.integers(lo, hi + 1))
        s = 0 if r == 0 else len(GENOME) - L if r == 1 else int(rng.integers(0, len(GENOME) - L))
        piece = GENOME[s:s + L]
        if r % 4 in (1, 3):
            piece = fc.substituted(piece, int(rng.integers(21, 40)))
        if r % 4 in (2, 3):
            at = int(rng.integers(30, L - 30))
            piece = piece[:at] + piece[at + 2:] if r % 8 < 4 else piece[:at] + b"GA" + piece[at:]
        if r % 20 == 10:  # a chimera of three loci, the middle one from the other strand: candidates on both strands
            a, b = (int(v) for v in rng.integers(0, len(GENOME) - 50, size=2))
            piece = GENOME[s:s + 45] + fc.revcomp(GENOME[a:a + 40]) + GENOME[b:b + 35]
        if r >= n - 6:
            piece = fc.random_dna(L, 1000 + r)
        reads.append(fc.revcomp(piece) if r % 2 else piece)
        starts.append(s)
    return reads, starts


@functools.lru_cache(maxsize=None)
def parity_case():
    reads, _ = mixed_reads(200, 7)
    buf, off = fc.concat(reads)
    return buf, off, oracle(GENOME, buf, off)


def smem_call(fm, buf, off, strands=3, **kw):
    allow = {k: kw.pop(k) for k in ("allow_truncated", "allow_out_of_alphabet") if k in kw}
    prm = dict(PRM)
    prm.update(kw)
    return seed_extend_smem_arrays(fm, SC, buf, off, SmemSeedParams(**prm), strands=strands, **allow)


def dev_call(fm, buf, off, strands=3, stride_delta=0, **kw):
    """the device flavour with every optional output: (hits, strand, ops slots, stride, totals)"""
    prm = dict(PRM)
    prm.update(kw)
    n, max_len = len(off) - 1, int(np.diff(off).max())
    stride = 2 * max_len + 2 * prm["pad"] + 4 + stride_delta
    d_reads = torch.from_numpy(buf.copy()).to(DEV)
    d_off = torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_hits = torch.full((n * 96,), 0x5A, dtype=torch.uint8, device=DEV)
    d_strand = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
    d_ops = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    tot = np.zeros(2, dtype=np.uint64)
    try:
        seed_extend_smem_dev(fm, SC, n, d_reads.data_ptr(), d_off.data_ptr(), max_len, d_hits.data_ptr(), d_strand.data_ptr(),
                             d_ops.data_ptr(), stride, SmemSeedParams(**prm), strands, torch.cuda.current_stream().cuda_stream, tot)
    finally:
        torch.cuda.synchronize()
    return d_hits.cpu().numpy().view(_lib.SEED_HIT_DTYPE), d_strand.cpu().numpy(), d_ops.cpu().numpy(), stride, tot, d_hits


@pytest.mark.parametrize("sampled", [0, 8])
def test_parity_with_the_oracle(sampled):
    """200 ragged reads of 100 - 150 bases, half of them reverse complemented, some with substitutions and an indel"""
    buf, off, res = parity_case()
    want = sso.expected(res)
    fm = device_index(GENOME, sampled)
    hits, strand, ops = smem_call(fm, buf, off)
    sso.compare(hits, strand, ops, want, sampled)
    st, nc = np.array([w[0] for w in want]), np.array([w[2] for w in want])
    plain = (np.arange(200) % 20 != 10) & (np.arange(200) < 194)
    assert (st[plain] == np.arange(200)[plain] % 2).all() and (st[194:] == NONE).all()  # every kind of read on its own strand
    assert (nc[10:194:20] == 3).all() and not res["truncated"].any()  # the chimeras: two forward candidates and a reverse one
    fm.close()


def test_reads_no_fixed_window_survives():
    """150-base reads with a substitution at 15, 35, 55, ...: every window [10 j, 10 j + 20) holds one, so the fixed-seed call
    (20 / 10 / 16 / 25, forward index of T) places none at its locus; the 19-base stretches between them are SMEMs"""
    rng = np.random.default_rng(3)
    starts = rng.integers(0, len(GENOME) - 150, size=32)
    rev = np.arange(32) % 2 == 1
    reads = []
    for s, rv in zip(starts, rev):
        piece = fc.substituted(GENOME[int(s):int(s) + 150], 20, start=15)
        reads.append(fc.revcomp(piece) if rv else piece)
    buf, off = fc.concat(reads)
    want_strand = np.where(rev, R, F)
    # the existing call on a forward index of T
    t = np.frombuffer(GENOME + b"$", np.uint8)
    sa = suffix_array(t)
    b = bwt(t, sa)
    alpha = b"ACGTNacgtn$"
    plain = FMIndex(b, less(b, alpha), Occ(b, 64, alpha))
    SampledSuffixArray(sa, t, b, 8, fmindex=plain)
    attach_text(plain, t)
    fh, fs, _ = seed_extend_strands_arrays(plain, SC, buf, off, SeedParams(20, 10, 16, 25))
    assert not ((fh["ref_start"] == starts) & (fs == want_strand)).any()
    plain.close()
    # the SMEM call
    fm = device_index(GENOME, 8)
    hits, strand, ops = smem_call(fm, buf, off)
    assert (hits["ref_start"] == starts).all() and (hits["ref_end"] == starts + 150).all() and (strand == want_strand).all()
    assert (hits["aln"]["score"] == 150 - 2 * 7).all()
    sso.compare(hits, strand, ops, sso.expected(oracle(GENOME, buf, off)))
    fm.close()


def test_one_strand_at_a_time_and_the_reads_reverse_complements():
    buf, off, both = parity_case()
    fm = device_index(GENOME, 0)
    for strands in (sso.STRAND_FORWARD, sso.STRAND_REVERSE):
        res = oracle(GENOME, buf, off, strands=strands)
        hits, strand, ops = smem_call(fm, buf, off, strands=strands)
        sso.compare(hits, strand, ops, sso.expected(res), strands)
        assert set(strand.tolist()) == {strands - 1, NONE}
    # revcomp(reads): the same loci with the strands swapped, on the reads with one candidate (a unique best on either strand)
    rc = np.concatenate([np.frombuffer(fc.revcomp(buf[int(off[r]):int(off[r + 1])].tobytes()), np.uint8) for r in range(len(off) - 1)])
    hits, strand, ops = smem_call(fm, buf, off)
    rhits, rstrand, rops = smem_call(fm, rc, off)
    one = (hits["n_candidates"] == 1) & (rhits["n_candidates"] == 1)
    assert one.sum() > 150 and (hits["n_candidates"] == rhits["n_candidates"]).all()
    for f in ("ref_start", "ref_end", "window_start"):
        assert (hits[f][one] == rhits[f][one]).all(), f
    assert (hits["aln"]["score"][one] == rhits["aln"]["score"][one]).all()
    assert (strand[one] == 1 - rstrand[one]).all()
    fm.close()


def chimeras():
    """chimeric reads of six 25-base pieces from six loci (six records each) among ordinary reads"""
    rng = np.random.default_rng(17)
    reads, _ = mixed_reads(40, 19)
    for k in range(12):
        loci = rng.integers(0, len(GENOME) - 25, size=6)
        chim = b"".join(GENOME[int(s):int(s) + 25] for s in loci)
        reads.insert(3 * k + 1, fc.revcomp(chim) if k % 2 else chim)
    return fc.concat(reads)


def test_truncation_to_max_smems():
    buf, off = chimeras()
    res = oracle(GENOME, buf, off, max_smems=4)
    assert res["truncated"].sum() >= 12 and (~res["truncated"]).sum() >= 30
    fm = device_index(GENOME, 0)
    with pytest.raises(_lib.BiogpuError) as e:
        smem_call(fm, buf, off, max_smems=4)
    assert e.value.status == OPS_CAP
    hits, strand, ops = smem_call(fm, buf, off, max_smems=4, allow_truncated=True)
    sso.compare(hits, strand, ops, sso.expected(res))
    # with room for every record the call is clean, and the chimeras have more candidates
    full = oracle(GENOME, buf, off)
    assert not full["truncated"].any()
    hits16, strand16, ops16 = smem_call(fm, buf, off)
    sso.compare(hits16, strand16, ops16, sso.expected(full))
    assert (hits16["n_candidates"] >= hits["n_candidates"]).all()
    assert (hits16["n_candidates"][1:36:3] > hits["n_candidates"][1:36:3]).all()  # the chimeras
    # a read the reference panics on in the same batch: that status comes first
    bad, boff = fc.concat([buf[int(off[r]):int(off[r + 1])].tobytes() for r in range(len(off) - 1)] + [fc.with_byte(GENOME[50:150], 40, 0xFF)])
    with pytest.raises(_lib.AlphabetError):
        smem_call(fm, bad, boff, max_smems=4, allow_truncated=True)
    fm.close()


def test_max_occ():
    """a 200-base segment planted five times: reads inside it do not vote with max_occ = 4 and propose all five copies with 8"""
    seg = GENOME[29_000:29_200]
    g = bytearray(GENOME[:25_000])
    at = [2_000, 7_000, 12_000, 17_000, 22_000]
    for a in at:
        g[a:a + 200] = seg
    g = bytes(g)
    reads = [seg[o:o + 100] for o in (0, 37, 100)] + [fc.revcomp(seg[20:140]), g[500:620]]
    buf, off = fc.concat(reads)
    fm = device_index(g, 8)
    lo, lo_strand, lo_ops = smem_call(fm, buf, off, max_occ=4)
    assert (lo["n_candidates"][:4] == 0).all() and (lo_strand[:4] == NONE).all() and (lo["n_seed_hits"][:4] == 0).all()
    assert lo["n_candidates"][4] == 1 and lo["ref_start"][4] == 500
    hi, hi_strand, hi_ops = smem_call(fm, buf, off, max_occ=8)
    assert (hi["n_candidates"][:4] == 5).all() and (hi["n_seed_hits"][:4] == 5).all()
    assert (hi["ref_start"][:3] == [at[0], at[0] + 37, at[0] + 100]).all() and hi_strand[3] == R and hi["ref_start"][3] == at[0] + 20
    for got, occ in (((lo, lo_strand, lo_ops), 4), ((hi, hi_strand, hi_ops), 8)):
        sso.compare(*got, sso.expected(oracle(g, buf, off, max_occ=occ)), occ)
    fm.close()


def test_out_of_alphabet_and_foreign_bytes():
    """0xFF and z lie beyond `less`: the reference panics, K7 reports count 0xFFFFFFFF, the read is unmapped and the call says so;
    N, lower case and '$' in a read do not panic and follow the rule"""
    base = [GENOME[1_000 + 300 * k:1_100 + 300 * k] for k in range(12)]
    reads = list(base)
    reads[2] = fc.with_byte(base[2], 40, 0xFF)
    reads[7] = fc.revcomp(fc.with_byte(base[7], 99, ord("z")))
    reads[3] = fc.with_byte(base[3], 50, ord("N"))
    reads[4] = base[4][:30] + base[4][30:60].lower() + base[4][60:]
    reads[5] = fc.with_byte(base[5], 45, ord("$"))
    reads[6] = fc.revcomp(fc.with_byte(base[6], 0, ord("$")))
    reads[8] = GENOME[-60:] + b"$" + fc.revcomp(GENOME)[:39]  # T's tail, the sentinel and R's head: a match across the sentinel
    buf, off = fc.concat(reads)
    res = oracle(GENOME, buf, off)
    assert list(np.nonzero(res["panicked"])[0]) == [2, 7]
    fm = device_index(GENOME, 0)
    with pytest.raises(_lib.AlphabetError) as e:
        smem_call(fm, buf, off)
    assert e.value.status == OUT_OF_ALPHABET
    hits, strand, ops = smem_call(fm, buf, off, allow_out_of_alphabet=True)
    sso.compare(hits, strand, ops, sso.expected(res))
    assert strand[2] == NONE and strand[7] == NONE and hits["n_seed_hits"][2] == 0
    clean_buf, clean_off = fc.concat(base)
    chits, cstrand, _ = smem_call(fm, clean_buf, clean_off)
    keep = np.array([0, 1, 9, 10, 11])
    for f in ("ref_start", "ref_end", "n_candidates", "n_seed_hits"):
        assert (hits[f][keep] == chits[f][keep]).all(), f
    assert (strand[keep] == cstrand[keep]).all() and (strand[[3, 4, 5]] == F).all() and strand[6] == R
    fm.close()


@functools.lru_cache(maxsize=None)
def device_case():
    reads, _ = mixed_reads(520, 29)
    buf, off = fc.concat(reads)
    return buf, off, oracle(GENOME, buf, off)


@pytest.mark.parametrize("chunk", [0, 256, 999])
def test_device_flavour_slots_totals_and_passes(chunk):
    buf, off, res = device_case()
    want = sso.expected(res)
    fm = device_index(GENOME, 8)
    fm.ctx.set_option("seed_chunk_reads", chunk)
    try:
        hits, strand, ops, stride, tot, _ = dev_call(fm, buf, off)
    finally:
        fm.ctx.set_option("seed_chunk_reads", 0)
    n = len(off) - 1
    assert (hits["aln"]["ops_off"] == (np.arange(n) + 1) * stride - hits["aln"]["n_ops"]).all()
    sso.compare(hits, strand, ops, want, chunk)
    assert int(tot[0]) == res["rows"] and int(tot[1]) == sum(w[2] for w in want)
    if chunk == 0:  # an operation slot one byte short: refused before anything is launched
        with pytest.raises(_lib.BiogpuError) as e:
            short = dev_call(fm, buf, off, stride_delta=-1)
        assert e.value.status == OPS_CAP
        d_hits = torch.full((n * 96,), 0x5A, dtype=torch.uint8, device=DEV)
        d_reads, d_off = torch.from_numpy(buf.copy()).to(DEV), torch.from_numpy(off.astype(np.int64)).to(DEV)
        d_ops = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
        with pytest.raises(_lib.BiogpuError):
            seed_extend_smem_dev(fm, SC, n, d_reads.data_ptr(), d_off.data_ptr(), int(np.diff(off).max()), d_hits.data_ptr(), 0,
                                 d_ops.data_ptr(), stride - 1, SmemSeedParams(**PRM), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (d_hits == 0x5A).all()
    fm.close()


def test_wide_layout_gives_the_same_answers():
    """fm_wide_from lowered: the same index on 64-bit positions (fm_wide.hip, proposals sorted as uint64 keys)"""
    buf, off, res = parity_case()
    narrow = device_index(GENOME, 8)
    hits, strand, ops = smem_call(narrow, buf, off)
    narrow.close()
    for sampled in (0, 8):
        ctx = _lib.Context(0)
        ctx.set_option("fm_wide_from", 1)
        ctx.set_option("fm_wide_sb_shift", 2)
        wide = device_index(GENOME, sampled, ctx=ctx)
        whits, wstrand, wops = smem_call(wide, buf, off)
        assert whits.tobytes() == hits.tobytes() and (wstrand == strand).all() and wops.tobytes() == ops.tobytes()
        wide.close()
    sso.compare(hits, strand, ops, sso.expected(res))


def test_arguments():
    reads, _ = mixed_reads(8, 5)
    buf, off = fc.concat(reads)

    def refused(fm, status, strands=3, **kw):
        with pytest.raises(_lib.BiogpuError) as e:
            smem_call(fm, buf, off, strands=strands, **kw)
        assert e.value.status == status, (kw, strands, e.value.status)
        with pytest.raises(_lib.BiogpuError) as e:
            got = dev_call(fm, buf, off, strands=strands, **kw)
        assert e.value.status == status, (kw, strands, e.value.status)

    fm = device_index(GENOME, 8)
    for zero in ("min_seed_len", "max_smems", "max_occ"):
        refused(fm, INVALID_ARG, **{zero: 0})
    refused(fm, UNSUPPORTED, max_smems=41, max_occ=25)  # 1025 proposals per read
    smem_call(fm, buf, off, max_smems=32, max_occ=32)   # 1024 are fine
    for strands in (0, 4):
        refused(fm, INVALID_ARG, strands=strands)
    fm.close()
    for kw in (dict(with_text=False), dict(with_sa=False)):
        bare = device_index(GENOME, 0, **kw)
        refused(bare, INVALID_ARG)
        bare.close()
    # a plain FM index of T$: an odd number of symbols
    t = np.frombuffer(GENOME + b"$", np.uint8)
    sa = suffix_array(t)
    b = bwt(t, sa)
    plain = FMIndex(b, less(b, fc.ALPHA + b"$"), Occ(b, 64, fc.ALPHA + b"$"))
    RawSuffixArray(sa, plain)
    attach_text(plain, t)
    refused(plain, INVALID_ARG)
    plain.close()
    # an index whose BWT is not a word over the DNA alphabet with N and '$': no FMD index (the check K7 makes)
    alpha = bytes(sorted(b"ACGTR"))
    t = np.frombuffer(GENOME[:999].replace(b"A", b"R", 5) + b"$" + GENOME[:999] + b"$", np.uint8)
    sa = suffix_array(t)
    b = bwt(t, sa)
    other = FMIndex(b, less(b, alpha), Occ(b, 64, alpha))
    RawSuffixArray(sa, other)
    attach_text(other, t)
    refused(other, UNSUPPORTED)
    other.close()


def test_sam_records_of_the_hits():
    """bg_sam_emit_batch on the call's hits with T as the one contig equals the SAM statement on the oracle's hits"""
    from rust_bio_amd import fastq
    buf, off, res = parity_case()
    n = len(off) - 1
    seqs = [buf[int(off[r]):int(off[r + 1])].tobytes() for r in range(n)]
    rng = np.random.default_rng(1)
    fq = b"".join(b"@r%d\n" % r + s + b"\n+\n" + bytes(rng.integers(33, 127, size=len(s)).astype(np.uint8)) + b"\n" for r, s in enumerate(seqs))
    fm = device_index(GENOME, 8)
    parsed = fastq.parse_arrays(fq, ctx=fm.ctx)
    assert parsed.status == "ok" and len(parsed) == n
    entries = [(b"chr1", 0, len(GENOME))]
    hits, strand, ops = seed_extend_smem_arrays(fm, SC, parsed.seq, parsed.seq_off, SmemSeedParams(**PRM))
    ohits, ostrand, oops = sso.to_arrays(sso.expected(res), _lib.SEED_HIT_DTYPE)
    flags = sam.SAM_TAG_NM | sam.SAM_TAG_MD
    want = so.lines(entries, parsed, ohits, ostrand, oops, flags, 1, None, None, fc.full_text(GENOME))
    text, out_off = sam.emit_arrays(fm, sam.SamParams(flags, 1), sam.Contigs(entries), parsed, hits, strand, ops)
    assert (np.asarray(out_off) == so.offsets(want)).all() and text == b"".join(want)
    assert sum(w.split(b"\t")[1] == b"16" for w in want) > 80 and sum(w.split(b"\t")[1] == b"4" for w in want) == 6
    fm.close()

"""The `*_dev` entry points of the format layer one after the other on ONE fresh context, so that a call finds the scratch
buffers (ctx->aux, ctx->tb, ctx->bnd) as a different call left them.  Every entry point lays its arrays out with the carver
(csrc/bg_carve.h through bg_reserve_carved); a layout bound before its reserve, or measured a few bytes short, shows only when a
call has to grow a buffer that an earlier call left just too small, or runs in one that another call left larger.

Two passes over the same steps.  The first goes from the smallest case of every family to the largest, so that calls keep
growing the buffers; the second goes back in reverse order, so that every call runs in buffers left larger by another.  The
families and their cases are those of the per-feature tests, at those tests' sizes: FASTQ trim -> filter -> emit
(fastq_write_cases; the reader in front of them keeps its own hand-written layout and is not part of this), SAM duplicate
marking, keys and sort (sam_sort_cases, sam_edge_cases), BAM records / reads / index (bam_read_cases, bai_cases), BGZF blocks /
inflate / deflate (bgzf_inflate_cases, bgzf_deflate_cases), pileup / sites / indels (bam_pileup_cases, bam_sites_cases,
bam_indels_cases: up to a few hundred records over several tiles).  A step is the per-feature test's own checked call: its
result is held to that test's oracle in both passes, and where the call hands the device's bytes back, the second pass must
give the bytes of the first."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

import bai_cases as bc
import bai_oracle as ba
import bam_indels_cases as ic
import bam_pileup_cases as pc
import bam_read_cases as rc
import bam_read_oracle as ro
import bam_sites_cases as sc
import bgzf_deflate_cases as dc
import bgzf_inflate_cases as zc
import bam_oracle as bo
import myers_oracle as mo
import sam_edge_cases as ec
import sam_sort_oracle as sso
import test_gpu_bam_indels as t_indels
import test_gpu_bam_index as t_index
import test_gpu_bam_pileup as t_pileup
import test_gpu_bam_reads as t_reads
import test_gpu_bam_records as t_records
import test_gpu_bam_sites as t_sites
import test_gpu_bgzf_deflate as t_deflate
import test_gpu_bgzf_inflate as t_inflate
import test_gpu_fastq_emit as t_emit
import test_gpu_fastq_filter as t_filter
import test_gpu_fastq_trim as t_trim
import test_gpu_sam_markdup as t_markdup
import test_gpu_sam_sort as t_sort
from fastq_write_cases import Batch, random_records
from rust_bio_amd import _lib, bam, myers, sam
from sam_sort_cases import LINE_LENGTHS, random_batch, synthetic_lines

pytestmark = pytest.mark.gpu
RANKS = 3  # cases a family: its smallest, one in the middle, its largest


def three(items, size):
    """the smallest, the median and the largest of `items` by `size`"""
    items = sorted(items, key=size)
    return [items[0], items[len(items) // 2], items[-1]]


def fastq_steps():
    out = []
    for rank, n in enumerate((3, 300, 2049)):
        batch = Batch(random_records(random.Random(70 + n), n, 1, 40, equal=1.0))
        # hits as the matcher leaves them: none, or a match somewhere in the read (or just beyond it), in either of two patterns
        rng = np.random.default_rng(75 + n)
        hits = np.zeros(2 * n, dtype=_lib.ALN_DTYPE)
        hits["score"] = np.where(rng.random(2 * n) < 0.5, mo.MIN_SCORE, 1)
        hits["ystart"] = rng.integers(0, 30, 2 * n)
        hits["yend"] = hits["ystart"] + rng.integers(0, 15, 2 * n)
        cols = SimpleNamespace(recs=batch.recs, seq=np.frombuffer(batch.seq, np.uint8), seq_off=batch.seq_off,
                               qual=np.frombuffer(batch.qual, np.uint8), qual_off=batch.qual_off)

        def trim(cols=cols, hits=hits, mode=(mo.TRIM_3P, mo.TRIM_5P)[rank & 1]):
            got = myers.trim(mode, hits, 2, cols.recs, cols.seq, cols.seq_off, cols.qual, cols.qual_off)
            t_trim.same_columns(got, t_trim.expected(mode, hits, 2, cols))
            return [np.asarray(g).tobytes() for g in got]

        out += [(rank, "fastq trim %d" % n, trim),
                (rank, "fastq filter %d" % n, lambda batch=batch: [np.asarray(c).tobytes() for c in t_filter.filter_checked(batch, min_len=10, max_n=2)]),
                (rank, "fastq emit %d" % n, lambda batch=batch: t_emit.emit_checked(batch, shift=3))]
    return out


def sam_steps():
    out = []
    for rank, n in enumerate((2, 256, 2800)):
        fq, hits, strand = random_batch(random.Random(80 + n), n, paired=True)
        out.append((rank, "sam markdup %d" % n, lambda a=(fq, hits, strand): [x if isinstance(x, list) else np.asarray(x).tobytes() for x in
                                                                              t_markdup.check(*a, flags=sam.SAM_PAIRED)]))
    for rank, b in enumerate(three(ec.key_batches(), lambda b: b.n * b.K)):
        def keys(b=b):
            got = sam.sort_keys_arrays(sam.SamParams(b.flags, b.K), sam.Contigs(b.contigs), b.n, b.hits, b.strand)
            assert (got == sso.sort_keys(b.contigs, b.hits, b.strand, b.flags, b.K)).all()
            return got.tobytes()
        out.append((rank, "sam keys " + b.name, keys))
    for rank, (n, long_at) in enumerate(((1, None), (40, None), (600, 311))):
        rng = random.Random(90 + n)
        recs, _, _ = synthetic_lines(rng, n, lengths=LINE_LENGTHS + (40, 77), long_at=long_at)
        key = [rng.randrange(40) for _ in recs]
        out.append((rank, "sam sort %d" % n, lambda key=key, recs=recs: [a.tobytes() for a in t_sort.check(key, recs, host=False)]))
    return out


def bam_steps():
    out, walked = [], []
    for name, s, n_ref in rc.corpus():
        try:
            walked.append((name, s, n_ref, ro.walk(s, rc.BODY, n_ref)))
        except ro.Refused:
            pass
    for rank, (name, s, n_ref, off) in enumerate(three(walked, lambda w: len(w[1]))):
        def records(s=s, n_ref=n_ref, off=off):
            got = t_records.table_dev(s, n_ref)
            assert got == (off, len(ro.candidates(s, rc.BODY, n_ref)))
            return got

        def reads(s=s, n_ref=n_ref, off=off):
            got, _ = t_reads.reads_dev(s, off, n_ref, r_in=5, r_seq=3, r_qual=9)
            assert t_reads.same(got, ro.reads(s, off, n_ref))
            return (got[0].tobytes(),) + tuple(got[1:])
        out += [(rank, "bam records: " + name, records), (rank, "bam reads: " + name, reads)]
    for rank, (name, (slots, contigs)) in enumerate(three(bc.shapes().items(), lambda kv: len(kv[1][0]))):
        def index(slots=slots, contigs=contigs):
            got = t_index.index_dev(slots, contigs)
            assert got == ba.build(slots, contigs, ba.stored_voff())
            return got
        out.append((rank, "bam index: " + name, index))
    return out


def bgzf_steps(tmp):
    out = []
    good = zc.good_members()
    for rank, (first, n) in enumerate(((0, 2), (30, 20), (60, 60))):
        part = good[first:first + n]
        f = b"".join(m for _, m, _ in part)

        def blocks(f=f):
            rcode, block_off, out_off, _ = zc.walk(f)
            got = t_inflate.blocks_dev(f, 5)
            assert rcode == 0 and got == (block_off, out_off)
            return got

        def inflate(f=f, part=part):
            _, block_off, out_off, _ = zc.walk(f)
            err, status, data = t_inflate.inflate_dev(f, block_off, out_off, 1, 2)
            assert err is None and status == [0] * len(part) and data == b"".join(d for _, _, d in part)
            return data
        out += [(rank, "bgzf blocks %d" % n, blocks), (rank, "bgzf inflate %d" % n, inflate)]
    # the deflated blocks are the CPU run's of the same bodies, as in tests/test_gpu_bgzf_deflate.py
    named = dict(dc.payloads() + t_deflate.long_inputs())
    datas = [named[k] for k in ("one symbol, length 1", "text 259", "text %d" % (2 * dc.P + 77))]
    parts = [t_deflate.cut(d) for d in datas]
    _, cpu = dc.run_program(dc.build_program(str(tmp / "bodies"), sanitize=False), tmp, [], [p for ps in parts for p in ps])
    at = 0
    for rank, (data, ps) in enumerate(zip(datas, parts)):
        want = b"".join(b for b, _, _ in cpu[at:at + len(ps)]) + bo.EOF_BLOCK
        at += len(ps)

        def deflate(data=data, want=want):
            got, off = t_deflate.deflate_dev(data, bam.BGZF_EOF, 7, 3)
            assert got == want
            return got, off.tobytes()
        out.append((rank, "bgzf deflate %d" % len(data), deflate))
    return out


def pileup_steps():
    out = []
    families = (("pileup", pc, t_pileup.rows_dev, ("every op kind", "tile borders", "random records")),
                ("sites", sc, t_sites.sites_dev, ("every op kind", "sites across a tile border", "random records, strict")),
                ("indels", ic, t_indels.indels_dev, ("every op kind", "anchors at T - 1 and T, a deletion into the next tile, regions one behind and only the anchor",
                                                     "random records, no threshold")))
    for what, cases, call, names in families:
        by = {c["name"]: c for c in cases.corpus(with_deep=False)}
        for rank, name in enumerate(names):
            c, want = by[name], cases.want_of(by[name])  # the oracle once, shared by the two passes

            def step(c=c, want=want, call=call):
                got = [g.tolist() if isinstance(g, np.ndarray) else g for g in call(c)]
                assert got == [w.tolist() if isinstance(w, np.ndarray) else w for w in want]
                return got
            out.append((rank, "%s: %s" % (what, name), step))
    return out


def test_calls_of_different_sizes_share_one_contexts_scratch(monkeypatch, tmp_path):
    steps = fastq_steps() + sam_steps() + bam_steps() + bgzf_steps(tmp_path) + pileup_steps()
    assert all(sum(r == rank for r, _, _ in steps) == len(steps) // RANKS for rank in range(RANKS))
    up = [s for rank in range(RANKS) for s in steps if s[0] == rank]  # every family's smallest, then the next size, then the largest
    ctx = _lib.Context(_lib.default_context().device)  # fresh: no earlier test has grown its scratch
    monkeypatch.setitem(_lib._default_ctx, ctx.device, ctx)
    first = {}
    for _, name, step in up:
        first[name] = step()
    assert len(first) == len(steps)
    for _, name, step in up[::-1]:
        assert step() == first[name], name

"""The cases of tests/test_gpu_seed_extend_edges.py without a GPU: their seed hit counts are the ones planted (tests/seed_edges.py),
checked against exact occurrence counts in the text and against the oracle's composition (oracle/pipeline.cpp), read by read —
n_seed_hits, and n_candidates against the header's merge rule restated on the proposals."""
import numpy as np
import pytest

import oracle_py as orc
import pair_oracle as po
import seed_edges as se
from rust_bio_amd.bwt import bwt, less
from rust_bio_amd.suffix_array import suffix_array

ALPHA = b"ACGTNacgtn$"
SC = (-5, -1, 1, -1)


@pytest.fixture(scope="module")
def case():
    c = se.Case()
    sa = suffix_array(c.text)
    b = bwt(c.text, sa)
    ls = less(b, ALPHA)
    return c, sa, b, ls, orc.Occ(b, 64, ALPHA)


def test_kmer_table_counts_are_exact(case):
    """the sorted 20-mer table against bytes.find on the text, for seeds of every kind of edge read"""
    c = case[0]
    tb = c.g.tobytes()
    rng = np.random.default_rng(1)
    for rd in c.main_reads[::3] + c.wide_reads[::4] + c.pair_reads[::3]:
        for k in rng.choice(len(rd.c), size=min(3, len(rd.c)), replace=False) if len(rd.c) else ():
            o = int(k) * rd.stride
            seed = rd.x[o:o + se.SEED_LEN].tobytes()
            occs, at = [], tb.find(seed)
            while at >= 0:
                occs.append(at)
                at = tb.find(seed, at + 1)
            assert c.table.find(rd.x[o:o + se.SEED_LEN]).tolist() == occs


@pytest.mark.parametrize("batch", ["main", "wide"])
def test_planted_counts_are_the_texts(case, batch):
    c = case[0]
    reads = c.main_reads if batch == "main" else c.wide_reads
    prm = se.MAIN if batch == "main" else se.WIDE_OCC
    rs = se.restate(c.table, c.n_text, *getattr(c, batch), prm["stride"], prm["max_occ"], 25)
    for r, (rd, d) in enumerate(zip(reads, rs)):
        assert (d["counts"] == rd.c).all(), r
        assert d["nh"] == rd.planned(prm["max_occ"]), r
    nh = {d["nh"] for d in rs}
    want = se.NH_VALUES if batch == "main" else (0, 1, 64, 65, 512, 513, 1023, 1024)
    assert set(want) <= nh
    if batch == "main":
        assert max(d["counts"].max(initial=0) for d in rs) == prm["max_occ"] + 1  # a seed one copy over max_occ
        rev = se.restate(c.table, c.n_text, *se.flat([rd.x for rd in c.main_rev.values()]), 1, 16, 25)
        for rc, d in zip(c.main_rev.values(), rev):
            assert (d["counts"] == rc.c).all() and d["nh"] == rc.planned(16) >= 200


@pytest.mark.parametrize("pad,max_occ", [(25, 16), (1, 16), (25, 1)])
def test_oracle_on_the_main_batch(case, pad, max_occ):
    """the oracle's composition gives the restated hit and candidate counts, and the cases reach the kernels' edges"""
    c, sa, b, ls, occ = case
    reads, off = c.main
    h, _, _ = orc.seed_extend_batch(b, ls, occ, sa, c.text, c.n_text, orc.make_scoring(*SC), reads, off, seed_len=20, stride=1,
                                    max_occ=max_occ, pad=pad, threads=8, want_ops=False)
    rs = se.restate(c.table, c.n_text, reads, off, 1, max_occ, pad)
    assert (h["n_seed_hits"] == [d["nh"] for d in rs]).all()
    assert (h["n_candidates"] == [len(d["kept"]) for d in rs]).all()
    if max_occ == 16:
        assert set(se.NH_VALUES) <= set(h["n_seed_hits"].tolist())
        assert h["n_candidates"].max() == 1024
        assert se.merges_at(rs, pad // 2)
        assert any(d["dropped"] and d["nh"] > 64 for d in rs)  # s < 0: counted, not a candidate
        starts = [s for d in rs for s in d["kept"]]
        assert min(starts) == 0 and max(starts) + se.MAIN["L"] + pad > c.n_text  # windows clipped at both ends


def test_oracle_on_the_wide_batch(case):
    c, sa, b, ls, occ = case
    reads, off = c.wide
    h, _, _ = orc.seed_extend_batch(b, ls, occ, sa, c.text, c.n_text, orc.make_scoring(*SC), reads, off, seed_len=20, stride=2,
                                    max_occ=32, pad=25, threads=8, want_ops=False)
    rs = se.restate(c.table, c.n_text, reads, off, 2, 32, 25)
    assert (h["n_seed_hits"] == [d["nh"] for d in rs]).all()
    assert (h["n_candidates"] == [len(d["kept"]) for d in rs]).all()
    assert {0, 1, 64, 65, 512, 513, 1023, 1024} <= set(h["n_seed_hits"].tolist())


def test_pair_cases_pick_the_planted_fragments(case):
    """the pair rule on the pair batch: the winning combinations use the candidates the construction meant (the last of a
    1024-candidate list, the first of both lists, the copy the partner mate sits next to)"""
    c, sa, b, ls, occ = case
    reads, off = c.pairs
    vr, voff = po.virtual_reads(reads, off)
    cands, nh = po.candidates(orc, b, ls, occ, sa, c.text, c.n_text, orc.make_scoring(*SC), vr, voff, stride=1)
    er, ep = po.expected(cands, nh, len(c.pair_info), 0, 1000, 17)
    for p, (kind, F, R) in enumerate(c.pair_info):
        assert ep[p][0], kind  # proper
        v = cands[4 * p:4 * p + 4]
        (s1, c1, _, _), (s2, c2, _, _) = er[2 * p], er[2 * p + 1]
        fwd_m, rev_m = (0, 1) if kind != "top_b" else (1, 0)
        cf, cr = (c1, c2) if fwd_m == 0 else (c2, c1)
        assert cf["start"] == F and cr["start"] == R, kind
        lf, lr = v[2 * fwd_m], v[2 * rev_m + 1]
        i, j = lf.index(cf), lr.index(cr)
        if kind == "top":
            assert (i, len(lf)) == (1023, 1024) and len(lr) >= 300
        elif kind == "top_b":
            assert (i, len(lf)) == (1023, 1024) and j == len(lr) - 1 >= 500
        elif kind == "bottom":
            assert (i, j) == (0, 0) and len(lf) > 64 and len(lr) > 64
        else:
            st, k = po.strand_best(v[0], v[1])  # on its own, mate 1 goes to the first of its two equal copies
            assert st == po.HIT_FORWARD and k < i and v[0][k]["score"] == cf["score"] and v[0][k]["start"] < F

"""`bg_myers_best_batch[_dev]` and `bg_myers_find_all_batch[_dev]` (with and without BG_MYERS_ENDS_ONLY) on the
reference's known answers (tests/golden/myers_kats.json): records, operations and counts of both flavours byte for byte
against the restatement (tests/myers_oracle.py) and value for value against the transcribed answers, the mirror's
one-text methods, and the known alignments through `bg_cigar_batch_dev` as the `bg_alignment_t` they are."""
import itertools

import numpy as np
import pytest
import torch

import myers_cases as mc
import myers_oracle as mo
from rust_bio_amd import _lib, myers

pytestmark = pytest.mark.gpu
DEV = mc.DEV


@pytest.mark.parametrize("case", mc.KATS, ids=lambda c: c["name"])
def test_known_answers_through_every_call(case):
    my, want_my, text, k = mc.mirror(case), mc.restatement(case), case["text"].encode(), mc.k_of(case)
    assert [int(v) for v in my.peq] == want_my.peq
    stride = 2 * my.m
    # find-all with starts and ENDS_ONLY, both flavours, against the restatement and the transcribed tuples
    for ends_only in (False, True):
        want = mo.find_all_records([want_my], [text], k, 64, ends_only)
        for rec, count in mc.both_find_all([my], [text], k, 64, ends_only):
            assert rec.tobytes() == want[0].tobytes() and (count == want[1]).all()
    full = my.find_all(text, k)
    ends = my.find_all_end(text, k)
    # the path of a named hit: the best call on the text up to the hit's end with the hit's distance as the bound, where
    # that hit is the best of its prefix (all named hits of the reference's tests; two of the four printed in mod.rs:134-172)
    paths = {}
    for h in (h for h in mc.named_hits(case) if mc.best_of_prefix(case, h)):
        s, e, d = full[h]
        for rec, ops in mc.both_best([my], [text[:e]], d, stride):
            assert (int(rec["ystart"][0]), int(rec["yend"][0]), int(rec["score"][0])) == (s, e, d)
            got = list(ops[int(rec["ops_off"][0]):int(rec["ops_off"][0]) + int(rec["n_ops"][0])])
            assert paths.setdefault(h, got) == got
    # the best call on the whole text
    best = None
    for got in mc.both_best([my], [text], k, stride):
        mc.same_best(got, mo.best_records([want_my], [text], k, stride), stride)
        rec, ops = got
        if rec["score"][0] != mo.MIN_SCORE:
            best = (int(rec["ystart"][0]), int(rec["yend"][0]), int(rec["score"][0]),
                    list(ops[int(rec["ops_off"][0]):int(rec["ops_off"][0]) + int(rec["n_ops"][0])]))
    mc.check_case(case, my.distance(text), ends, full, paths, best)
    if "best_end" in case:
        assert list(my.find_best_end(text)) == case["best_end"]
        best = my.best_alignment(text)
        assert (best["yend"] - 1, best["score"]) == tuple(case["best_end"])


def test_all_cases_in_one_batch():
    """every known text against every known plain pattern in one call (23 texts x 16 distinct patterns, k = 2)"""
    texts = [c["text"].encode() for c in mc.KATS] + [b""]
    patterns = sorted({c["pattern"].encode() for c in mc.KATS})
    pats, want_pats = [myers.Myers(p) for p in patterns], [mo.Myers(p) for p in patterns]
    for got in mc.both_best(pats, texts, 2, 128):
        mc.same_best(got, mo.best_records(want_pats, texts, 2, 128), 128)
    for ends_only, max_hits in itertools.product((False, True), (3,)):
        want = mo.find_all_records(want_pats, texts, 2, max_hits, ends_only)
        for rec, count in mc.both_find_all(pats, texts, 2, max_hits, ends_only):
            assert rec.tobytes() == want[0].tobytes() and (count == want[1]).all()


def test_mirror_raises_where_the_reference_panics():
    my = myers.Myers(b"ACGT")
    assert my.distance(b"") == 255
    with pytest.raises(ValueError):
        my.find_best_end(b"")
    assert my.find_all(b"", 4) == [] and my.find_all_end(b"", 4) == [] and my.best_alignment(b"") is None


def _cigar(ops):
    return "".join(f"{len(list(g))}{'=XDI'[o]}" for o, g in itertools.groupby(ops))


def test_known_alignments_are_real_alignment_records():
    """the cases that pin a path, as one batch through bg_cigar_batch_dev"""
    jobs = []
    for case in mc.KATS:
        for h in (h for h in mc.named_hits(case) if mc.best_of_prefix(case, h)):
            want = mc.restatement(case).find_all(case["text"].encode(), mc.k_of(case))[h]
            ops = next(p["ops"] for p in case.get("paths", []) + ([case["alignment"]] if "alignment" in case else []) if p["hit"] == h)
            jobs.append((mc.mirror(case), case["text"].encode()[:want[1]], want[2], [mc.OPS[c] for c in ops]))
    assert len(jobs) == 9
    stride = 128
    d_alns, d_opss = [], []
    stream = torch.cuda.current_stream().cuda_stream
    for j, (my, text, d, _) in enumerate(jobs):  # one pattern and one bound per job: a call each, results side by side
        d_aln, d_ops = myers.best_batch_dev([my], mc.dev(np.frombuffer(text, np.uint8)), mc.dev(np.array([0, len(text)]), np.int64), d,
                                            ops_stride=stride, stream=stream)
        rec = myers.records(d_aln).copy()
        rec["ops_off"] += j * stride
        d_alns.append(rec)
        d_opss.append(d_ops)
    d_aln = mc.dev(np.concatenate(d_alns))
    d_ops = torch.cat(d_opss)
    out_stride = 2 * stride + 24
    d_out = torch.zeros(len(jobs) * out_stride, dtype=torch.uint8, device=DEV)
    d_len = torch.zeros(len(jobs), dtype=torch.int32, device=DEV)
    ctx = _lib.default_context()
    _lib.check(_lib.lib().bg_cigar_batch_dev(ctx.h, len(jobs), d_aln.data_ptr(), d_ops.data_ptr(), 0, d_out.data_ptr(), out_stride,
                                             d_len.data_ptr(), stream), "bg_cigar_batch_dev")
    torch.cuda.synchronize()
    out, lens = d_out.cpu().numpy(), d_len.cpu().numpy()
    for j, (_, _, _, ops) in enumerate(jobs):
        assert out[j * out_stride:j * out_stride + int(lens[j])].tobytes().decode() == _cigar(ops), j

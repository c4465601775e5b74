"""Shared by the tests of the block-based Myers kernels (csrc/myers_long.hip): the reference's known answers
(tests/golden/myers_long_kats.json), a pattern as (mirror, restatement), the
calls of both flavours, and the comparison of everything a batch returns with the restatement at w = 64
(tests/myers_long_oracle.py)."""
import json
import os

import numpy as np

import myers_long_oracle as ml
from myers_cases import DEV, dev, same_best

KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "myers_long_kats.json")))["cases"]


def pair(pattern, ambigs=None, wildcards=None):
    """(mirror, restatement) of one pattern"""
    from rust_bio_amd import myers
    b = myers.MyersBuilder()
    for sym, eq in (ambigs or {}).items():
        b.ambig(sym, eq)
    for w in wildcards or ():
        b.text_wildcard(w)
    return b.build_long_64(pattern), ml.MyersLong(pattern, ambigs, wildcards)


def device_texts(texts):
    import torch
    from rust_bio_amd import _lib
    buf, off = _lib.concat(texts)
    return buf, off, (dev(buf) if len(buf) else torch.zeros(1, dtype=torch.uint8, device=DEV)), dev(off, np.int64)


def both_best(pats, texts, k, stride, ctx=None):
    """the best call of both flavours: [(records, ops)]"""
    import torch
    from rust_bio_amd import myers
    buf, off, d_text, d_off = device_texts(texts)
    host = myers.long_best_batch(pats, buf, off, k, ops_stride=stride, ctx=ctx)
    d_aln, d_ops = myers.long_best_batch_dev(pats, d_text, d_off, k, ops_stride=stride, ctx=ctx, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [host, (myers.records(d_aln), d_ops.cpu().numpy() if d_ops is not None else None)]


def both_find_all(pats, texts, k, max_hits, ends_only, ctx=None):
    import torch
    from rust_bio_amd import myers
    buf, off, d_text, d_off = device_texts(texts)
    host = myers.long_find_all_batch(pats, buf, off, k, max_hits, ends_only, ctx=ctx)
    d_aln, d_count = myers.long_find_all_batch_dev(pats, d_text, d_off, k, max_hits, ends_only, ctx=ctx,
                                                   stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [host, (myers.records(d_aln), d_count.cpu().numpy().astype(np.uint32))]


def check_all(pairs, texts, k, max_hits=4, stride=None, ctx=None):
    """the best call and both find-all calls, host and device flavour, against the restatement; returns the best records"""
    pats, want = [p[0] for p in pairs], [p[1] for p in pairs]
    stride = stride or 2 * max(w.m for w in want)
    wbest = ml.best_records(want, texts, k, stride)
    for got in both_best(pats, texts, k, stride, ctx):
        same_best(got, wbest, stride)
    for ends_only in (False, True):
        wrec, wcount = ml.find_all_records(want, texts, k, max_hits, ends_only)
        for rec, count in both_find_all(pats, texts, k, max_hits, ends_only, ctx):
            assert (count == wcount).all()
            assert rec.tobytes() == wrec.tobytes()
    return wbest[0]

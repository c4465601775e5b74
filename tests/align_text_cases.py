"""Hand-made alignment records for the tests of the two alignment texts (tests/align_text_oracle.py states the rule): a record
as a plain dict, seeded random records that are consistent by construction, and the packing of a list of records into the
`bg_alignment_t` array and the operation buffer the calls take.  numpy only: the CPU and the GPU tests share it."""
import numpy as np

import align_text_oracle as ato
from rust_bio_amd import _lib

U32 = 2**32 - 1
RUNS = (1, 2, 9, 10, 11, 99, 100)
CLIPS = (0, 1, 9, 10, U32)
LETTERS = np.frombuffer(b"ACGTNRYKMSWBDHV", np.uint8)


def rec(mode, ops, x=b"", y=b"", xstart=0, ystart=0, xend=None, yend=None, xlen=None, ylen=None, clips=()):
    """one record; `ops` a string over "MSDIXY" or the operation bytes.  xend / yend / xlen / ylen default to what the
    operations and the sequences say."""
    if isinstance(ops, str):
        ops = ["MSDIXY".index(c) for c in ops]
    ops = np.asarray(ops, dtype=np.uint8)
    ax, ay = int(np.isin(ops, (0, 1, 3)).sum()), int(np.isin(ops, (0, 1, 2)).sum())
    r = {"mode": ato.mode_of(mode), "ops": ops, "clips": list(clips), "x": bytes(x), "y": bytes(y), "xstart": xstart, "ystart": ystart}
    r["xend"] = xstart + ax if xend is None else xend
    r["yend"] = ystart + ay if yend is None else yend
    r["xlen"] = len(r["x"]) if xlen is None else xlen
    r["ylen"] = len(r["y"]) if ylen is None else ylen
    assert len(r["clips"]) <= 4 and all(0 <= r[f] <= U32 for f in ("xstart", "xend", "ystart", "yend", "xlen", "ylen"))
    return r


def want_cigar(r, hard):
    return ato.cigar(r["xstart"], r["xend"], r["xlen"], r["mode"], r["ops"], hard)


def want_pretty(r, ncol):
    return ato.pretty(r, r["ops"], r["clips"], r["x"], r["y"], ncol)


def u64_tokens(r):
    """the operations as oracle_py takes them: kind | clip length << 8"""
    clip = iter(r["clips"])
    return [int(o) | ((next(clip, 0) if o >= 4 else 0) << 8) for o in r["ops"]]


def pack(records, order=None, share=True):
    """-> (bg_alignment_t array, operation buffer).  `order`: the order in which the records' operations lie in the buffer
    (default: the records' own); records that hold the very same `ops` array share one run of the buffer when `share`."""
    out = np.zeros(len(records), dtype=_lib.ALN_DTYPE)
    buf, at, placed = [], 0, {}
    for p in (range(len(records)) if order is None else order):
        r = records[p]
        key = id(r["ops"])
        if not (share and key in placed):
            placed[key] = at
            buf.append(r["ops"])
            at += len(r["ops"])
        out[p]["ops_off"] = placed[key]
    for p, r in enumerate(records):
        a = out[p]
        for f in ("xstart", "xend", "ystart", "yend", "xlen", "ylen", "mode"):
            a[f] = r[f]
        a["n_ops"], a["n_clips"] = len(r["ops"]), len(r["clips"])
        a["clip_len"][:len(r["clips"])] = r["clips"]
        a["score"] = p - 7
    return out, (np.concatenate(buf) if buf else np.zeros(0, np.uint8)).astype(np.uint8)


def rec_dict(a):
    """a bg_alignment_t (numpy record) as the mapping the restatement takes"""
    return {f: int(a[f]) for f in ("xstart", "xend", "ystart", "yend", "xlen", "ylen", "mode")}


def random_runs(rng, kinds=(0, 1, 2, 3), max_runs=6):
    k = int(rng.integers(1, max_runs + 1))
    return np.concatenate([np.full(int(rng.choice(RUNS)), int(rng.choice(kinds)), dtype=np.uint8) for _ in range(k)])


def random_cigar_record(rng, mode=None, inner_clips=None):
    """runs from RUNS, both clips from CLIPS (the fields are cut to 32 bits where lead + aligned + trail does not fit), a fifth
    with clip bytes inside; every tenth without operations"""
    mode = int(rng.integers(0, 4)) if mode is None else mode
    ops = random_runs(rng) if rng.integers(0, 10) else np.zeros(0, np.uint8)
    if (rng.integers(0, 5) == 0 if inner_clips is None else inner_clips) and len(ops):
        for at in sorted(rng.integers(0, len(ops) + 1, size=int(rng.integers(1, 4))))[::-1]:
            ops = np.insert(ops, at, rng.choice((4, 5)))
    lead, trail = int(rng.choice(CLIPS)), int(rng.choice(CLIPS))
    ax = int(np.isin(ops, (0, 1, 3)).sum())
    xend = min(lead + ax, U32 - trail)
    return rec(mode, ops, xstart=lead, xend=xend, xlen=xend + trail)


def random_pretty_record(rng, mode=None, inner_clips=None, flanks=(0, 1, 9, 10), max_runs=4):
    """a record with the sequences it fits: flanks (standard modes) or up to four clip operations around the runs (Custom) from
    CLIPS, the 2^32 - 1 only in front (it prints the whole sequence: what follows it panics or is all Del / Ins); a fifth of
    the standard-mode records with clip bytes inside, their sequences longer by what those consume"""
    mode = int(rng.integers(0, 4)) if mode is None else mode
    ops = random_runs(rng, max_runs=max_runs) if rng.integers(0, 12) else np.zeros(0, np.uint8)
    ax, ay = int(np.isin(ops, (0, 1, 3)).sum()), int(np.isin(ops, (0, 1, 2)).sum())
    clips, xs, ys = [], 0, 0
    pre = [int(rng.choice(flanks)) for _ in range(4)]  # x prefix, y prefix, x suffix, y suffix
    huge = int(rng.integers(0, 40))  # 0 / 1: the x / y prefix is 2^32 - 1
    if mode == ato.CUSTOM:
        head = [(k, pre[k - 4]) for k in (4, 5) if rng.integers(0, 2)]
        tail = [(k, pre[k - 2]) for k in (4, 5) if rng.integers(0, 2)]
        if rng.integers(0, 2):
            head, tail = head[::-1], tail[::-1]
        if huge < 2 and head:
            head[0] = (head[0][0], U32)
        ops = np.concatenate([np.array([k for k, _ in head], np.uint8), ops, np.array([k for k, _ in tail], np.uint8)]).astype(np.uint8)
        clips = [c for _, c in head + tail]
        xl = ax + sum(c for k, c in head + tail if k == 4 and c != U32)
        yl = ay + sum(c for k, c in head + tail if k == 5 and c != U32)
    else:
        if (rng.integers(0, 5) == 0 if inner_clips is None else inner_clips) and len(ops):
            for at in sorted(rng.integers(0, len(ops) + 1, size=int(rng.integers(1, 4))))[::-1]:
                k, c = int(rng.choice((4, 5))), int(rng.choice(flanks))
                ops = np.insert(ops, at, k)
                clips.insert(0, c)
                xs, ys = xs + c * (k == 4), ys + c * (k == 5)
        xl, yl = pre[0] + ax + xs + pre[2], pre[1] + ay + ys + pre[3]
    x = bytes(rng.choice(LETTERS, size=xl))
    y = bytes(rng.choice(LETTERS, size=yl)).lower()
    if mode == ato.CUSTOM:
        return rec(mode, ops, x, y, clips=clips)
    xstart = U32 if huge == 0 else pre[0]
    ystart = U32 if huge == 1 else pre[1]
    return rec(mode, ops, x, y, xstart=xstart, ystart=ystart, xend=min(xstart + ax + xs, U32), yend=min(ystart + ay + ys, U32), clips=clips)


def pretty_or_none(fn, *args):
    try:
        return fn(*args)
    except AssertionError:
        return None

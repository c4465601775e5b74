"""A restatement in plain Python of THE RULE of bg_bam_indels_left in include/biogpu.h: the raw events of tests/bam_indels_oracle.py
(`raw_events`), each shifted to the left against the contig's text with its record's `pos`, as the rule's words say it — the
inserted sequence of a shifted event is put together from text bytes and the record's bytes, exactly as the rule defines byte i
— then tallied and judged by that oracle's `from_depths`.  Nothing here knows of tiles, sorts, scans or rotations.  Shares no
code with the product."""
import bam_indels_oracle as io
import bam_pileup_oracle as po

INVALID_ARG = io.INVALID_ARG
NONE = io.NONE
DEL, INS = io.DEL, io.INS
NO_LIMIT = 0xFFFFFFFF
CODE = {65: 1, 67: 2, 71: 4, 84: 8}  # a text base takes the code of its letter
Refused = io.Refused


def params(max_shift=NO_LIMIT, **kw):
    return dict(io.params(**kw), max_shift=max_shift)


def fold(b):
    return b - 32 if 97 <= b <= 122 else b


def shift(F, clen, pos, anchor, kind, n, codes, max_shift):
    """one raw event -> (anchor', codes', k).  F(p): the folded text byte of position p of the record's contig"""
    a, k = anchor, 0
    if kind == DEL:
        while k < max_shift and a > pos and a + n < clen and F(a) == F(a + n) and F(a) in b"ACGT":
            a, k = a - 1, k + 1
        return a, (), k
    s = [io.ASCII[c] for c in codes]
    while k < max_shift and a - k > pos:
        c = s[n - 1 - k] if k < n else F(a - k + n)
        if c != F(a - k) or c not in b"ACGT":
            break
        k += 1
    a = anchor - k
    shifted = [F(a + 1 + i) if i < min(k, n) else s[i - k] for i in range(n)]
    return a, tuple(CODE[b] if i < min(k, n) else codes[i - k] for i, b in enumerate(shifted)), k


def shifted_events(slots, contigs, text, p):
    """[(ref, strand, raw (anchor, kind, n, codes), shifted (anchor, kind, n, codes), k, pos)] over the kept records"""
    out = []
    for rec in slots:
        if not rec:
            continue
        f = po.fields(rec)
        if not po.kept(f, p["require"], p["exclude"], p["min_mapq"]):
            continue
        start, clen = contigs[f["ref"]][1], contigs[f["ref"]][2]
        for anchor, kind, n, codes in io.raw_events(f):
            a, c, k = shift(lambda q: fold(text[start + q]), clen, f["pos"], anchor, kind, n, codes, p["max_shift"])
            out.append((f["ref"], 1 if f["flag"] & 0x10 else 0, (anchor, kind, n, codes), (a, kind, n, c), k, f["pos"]))
    return out


def tally(slots, contigs, text, p, refs=None):
    """{(ref, shifted anchor, kind, len, shifted codes): [forward, reverse]}; refs: only the contigs that some region names (the
    text of another contig need not exist)"""
    counts = {}
    only = [rec if rec and (refs is None or po.fields(rec)["ref"] in refs) else b"" for rec in slots]
    for ref, strand, _, (a, kind, n, codes), _, _ in shifted_events(only, contigs, text, p):
        counts.setdefault((ref, a, kind, n, codes), [0, 0])[strand] += 1
    return counts


def check(contigs, regions, n_text, p):
    if p["min_alt_permille"] > 1000:
        raise Refused(INVALID_ARG)
    for ref, beg, end in regions:  # (all region checks come before the slots)
        if not (0 <= ref < len(contigs) and 0 <= beg <= end <= contigs[ref][2]):
            raise Refused(INVALID_ARG)
        if contigs[ref][1] + contigs[ref][2] > n_text:
            raise Refused(INVALID_ARG)


def indels(slots, contigs, text, regions, n_text=None, **kw):
    """-> ([event tuples], seq bytes, event_off); raises Refused as the call refuses"""
    p = params(**kw)
    check(contigs, regions, len(text) if n_text is None else n_text, p)
    rows, row_off = po.pileup(slots, contigs, regions, flags=po.STRANDS, require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"],
                              min_baseq=p["min_baseq"])
    counts = tally(slots, contigs, text, p, refs={r[0] for r in regions})
    return io.from_depths(counts, lambda r, pos: io.depth_of(rows[row_off[r] + pos - regions[r][1]]), regions, p)


def from_rows(slots, contigs, text, rows16, row_off, regions, **kw):
    """the same with the depth taken from 16-column pileup rows that something else produced"""
    p = params(**kw)
    counts = tally(slots, contigs, text, p, refs={r[0] for r in regions})
    return io.from_depths(counts, lambda r, pos: io.depth_of(rows16[int(row_off[r]) + pos - regions[r][1]]), regions, p)

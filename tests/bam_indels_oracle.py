"""A restatement in plain Python of THE RULE of bg_bam_indels in include/biogpu.h: the indel events of a batch of regions.  The
records are walked as tests/bam_pileup_oracle.py walks them (its `check`, `fields` and `kept`), operation by operation, into a
dictionary keyed by (reference, anchor, kind, length, codes); the depth of an anchor comes from that oracle's counters.  Nothing
here knows of tiles, sorts or scans.  `depths_from_rows` takes the depth from pileup rows that something else produced.  Shares
no code with the product."""
import bam_pileup_oracle as po

INVALID_ARG, TOO_LARGE, OPS_CAP, UNSUPPORTED = po.INVALID_ARG, po.TOO_LARGE, po.OPS_CAP, po.UNSUPPORTED
NONE = po.NONE
DEL, INS = 1, 2
ASCII = b"=ACMGRSVTWYHKDBN"
DEFAULT = dict(require=0, exclude=0x704, min_mapq=0, min_baseq=0, min_depth=0, min_alt=1, min_alt_permille=0, min_alt_strand=0)
EVENT_FIELDS = ("ref", "pos", "region", "kind", "len", "depth", "alt_fwd", "alt_rev", "seq_off")
Refused = po.Refused


def params(**kw):
    return dict(DEFAULT, **kw)


def raw_events(f):
    """[(anchor, kind, len, codes)] of one kept record, in the order of its operations"""
    out, r, q = [], f["pos"], 0
    for op, n in f["cigar"]:
        if op in po.M_OPS:
            r, q = r + n, q + n
        elif op == 1:
            if n >= 1 and r > f["pos"] and f["l_seq"]:
                out.append((r - 1, INS, n, tuple(f["codes"][q:q + n])))
            q += n
        elif op == 2:
            if n >= 1 and r > f["pos"]:
                out.append((r - 1, DEL, n, ()))
            r += n
        elif op == 3:
            r += n
        elif op == 4:
            q += n
    return out


def tally(slots, p):
    """{(ref, anchor, kind, len, codes): [forward, reverse]} over the kept records"""
    counts = {}
    for rec in slots:
        if not rec:
            continue
        f = po.fields(rec)
        if not po.kept(f, p["require"], p["exclude"], p["min_mapq"]):
            continue
        for anchor, kind, n, codes in raw_events(f):
            counts.setdefault((f["ref"], anchor, kind, n, codes), [0, 0])[1 if f["flag"] & 0x10 else 0] += 1
    return counts


def is_kept(fwd, rev, depth, p):
    alt = fwd + rev
    return (depth >= p["min_depth"] and alt >= max(p["min_alt"], 1) and alt * 1000 >= p["min_alt_permille"] * depth
            and fwd >= p["min_alt_strand"] and rev >= p["min_alt_strand"])


def depth_of(row):
    """a 16-column row: A + C + G + T + OTHER + DEL over both strands"""
    return sum(int(row[c]) + int(row[po.COLS + c]) for c in (po.A, po.C, po.G, po.T, po.OTHER, po.DEL))


def from_depths(counts, depth_at, regions, p):
    """events from the tally and a function (region index, position) -> depth: -> ([event tuples in EVENT_FIELDS order], seq bytes,
    event_off)"""
    by_pos = {}
    for (ref, anchor, kind, n, codes), (fwd, rev) in counts.items():
        by_pos.setdefault((ref, anchor), []).append((kind, n, codes, fwd, rev))
    events, seq, event_off = [], bytearray(), [0]
    for r, (ref, beg, end) in enumerate(regions):
        here = sorted(pos for c, pos in by_pos if c == ref and beg <= pos < end)
        for pos in here:
            depth = depth_at(r, pos)
            for kind, n, codes, fwd, rev in sorted(by_pos[(ref, pos)]):
                if is_kept(fwd, rev, depth, p):
                    events.append((ref, pos, r, kind, n, depth, fwd, rev, len(seq)))
                    seq += bytes(ASCII[c] for c in codes)
        event_off.append(len(events))
    return events, bytes(seq), event_off


def indels(slots, contigs, regions, **kw):
    """-> ([event tuples], seq bytes, event_off); raises Refused as the call refuses"""
    p = params(**kw)
    if p["min_alt_permille"] > 1000:
        raise Refused(INVALID_ARG)
    rows, row_off = po.pileup(slots, contigs, regions, flags=po.STRANDS, require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"],
                              min_baseq=p["min_baseq"])
    return from_depths(tally(slots, p), lambda r, pos: depth_of(rows[row_off[r] + pos - regions[r][1]]), regions, p)


def from_rows(slots, rows16, row_off, regions, **kw):
    """the same with the depth taken from 16-column pileup rows that something else produced"""
    p = params(**kw)
    return from_depths(tally(slots, p), lambda r, pos: depth_of(rows16[int(row_off[r]) + pos - regions[r][1]]), regions, p)


def as_tuples(arr):
    """a BAM_INDEL_DTYPE array as the oracle's tuples"""
    return [tuple(int(rec[f]) for f in EVENT_FIELDS) for rec in arr]


def strings(events, seq):
    """the inserted string of every event (b"" for a deletion)"""
    return [bytes(seq[e[8]:e[8] + e[4]]) if e[3] == INS else b"" for e in events]

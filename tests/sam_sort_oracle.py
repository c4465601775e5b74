"""CPU statement of the rules of bg_sam_markdup, bg_sam_sort_keys and bg_sam_sort (include/biogpu.h), for the tests: plain
Python over numpy records — dictionaries and `sorted`.  Placement is `sam_oracle.Slot`.  `check_sorted_text` is a second,
independent check of the sort that reads only SAM text."""
from collections import defaultdict

import numpy as np

import sam_oracle as so

U64_MAX = 2**64 - 1
PAIRED = so.PAIRED


def score_of(qual, phred_offset, min_qual):
    """the sum of q - phred_offset over the quality bytes with q >= phred_offset + min_qual, as a 32-bit integer"""
    return sum(q - phred_offset for q in bytes(qual) if q >= phred_offset + min_qual) & 0xFFFFFFFF


def end_of(slot, events=None):
    """(contig, u5, rev) of a placed slot, None otherwise"""
    if not slot.placed:
        return None
    aln = slot.hit["aln"]
    if slot.strand == so.HIT_REVERSE:
        clip = int(aln["xlen"]) - int(aln["xend"])
        end = (slot.contig, slot.ref_end - 1 + clip, 1)
    else:
        clip = int(aln["xstart"])
        end = (slot.contig, max(slot.ref_start - clip, 0), 0)
    if events is not None:
        events["reverse"] += end[2]
        events["clip term non-zero"] += clip != 0
    return end


def _settle(groups, score, events, what):
    """the losers of every group: all but the highest score, then the smallest index"""
    losers = []
    for members in groups.values():
        order = sorted(members, key=lambda i: (-score[i], i))
        losers += order[1:]
        if events is not None:
            if len(order) == 1:
                events["group of one"] += 1
            else:
                events["group won on score" if score[order[0]] > score[order[1]] else "group won on index"] += 1
                events[what] += 1
    return losers


def markdup(contigs, fq, hits, strand, flags=0, K=1, phred_offset=33, min_qual=15, events=None):
    """dup (uint8[n_reads]) and counts [reads with an end, reads flagged, pairs flagged, fragments flagged by a pair's end].
    contigs: [(name, start, len)]; fq: recs / qual; hits, strand: n_reads * K entries.  events: a dictionary that counts
    what happened (for the tests that require their cases to happen)."""
    hits, strand = np.asarray(hits).reshape(-1), np.asarray(strand).reshape(-1)
    n = len(fq.recs)
    assert len(hits) == len(strand) == n * K
    if events is not None:
        for k in ("group of one", "group won on score", "group won on index", "pair group", "fragment flagged by a pair", "fragment group",
                  "unplaced", "reverse", "clip term non-zero", "single group"):
            events.setdefault(k, 0)
    starts = [c[1] for c in contigs]
    quals = bytes(fq.qual)
    ends, score = [], []
    for r in range(n):
        ends.append(end_of(so.Slot(hits[K * r], strand[K * r], starts, contigs), events))
        rec = fq.recs[r]
        score.append(score_of(quals[int(rec["qual_off"]):int(rec["qual_off"]) + int(rec["qual_len"])], phred_offset, min_qual))
    if events is not None:
        events["unplaced"] += sum(e is None for e in ends)
    dup = np.zeros(n, dtype=np.uint8)
    counts = [sum(e is not None for e in ends), 0, 0, 0]
    if not flags & PAIRED:
        groups = defaultdict(list)
        for r, e in enumerate(ends):
            if e is not None:
                groups[e].append(r)
        for r in _settle(groups, score, events, "single group"):
            dup[r] = 1
        counts[1] = int(dup.sum())
        return dup, counts
    assert K == 1 and n % 2 == 0
    pair_groups, pair_score, pair_ends, fragments = defaultdict(list), {}, set(), []
    for p in range(n // 2):
        e1, e2 = ends[2 * p], ends[2 * p + 1]
        if e1 is not None and e2 is not None:
            lo, hi = sorted([e1 + (1,), e2 + (2,)])
            pair_groups[(lo[:3], hi[:3], lo[3] == 2)].append(p)
            pair_score[p] = score[2 * p] + score[2 * p + 1]
            pair_ends.update((e1, e2))
        elif e1 is not None or e2 is not None:
            fragments.append(2 * p if e1 is not None else 2 * p + 1)
    for p in _settle(pair_groups, pair_score, events, "pair group"):
        dup[2 * p] = dup[2 * p + 1] = 1
        counts[2] += 1
    frag_groups = defaultdict(list)
    for r in fragments:
        if ends[r] in pair_ends:
            dup[r] = 1
            counts[3] += 1
        else:
            frag_groups[ends[r]].append(r)
    if events is not None:
        events["fragment flagged by a pair"] += counts[3]
    for r in _settle(frag_groups, score, events, "fragment group"):
        dup[r] = 1
    counts[1] = int(dup.sum())
    return dup, counts


def sort_keys(contigs, hits, strand, flags=0, K=1, events=None):
    """key (uint64[n_reads * K]): ref_start of a placed slot that writes a line, the placed mate's of a paired unplaced one,
    2^64 - 1 for everything else"""
    hits, strand = np.asarray(hits).reshape(-1), np.asarray(strand).reshape(-1)
    starts = [c[1] for c in contigs]
    slots = [so.Slot(hits[s], strand[s], starts, contigs) for s in range(len(hits))]
    key = np.full(len(slots), U64_MAX, dtype=np.uint64)
    for s, me in enumerate(slots):
        r, k = divmod(s, K)
        writes = k == 0 or bool(flags & so.SECONDARY and me.placed and slots[r * K].placed)
        if writes and me.placed:
            key[s] = me.ref_start
        elif writes and flags & PAIRED and slots[s ^ 1].placed:
            key[s] = slots[s ^ 1].ref_start
    if events is not None:
        events["key UINT64_MAX"] = events.get("key UINT64_MAX", 0) + int((key == U64_MAX).sum())
    return key


def sort(key, records):
    """perm (the stable ascending sort of the indices by key), out_off and the permuted bytes of a list of bytes records"""
    perm = sorted(range(len(records)), key=lambda i: int(key[i]))  # sorted() is stable
    out = [records[i] for i in perm]
    return np.array(perm, dtype=np.uint64), so.offsets(out), b"".join(out)


def split(text, off):
    """the records of a buffer as a list of bytes"""
    text = bytes(text)
    return [text[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def add_dup_flag(lines, dup, K=1):
    """0x400 in FLAG of every placed line (0x4 clear) of a read with dup[r] != 0"""
    out = []
    for s, line in enumerate(lines):
        f = line.split(b"\t")
        if line and dup[s // K] and not int(f[1]) & 0x4:
            f[1] = b"%d" % (int(f[1]) | 0x400)
        out.append(b"\t".join(f))
    return out


def check_sorted_text(contig_names, unsorted_body, sorted_body):
    """Reads only SAM text: RNAME and POS of every line, RNAME mapped to its index in the contig list with "*" last; the sorted
    body must be the stable sort of the unsorted body's lines by (index, POS)."""
    rank = {name: i for i, name in enumerate(contig_names)}
    rank[b"*"] = len(contig_names)

    def where(line):
        f = line.split(b"\t")
        return rank[f[2]], int(f[3])
    before = bytes(unsorted_body).splitlines(keepends=True)
    after = bytes(sorted_body).splitlines(keepends=True)
    assert after == sorted(before, key=where), "the body is not the stable sort of its lines by (contig index, POS)"
    places = [where(line) for line in after]
    assert places == sorted(places)
    return places

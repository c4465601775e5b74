"""A restatement in plain Python of THE RULE of bg_bam_sites in include/biogpu.h: the candidate variant sites and the region
summaries of a batch of regions.  The counters come from tests/bam_pileup_oracle.py (16 columns, always), the reference is read
byte by byte, every position is judged on its own: nothing here knows of tiles, scans or shares.  `from_rows` derives the same
answer from pileup rows that something else produced.  Shares no code with the product."""
import bam_pileup_oracle as po

INVALID_ARG, TOO_LARGE, OPS_CAP, UNSUPPORTED = po.INVALID_ARG, po.TOO_LARGE, po.OPS_CAP, po.UNSUPPORTED
NONE = po.NONE
SNV, DEL, INS = 0, 1, 2
DEFAULT = dict(require=0, exclude=0x704, min_mapq=0, min_baseq=0, min_depth=0, min_alt=1, min_alt_permille=0, min_alt_strand=0, cover=(1, 10, 20, 30))
SITE_FIELDS = ("ref", "pos", "region", "kind", "ref_base", "alt", "depth", "ref_count", "alt_fwd", "alt_rev")
Refused = po.Refused


def params(**kw):
    return dict(DEFAULT, **kw)


def fold(b):
    return b - 32 if 97 <= b <= 122 else b


def check_text(regions, contigs, n_text):
    """the region error of the sites' own: a region's contig must lie inside the text"""
    for ref, beg, end in regions:
        if 0 <= ref < len(contigs) and contigs[ref][1] + contigs[ref][2] > n_text:
            raise Refused(INVALID_ARG)


def judge(row, ref_byte, ref, pos, region, p):
    """one position: ([site tuples in SITE_FIELDS order], depth, match, mismatch, unjudged)"""
    fwd, rev = row[:po.COLS], row[po.COLS:]
    both = [a + b for a, b in zip(fwd, rev)]
    depth = sum(both[c] for c in (po.A, po.C, po.G, po.T, po.OTHER, po.DEL))
    base = fold(ref_byte)
    if base not in b"ACGT":
        return [], depth, 0, 0, True
    ref_col = b"ACGT".index(base)
    candidates = [(SNV, c, b"ACGT"[c]) for c in range(4) if c != ref_col] + [(DEL, po.DEL, 0), (INS, po.INS, 0)]
    sites = []
    for kind, c, alt_byte in candidates:
        alt = fwd[c] + rev[c]
        if (depth >= p["min_depth"] and alt >= max(p["min_alt"], 1) and alt * 1000 >= p["min_alt_permille"] * depth
                and fwd[c] >= p["min_alt_strand"] and rev[c] >= p["min_alt_strand"]):
            sites.append((ref, pos, region, kind, base, alt_byte, depth, both[ref_col], fwd[c], rev[c]))
    return sites, depth, both[ref_col], sum(both[c] for c in range(4) if c != ref_col), False


def from_rows(rows16, row_off, regions, contigs, text, p):
    """sites, site_off and summaries from 16-column pileup rows: -> ([site tuples], site_off, [summary dicts])"""
    if p["min_alt_permille"] > 1000:
        raise Refused(INVALID_ARG)
    sites, site_off, summaries = [], [0], []
    for r, (ref, beg, end) in enumerate(regions):
        s = dict(sum_depth=0, match=0, mismatch=0, covered=[0, 0, 0, 0], max_depth=0, n_ref_other=0)
        for pos in range(beg, end):
            row = [int(v) for v in rows16[int(row_off[r]) + pos - beg]]
            got, depth, match, mismatch, unjudged = judge(row, text[contigs[ref][1] + pos], ref, pos, r, p)
            sites += got
            s["sum_depth"] += depth
            s["match"] += match
            s["mismatch"] += mismatch
            s["max_depth"] = max(s["max_depth"], depth)
            s["n_ref_other"] += unjudged
            for k in range(4):
                s["covered"][k] += depth >= p["cover"][k]
        site_off.append(len(sites))
        summaries.append(s)
    return sites, site_off, summaries


def sites(slots, contigs, text, regions, n_text=None, **kw):
    """-> ([site tuples], site_off, [summary dicts]); raises Refused as the call refuses.  n_text: the length the call is told
    where it is not len(text) (a refusal reads no byte)"""
    p = params(**kw)
    if p["min_alt_permille"] > 1000:
        raise Refused(INVALID_ARG)
    for ref, beg, end in regions:  # (all region checks come before the slots)
        if not (0 <= ref < len(contigs) and 0 <= beg <= end <= contigs[ref][2]):
            raise Refused(INVALID_ARG)
    check_text(regions, contigs, len(text) if n_text is None else n_text)
    rows, row_off = po.pileup(slots, contigs, regions, flags=po.STRANDS, require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"],
                              min_baseq=p["min_baseq"])
    return from_rows(rows, row_off, regions, contigs, text, p)


def as_tuples(arr):
    """a BAM_SITE_DTYPE array as the oracle's tuples"""
    return [tuple(int(rec[f]) for f in SITE_FIELDS) for rec in arr]


def as_dicts(arr):
    """a BAM_REGION_SUMMARY_DTYPE array as the oracle's dictionaries"""
    return [dict(sum_depth=int(s["sum_depth"]), match=int(s["match"]), mismatch=int(s["mismatch"]), covered=[int(v) for v in s["covered"]],
                 max_depth=int(s["max_depth"]), n_ref_other=int(s["n_ref_other"])) for s in arr]

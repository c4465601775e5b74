"""A restatement in plain Python of THE RULE of bg_bam_pileup in include/biogpu.h, written from the SAM specification (v1.6,
sections 1.4, 4.2 and 5.1.1): which slots are refused, which records are kept, what the walk of a CIGAR adds to which counter,
and where the rows of a batch of regions lie.  It walks every operation base by base into a dictionary keyed by (reference,
position) and knows nothing of tiles, keys or searches.  Shares no code with the product; `bam_oracle` only encodes records."""
import struct

import bam_oracle

INVALID_ARG, TOO_LARGE, OPS_CAP, UNSUPPORTED = -1, -8, -9, -11
NONE = 2**64 - 1
A, C, G, T, OTHER, DEL, SKIP, INS, COLS = range(9)
NAMES = ["A", "C", "G", "T", "OTHER", "DEL", "SKIP", "INS"]
STRANDS = 1
MAX_END = 1 << 29
M_OPS, REF_OPS, QUERY_OPS = (0, 7, 8), (0, 2, 3, 7, 8), (0, 1, 4, 7, 8)  # of MIDNSHP=X


class Refused(Exception):
    def __init__(self, status, slot=None):
        super().__init__(status, slot)
        self.status, self.slot = status, slot


def fields(rec):
    """the fixed fields, the CIGAR as (op, len), the 4-bit codes and the raw qualities of a record that passed `verdict`"""
    block, ref, pos, l_name, mapq, _, n_cigar, flag, l_seq = struct.unpack_from("<IiiBBHHHI", rec, 0)
    at = 36 + l_name
    words = struct.unpack_from("<%dI" % n_cigar, rec, at)
    at += 4 * n_cigar
    packed = rec[at:at + (l_seq + 1) // 2]
    codes = [(packed[k >> 1] >> (0 if k & 1 else 4)) & 15 for k in range(l_seq)]
    qual = rec[at + (l_seq + 1) // 2:at + (l_seq + 1) // 2 + l_seq]
    return dict(ref=ref, pos=pos, mapq=mapq, flag=flag, l_seq=l_seq, cigar=[(w & 15, w >> 4) for w in words], codes=codes, qual=qual)


def verdict(rec, contigs):
    """None, INVALID_ARG or UNSUPPORTED for one non-empty slot on its own; contigs: [(name, start, len)]"""
    if len(rec) < 36:
        return INVALID_ARG
    block, ref, pos, l_name, mapq, _, n_cigar, flag, l_seq = struct.unpack_from("<IiiBBHHHI", rec, 0)
    if block + 4 != len(rec) or 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > len(rec):
        return INVALID_ARG
    if ref >= len(contigs) or pos < -1:
        return INVALID_ARG
    cigar = [(w & 15, w >> 4) for w in struct.unpack_from("<%dI" % n_cigar, rec, 36 + l_name)]
    end = None
    if ref >= 0:
        span = sum(n for op, n in cigar if op in REF_OPS)
        end = pos + (span or 1)
        if end > 0 and end > contigs[ref][2]:
            return INVALID_ARG
    if any(op > 9 for op, _ in cigar):
        return INVALID_ARG
    if cigar and l_seq and sum(n for op, n in cigar if op in QUERY_OPS) != l_seq:
        return INVALID_ARG
    if end is not None and end > MAX_END:
        return UNSUPPORTED
    if ref >= 0 and len(cigar) == 2 and cigar[0] == (4, l_seq) and cigar[1][0] == 3:
        return UNSUPPORTED
    return None


def check(slots, contigs, regions):
    """raises Refused as the call refuses: the regions first, then the first offending slot (INVALID before UNSUPPORTED)"""
    for ref, beg, end in regions:
        if not (0 <= ref < len(contigs) and 0 <= beg <= end <= contigs[ref][2]):
            raise Refused(INVALID_ARG)
    prev = None
    for i, rec in enumerate(slots):
        if not rec:
            continue
        v = verdict(rec, contigs)
        ref, pos = struct.unpack_from("<ii", rec, 4) if len(rec) >= 12 else (-1, -1)
        key = (ref & 0xFFFFFFFF, pos)
        if v != INVALID_ARG and prev is not None and key < prev:
            v = INVALID_ARG
        if v is not None:
            raise Refused(v, i)
        prev = key


def kept(f, require, exclude, min_mapq):
    return (f["ref"] >= 0 and f["pos"] >= 0 and not f["flag"] & 4 and (f["flag"] & require) == require and not f["flag"] & exclude
            and f["mapq"] >= min_mapq)


def column(code):
    return {1: A, 2: C, 4: G, 8: T}.get(code, OTHER)


def walk(f, min_baseq):
    """[(position, column)] of one kept record, every count one entry"""
    out, r, q = [], f["pos"], 0
    for op, n in f["cigar"]:
        if op in M_OPS:
            for k in range(n):
                if not f["l_seq"]:
                    out.append((r + k, OTHER))
                elif f["qual"][q + k] >= min_baseq:
                    out.append((r + k, column(f["codes"][q + k])))
            r, q = r + n, q + n
        elif op == 1:
            if r > f["pos"]:
                out.append((r - 1, INS))
            q += n
        elif op in (2, 3):
            out += [(r + k, DEL if op == 2 else SKIP) for k in range(n)]
            r += n
        elif op == 4:
            q += n
    return out


def pileup(slots, contigs, regions, flags=0, require=0, exclude=0x704, min_mapq=0, min_baseq=0):
    """-> (rows: [[W counters]], row_off); raises Refused"""
    check(slots, contigs, regions)
    w = 2 * COLS if flags & STRANDS else COLS
    wanted = {ref for ref, beg, end in regions if end > beg}
    counts = {}
    for rec in slots:
        if not rec:
            continue
        f = fields(rec)
        if not kept(f, require, exclude, min_mapq) or f["ref"] not in wanted:
            continue
        base = COLS if flags & STRANDS and f["flag"] & 0x10 else 0
        for p, c in walk(f, min_baseq):
            counts.setdefault((f["ref"], p), [0] * w)[base + c] += 1
    rows, row_off = [], [0]
    zero = [0] * w
    for ref, beg, end in regions:
        rows += [list(counts.get((ref, p), zero)) for p in range(beg, end)]
        row_off.append(len(rows))
    return rows, row_off


# ---- records from SAM fields ------------------------------------------------------------------------------------------------
def record(name, flag, ref_name, pos1, mapq, cigar, seq, contigs, qual=b"*"):
    """the BAM record of a SAM line given by its fields (POS 1-based); qual: SAM text, b"*" for none"""
    line = b"\t".join([name, b"%d" % flag, ref_name, b"%d" % pos1, b"%d" % mapq, cigar, b"*", b"0", b"0", seq, qual]) + b"\n"
    return bam_oracle.record(line, contigs)


def sparse(rows, beg=0):
    """{position: {column name or index: count}} of the non-zero counters, as tests/golden/bam_pileup_kats.json writes rows"""
    out = {}
    for k, row in enumerate(rows):
        cells = {(NAMES[c] if c < COLS else str(c)): v for c, v in enumerate(row) if v}
        if cells:
            out[str(beg + k)] = cells
    return out

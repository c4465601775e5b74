"""A restatement in plain Python of the BAI rule of include/biogpu.h (SAM v1.6, section 5.2) on decoded records: `build` gives
the bytes bg_bam_index[_dev] must give, `parse` reads an index as a reader written from the specification would, and `query`
lists the chunks such a reader visits for a region (the specification's reg2bins and the linear-index cut).  Shares no code with
the product."""
import struct

from bam_oracle import CIGAR_OPS, PAYLOAD, offsets, reg2bin, split_records  # noqa: F401

PSEUDO_BIN = 37450
MAX_END = 2**29
INVALID_ARG, UNSUPPORTED = -1, -11


class Refused(Exception):
    """the rule refuses the records: status (INVALID_ARG or UNSUPPORTED) and the first offending slot"""

    def __init__(self, status, slot):
        super().__init__(status, slot)
        self.status, self.slot = status, slot


def stored_voff(base=0):
    """byte o of a stream framed by one bg_bgzf_frame call whose output starts at byte `base` of the file"""
    return lambda o: ((base + (o // PAYLOAD) * (PAYLOAD + 31)) << 16) | (o % PAYLOAD)


def table_voff(block_off, base=0):
    """... by one bg_bgzf_deflate call with the block table block_off"""
    return lambda o: ((base + int(block_off[o // PAYLOAD])) << 16) | (o % PAYLOAD)


def fields(rec, contigs):
    """(ref, pos, end, unmapped) of one record, or the status it is refused with"""
    if len(rec) < 36 or struct.unpack_from("<I", rec, 0)[0] + 4 != len(rec):
        return INVALID_ARG
    ref, pos, l_name, _, _, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHI", rec, 4)
    if 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > len(rec) or ref >= len(contigs) or pos < -1:
        return INVALID_ARG
    if ref < 0:
        return ref, pos, 0, bool(flag & 4)
    words = struct.unpack_from("<%dI" % n_cigar, rec, 36 + l_name)
    span = sum(w >> 4 for w in words if CIGAR_OPS[w & 15:(w & 15) + 1] in b"MDN=X")
    end = pos + (span or 1)
    if end > contigs[ref][2]:
        return INVALID_ARG
    if end > MAX_END:
        return UNSUPPORTED
    return ref, pos, end, bool(flag & 4)


def build(recs, contigs, voff):
    """recs: the record of every slot (b"": an empty slot); contigs: [(name, start, len)]; voff: stream offset -> virtual
    offset.  The bytes of the index; raises Refused."""
    at, prev = 0, None
    placed = [[] for _ in contigs]  # per reference, in file order: (beg offset, end offset, pos, end, unmapped)
    n_no_coor = 0
    for slot, rec in enumerate(recs):
        if not rec:
            continue
        f = fields(rec, contigs)
        if f == INVALID_ARG:
            raise Refused(INVALID_ARG, slot)
        key = struct.unpack_from("<Ii", rec, 4)  # ((uint32) refID, pos)
        if prev is not None and key < prev:
            raise Refused(INVALID_ARG, slot)
        if f == UNSUPPORTED:
            raise Refused(UNSUPPORTED, slot)
        prev = key
        if f[0] < 0:
            n_no_coor += 1
        else:
            placed[f[0]].append((at, at + len(rec), f[1], f[2], f[3]))
        at += len(rec)
    out = b"BAI\1" + struct.pack("<i", len(contigs))
    for rs in placed:
        if not rs:
            out += struct.pack("<ii", 0, 0)
            continue
        bins, last_bin = {}, None
        for beg, end_off, pos, end, _ in rs:
            b = reg2bin(pos, end)
            if b == last_bin:
                bins[b][-1][1] = voff(end_off)
            else:
                bins.setdefault(b, []).append([voff(beg), voff(end_off)])
            last_bin = b
        out += struct.pack("<i", len(bins) + 1)
        for b in sorted(bins):
            out += struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b])
        unmapped = sum(1 for r in rs if r[4])
        out += struct.pack("<IiQQQQ", PSEUDO_BIN, 2, voff(rs[0][0]), voff(rs[-1][1]), len(rs) - unmapped, unmapped)
        max_end = max(r[3] for r in rs)
        n_intv = ((max_end - 1) >> 14) + 1 if max_end > 0 else 0
        out += struct.pack("<i", n_intv)
        for w in range(n_intv):
            out += struct.pack("<Q", next(voff(r[0]) for r in rs if r[3] > w << 14))
    return out + struct.pack("<Q", n_no_coor)


def parse(bai):
    """-> (refs, n_no_coor); refs[r] = {"bins": {bin: [(beg, end)]}, "meta": None or (beg, end, mapped, unmapped),
    "intv": [ioffset]}.  Asserts what the specification fixes."""
    assert bai[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", bai, 4)
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", bai, at)
        at += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", bai, at + 16 * c) for c in range(n_chunk)]
            at += 16 * n_chunk
            assert b not in bins and (b < 37449 or b == PSEUDO_BIN)
            if b == PSEUDO_BIN:
                assert n_chunk == 2 and meta is None
                meta = chunks[0] + chunks[1]
            else:
                assert n_chunk > 0 and all(beg < end for beg, end in chunks)
                bins[b] = chunks
        n_intv, = struct.unpack_from("<i", bai, at)
        at += 4
        intv = list(struct.unpack_from("<%dQ" % n_intv, bai, at))
        at += 8 * n_intv
        refs.append({"bins": bins, "meta": meta, "intv": intv})
    n_no_coor, = struct.unpack_from("<Q", bai, at)
    assert at + 8 == len(bai)
    return refs, n_no_coor


def reg2bins(beg, end):
    """the specification's list of bins that may hold records overlapping [beg, end)"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def query(parsed, ref, beg, end):
    """the chunks a reader visits for [beg, end) of reference `ref`: those of reg2bins' bins that do not end at or before the
    linear index's offset for beg's window, sorted by start"""
    r = parsed[0][ref]
    if beg >= end:
        return []
    w = beg >> 14  # (behind the last window no record of the reference overlaps: any offset will do)
    min_off = r["intv"][w] if w < len(r["intv"]) else 0
    return sorted(c for b in reg2bins(beg, end) for c in r["bins"].get(b, ()) if c[1] > min_off)

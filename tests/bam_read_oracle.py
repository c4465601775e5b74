"""A restatement in plain Python of the rules of reading BAM in include/biogpu.h, written from the SAM specification (v1.6,
sections 4.2 and 5.2): the header parser, the verdict on a position, the serial walk over the records, the read decoder, the
coordinate key and the virtual offset of a byte of a stream in any BGZF framing.  Shares no code with the product; the tests
hold bg_bam_header_parse, bg_bam_records, bg_bam_reads, bg_bam_sort_keys and bg_bam_index_blocks to it."""
import struct

INVALID_ARG, OPS_CAP = -1, -9
NONE = 2**64 - 1
BASES = b"=ACMGRSVTWYHKDBN"
COMPLEMENT = dict(zip(b"AGCTYRWSKMDVHBN=", b"TCGARYWSMKHBDVN="))
ORIGINAL = 1
CHECK_OK, CHECK_EMPTY_ID, CHECK_NONASCII_SEQ, CHECK_INVALID_SEQ, CHECK_NONASCII_QUAL, CHECK_UNEQUAL = range(6)


class Short(Exception):
    """the prefix ends inside the header; need: the smallest length known to be required"""

    def __init__(self, need):
        super().__init__(need)
        self.need = need


class Refused(Exception):
    def __init__(self, first_bad=None):
        super().__init__(first_bad)
        self.first_bad = first_bad


def parse_header(b):
    """-> (text, [(name, start, len)], body_off); raises Short or Refused"""
    if len(b) >= 4 and b[:4] != b"BAM\1":
        raise Refused()
    if len(b) < 8:
        raise Short(12)
    l_text, = struct.unpack_from("<i", b, 4)
    if l_text < 0:
        raise Refused()
    at = 8 + l_text
    if len(b) < at + 4:
        raise Short(at + 4)
    n_ref, = struct.unpack_from("<i", b, at)
    if n_ref < 0:
        raise Refused()
    at += 4
    contigs, start = [], 0
    for i in range(n_ref):
        rest = 9 * (n_ref - i - 1)
        if len(b) < at + 4:
            raise Short(at + 9 + rest)
        l_name, = struct.unpack_from("<i", b, at)
        if l_name < 1:
            raise Refused()
        if len(b) < at + 4 + l_name + 4:
            raise Short(at + 4 + l_name + 4 + rest)
        if b[at + 4 + l_name - 1] != 0:
            raise Refused()
        l_ref, = struct.unpack_from("<i", b, at + 4 + l_name)
        if l_ref < 0:
            raise Refused()
        contigs.append((bytes(b[at + 4:at + 4 + l_name - 1]), start, l_ref))
        start += l_ref + 1
        at += 4 + l_name + 4
    return bytes(b[8:8 + l_text]), contigs, at


def verdict(s, o, n_ref, end=None):
    """the length of the accepted record at byte o of s[:end], or None"""
    end = len(s) if end is None else end
    if end - o < 36:
        return None
    block, ref, pos, l_name, _, _, n_cigar, _, l_seq, next_ref, next_pos = struct.unpack_from("<IiiBBHHHiii", s, o)
    if l_name < 1 or l_seq < 0:
        return None
    if block < 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq or o + 4 + block > end:
        return None
    if s[o + 36 + l_name - 1] != 0:
        return None
    if not (-1 <= ref < n_ref and -1 <= next_ref < n_ref and pos >= -1 and next_pos >= -1):
        return None
    return 4 + block


def walk(s, body_off, n_ref):
    """the record table: [body_off, ..., len(s)]; raises Refused with the records in front of what is no record"""
    off, at = [body_off], body_off
    while at != len(s):
        n = verdict(s, at, n_ref)
        if n is None:
            raise Refused(len(off) - 1)
        at += n
        off.append(at)
    return off


def candidates(s, body_off, n_ref):
    return [o for o in range(body_off, len(s)) if verdict(s, o, n_ref) is not None]


def slot_ok(s, o0, o1, n_ref):
    return o1 >= o0 and verdict(s, o0, n_ref, end=o1) == o1 - o0


def reads(s, off, n_ref, flags=0, require=0, exclude=0):
    """-> ([record dict], seq, seq_off, qual, qual_off, src) of the kept records; raises Refused with the first bad slot"""
    recs, seq, qual, seq_off, qual_off, src = [], b"", b"", [0], [0], []
    for i, (o0, o1) in enumerate(zip(off, off[1:])):
        if o0 == o1:
            continue
        if not slot_ok(s, o0, o1, n_ref):
            raise Refused(i)
    for i, (o0, o1) in enumerate(zip(off, off[1:])):
        if o0 == o1:
            continue
        l_name, _, _, n_cigar, flag, l_seq = struct.unpack_from("<BBHHHi", s, o0 + 12)
        if (flag & require) != require or (flag & exclude):
            continue
        at = o0 + 36 + l_name + 4 * n_cigar
        packed = s[at:at + (l_seq + 1) // 2]
        bases = bytes(BASES[(packed[k >> 1] >> (0 if k & 1 else 4)) & 15] for k in range(l_seq))
        q = s[at + (l_seq + 1) // 2:at + (l_seq + 1) // 2 + l_seq]
        q = b"" if l_seq and q[0] == 0xFF else bytes((b + 33) & 0xFF for b in q)
        if (flags & ORIGINAL) and (flag & 0x10):
            bases, q = bytes(COMPLEMENT[b] for b in reversed(bases)), q[::-1]
        id_len = l_name - 1
        if s[o0 + 36:o0 + 36 + id_len] == b"*":
            id_len = 0
        check = (CHECK_EMPTY_ID if id_len == 0 else CHECK_INVALID_SEQ if b"=" in bases else CHECK_NONASCII_QUAL if any(b >= 0x80 for b in q)
                 else CHECK_UNEQUAL if len(bases) != len(q) else CHECK_OK)
        recs.append(dict(id_off=o0 + 36, desc_off=o0 + 36 + id_len, seq_off=len(seq), qual_off=len(qual), id_len=id_len, desc_len=0,
                         seq_len=len(bases), qual_len=len(q), has_desc=0, check=check))
        seq += bases
        qual += q
        seq_off.append(len(seq))
        qual_off.append(len(qual))
        src.append(i)
    return recs, seq, seq_off, qual, qual_off, src


def fastq_text(s, recs, seq, qual):
    """the text bg_fastq_emit writes for these columns: @id, the bases, +, the qualities"""
    out = b""
    for r in recs:
        out += (b"@" + bytes(s[r["id_off"]:r["id_off"] + r["id_len"]]) + b"\n" + seq[r["seq_off"]:r["seq_off"] + r["seq_len"]] + b"\n+\n" +
                qual[r["qual_off"]:r["qual_off"] + r["qual_len"]] + b"\n")
    return out


def keys(s, off, contigs):
    """contigs: [(name, start, len)]; raises Refused"""
    out = []
    for i, (o0, o1) in enumerate(zip(off, off[1:])):
        if o0 == o1:
            out.append(NONE)
            continue
        if not slot_ok(s, o0, o1, len(contigs)):
            raise Refused(i)
        ref, pos = struct.unpack_from("<ii", s, o0 + 4)
        out.append(contigs[ref][1] + pos if ref >= 0 and pos >= 0 else NONE)
    return out


def blocks_voff(block_off, out_off):
    """the virtual offset of byte o of a stream framed into the members the tables name (bg_bgzf_blocks' tables)"""
    block_off, out_off = [int(x) for x in block_off], [int(x) for x in out_off]
    n = len(block_off) - 1

    def voff(o):
        b = next((b for b in range(n) if out_off[b + 1] > o), None)
        if b is None:
            b = next((b for b in range(n) if out_off[b] == o), n)
        return (block_off[b] << 16) | (o - out_off[b])
    return voff

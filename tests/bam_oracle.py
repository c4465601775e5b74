"""A restatement in plain Python of the BAM rule of include/biogpu.h (SAM v1.6, section 4.2): SAM line + contig table -> BAM
record, the BAM header, the BGZF framing (with zlib.crc32), and the way back: BAM record -> SAM fields.  Shares no code with
the product; the GPU tests compare `bg_bam_emit_batch[_dev]` and `bg_bgzf_frame[_dev]` with it byte for byte."""
import re
import struct
import zlib

PAYLOAD = 65280
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BASES = b"=ACMGRSVTWYHKDBN"
CIGAR_OPS = b"MIDNSHP=X"
MAX_REF = 2**31 - 1
MAX_QNAME = 254
MAX_CIGAR = 65535


class Unrepresentable(Exception):
    """the line is legal SAM that BAM has no encoding for"""


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def int_tag(v):
    """the smallest type that holds v, htslib's rule"""
    if v < 0:
        return (b"c", "<b") if v >= -128 else (b"s", "<h") if v >= -32768 else (b"i", "<i")
    return (b"C", "<B") if v <= 255 else (b"S", "<H") if v <= 65535 else (b"I", "<I")


def cigar_words(cigar):
    if cigar == b"*":
        return []
    return [(int(n) << 4) | CIGAR_OPS.index(op) for n, op in re.findall(rb"(\d+)([MIDNSHP=X])", cigar)]


def ref_length(words):
    return sum(w >> 4 for w in words if CIGAR_OPS[w & 15:(w & 15) + 1] in b"MDN=X")


def pack_seq(seq):
    codes = [BASES.index(bytes([b]).upper()) if bytes([b]).upper() in BASES else 15 for b in seq]
    if len(codes) & 1:
        codes.append(0)
    return bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))


def record(line, contigs):
    """the BAM record of one SAM line (with its newline); contigs: [(name, start, len)]"""
    f = line[:-1].split(b"\t")
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    names = [c[0] for c in contigs]

    def ref(name):
        if name == b"*":
            return -1
        c = names.index(name)
        if contigs[c][2] > MAX_REF:
            raise Unrepresentable(name)
        return c
    if len(qname) > MAX_QNAME:
        raise Unrepresentable(qname)
    ref_id = ref(rname)
    next_id = ref_id if rnext == b"=" else ref(rnext)
    pos0, next0 = int(pos) - 1, int(pnext) - 1
    words = cigar_words(cigar)
    span = ref_length(words)
    l_seq = 0 if seq == b"*" else len(seq)
    tags = b""
    for t in f[11:]:
        name, typ, val = t[:2], t[3:4], t[5:]
        if typ == b"i":
            code, fmt = int_tag(int(val))
            tags += name + code + struct.pack(fmt, int(val))
        else:
            assert typ == b"Z"
            tags += name + b"Z" + val + b"\0"
    field = words
    if len(words) > MAX_CIGAR:
        field = [(l_seq << 4) | 4, (span << 4) | 3]
        tags += b"CGBI" + struct.pack("<I", len(words)) + struct.pack("<%dI" % len(words), *words)
    body = struct.pack("<iiBBHHHIiii", ref_id, pos0, len(qname) + 1, int(mapq), reg2bin(pos0, pos0 + (span or 1)) & 0xFFFF, len(field), int(flag),
                       l_seq, next_id, next0, int(tlen))
    body += qname + b"\0" + struct.pack("<%dI" % len(field), *field)
    if l_seq:
        body += pack_seq(seq) + (b"\xff" * l_seq if qual == b"*" else bytes((q - 33) & 0xFF for q in qual))
    body += tags
    return struct.pack("<i", len(body)) + body


def records(lines, contigs):
    """the record of every slot (b"" where the slot writes no line); raises Unrepresentable if any line is"""
    return [record(ln, contigs) if ln else b"" for ln in lines]


def header(sam_text, contigs):
    out = b"BAM\1" + struct.pack("<i", len(sam_text)) + sam_text + struct.pack("<i", len(contigs))
    for name, _, ln in contigs:
        if ln > MAX_REF:
            raise Unrepresentable(name)
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", ln)
    return out


def block(payload):
    assert len(payload) <= PAYLOAD
    n = len(payload)
    return (b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, n + 30) +
            b"\x01" + struct.pack("<HH", n, n ^ 0xFFFF) + payload + struct.pack("<II", zlib.crc32(payload), n))


def frame(data, eof=False):
    data = bytes(data)
    return b"".join(block(data[i:i + PAYLOAD]) for i in range(0, len(data), PAYLOAD)) + (EOF_BLOCK if eof else b"")


def decode(rec, contigs):
    """the SAM fields (as sam_edge_cases.fields gives them for the line) of one BAM record"""
    size, = struct.unpack_from("<i", rec, 0)
    assert size + 4 == len(rec)
    ref_id, pos0, l_name, mapq, bin_, n_cigar, flag, l_seq, next_id, next0, tlen = struct.unpack_from("<iiBBHHHIiii", rec, 4)
    at = 36
    qname = rec[at:at + l_name - 1]
    assert rec[at + l_name - 1] == 0
    at += l_name
    words = list(struct.unpack_from("<%dI" % n_cigar, rec, at))
    at += 4 * n_cigar
    packed = rec[at:at + (l_seq + 1) // 2]
    at += (l_seq + 1) // 2
    seq = bytes(BASES[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
    q = rec[at:at + l_seq]
    at += l_seq
    qual = b"*" if not l_seq or q == b"\xff" * l_seq else bytes((b + 33) & 0xFF for b in q)
    tags = []
    while at < len(rec):
        name, typ = rec[at:at + 2], rec[at + 2:at + 3]
        at += 3
        if typ in b"cCsSiI":
            fmt = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}[typ]
            v, = struct.unpack_from(fmt, rec, at)
            assert int_tag(v)[0] == typ
            at += struct.calcsize(fmt)
            tags.append(name + b":i:%d" % v)
        elif typ == b"Z":
            end = rec.index(b"\0", at)
            tags.append(name + b":Z:" + rec[at:end])
            at = end + 1
        else:
            assert typ == b"B" and rec[at:at + 1] == b"I" and name == b"CG"
            n, = struct.unpack_from("<I", rec, at + 1)
            real = list(struct.unpack_from("<%dI" % n, rec, at + 5))
            at += 5 + 4 * n
            assert words == [(l_seq << 4) | 4, (ref_length(real) << 4) | 3] and n > MAX_CIGAR
            words = real
    assert at == len(rec)
    assert bin_ == reg2bin(pos0, pos0 + (ref_length(words) or 1)) & 0xFFFF
    cigar = b"".join(b"%d%c" % (w >> 4, CIGAR_OPS[w & 15]) for w in words) or b"*"

    def name_of(c):
        return b"*" if c < 0 else contigs[c][0]
    rnext = b"=" if next_id >= 0 and next_id == ref_id else name_of(next_id)
    return [qname, b"%d" % flag, name_of(ref_id), b"%d" % (pos0 + 1), b"%d" % mapq, cigar, rnext, b"%d" % (next0 + 1), b"%d" % tlen,
            seq if l_seq else b"*", qual] + tags


def split_records(body):
    """the records of a BAM body, one after the other"""
    out, at = [], 0
    while at < len(body):
        size, = struct.unpack_from("<i", body, at)
        out.append(body[at:at + 4 + size])
        at += 4 + size
    assert at == len(body)
    return out


def offsets(recs):
    import numpy as np
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs], dtype=np.uint64)
    return off

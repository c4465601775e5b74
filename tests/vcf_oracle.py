"""A restatement in plain Python of THE RULE of bg_vcf_emit in include/biogpu.h: the VCF lines of a list of candidate sites
(BAM_SITE_DTYPE records) and a list of indel events (BAM_INDEL_DTYPE records) with their inserted bases, against a contig
table ((name, start, len) triples) and the index text.  Every line is put together as a Python bytes object from its fields;
the order is a merge of the two lists written as such.  Nothing here knows of scans, binary searches, lanes or staging.  Shares
no code with the product."""
INVALID_ARG, TOO_LARGE, OPS_CAP = -1, -8, -9
NONE = 2**64 - 1
SNV, DEL, INS = 0, 1, 2
REF_TABLE = {**{b: b for b in b"ACGTN"}, **{b: ord("A") for b in b"MRWDHV"}, **{b: ord("C") for b in b"YSB"}, ord("K"): ord("G")}
TYPE = {SNV: b"snp", DEL: b"del", INS: b"ins"}


class Refused(Exception):
    def __init__(self, status, first_bad):
        super().__init__(status, first_bad)
        self.status, self.first_bad = status, first_bad


def fold(b):
    return b - 32 if 97 <= b <= 122 else b


def R(text, contigs, ref, p):
    return REF_TABLE.get(fold(text[contigs[ref][1] + p]), ord("N"))


def S(b):
    return b if b in b"ACGT" else ord("N")


def header(contigs):
    out = b"##fileformat=VCFv4.3\n##source=biogpu\n"
    for name, _, ln in contigs:
        out += b"##contig=<ID=" + bytes(name) + b",length=" + str(ln).encode() + b">\n"
    for key, kind, what in (("DP", "Integer", "Depth at the position or anchor"), ("RO", "Integer", "Reference observations"),
                            ("AO", "Integer", "Alternate observations"), ("SAF", "Integer", "Alternate observations on the forward strand"),
                            ("SAR", "Integer", "Alternate observations on the reverse strand"), ("TYPE", "String", "snp, del or ins")):
        out += ('##INFO=<ID=%s,Number=1,Type=%s,Description="%s">\n' % (key, kind, what)).encode()
    return out + b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def place_ok(ref, pos, contigs, n_text):
    return 0 <= ref < len(contigs) and contigs[ref][1] + contigs[ref][2] <= n_text and 0 <= pos < contigs[ref][2]


def site_ok(s, prev, contigs, text, n_text):
    ref, pos = int(s["ref"]), int(s["pos"])
    if not place_ok(ref, pos, contigs, n_text) or int(s["kind"]) not in (SNV, DEL, INS) or int(s["reserved"]):
        return False
    if prev is not None and (int(s["region"]), pos) < (int(prev["region"]), int(prev["pos"])):
        return False
    if int(s["kind"]) != SNV:
        return True
    return int(s["ref_base"]) == fold(text[contigs[ref][1] + pos]) and int(s["alt"]) in b"ACGT" and int(s["alt"]) != int(s["ref_base"])


def event_ok(e, prev, contigs, n_text, n_seq):
    ref, pos, n = int(e["ref"]), int(e["pos"]), int(e["len"])
    if not place_ok(ref, pos, contigs, n_text) or int(e["kind"]) not in (DEL, INS) or any(int(v) for v in e["reserved"]):
        return False
    if prev is not None and (int(e["region"]), pos) < (int(prev["region"]), int(prev["pos"])):
        return False
    if n == 0:
        return False
    if int(e["kind"]) == DEL:
        return pos + n < contigs[ref][2]
    return int(e["seq_off"]) + n <= n_seq


def check(sites, events, seq, contigs, text, n_text=None):
    """raises Refused(INVALID_ARG, the smallest index of the combined list that fails a check)"""
    n_text = len(text) if n_text is None else n_text
    for i, s in enumerate(sites):
        if not site_ok(s, sites[i - 1] if i else None, contigs, text, n_text):
            raise Refused(INVALID_ARG, i)
    for j, e in enumerate(events):
        if not event_ok(e, events[j - 1] if j else None, contigs, n_text, len(seq)):
            raise Refused(INVALID_ARG, len(sites) + j)


def site_line(s, contigs, text):
    ref, pos = int(s["ref"]), int(s["pos"])
    fwd, rev = int(s["alt_fwd"]), int(s["alt_rev"])
    info = "DP=%d;RO=%d;AO=%d;SAF=%d;SAR=%d;TYPE=snp" % (int(s["depth"]), int(s["ref_count"]), fwd + rev, fwd, rev)
    return b"\t".join([bytes(contigs[ref][0]), str(pos + 1).encode(), b".", bytes([R(text, contigs, ref, pos)]), bytes([int(s["alt"])]), b".", b".",
                       info.encode()]) + b"\n"


def event_line(e, seq, contigs, text):
    ref, pos, n, kind = int(e["ref"]), int(e["pos"]), int(e["len"]), int(e["kind"])
    fwd, rev = int(e["alt_fwd"]), int(e["alt_rev"])
    anchor = bytes([R(text, contigs, ref, pos)])
    if kind == DEL:
        ref_col, alt_col = anchor + bytes(R(text, contigs, ref, pos + 1 + k) for k in range(n)), anchor
    else:
        o = int(e["seq_off"])
        ref_col, alt_col = anchor, anchor + bytes(S(b) for b in seq[o:o + n])
    info = "DP=%d;AO=%d;SAF=%d;SAR=%d;TYPE=%s" % (int(e["depth"]), fwd + rev, fwd, rev, TYPE[kind].decode())
    return b"\t".join([bytes(contigs[ref][0]), str(pos + 1).encode(), b".", ref_col, alt_col, b".", b".", info.encode()]) + b"\n"


def lines(sites, events, seq, contigs, text, n_text=None):
    """-> [bytes]: the lines in the rule's order; raises Refused as the call refuses"""
    check(sites, events, seq, contigs, text, n_text)
    seq = bytes(seq)
    snvs = [s for s in sites if int(s["kind"]) == SNV]
    out, j = [], 0
    for s in snvs:  # a merge: the events with a smaller (region, pos) go first, an SNV in front of the events of its own key
        key = (int(s["region"]), int(s["pos"]))
        while j < len(events) and (int(events[j]["region"]), int(events[j]["pos"])) < key:
            out.append(event_line(events[j], seq, contigs, text))
            j += 1
        out.append(site_line(s, contigs, text))
    out += [event_line(e, seq, contigs, text) for e in events[j:]]
    return out


def emit(sites, events, seq, contigs, text, n_text=None):
    """-> (bytes, line_off)"""
    got = lines(sites, events, seq, contigs, text, n_text)
    off = [0]
    for ln in got:
        off.append(off[-1] + len(ln))
    return b"".join(got), off

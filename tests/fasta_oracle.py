"""bio::io::fasta::Reader::read / Records / Record::check (io/fasta.rs:334-359, 982-1009, 1090-1111) restated line by line on
`bytes`, and the reference-text rule of bg_fasta_reference[_dev] (include/biogpu.h) in numpy.  Test infrastructure: the
product never imports it."""
import numpy as np

# char::is_whitespace = the Unicode White_Space property, written out: bytes.rstrip strips fewer (ASCII only) and
# str.isspace more (U+001C..001F) than str::trim_end does
WHITE_SPACE = frozenset([0x9, 0xA, 0xB, 0xC, 0xD, 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F,
                         0x3000])


def trim_end(s):  # str::trim_end
    n = len(s)
    while n and ord(s[n - 1]) in WHITE_SPACE:
        n -= 1
    return s[:n]


class IoError(Exception):
    def __init__(self, pos):
        super().__init__(f"stream did not contain valid UTF-8 (line at byte {pos})")
        self.pos = pos


class MissingGt(Exception):
    pass


class _Reader:
    def __init__(self, text):
        self.text, self.pos, self.line, self.line_pos = bytes(text), 0, "", 0

    def read_line(self):  # BufRead::read_line into a cleared String: up to and including '\n', must be UTF-8
        a = self.pos
        e = self.text.find(b"\n", a)
        e = len(self.text) if e < 0 else e + 1
        try:
            s = self.text[a:e].decode("utf-8", "strict")
        except UnicodeDecodeError:
            raise IoError(a) from None
        self.pos, self.line, self.line_pos = e, s, a

    def read(self):  # fasta.rs:334-359
        if not self.line:
            self.read_line()
            if not self.line:
                return {"id": b"", "desc": None, "seq": b""}
        if not self.line.startswith(">"):
            raise MissingGt()
        body = trim_end(self.line[1:])
        cut = next((i for i, ch in enumerate(body) if ord(ch) in WHITE_SPACE), None)  # splitn(2, char::is_whitespace)
        rec = {"id": (body if cut is None else body[:cut]).encode(), "desc": None if cut is None else body[cut + 1:].encode(), "seq": b""}
        while True:
            self.line = ""
            self.read_line()
            if not self.line or self.line.startswith(">"):
                break
            rec["seq"] += trim_end(self.line).encode()
        return rec


def check(rec):  # fasta.rs:993-1009
    if not rec["id"]:
        return "EmptyId"
    if any(b >= 0x80 for b in rec["seq"]):
        return "NonAsciiSequence"
    if not all((65 <= b <= 90) or (97 <= b <= 122) or b in b"-.*" for b in rec["seq"]):
        return "InvalidSequence"
    return "ok"


def parse(text):
    """Records (fasta.rs:1090-1111) to its end: (records with their check, status, err_pos)"""
    r = _Reader(text)
    out = []
    while True:
        try:
            rec = r.read()
        except IoError as e:
            return out, "Io", e.pos
        except MissingGt:
            return out, "MissingGt", 0
        if not rec["id"] and rec["desc"] is None and not rec["seq"]:  # is_empty: the iterator ends
            return out, "ok", 0
        rec["check"] = check(rec)
        out.append(rec)


_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"AGCTYRWSKMDVHBN", b"TCGARYWSMKHBDVN"):  # dna::complement, as bg_revcomp_batch_dev maps bytes
    _COMP[_a], _COMP[_a + 32] = _b, _b + 32


def reference(records, fmd=False, upper=False):
    """(text: uint8 array, [(name, start, len)]): S0 $ S1 $ ... S(k-1) $, or T $ R $ with T = S0 $ ... S(k-1), R = revcomp(T)"""
    seqs = [np.frombuffer(r["seq"], dtype=np.uint8).copy() for r in records]
    if upper:
        for s in seqs:
            s[(s >= 97) & (s <= 122)] -= 32
    dollar = np.frombuffer(b"$", dtype=np.uint8)
    parts, contigs, start = [], [], 0
    for r, s in zip(records, seqs):
        contigs.append((r["id"], start, len(s)))
        parts += [s, dollar]
        start += len(s) + 1
    t = np.concatenate(parts)
    if not fmd:
        return t, contigs
    t = t[:-1]
    return np.concatenate([t, dollar, _COMP[t[::-1]], dollar]), contigs

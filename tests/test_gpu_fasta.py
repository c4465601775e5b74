"""bg_fasta_parse[_dev] and bg_fasta_reference[_dev] against the Python restatement (tests/fasta_oracle.py): the reference's own
cases, texts built around the kernels' tile size B (every carry between tiles: the open line's type, a pending run of white
space, a character or an invalid sequence that straddles the boundary, the running counts), one random text of ~300 tiles so
that the scan works across its chunks, and the reference builder in both layouts with its refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fasta_oracle as fo
from rust_bio_amd import _lib, fasta

pytestmark = pytest.mark.gpu
B = fasta.B
KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fasta_kats.json")))
EM = "\u2003".encode()  # E2 80 83, a three-byte member of White_Space


def fill(n, end_nl):
    """n bytes of 60-column sequence lines that end in a newline, or in a base"""
    s = bytearray()
    while len(s) < n:
        s += b"ACGTTGCAACGGATCCTTAGACGTTGCAACGGATCCTTAGACGTTGCAACGGATCCTTAG\n"
    s = s[:n]
    if n:
        s[-1] = 10 if end_nl else (65 if s[-1] == 10 else s[-1])
    return bytes(s)


def upto(pos, end_nl, head=b">r0 first\n"):
    """a text of exactly `pos` bytes: a header and sequence lines"""
    return head + fill(pos - len(head), end_nl)


def dev_parse(text, shift=0, rec_cap=None):
    """the device flavour as a fasta.Parsed; `shift`: bytes the text's base pointer is off a 256-byte boundary"""
    import torch
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    buf = torch.zeros(len(t) + shift + 16, dtype=torch.uint8, device="cuda")
    d_text = buf[shift:shift + len(t)]
    d_text.copy_(torch.from_numpy(t.copy()))
    n, status, err_pos, d_recs, d_seq, d_so = fasta.parse_dev(d_text, rec_cap=rec_cap)
    recs = d_recs.cpu().numpy().view(_lib.FAREC_DTYPE)
    so = d_so.cpu().numpy().view(np.uint64)
    seq = d_seq.cpu().numpy()[:int(so[n])]
    return fasta.Parsed(t, recs, seq, so, fasta.STATUS.index(status), err_pos)


def same(text, got, want=None):
    wrecs, wstatus, wpos = want or fo.parse(text)
    assert (got.status, got.err_pos, len(got)) == (wstatus, wpos, len(wrecs))
    assert int(got.seq_off[0]) == 0
    for k, w in enumerate(wrecs):
        r = got.record(k)
        assert (r._id, r._desc, r._seq, fasta.CHECK[r._check]) == (w["id"], w["desc"], w["seq"], w["check"]), k
        assert (int(got.recs["seq_off"][k]), int(got.recs["seq_len"][k])) == (int(got.seq_off[k]), len(w["seq"])), k


def both(text, shift=3):
    want = fo.parse(text)
    same(text, fasta.parse_arrays(text), want)
    same(text, dev_parse(text, shift), want)
    return want


@pytest.mark.parametrize("case", KATS["read"], ids=lambda c: c["name"])
def test_reference_cases(case):
    text = case["text"].encode("latin-1")
    recs, status, _ = both(text)
    assert status == case["status"] and [(r["id"], r["seq"], r["check"]) for r in recs] == [
        (w["id"].encode("latin-1"), w["seq"].encode("latin-1"), w["check"]) for w in case["records"]]


@pytest.mark.parametrize("case", KATS["check"], ids=lambda c: c["check"] + "@" + c["source"])
def test_reference_check_cases(case):
    text = b">" + case["id"].encode("latin-1") + (b" " + case["desc"].encode("latin-1") if case["desc"] is not None else b"") + b"\n" + \
        case["seq"].encode("latin-1") + b"\n"
    recs, _, _ = both(text)
    assert [r["check"] for r in recs] == [case["check"]]


TAIL = b">r1 second one\nACGTAC\nGT\n>r2\nTTGA\n"


def boundary_texts():
    out = {}
    for off in (B - 1, B, B + 1):
        out[f"gt-at-{off - B:+d}"] = upto(off, True) + TAIL  # a header starts there ('\n' at B - 1 with '>' at B among them)
        out[f"gt-inside-a-line-at-{off - B:+d}"] = upto(off, False) + b">ACGT\n" + TAIL
        out[f"no-trailing-lf-{off - B:+d}"] = upto(off, False)
        out[f"ends-in-lf-{off - B:+d}"] = upto(off, True)
    out["crlf-across"] = upto(B - 1, False) + b"\r\nACGT\n" + TAIL
    out["run-across-kept"] = upto(B - 3, False) + b"      AC\n" + TAIL
    out["run-across-trimmed"] = upto(B - 3, False) + b"  \t   \nAC\n" + TAIL
    out["run-to-the-boundary-trimmed"] = upto(B - 4, False) + b"    \nAC\n" + TAIL
    out["run-to-the-boundary-kept"] = upto(B - 4, False) + b"    AC\n" + TAIL
    for name, end in (("kept", b"G\nAC\n"), ("trimmed", b"\nAC\n"), ("at-the-end", b"")):
        out[f"long-run-{name}"] = b">r0\nAC" + b" " * (B + 100) + end + (TAIL if end else b"")
        out[f"very-long-run-{name}"] = upto(B - 40, False) + b" " * (3 * B + 17) + end + (TAIL if end else b"")
    out["long-run-in-a-header"] = b">r0 d" + b" " * (B + 100) + b"\nAC\n" + TAIL
    out["long-header"] = b">" + b"x" * (2 * B + 50) + b" some desc\nACGT\n" + TAIL
    out["long-description"] = upto(B - 100, True) + b">id " + b"d e " * (B // 2) + b"\nACGT\n" + TAIL
    for inner in (1, 2):  # the boundary falls in front of byte `inner` of the character
        out[f"em-trailing-trimmed-{inner}"] = upto(B - inner, False) + EM + b"\nAC\n" + TAIL
        out[f"em-trailing-kept-{inner}"] = upto(B - inner, False) + EM + b"AC\n" + TAIL
        out[f"em-separator-{inner}"] = upto(B - inner - 6, True) + b">ididi" + EM + b"desc " + EM + b"\nAC\n" + TAIL
        out[f"em-then-nbsp-trimmed-{inner}"] = upto(B - inner, False) + EM + b"\xc2\xa0 \xe3\x80\x80\r\nAC\n" + TAIL
        out[f"smiley-across-{inner}"] = upto(B - inner, False) + b"\xe2\x98\xb9 \nAC\n" + TAIL  # not white space: kept, NonAscii
        out[f"truncated-character-{inner}"] = upto(B - inner, False) + EM[:2] + b"AC\n" + TAIL
    for off in (B - 1, B):
        out[f"invalid-in-a-sequence-line-{off - B:+d}"] = upto(off, False) + b"\xffAC\n" + TAIL
        out[f"invalid-in-the-next-header-{off - B:+d}"] = upto(off - 3, True) + b">r1\xff d\nAC\n" + TAIL
        out[f"stray-continuation-{off - B:+d}"] = upto(off, False) + b"\x83AC\n" + TAIL
    out["invalid-in-the-first-line"] = b">r\xc0\x80\nAC\n" + TAIL
    out["invalid-after-an-empty-record"] = upto(B + 5, True) + b">\n\n" + upto(B, True) + b">z\xff\n"
    out["invalid-in-a-long-line"] = b">r0\n" + b"ACGT" * (B // 2) + b"\xf5" + b"ACGT" * B + b"\n" + TAIL
    out["empty-record-in-the-middle"] = b">a\nAC\n>\n\n>x\nAC\n"
    out["empty-record-across"] = upto(B - 1, True) + b">\n\r\n \n" + TAIL
    out["blank-header-with-a-sequence"] = upto(B - 1, True) + b">\n\r\n A\n" + TAIL
    out["empty"] = b""
    out["lf"] = b"\n"
    out["gt"] = b">"
    out["blank-first-line"] = b"\n" + TAIL
    out["eight-tiles-one-line"] = b">chr\n" + b"ACGTN" * (8 * B // 5 - 10)
    out["lines-of-one-byte"] = b">a\n" + b"A\n" * (B + 7) + TAIL
    out["headers-only"] = b"".join(b">h%d\n" % i for i in range(B // 3))
    return out


TEXTS = boundary_texts()


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_around_the_tile_boundary(name):
    assert len(TEXTS[name]) <= 8 * B + 100
    both(TEXTS[name])


def test_rec_cap_one_short():
    text = TEXTS["gt-at-+0"]  # three records
    for parse in (lambda cap: fasta.parse_arrays(text, rec_cap=cap), lambda cap: dev_parse(text, 5, rec_cap=cap)):
        same(text, parse(3))
        with pytest.raises(fasta.TooManyRecords) as e:
            parse(2)
        assert e.value.n_records == 3
        # header lines beyond rec_cap that an empty record cuts off: the count stays exact, and the records that fit are delivered
        cut = text + b">\n\n>x\nAC\n>y\nAC\n"
        same(cut, parse(3))
        with pytest.raises(fasta.TooManyRecords) as e:
            parse(2)
        assert e.value.n_records == 3


def random_text(seed, tiles):
    rng = np.random.default_rng(seed)
    parts, size, k = [], 0, 0
    while size < tiles * B:
        n = int(rng.choice([0, 1, 40, 700, B - 1, B, B + 1, 2 * B + 3, 3 * B])) if rng.random() < 0.6 else int(rng.integers(0, 3 * B))
        width = int(rng.choice([1, 50, 60, 61, 70, 80, 200]))
        eol = b"\r\n" if rng.random() < 0.3 else b"\n"
        s = rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), n).tobytes()
        rec = b">seq%d" % k + (b" len=%d  w=%d" % (n, width) if rng.random() < 0.7 else b"") + eol
        for a in range(0, n, width):
            w = width if rng.random() < 0.9 else int(rng.integers(1, width + 1))
            rec += s[a:a + width][:w] + (b" " * int(rng.integers(1, 4)) if rng.random() < 0.05 else b"") + eol
            if w < width:
                rec += s[a + w:a + width] + eol
        parts.append(rec)
        size += len(rec)
        k += 1
    return b"".join(parts)


def test_random_text_across_many_tiles():
    text = random_text(11, 300)
    want = fo.parse(text)
    assert want[1] == "ok" and len(want[0]) > 50
    same(text, dev_parse(text, 7), want)
    same(text, fasta.parse_arrays(text), want)


REF_TEXT = b">chr1 the first\nACGTacgtNNRY\nkmACGT\n>none\n>chrM\nggatccGGATCC\n" + upto(B + 77, True, b">long soft-masked\n").replace(b"TTAG", b"ttag")


@pytest.mark.parametrize("flags", [0, fasta.REF_FMD, fasta.REF_UPPER, fasta.REF_FMD | fasta.REF_UPPER])
def test_reference_builder(flags):
    import torch
    records, status, _ = fo.parse(REF_TEXT)
    assert status == "ok" and [len(r["seq"]) for r in records][:3] == [18, 0, 12]
    want, contigs = fo.reference(records, fmd=bool(flags & fasta.REF_FMD), upper=bool(flags & fasta.REF_UPPER))
    text, got = fasta.reference_arrays(fasta.parse_arrays(REF_TEXT), flags)
    assert text.tobytes() == want.tobytes()
    assert [(got.name(c), int(got.table["start"][c]), int(got.table["len"][c])) for c in range(len(got))] == contigs
    d_fa = torch.from_numpy(np.frombuffer(REF_TEXT, np.uint8).copy()).cuda()
    n, _, _, d_recs, d_seq, _ = fasta.parse_dev(d_fa)
    d_text, d_contigs, d_names, dgot = fasta.reference_dev(n, d_recs, d_fa, d_seq, flags)  # (a sizing call, then the build)
    assert d_text.cpu().numpy().tobytes() == want.tobytes()
    assert dgot.table.tobytes() == got.table.tobytes() and dgot.names.tobytes() == got.names.tobytes()


def test_reference_builder_refusals():
    import torch
    L = _lib.lib()
    ctx = _lib.default_context()
    d_fa = torch.from_numpy(np.frombuffer(REF_TEXT, np.uint8).copy()).cuda()
    n, _, _, d_recs, d_seq, _ = fasta.parse_dev(d_fa)
    nt, nb, bad = (C.c_uint64(0) for _ in range(3))
    tail = (C.byref(nt), C.byref(nb), C.byref(bad), None)
    want, _ = fo.reference(fo.parse(REF_TEXT)[0])
    d_out = torch.full((len(want) + 16,), 7, dtype=torch.uint8, device="cuda")
    d_tab = torch.full((n * 32,), 7, dtype=torch.uint8, device="cuda")
    d_names = torch.full((64,), 7, dtype=torch.uint8, device="cuda")

    def call(n_records=n, flags=0, text_cap=len(want), names_cap=64, recs=d_recs):
        return L.bg_fasta_reference_dev(ctx.h, n_records, recs.data_ptr(), d_fa.data_ptr(), d_seq.data_ptr(), flags, d_out.data_ptr(), text_cap,
                                        d_tab.data_ptr(), d_names.data_ptr(), names_cap, *tail)

    def untouched():
        torch.cuda.synchronize()
        return bool((d_out == 7).all() and (d_tab == 7).all() and (d_names == 7).all())

    assert call(n_records=0) == -1 and call(flags=4) == -1 and untouched()
    assert call(text_cap=len(want) - 1) == -9 and (nt.value, nb.value) == (len(want), 16) and untouched()
    assert call(names_cap=15) == -9 and untouched()
    # a record that fails check(): here '$' in a sequence, and an empty name in front of it would win
    bad_text = b">a\nAC\n>b\nA$C\n>\nGT\n"
    d_bad = torch.from_numpy(np.frombuffer(bad_text, np.uint8).copy()).cuda()
    nb_, _, _, d_brecs, d_bseq, _ = fasta.parse_dev(d_bad)
    assert nb_ == 3
    with pytest.raises(fasta.BadRecord) as e:
        fasta.reference_dev(nb_, d_brecs, d_bad, d_bseq)
    assert e.value.index == 1
    with pytest.raises(fasta.BadRecord) as e:
        fasta.reference_arrays(fasta.parse_arrays(bad_text), fasta.REF_FMD)
    assert e.value.index == 1
    assert call() == 0
    torch.cuda.synchronize()
    assert d_out.cpu().numpy()[:len(want)].tobytes() == want.tobytes() and (d_out[len(want):] == 7).all()

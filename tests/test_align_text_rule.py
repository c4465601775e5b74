"""The plain restatement of the two alignment texts (tests/align_text_oracle.py) pinned without a GPU: against the known answer
of tests/golden/fastq_kats.json, against the literal layouts of tests/test_oracle_pretty.py, against strings derived by hand
from the words of include/biogpu.h, and against the C++ oracle (`oracle_py.cigar` / `oracle_py.pretty`, a differently
structured statement of the same rule) on seeded random records that are consistent by construction."""
import numpy as np
import pytest

import align_text_cases as atc
import align_text_oracle as ato
import oracle_py as orc
from kat_util import load

U32 = atc.U32
X, Y = b"CCGTCCGGCAAGGG", b"AAAAACCGTTGACGGCCAA"


def test_cigar_known_answer():
    for c in load("fastq_kats.json")["cigar"]:
        ops = [{"Match": 0, "Subst": 1, "Del": 2, "Ins": 3}[o] for o in c["ops"]]
        assert ato.cigar(c["xstart"], c["xend"], c["xlen"], c["mode"], ops, False) == c["soft"]
        assert ato.cigar(c["xstart"], c["xend"], c["xlen"], c["mode"], ops, True) == c["hard"]
        assert ato.cigar(c["xstart"], c["xend"], c["xlen"], "custom", ops, False) is None


def test_cigar_hand_derived():
    M, S, D, I, XC, YC = range(6)
    for mode in (1, 2, 3):
        assert ato.cigar(0, 4, 4, mode, [M, M, XC, M, M], False) == "2=2="  # a clip byte prints nothing and ends the run
        assert ato.cigar(0, 4, 4, mode, [M, M, YC, XC, M, M], True) == "2=2="
        assert ato.cigar(0, 0, 0, mode, [XC], False) == ""  # only clip bytes
        assert ato.cigar(0, 0, 0, mode, [XC, YC, XC], True) == ""
        assert ato.cigar(3, 3, 5, mode, [YC, YC], False) == "3S2S"  # (there are operations: the two clips of x are written)
        assert ato.cigar(7, 9, 12, mode, [], False) == ""  # no operations: nothing, whatever the coordinates say
        assert ato.cigar(7, 9, 12, mode, [], True) == ""
        assert ato.cigar(2, 9, 8, mode, [M, S, S], False) == "2S1=2X"  # xlen < xend: no trailing clip
        assert ato.cigar(0, 3, 3, mode, [M, S, S], True) == "1=2X"
        assert ato.cigar(U32, 0, U32, mode, [D] * 12 + [I], True) == "4294967295H12D1I4294967295H"
        assert ato.cigar(1, 2, 3, mode, [I] * 10 + [M] * 100 + [I], False) == "1S10I100=1I1S"
    assert ato.cigar(0, 0, 0, 0, [], False) is None


def tokens_to_ops(tokens):
    return ["MSDIXY".index(t[0]) for t in tokens], [int(t[1:]) for t in tokens if t[0] in "XY"]


def reference_pair(mode, ncol=100, **kw):
    a = orc.align(orc.make_scoring(-5, -1, 1, -1, **kw), mode, X, Y)
    ops, clips = tokens_to_ops(a["ops"])
    return a, ato.pretty(dict(a, mode=mode), ops, clips, X, Y, ncol)


def test_pretty_literal_layouts():
    """the rows of tests/test_oracle_pretty.py"""
    _, s = reference_pair("local")
    assert s == ("     CCGTCCGGCAAGGG          \n"
                 "     ||||                    \n"
                 "AAAAACCGT          TGACGGCCAA\n\n\n")
    _, s = reference_pair("global")
    assert s == ("-----CCGTCCGGCAAGGG\n"
                 "xxxxx||||\\\\\\\\\\\\\\\\\\\\\n"
                 "AAAAACCGTTGACGGCCAA\n\n\n")
    _, s = reference_pair("local", ncol=10)
    blocks = s.split("\n\n\n")
    assert blocks[-1] == "" and len(blocks) == 4  # 29 columns -> 10 + 10 + 9
    rows = [b.split("\n") for b in blocks[:-1]]
    assert [len(r[0]) for r in rows] == [10, 10, 9] and all(len(r) == 3 and len(r[0]) == len(r[1]) == len(r[2]) for r in rows)
    assert "".join(r[0] for r in rows) == "     CCGTCCGGCAAGGG          "
    assert "".join(r[1] for r in rows) == "     ||||                    "
    assert "".join(r[2] for r in rows) == "AAAAACCGT          TGACGGCCAA"
    a, s = reference_pair("custom", xclip_prefix=-1, xclip_suffix=-1, yclip_prefix=0, yclip_suffix=0)
    assert any(t[0] in "XY" for t in a["ops"])
    rows = s.split("\n")
    assert len(rows[0]) == len(rows[1]) == len(rows[2]) == sum(int(t[1:]) if t[0] in "XY" else 1 for t in a["ops"])
    assert ato.pretty({"mode": "local", "xstart": 0, "ystart": 0}, [], [], b"", b"", 80) == ""


def test_pretty_hand_derived():
    r = atc.rec("custom", "MMMMX", b"ACGTTT", b"ACGT", clips=[2])  # a suffix Xclip(2) prints the FIRST two symbols of x
    assert atc.want_pretty(r, 80) == "ACGTAC\n||||  \nACGT  \n\n\n"
    r = atc.rec("custom", "YMMX", b"ACG", b"ttAC", clips=[2, 0])  # Yclip(2) in front, a zero-length Xclip behind
    assert atc.want_pretty(r, 80) == "  AC\n  ||\nttAC\n\n\n"
    r = atc.rec("global", "MSIDM", b"ACGT", b"AGtT")
    assert atc.want_pretty(r, 80) == "ACG-T\n|\\+x|\nAG-tT\n\n\n"
    assert atc.want_pretty(r, 2) == "AC\n|\\\nAG\n\n\nG-\n+x\n-t\n\n\nT\n|\nT\n\n\n"
    assert atc.want_pretty(r, 1) == "A\n|\nA\n\n\nC\n\\\nG\n\n\nG\n+\n-\n\n\n-\nx\nt\n\n\nT\n|\nT\n\n\n"
    assert atc.want_pretty(r, 5) == atc.want_pretty(r, 6) == atc.want_pretty(r, U32)
    r = atc.rec("local", "MMM", b"TTACGGG", b"cACGa", xstart=2, ystart=1)  # x prefix, y prefix, operations, x suffix, y suffix
    assert atc.want_pretty(r, 80) == "TT ACGGG \n   |||   \n  cACG  a\n\n\n"
    r = atc.rec("semiglobal", "MMM", b"CGT", b"aaCGTtt", ystart=2)
    assert atc.want_pretty(r, 80) == "  CGT  \n  |||  \naaCGTtt\n\n\n"
    r = atc.rec("global", "MMXMM", b"ACGGT", b"ACGT", clips=[1])  # a clip byte in a standard mode: x[0] again, the cursor moves on
    assert atc.want_pretty(r, 80) == "ACAGT\n|| ||\nAC GT\n\n\n"
    assert atc.want_pretty(atc.rec("local", "", b"ACGT", b"AC", xstart=1), 3) == ""
    for bad in (atc.rec("global", "MM", b"A", b"AC", xlen=1), atc.rec("global", "MM", b"AC", b"A"),  # past the end of x, of y
                atc.rec("local", "M", b"\x80A", b"A", xstart=1), atc.rec("global", "MI", b"A\xff", b"A"),  # flank, operation column
                atc.rec("global", "M", b"A", b"A", xlen=2)):  # not the record's sequences
        with pytest.raises(AssertionError):
            atc.want_pretty(bad, 80)
    with pytest.raises(ValueError):
        atc.want_pretty(r, 0)


def test_cigar_against_the_cpp_oracle_on_random_records():
    rng = np.random.default_rng(41)
    n_inner = n_text = 0
    for _ in range(6000):
        r = atc.random_cigar_record(rng)
        n_inner += bool((r["ops"] >= 4).any())
        for hard in (False, True):
            want = orc.cigar(r, r["ops"].astype(np.uint64), hard)
            assert atc.want_cigar(r, hard) == want, (r, hard)
            n_text += bool(want)
    assert n_inner >= 800 and n_text >= 7000, (n_inner, n_text)


@pytest.mark.parametrize("ncol", [1, 7, 16, 1000])
def test_pretty_against_the_cpp_oracle_on_random_records(ncol):
    rng = np.random.default_rng(100 + ncol)
    seen = {"text": 0, "panic": 0, "inner": 0, "modes": set()}
    for _ in range(2000):
        r = atc.random_pretty_record(rng)
        want = atc.pretty_or_none(orc.pretty, r, atc.u64_tokens(r), r["x"], r["y"], ncol)
        got = atc.pretty_or_none(atc.want_pretty, r, ncol)
        assert got == want, (r, ncol)
        seen["text"] += bool(want)
        seen["panic"] += want is None
        seen["inner"] += bool(r["mode"] and (r["ops"] >= 4).any())
        seen["modes"].add(r["mode"])
    assert seen["text"] >= 1500 and seen["panic"] >= 5 and seen["inner"] >= 200 and seen["modes"] == {0, 1, 2, 3}, seen

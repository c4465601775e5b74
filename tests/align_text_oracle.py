"""A second, plain statement of the two alignment texts of include/biogpu.h (`bg_cigar_batch[_dev]`, `bg_pretty_batch`), for the
tests.  Pure Python, written from the header's words and on purpose NOT in the shape of the kernels or of the C++ oracle
(oracle/fastq.cpp walks the operations with a `last` / counter pair and appends to three strings as it goes): the CIGAR is a
run-length grouping of the operation bytes, the pretty text three whole column lists that are cut into blocks afterwards.
Parity with bio-types itself stays unpinned, as the header says: the crate is not in the reference tree.

CIGAR.  "" without operations.  Otherwise `xstart` as a leading clip when > 0, one "<count><letter>" per run of equal
operation bytes with Match '=', Subst 'X', Del 'D', Ins 'I' — a clip byte inside the list prints nothing but does end the run
before it — and `xlen - xend` as the trailing clip when xlen > xend.  AlignmentMode::Custom is the crate's panic: None.

Pretty.  Rows x / marks / y, a column per operation ('|' Match, '\\\\' Subst, 'x' Del under a '-' in x, '+' Ins over a '-' in y).
The standard modes put x[:xstart] and then y[:ystart] in front and what the operations left of x, then of y, behind, against
blanks.  An Xclip / Yclip operation (AlignmentMode::Custom, or a clip byte in a standard-mode list) prints the FIRST `len`
symbols of its sequence, wherever it stands, and moves that sequence's cursor by as many.  The rows are cut every `ncol`
columns; a block is "x\\nmarks\\ny\\n\\n\\n".  "" without operations.  Where the crate panics — an operation past the end of a
sequence, or a byte >= 0x80 in a printed column (from_utf8_lossy widens it, the row-length assert fires) — and where the
sequences are not of the record's xlen / ylen (the C API's own refusal), `pretty` raises AssertionError."""
from itertools import groupby

CUSTOM, GLOBAL, SEMIGLOBAL, LOCAL = 0, 1, 2, 3
MATCH, SUBST, DEL, INS, XCLIP, YCLIP = 0, 1, 2, 3, 4, 5
LETTER = {MATCH: "=", SUBST: "X", DEL: "D", INS: "I"}
MODE_OF = {"custom": CUSTOM, "global": GLOBAL, "semiglobal": SEMIGLOBAL, "local": LOCAL}
BLANK, GAP = ord(" "), ord("-")


def mode_of(mode):
    return MODE_OF[mode.lower()] if isinstance(mode, str) else int(mode)


def cigar(xstart, xend, xlen, mode, ops, hard):
    """ops: the operation bytes (BG_OP_*).  -> str, or None where the crate panics (Custom)."""
    if mode_of(mode) == CUSTOM:
        return None
    ops = [int(o) for o in ops]
    if not ops:
        return ""
    clip = "H" if hard else "S"
    runs = [(kind, sum(1 for _ in g)) for kind, g in groupby(ops)]
    body = "".join("%d%s" % (k, LETTER[kind]) for kind, k in runs if kind in LETTER)
    lead = "%d%s" % (xstart, clip) if xstart > 0 else ""
    trail = "%d%s" % (xlen - xend, clip) if xlen > xend else ""
    return lead + body + trail


def pretty(rec, ops, clips, x, y, ncol):
    """rec: a mapping with mode, xstart, ystart and optionally xlen, ylen; ops: the operation bytes; clips: the lengths of the
    clip operations in their order (bg_alignment_t.clip_len: a fifth clip and later ones have length 0)."""
    x, y = bytes(x), bytes(y)
    if ncol < 1:
        raise ValueError("ncol == 0")
    if "xlen" in rec and "ylen" in rec:
        assert (len(x), len(y)) == (int(rec["xlen"]), int(rec["ylen"])), "not the sequences of this alignment"
    ops = [int(o) for o in ops]
    if not ops:
        return ""
    standard = mode_of(rec["mode"]) != CUSTOM
    clips = [int(c) for c in clips][:4]
    col_x, col_m, col_y = [], [], []

    def x_only(seg):
        col_x.extend(seg)
        col_m.extend([BLANK] * len(seg))
        col_y.extend([BLANK] * len(seg))

    def y_only(seg):
        col_y.extend(seg)
        col_m.extend([BLANK] * len(seg))
        col_x.extend([BLANK] * len(seg))

    xi = yi = 0
    if standard:
        xi, yi = int(rec["xstart"]), int(rec["ystart"])
        x_only(x[:xi])
        y_only(y[:yi])
    n_clip = 0
    for op in ops:
        if op >= XCLIP:
            length = clips[n_clip] if n_clip < len(clips) else 0
            n_clip += 1
            if op == XCLIP:
                x_only(x[:length])
                xi += len(x[:length])
            else:
                y_only(y[:length])
                yi += len(y[:length])
            continue
        takes_x, takes_y = op != DEL, op != INS
        assert not (takes_x and xi >= len(x)) and not (takes_y and yi >= len(y)), "an operation past the end of a sequence"
        col_x.append(x[xi] if takes_x else GAP)
        col_y.append(y[yi] if takes_y else GAP)
        col_m.append(b"|\\x+"[op])
        xi += takes_x
        yi += takes_y
    if standard:
        x_only(x[xi:])
        y_only(y[yi:])
    assert len(col_x) == len(col_m) == len(col_y)
    assert all(c < 0x80 for c in col_x + col_y), "a non-ASCII byte in a printed column"
    rows = [bytes(c).decode("ascii") for c in (col_x, col_m, col_y)]
    return "".join("".join(r[at:at + ncol] + "\n" for r in rows) + "\n\n" for at in range(0, len(col_m), ncol))

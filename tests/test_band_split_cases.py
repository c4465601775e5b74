"""The cases of tests/band_split_cases.py hold what they are for — shown with the CPU oracle alone, without a GPU: the
case file's copies of the kernels' constants equal the sources, every band is monotone with one interval per row,
split_of gives the (s_a, s_b) each name states, every listed combination is present, the oracle aligns every case
(orc.banded_align_bands: compute_alignment over the caller's band), and the gaps and mismatches of the border-move
family stand on the rows they are meant for in the oracle's own operation list."""
import os
import re

import numpy as np
import pytest

import band_split_cases as bc
import oracle_py as orc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rust-bio_amd", "csrc")


@pytest.fixture(scope="module")
def fam():
    f = dict(borders=bc.run_borders(), shapes=bc.row_shapes(), moves=bc.border_moves())
    f["mixes"] = bc.wavefront_mixes(f["borders"], f["shapes"], f["moves"])
    return f


def every_case(fam):
    return fam["borders"] + fam["shapes"] + fam["moves"]


def osc(kw):
    return orc.make_scoring(**kw)


def walk(rec):
    """[(op, row, column)] of an alignment: the cell each M / S / I / D arrives in"""
    i, j, out = rec["xstart"], rec["ystart"], []
    for op in rec["ops"]:
        if op[0] in "XY":
            continue  # (clips: xstart / ystart / xend / yend carry them)
        i += op in "MSI"
        j += op in "MSD"
        out.append((op, i, j))
    return out


def test_constants_equal_the_sources():
    def read(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def one(pattern, text):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return int(found[0])

    hdr = read("banded_kernels.h")
    assert one(r"constexpr uint32_t kSplitStripRows = (\d+);", hdr) == bc.STRIP_ROWS == 32
    assert one(r"constexpr uint32_t kTbRowAlign = (\d+);", hdr) == bc.TB_ROW_ALIGN == 16
    assert one(r"constexpr uint32_t kTbLineRows = (\d+);", hdr) == bc.TB_LINE_ROWS == 8
    for name in ("banded_fill2i.hip", "banded_fill2p.hip"):
        src = read(name)
        assert one(r"constexpr int RING = (\d+);", src) == bc.RING == 32, name
        flush = re.findall(r"constexpr int FLUSH = (RING / 2|\d+);", src)
        assert len(flush) == 1 and (bc.RING // 2 if flush[0] == "RING / 2" else int(flush[0])) == bc.FLUSH == 16, name
    # the rule split_of restates, and K4's two borders
    assert "s_a = max(1u, (rows0 + RS - 1) / RS);" in hdr and "s_b = min((bp.start_n - 1) / RS, (m - 1) / RS);" in hdr
    assert "if (m < 2 || bp.start_n < 1) return false;" in hdr and "return s_a < s_b;" in hdr
    k4 = read("banded_traceback.hip")
    assert "in_lo = s_a * kSplitStripRows + 1;" in k4 and "in_hi = s_b * kSplitStripRows;" in k4


def test_bands_are_monotone_with_one_interval_per_row(fam):
    for c in every_case(fam):
        assert len(c.start) == len(c.end) == c.n + 1 and c.n >= 1, c
        assert bc.monotone(c.start, c.end), c
        assert all(int(e) <= c.m + 1 for s, e in zip(c.start, c.end) if e > s), c
        rows = bc.rows_of(c.start, c.end, c.m)
        assert all(cells == max(cl - cf + 1, 0) for cf, cl, cells in rows), c  # (a hole: the device refuses the band)
        assert c.m <= 320 and c.n <= 400, c


def test_split_of_gives_what_each_name_states(fam):
    for c in every_case(fam):
        got = bc.split_of(c.start, c.end, c.m)
        stated = re.search(r":(?:a(\d+)b(\d+)|early)$", c.name)
        assert stated, c.name
        s_a, s_b = (int(stated.group(1)), int(stated.group(2))) if stated.group(1) else (0, 0)
        assert got == (s_a < s_b, s_a, s_b) == (c.has_run, c.s_a, c.s_b), (c, got)


def test_run_border_family_holds_every_border(fam):
    rb = fam["borders"]
    grid = [c for c in rb if re.match(r"rb\.e\d+\.s\d+\.m\d+:", c.name)]
    seen = {(c.meta["end_0"], c.meta["start_n"], c.m) for c in grid}
    assert seen == {(e, s, m) for e in bc.END_0 for s in bc.START_N for m in bc.RB_M if s <= m + 1}
    for c in grid:
        assert int(c.end[0]) == c.meta["end_0"] and (int(c.start[0]) == 0 or c.meta["end_0"] == 0), c
        assert int(c.start[-1]) == c.meta["start_n"], c
        assert (int(c.end[-1]) == c.m + 1) == (c.meta["start_n"] <= c.m), c
    # column 0 outside the band, the last column empty
    assert any(c.meta["end_0"] == 0 and c.end[0] <= c.start[0] for c in grid)
    assert any(c.end[-1] <= c.start[-1] and c.has_run for c in grid)
    # each term of s_b binds at least once, strictly
    assert any((c.m - 1) // 32 < (c.meta["start_n"] - 1) // 32 and c.has_run for c in grid)
    assert any((c.m - 1) // 32 > (c.meta["start_n"] - 1) // 32 and c.has_run for c in grid)
    # runs of exactly 0, 1 and 2 strips; one row (of column 0, of column n, of x) more or less decides
    assert {0, 1, 2} <= {c.s_b - c.s_a for c in grid}
    assert {c.strips for c in grid} == {0, 1, 2}
    by = {(c.meta["end_0"], c.meta["start_n"], c.m): c for c in grid}
    assert by[(32, 65, 65)].strips == 1 and by[(33, 65, 65)].strips == 0
    assert by[(1, 64, 65)].strips == 0 and by[(1, 65, 65)].strips == 1
    assert by[(1, 65, 64)].strips == 0 and by[(1, 65, 65)].strips == 1
    assert by[(64, 97, 97)].strips == 1 and by[(65, 97, 97)].strips == 0
    assert len(bc.one_row_short(rb)) >= 20 and all(c.s_a == c.s_b for c in bc.one_row_short(rb))
    # no run for another reason
    sn0 = [c for c in rb if c.m >= 2 and int(c.start[-1]) == 0]
    assert sn0 and not any(c.has_run for c in sn0)
    col0 = [c for c in rb if c.m >= 2 and int(c.start[-1]) >= 1 and bc.rows_of(c.start, c.end, c.m)[c.m][:2] == (0, 0)]
    assert col0 and not any(c.has_run for c in col0)
    assert any(c.m == 1 for c in rb) and sum(c.m == 0 for c in rb) >= 2


def test_row_shape_family_holds_every_shape(fam):
    shapes = fam["shapes"]
    seen = set()
    for c in shapes:
        rows = bc.rows_of(c.start, c.end, c.m)
        in_lo, in_hi = c.s_a * bc.STRIP_ROWS + 1, c.s_b * bc.STRIP_ROWS
        if "width" in c.meta:
            cf, cl, _ = rows[in_lo]
            assert cl - cf + 1 == c.meta["width"] and cf % bc.TB_ROW_ALIGN == c.meta["residue"], (c, cf, cl)
            assert cf >= 1
            if c.meta["width"] % 2 == 0:
                assert c.meta["left"] != c.meta["width"] - 1 - c.meta["left"]
            assert all(r[1] - r[0] + 1 == c.meta["width"] for r in rows[in_lo:in_hi + 1]), c  # every row of the run
            seen.add((c.meta["width"], c.meta["residue"]))
        for r, d in c.meta.get("jumps", ()):
            assert in_lo <= r < in_hi and rows[r + 1][0] - rows[r][0] == d, (c, r, rows[r], rows[r + 1])
        if "hold" in c.meta:
            r, k = c.meta["hold"]
            assert in_lo <= r and r + k <= in_hi
            assert len({rows[r + t][0] for t in range(k + 1)}) == 1 and rows[r - 1][0] != rows[r][0] != rows[r + k + 1][0], c
    assert seen == {(w, r) for w in bc.WIDTHS for r in bc.CF_RESIDUES}
    assert bc.WIDTHS == (1, 15, 16, 17, 31, 32, 33) and bc.CF_RESIDUES == (0, 1, 15)
    assert [d for _, d in bc.JUMPS] == [17, 40] and bc.HOLD[1] == 20
    assert any("jumps" in c.meta for c in shapes) and any("hold" in c.meta for c in shapes)


def test_wavefront_mixes_hold_every_combination(fam):
    mixes = fam["mixes"]
    assert sorted(mixes) == [1, 2, 7, 8, 9, 17] and all(len(b) == size for size, b in mixes.items())
    pool = {c.name for c in every_case(fam)}
    couples = set()
    for size, batch in mixes.items():
        assert all(c.name in pool for c in batch)
        couples |= {(batch[g].kind, batch[g + 1].kind) for g in range(0, size - 1, 2)}
        for g0 in range(0, size - 6, 8):  # every group of eight consecutive pairs (the batch of seven: its only group)
            group = batch[g0:g0 + 8]
            if len(group) < 7:
                continue
            runs = [c for c in group if c.has_run]
            assert any(not c.has_run and c.m >= 2 for c in group) and any(c.strips == 1 for c in group)
            longest = max(c.strips for c in every_case(fam))
            assert any(c.strips == longest for c in group), (size, g0)
            lo = min(c.s_a for c in runs)
            hi = max(c.s_b for c in runs)
            assert not any(c.s_a == lo and c.s_b == hi for c in runs), (size, g0)
    assert couples == {(a, b) for a in "NOLZ" for b in "NOLZ"}
    assert [size % 2 for size in sorted(mixes)] == [1, 0, 1, 0, 1, 1]  # the odd ones leave the last slot without a partner
    for batch in mixes.values():
        o = bc.orders(batch)
        assert [c.name for c in o["reversed"]] == [c.name for c in batch][::-1]
        assert [c.name for c in o["rotated"]] == [c.name for c in batch][1:] + [batch[0].name]


@pytest.mark.parametrize("scoring", bc.SCORINGS, ids=[s[0] for s in bc.SCORINGS])
def test_oracle_aligns_every_case(fam, scoring):
    _, mode, kw = scoring
    cases = bc.admitted(every_case(fam), kw)
    assert len(every_case(fam)) - len(cases) <= 1  # (row m inside column 0 only: no alignment without a y-suffix clip)
    panics = 0
    for c in cases:
        try:
            got = orc.banded_align_bands(osc(kw), mode, c.x, c.y, c.start, c.end)
        except RuntimeError:
            panics += 1
            continue
        assert got["band_cells"] == int(np.maximum(c.end.astype(np.int64) - c.start.astype(np.int64), 0).sum()), c
        assert (got["xlen"], got["ylen"]) == (c.m, c.n)
    assert panics == 0


def test_oracle_refuses_a_range_past_row_m():
    c = bc.border_moves()[0]
    end = c.end.copy()
    end[c.n // 2] = c.m + 2
    with pytest.raises(RuntimeError):
        orc.banded_align_bands(osc(bc.SCORINGS[0][2]), "semiglobal", c.x, c.y, c.start, end)


@pytest.mark.parametrize("scoring", bc.SCORINGS[:3], ids=[s[0] for s in bc.SCORINGS[:3]])
def test_border_moves_stand_on_their_rows(fam, scoring):
    """the oracle's own operations: Ins on every inserted row, the D run on the stated row, Subst on rows in_lo / in_hi"""
    _, mode, kw = scoring
    tags = set()
    for c in fam["moves"]:
        in_lo, in_hi = c.meta["in_lo"], c.meta["in_hi"]
        assert (in_lo, in_hi) == (c.s_a * bc.STRIP_ROWS + 1, c.s_b * bc.STRIP_ROWS)
        steps = walk(orc.banded_align_bands(osc(kw), mode, c.x, c.y, c.start, c.end))
        at = {}
        for op, i, j in steps:
            at.setdefault(i, []).append(op)
        if c.meta["ins_rows"]:
            rows = c.meta["ins_rows"]
            assert rows in ([in_lo - 2, in_lo - 1, in_lo, in_lo + 1], [in_hi - 1, in_hi, in_hi + 1, in_hi + 2])
            assert all(at[r][0] == "I" for r in rows) and at[rows[0] - 1][0] != "I" and at[rows[-1] + 1][0] != "I", (c, kw)
            tags.add("ins_lo" if rows[0] < in_lo else "ins_hi")
        for r in c.meta["del_rows"]:
            assert r in (in_lo - 1, in_lo, in_hi, in_hi + 1)
            assert at[r][1:] == ["D"] * bc.DEL_LEN and at[r][0] in "MS" and "D" not in at[r - 1] + at[r + 1], (c, kw, at[r])
            tags.add(("del_lo", r - in_lo) if r <= in_lo else ("del_hi", r - in_hi))
        if c.meta["sub_rows"]:
            assert c.meta["sub_rows"] == [in_lo, in_hi] and at[in_lo] == ["S"] and at[in_hi] == ["S"], (c, kw)
            tags.add("subst")
    assert tags == {"ins_lo", "ins_hi", ("del_lo", -1), ("del_lo", 0), ("del_hi", 0), ("del_hi", 1), "subst"}


def test_bands_entry_equals_the_match_entry_on_a_kmer_band():
    """a stripe built from real k-mer matches: banded_align_bands over the band banded_align_with reports is
    banded_align_with itself"""
    rng = np.random.default_rng(11)
    for t, (_, mode, kw) in enumerate(bc.SCORINGS):
        x, y, _, _ = bc.make_pair(rng, 300, 40, 8, 8, 1, 280, ins=[(120, 6)], dels=[(200, 9)], n_sub=15)
        x, y = x.tobytes(), y.tobytes()
        mm = orc.find_kmer_matches(x, y, 8)
        assert len(mm) > 50
        a = orc.banded_align_with(osc(kw), mode, 8, 6, x, y, mm, want_band=True)
        start, end = a.pop("band")
        b = orc.banded_align_bands(osc(kw), mode, x, y, start, end)
        assert a == b, (kw, a, b)
        assert bc.split_of(start, end, len(x))[0]  # (such a band has an interior run)

"""The inputs of tests/dev_align_cases.py hold what tests/test_gpu_dev_pointer_alignment.py relies on — shown without a GPU,
from the CPU oracles alone: the FASTQ texts parse, their records straddle the one-pass kernel's tiles and their headers put
the first space at every offset of the 8-byte scan, the packed lengths hit every remainder that matters, both dword cases of
the traceback's stores occur, the tiered batch copies re-seeded operations both with vectors and with bytes, the SAM lines
have every head / body / tail shape.  The case file's copies of the kernels' constants, and the address-dependent source
lines the GPU module's docstring lists, are compared with the sources: a tile size or a guard that changes fails here."""
import os
import re

import numpy as np
import pytest

import dev_align_cases as dc
import oracle_py as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-bio_amd", "csrc")


def source(name):
    with open(os.path.join(ROOT, "include", name) if name == "biogpu.h" else os.path.join(CSRC, name)) as f:
        return f.read()


def one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


def test_constants_equal_the_sources():
    fq = source("fastq_ingest.hip")
    assert one(r"constexpr uint32_t kTile = (\d+),", fq) == dc.FQ_TILE
    assert one(r"constexpr int32_t kHaloBytes = (\d+);", fq) == dc.FQ_HALO
    assert one(r"constexpr uint32_t kChunk = (\d+);", fq) == dc.FQ_CHUNK
    assert one(r"const uint64_t wstart = end >= (\d+) \? end - \d+ : 0;", fq) == dc.FQ_HALO
    assert one(r"#define BG_FASTA_TILE (\d+)", source("biogpu.h")) == dc.FA_TILE
    from rust_bio_amd import fasta
    assert fasta.B == dc.FA_TILE
    sam = source("sam_emit.hip")
    assert one(r"constexpr uint32_t kStage = (\d+);", sam) + 16 == dc.SAM_STAGE and "kStageBuf = kStage + 16;" in sam
    assert one(r"#define SAM_LONG_LINE (\d+)u", source("sam_rule.h")) == dc.SAM_LONG_LINE
    import sam_edge_cases as ec
    assert (ec.STAGE, ec.LONG_LINE) == (dc.SAM_STAGE, dc.SAM_LONG_LINE)
    import band_edge_cases as bec
    assert set(dc.BAND_TILE_N) <= set(bec.TILE_N) and bec.BAND_TILE == 2048


def test_the_listed_source_lines_are_where_the_gpu_module_says():
    """the file:line list of the GPU module's docstring, entry by entry: the line still holds the access or the guard"""
    import test_gpu_dev_pointer_alignment as gpu
    listed, name = set(), None
    for full, line in re.findall(r"(?:\b(\w+\.(?:hip|h))|[ (]):(\d+)\b", gpu.__doc__):
        name = full or name  # ":57" behind "fastq_ingest.hip:42" is a line of the same file
        listed.add((name, line))
    table = {(f, str(line)) for f, line, _ in gpu.ACCESSES}
    assert listed == table, (sorted(listed - table), sorted(table - listed))
    for name, line, snippet in gpu.ACCESSES:
        assert snippet in source(name).split("\n")[line - 1], (name, line, snippet)


# ---- FASTQ -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parsed():
    return {name: orc.fastq_parse(text) for name, (text, _) in dc.fastq_texts().items()}


def test_fastq_texts_parse_with_the_expected_record_count(parsed):
    texts = dc.fastq_texts()
    assert sorted(texts) == ["crlf", "lf", "long-lines", "mid-lines", "no-final-newline", "non-ascii"]
    left_out = [name for name in texts if name not in parsed]
    assert left_out == []
    for name, (text, n) in texts.items():
        recs, status, _ = parsed[name]
        assert status == "ok" and len(recs) == n, name
        assert len(dc.record_spans(text)) == n, name
        # every record but those made otherwise passes check(); an empty id is EmptyId
        for w in recs:
            assert w["check"] == ("ok" if w["id"] else "EmptyId"), (name, w["id"])
    assert b"\r\n" in texts["crlf"][0] and b"\r" not in texts["lf"][0]
    assert not texts["no-final-newline"][0].endswith(b"\n") and texts["lf"][0].endswith(b"\n")
    assert all(150 == len(w["seq"]) == len(w["qual"]) for name in ("lf", "crlf", "no-final-newline") for w in parsed[name][0])
    assert [w["qual"] for w in parsed["crlf"][0] if w["qual"].endswith(b"\r")] == []


def test_a_record_crosses_each_tile_boundary():
    for name in ("lf", "crlf", "no-final-newline", "non-ascii"):
        text, _ = dc.fastq_texts()[name]
        assert 3 * dc.FQ_TILE < len(text) < 3.3 * dc.FQ_TILE, name
        spans = dc.record_spans(text)
        for b in (dc.FQ_TILE, 2 * dc.FQ_TILE, 3 * dc.FQ_TILE):
            inside = [(s, e) for s, e in spans if s < b < e]
            assert len(inside) == 1, (name, b)
            # ... and the four newlines in front of the boundary lie in the halo: one window of the search
            assert text[b - dc.FQ_HALO:b].count(b"\n") >= 4, (name, b)


def test_the_first_space_of_a_header_stands_at_every_offset(parsed):
    for name in ("lf", "crlf", "no-final-newline"):
        recs = parsed[name][0]
        with_desc = {len(w["id"]) for w in recs if w["desc"] is not None}
        assert with_desc == set(dc.SPACE_OFFSETS), name
        assert any(w["desc"] is None and len(w["id"]) == 20 for w in recs), name  # no space at all: both words and the byte loop
        # the header's position mod 8 varies too: the scan starts before, inside and after the first 8-byte word
        text = dc.fastq_texts()[name][0]
        assert {(s + 1) % 8 for s, _ in dc.record_spans(text)} == set(range(8)), name
    assert {len(w["id"]) for w in parsed["long-lines"][0][:2]} == {3, 12}


def test_the_long_lines_exceed_a_tile(parsed):
    text, _ = dc.fastq_texts()["long-lines"]
    lines = text.split(b"\n")
    assert sorted(len(x) for x in lines)[-4:] == [20_000, 20_000, 20_011, 20_011] and 20_000 > dc.FQ_TILE
    assert len(text) // len(lines) > 256  # the general kernels gather with a wavefront per record
    for name in ("lf", "crlf"):
        t = dc.fastq_texts()[name][0]
        assert len(t) // t.count(b"\n") <= 256, name  # ... and with 16 lanes per record here
    # the search in front of a tile runs through all its windows and gives up: the general kernels take this text
    assert not dc.one_pass_finds_its_lines(text) and one(r"constexpr int kHaloWindows = (\d+);", source("fastq_ingest.hip")) == dc.FQ_WINDOWS
    for s, e in dc.record_spans(text)[:2]:
        last_tile = (e - 1) // dc.FQ_TILE * dc.FQ_TILE
        assert (last_tile - text.rfind(b"\n", 0, last_tile)) > 2 * dc.FQ_HALO  # several windows without a newline
    # lines of 9 - 14 KB stay with the one-pass kernel, like the short reads; the headers of the long records lie more than the
    # halo in front of the tile the record ends in (their 8-byte words are read from memory), with the first space in the first
    # word, in the second, behind both, and missing
    for name in ("lf", "crlf", "no-final-newline", "mid-lines"):
        assert dc.one_pass_finds_its_lines(dc.fastq_texts()[name][0]), name
    mid = dc.fastq_texts()["mid-lines"][0]
    spans = dc.record_spans(mid)[0::2]
    assert all((e - 1) // dc.FQ_TILE * dc.FQ_TILE - s > dc.FQ_HALO for s, e in spans) and len(spans) == 6
    ids = [w for w in parsed["mid-lines"][0][0::2]]
    assert [len(w["id"]) for w in ids] == [0, 5, 10, 20, 2, 7] and ids[3]["desc"] is None
    assert len({(s + 1) % 8 for s, _ in spans}) >= 4  # the header's second byte on and off the 8-byte boundary
    # every window of that search starts at a multiple of 16 of the text (tiles and windows are multiples of 1024, or 0):
    # the `(wstart & 15) == 0` half of the guard can never be false, only `aligned` decides
    assert dc.FQ_TILE % dc.FQ_HALO == 0 and dc.FQ_HALO % 16 == 0


def test_the_non_ascii_byte_lies_in_the_second_tile(parsed):
    text, _ = dc.fastq_texts()["non-ascii"]
    high = [i for i, c in enumerate(text) if c >= 0x80]
    assert len(high) == 2 and dc.FQ_TILE < high[0] < 2 * dc.FQ_TILE
    assert sum(w["desc"] == "é desc".encode() for w in parsed["non-ascii"][0]) == 1


# ---- pack2 -------------------------------------------------------------------------------------------------------------------
def test_pack_lengths_and_invalid_bytes():
    assert {n % 16 for n in dc.PACK_N} >= {0, 1, 15} and {n // 16 for n in dc.PACK_N} >= {0, 1, 2, 256}
    from rust_bio_amd.pack2 import pack_numpy
    names = set()
    for n in dc.PACK_N:
        cases = dc.pack_inputs(n)
        assert cases[0][2] == 0 and not set(cases[0][1]) - set(b"ACGT")
        assert b"A" not in cases[0][1][::16]  # a word whose first byte is dropped packs differently
        for name, data, bad in cases:
            names.add(name)
            assert len(data) == n and sum(c not in b"ACGT" for c in data) == bad
            words = pack_numpy(np.frombuffer(data, np.uint8))
            # the layout, restated once more: symbol s in bits 2 (s % 16) .. + 1 of dword s / 16, an invalid byte as code 0
            for s in (0, n // 2, n - 1):
                assert (int(words[s // 16]) >> (2 * (s % 16))) & 3 == max(0, b"ACGT".find(bytes([data[s]])))
        places = {name: [i for i, c in enumerate(data) if c == dc.INVALID] for name, data, _ in cases[1:]}
        assert places["first-word"] == [0]
        if n >= 32:
            assert places["last-whole-word"][0] // 16 == n // 16 - 1
        if n % 16 and n > 16:
            assert places["tail"][0] >= 16 * (n // 16)
    assert names == {"valid", "first-word", "last-whole-word", "tail"}


# ---- pairwise ----------------------------------------------------------------------------------------------------------------
def test_pairwise_batch_and_the_dword_cases():
    xs, ys = dc.sw_pairs()
    assert len(xs) == dc.SW_PAIRS == 37 and {len(x) for x in xs} == {dc.SW_M} and {len(y) for y in ys} == {dc.SW_N}
    assert dc.SW_PAIRS % 64 != 0 and all(s >= dc.SW_M + dc.SW_N + 4 for s in dc.SW_STRIDES)
    from rust_bio_amd import _lib
    x, xo = _lib.concat(xs)
    y, yo = _lib.concat(ys)
    ran = 0
    for mode in ("local", "semiglobal"):
        out, ops, stride = orc.align_batch(orc.make_scoring(**dc.SW_SCORES), mode, x, xo, y, yo, threads=8)
        assert len(out) == 37 and (out["n_ops"] > 0).sum() >= 30 and len({int(v) % 4 for v in out["n_ops"]}) == 4, mode
        ran += 1
    assert ran == 2
    even, odd = dc.SW_STRIDES
    assert even % 4 == 0 and odd % 4 == 1
    for res in dc.SW_OPS_RES:
        assert {dc.dword_ok(res, even, p) for p in range(37)} == {res == 0}
        assert {dc.dword_ok(res, odd, p) for p in range(37)} == {False, True}
        assert {(p + 1) * odd % 2 for p in range(37)} == {0, 1}


def test_revcomp_sequences():
    seqs = dc.revcomp_seqs()
    assert len(seqs) == 70 and {len(s) for s in seqs} == set(range(41))
    assert set(b"".join(seqs)) == set(dc.fc.ALPHA)


def test_band_pairs_are_the_tile_family():
    import band_edge_cases as bec
    pairs = dc.band_pairs()
    short = {p.name: p for p in bec.short_batch()}  # (what tests/test_band_edge_cases.py holds against the oracle)
    assert len(pairs) == 8 and all(p.name in short and (p.x, p.y) == (short[p.name].x, short[p.name].y) for p in pairs)
    assert sorted(len(p.y) for p in pairs) == sorted(2 * list(dc.BAND_TILE_N))
    # concatenated, the pairs start at several residues of x and of y besides the base pointer's
    xo = np.cumsum([0] + [len(p.x) for p in pairs[:-1]]) % 16
    yo = np.cumsum([0] + [len(p.y) for p in pairs[:-1]]) % 16
    assert len(set(xo.tolist())) >= 4 and len(set(yo.tolist())) >= 4


# ---- seed-and-extend ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiered():
    import test_gpu_seed_extend_tiered as t
    buf, off, planted = dc.seed_reads()
    return t.oracle(dc.seed_genome(), buf, off, reseed_below=dc.SEED_BELOW), planted


def test_tiered_batch_copies_operations_with_vectors_and_with_bytes(tiered):
    import tiered_seed_oracle as tso
    res, planted = tiered
    buf, off, _ = dc.seed_reads()
    assert len(off) - 1 == dc.SEED_READS == 64 and set(np.diff(off).tolist()) == {dc.SEED_LEN} and planted.sum() == 32
    assert res["status"] == 0 and int(res["totals"][2]) == 32
    tier = np.asarray(res["tier"])
    assert (tier[planted] == tso.TIER_SECOND).all() and (tier[~planted] == tso.TIER_NONE).all()
    winners = np.nonzero(tier == tso.TIER_SECOND)[0]
    n_ops = np.array([len(w[1]["ops"]) if w[1] is not None else 0 for w in res["want"]])
    assert (n_ops[winners] == dc.SEED_LEN).all()
    kinds = {res_: set(dc.copy_wave_kinds(winners, np.nonzero(tier != tso.TIER_NONE)[0], res_, n_ops).values()) for res_ in dc.SEED_OPS_RES}
    assert kinds == {0: {"vector", "bytes"}, 5: {"bytes"}}
    # both strands win
    assert {w[0] for w in res["want"]} == {0, 1}


def test_strands_batch_maps_on_both_strands():
    import test_gpu_dev_pointer_alignment as gpu
    hits, strand, ops, stride = gpu.strands_oracle()
    assert len(hits) == 64 and (hits["aln"]["score"][~dc.seed_reads()[2]] == dc.SEED_LEN).all()
    _, _, planted = dc.seed_reads()
    assert {int(s) for s in strand[~planted]} == {0, 1}  # HIT_FORWARD and HIT_REVERSE, no HIT_NONE: every exact read maps


# ---- SAM ---------------------------------------------------------------------------------------------------------------------
def test_sam_lines_have_every_copy_shape():
    import sam_oracle as so
    case = dc.sam_case()
    want = case.want()
    assert case.n == 40 and case.K == 1 and len(want) == 40
    lens = [len(w) for w in want]
    assert min(lens) == 22 and 32 in lens and max(lens) > dc.SAM_STAGE + 16
    off = so.offsets(want)
    for res in dc.SAM_OUT_RES:
        plans = [dc.copy_plan((res + int(off[s])) % 16, len(w)) for s, w in enumerate(want)]
        staged = [(res + int(off[s])) % 16 + len(w) <= dc.SAM_STAGE for s, w in enumerate(want)]
        assert any(body == 0 for _, body, _ in plans), res              # head and tail only: shorter than a vector
        assert any(head == 0 and body for head, body, _ in plans), res  # begins on a boundary
        assert any(head and body and tail for head, body, tail in plans), res
        assert {True, False} == set(staged), res
    assert sum(not int(w.split(b"\t")[1]) & 4 for w in want) == 24 and sum(int(w.split(b"\t")[1]) & 16 > 0 for w in want) >= 8


def test_sort_batch_has_every_copy_shape():
    import sam_oracle as so
    import sam_sort_oracle as sso
    b = dc.sort_batch()
    assert len(b.recs) == 40 and set(dc.SORT_LENS) <= {len(r) for r in b.recs}
    perm, out_off, _ = sso.sort(b.key, b.recs)
    assert perm.tolist() != sorted(perm.tolist())
    in_off = so.offsets(b.recs)
    for out_res in dc.SAM_OUT_RES:
        for in_res in dc.SAM_IN_RES:
            shapes = set()
            for j, i in enumerate(perm.tolist()):
                n = len(b.recs[i])
                head, body, tail = dc.copy_plan((out_res + int(out_off[j])) % 16, n)
                same = (in_res + int(in_off[i]) - out_res - int(out_off[j])) % 16 == 0
                shapes.add((body > 0, same, n > dc.SAM_LONG_LINE))
            # no vector at all; vectors from a source on and off the destination's alignment; both copy kernels
            assert {(False, True, False), (False, False, False)} & shapes and {s[2] for s in shapes} == {False, True}, (out_res, in_res)
            assert {s[1] for s in shapes if s[0]} == {False, True}, (out_res, in_res, shapes)


# ---- the FASTQ column calls --------------------------------------------------------------------------------------------------
def test_column_batches_do_something_under_every_rule():
    import fastq_demux_oracle as dm
    import fastq_qual_oracle as qo
    import fastq_write_oracle as fw
    import myers_oracle as mo
    from fastq_write_cases import Batch
    records = dc.column_records()
    b = Batch(records)
    assert len(b) == 40 and 0 in b.recs["seq_len"] and (b.recs["seq_len"] != b.recs["qual_len"]).any()
    keep = fw.filter_columns(*b.columns(), min_len=10, max_n=6)[5]
    assert 5 <= keep.sum() <= 35
    hits = dc.trim_hits(records)
    trimmed = 0
    for r, (_, _, s, q) in enumerate(records):
        h = [(int(x["score"]), int(x["ystart"]), int(x["yend"])) for x in hits[2 * r:2 * r + 2]]
        for mode in (mo.TRIM_3P, mo.TRIM_5P):
            (lo, hi), _ = mo.trim_range(mode, h, len(s), len(q))
            trimmed += (hi - lo) < len(s)
    assert trimmed >= 20
    bins = dc.split_bins(40)
    bin_off = dm.split(bins, 3, *b.columns())[7]
    assert (np.diff(bin_off.astype(np.int64)) > 0).all() and int(bin_off[-1]) == 40
    qb = Batch(dc.qual_records())
    for params in gpu_cut_params():
        _, (n_cut, removed), _ = qo.cut(qb.qual, qb.qual_off, **params)
        assert 5 <= n_cut <= 40 and removed > 0, params


def gpu_cut_params():
    import test_gpu_dev_pointer_alignment as gpu
    return gpu.CUT_PARAMS

"""The `__host__ __device__` bodies behind the pileup (csrc/bam_pileup_rule.h: the slot's checks, verdict and keys, the region
and tile arithmetic, the two searches for a tile's candidates, a lane's share of a record's counts clipped to the tile, the
transposing row store) run on the CPU by a stand-alone program (tests/bam_pileup_host_bodies.cpp: the kernels' steps, lanes
0 .. 15 and threads 0 .. 255 in turn; every record, table, counter tile and row buffer an exact-size heap buffer) built with
AddressSanitizer and UBSan.  Nothing is loaded into Python.  Everything is held to the Python restatement
(tests/bam_pileup_oracle.py), which shares no code with the product: the whole corpus and every refusal."""
import pytest

import bam_pileup_cases as pc
import bam_pileup_oracle as po


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bampileup")
    exe = pc.build_program("bam_pileup_host_bodies.cpp", str(tmp / "bodies"), sanitize=True)
    corpus = pc.corpus()
    refusals = [dict(name=name, slots=slots, contigs=contigs, regions=regions, params=dict(pc.DEFAULT), want=(status, slot))
                for name, slots, contigs, regions, status, slot in pc.refusals()]
    got = pc.run_program(exe, tmp, corpus + refusals)
    return corpus, got[:len(corpus)], refusals, got[len(corpus):]


def test_the_rows_of_the_corpus_are_the_oracles(ran):
    corpus, got, _, _ = ran
    shapes = set()
    for c, (rcode, bad, n_rows, rows, row_off) in zip(corpus, got):
        want, want_off = pc.want_of(c)
        assert (rcode, bad, n_rows, row_off) == (0, po.NONE, len(want), want_off), c["name"]
        assert (rows == want).all(), c["name"]
        shapes.add(rows.shape[1])
    assert shapes == {po.COLS, 2 * po.COLS}


def test_a_deep_pile_needs_more_than_16_bits(ran):
    corpus, got, _, _ = ran
    c, g = next((c, g) for c, g in zip(corpus, got) if c["name"] == "66 000 records at one position")
    assert int(g[3][10].sum()) == 66_000 > 0xFFFF and int(g[3][10].max()) == 16_500


def test_every_refusal_names_its_slot_and_kind(ran):
    _, _, refusals, got = ran
    kinds = set()
    for c, (rcode, bad, n_rows, rows, row_off) in zip(refusals, got):
        status, slot = c["want"]
        assert (rcode, bad, n_rows, rows) == (status, po.NONE if slot is None else slot, 0, None), c["name"]
        kinds.add((status, slot is None))
    assert kinds == {(po.INVALID_ARG, False), (po.UNSUPPORTED, False), (po.INVALID_ARG, True)}


def test_results_do_not_depend_on_the_tile(ran):
    """a region cut into pieces at arbitrary places gives the rows of the whole: no row knows where a tile began"""
    corpus, got, _, _ = ran
    c = next(c for c in corpus if c["name"] == "tile borders")
    whole, _ = pc.want_of(dict(c, regions=[(0, 0, pc.CONTIGS[0][2])]))
    g = next(g for cc, g in zip(corpus, got) if cc is c)
    for (ref, beg, end), o in zip(c["regions"], g[4]):
        assert (g[3][o:o + end - beg] == whole[beg:end]).all(), (beg, end)

"""The `__host__ __device__` bodies behind the candidate sites (csrc/bam_sites_rule.h: the region's check against the text, the
judgement of a position, the share of a region's summary with its packed word, the two steps around the in-block scan, the
record store in both forms) run on the CPU by a stand-alone program (tests/bam_sites_host_bodies.cpp: the kernels' steps,
threads 0 .. 255 in turn; every record, table, text, counter tile, scan array and site buffer an exact-size heap buffer) built
with AddressSanitizer and UBSan.  Nothing is loaded into Python.  Everything is held to the Python restatement
(tests/bam_sites_oracle.py), which shares no code with the product: the whole corpus, every refusal, and synthetic counter
tiles with counts of millions, where the permille product leaves 32 bits."""
import pytest

import bam_sites_cases as sc
import bam_sites_oracle as so


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bamsites")
    exe = sc.build_program(str(tmp / "bodies"), sanitize=True)
    corpus, refusals, synth = sc.corpus(), sc.refusals(), sc.synthetic()
    got, tiles = sc.run_program(exe, tmp, corpus + refusals, synth)
    return corpus, got[:len(corpus)], refusals, got[len(corpus):], synth, tiles


def test_the_sites_and_summaries_of_the_corpus_are_the_oracles(ran):
    corpus, got, _, _, _, _ = ran
    kinds, total = set(), 0
    for c, (rcode, bad, n_sites, sites, site_off, summary) in zip(corpus, got):
        want, want_off, want_sum = sc.want_of(c)
        assert (rcode, bad, n_sites, site_off) == (0, so.NONE, len(want), want_off), c["name"]
        assert so.as_tuples(sites) == want, c["name"]
        assert so.as_dicts(summary) == want_sum, c["name"]
        assert not sites["reserved"].any()
        kinds |= set(sites["kind"].tolist())
        total += n_sites
    assert kinds == {so.SNV, so.DEL, so.INS} and total > 10_000


def test_a_tile_of_2560_sites(ran):
    corpus, got, _, _, _, _ = ran
    c, g = next((c, g) for c, g in zip(corpus, got) if c["name"] == "a tile whose 512 positions all give 5 sites")
    assert g[2] == 5 * sc.T and g[3]["pos"].tolist() == [sc.T + k // 5 for k in range(5 * sc.T)]
    assert g[3]["kind"].tolist() == [so.SNV, so.SNV, so.SNV, so.DEL, so.INS] * sc.T


def test_every_refusal_names_its_slot_and_kind(ran):
    _, _, refusals, got, _, _ = ran
    kinds = set()
    for c, (rcode, bad, n_sites, sites, site_off, summary) in zip(refusals, got):
        status, slot = c["want"]
        assert (rcode, bad, n_sites, sites) == (status, so.NONE if slot is None else slot, 0, None), c["name"]
        with pytest.raises(so.Refused) as e:
            sc.want_of(c)
        assert (e.value.status, e.value.slot) == (status, slot), c["name"]
        kinds.add((status, slot is None))
    assert kinds == {(so.INVALID_ARG, False), (so.UNSUPPORTED, False), (so.INVALID_ARG, True)}


def test_the_permille_product_is_64_bits_wide(ran):
    _, _, _, _, synth, tiles = ran
    flips = []
    for (row, ref_byte, p), got in zip(synth, tiles):
        want = []
        for pos in (0, sc.T - 1):
            want += so.judge(row, ref_byte, 0, pos, 0, p)[0]
        assert so.as_tuples(got) == want
        alt, depth = row[1] + row[9], sum(row[c] + row[8 + c] for c in range(6))
        flips.append(((alt * 1000) % 2**32 >= (p["min_alt_permille"] * depth) % 2**32) != (alt * 1000 >= p["min_alt_permille"] * depth))
    assert flips == [True, True, True] and [len(t) for t in tiles] == [2, 0, 0]

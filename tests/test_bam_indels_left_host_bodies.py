"""The `__host__ __device__` bodies behind the left-aligned indel events (csrc/bam_indels_left_rule.h: the walk beyond the tile's
end, the shift of a deletion and of an insertion against the text, the shifted codes, the full-key comparison, the shifted bytes)
run on the CPU by a stand-alone program (tests/bam_indels_host_bodies.cpp, its left flavour: the kernels' steps; the places of a tile's raw
events handed out in another order than they were counted in; an unstable sort; every buffer an exact-size heap buffer, the text
of every contig included, so that a read of F(-1) or of the `$` stops it) built with AddressSanitizer and UBSan.  Nothing is
loaded into Python.  Everything is held to the Python restatement (tests/bam_indels_left_oracle.py), which shares no code with
the product: the whole corpus, where max_shift is 0 also to the older restatement, and every refusal."""
import pytest

import bam_indels_cases as ic
import bam_indels_left_cases as lc
import bam_indels_oracle as io


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bamindelsleft")
    exe = lc.build_program(str(tmp / "bodies"), sanitize=True)
    corpus, refusals = lc.corpus(), lc.refusals()
    got = lc.run_program(exe, tmp, corpus + refusals)
    return corpus, got[:len(corpus)], refusals, got[len(corpus):]


def test_the_events_and_sequences_of_the_corpus_are_the_oracles(ran):
    corpus, got, _, _ = ran
    kinds, total, longest, plain = set(), 0, 0, 0
    for c, (rcode, bad, n_events, n_seq, events, seq, event_off) in zip(corpus, got):
        want, want_seq, want_off = lc.want_of(c)
        assert (rcode, bad, n_events, n_seq, event_off) == (0, io.NONE, len(want), len(want_seq), want_off), c["name"]
        assert io.as_tuples(events) == want and seq == want_seq, c["name"]
        assert not events["reserved"].any()
        if c.get("plain"):  # max_shift 0: what bg_bam_indels gives, by the restatement that knows no shift
            assert (want, want_seq, want_off) == io.indels(c["slots"], c["contigs"], c["regions"], **{f: c["params"][f] for f in io.DEFAULT}), c["name"]
            plain += 1
        kinds |= set(events["kind"].tolist())
        total += n_events
        longest = max([longest] + events["len"][events["kind"] == io.INS].tolist())
    assert kinds == {io.DEL, io.INS} and total > 1_000 and longest >= 33 and plain == len(ic.corpus())


def test_one_event_of_1100_records_and_one_two_tiles_in_front(ran):
    corpus, got, _, _ = ran
    by = {c["name"]: g for c, g in zip(corpus, got)}
    g = by["1 100 records, seven spellings, one event"]
    assert io.as_tuples(g[4])[0] == (0, 299, 0, io.DEL, 1, 1100, 733, 367, 0)
    g = by["a deletion that lands two tiles in front of its raw anchor"]
    assert [e[:5] for e in io.as_tuples(g[4]) if e[2] == 0] == [(1, 49, 0, io.DEL, 1)]


def test_every_refusal_names_its_slot_and_kind(ran):
    _, _, refusals, got = ran
    kinds = set()
    for c, (rcode, bad, n_events, n_seq, events, seq, event_off) in zip(refusals, got):
        status, slot = c["want"]
        assert (rcode, bad, n_events, n_seq, events) == (status, io.NONE if slot is None else slot, 0, 0, None), c["name"]
        kinds.add((status, slot is None))
    assert kinds == {(io.INVALID_ARG, False), (io.UNSUPPORTED, False), (io.INVALID_ARG, True)}

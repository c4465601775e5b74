"""The `__host__ __device__` bodies behind the indel events (csrc/bam_indels_rule.h: the walk that yields raw events, the depth of
an anchor, the full-key comparison through the records' own bases, the verdict, the record store, the decoding of an inserted
sequence) run on the CPU by a stand-alone program (tests/bam_indels_host_bodies.cpp: the kernels' steps; the places of a tile's
raw events handed out in another order than they were counted in; every record, table, counter tile, scratch array, event and
sequence buffer an exact-size heap buffer) built with AddressSanitizer and UBSan.  Nothing is loaded into Python.  Everything is
held to the Python restatement (tests/bam_indels_oracle.py), which shares no code with the product: the whole corpus and every
refusal."""
import pytest

import bam_indels_cases as ic
import bam_indels_oracle as io


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bamindels")
    exe = ic.build_program(str(tmp / "bodies"), sanitize=True)
    corpus, refusals = ic.corpus(), ic.refusals()
    got = ic.run_program(exe, tmp, corpus + refusals)
    return corpus, got[:len(corpus)], refusals, got[len(corpus):]


def test_the_events_and_sequences_of_the_corpus_are_the_oracles(ran):
    corpus, got, _, _ = ran
    kinds, total, longest = set(), 0, 0
    for c, (rcode, bad, n_events, n_seq, events, seq, event_off) in zip(corpus, got):
        want, want_seq, want_off = ic.want_of(c)
        assert (rcode, bad, n_events, n_seq, event_off) == (0, io.NONE, len(want), len(want_seq), want_off), c["name"]
        assert io.as_tuples(events) == want and seq == want_seq, c["name"]
        assert not events["reserved"].any()
        kinds |= set(events["kind"].tolist())
        total += n_events
        longest = max([longest] + events["len"][events["kind"] == io.INS].tolist())
    assert kinds == {io.DEL, io.INS} and total > 1_000 and longest >= 33


def test_the_deep_pile_is_one_event(ran):
    corpus, got, _, _ = ran
    c, g = next((c, g) for c, g in zip(corpus, got) if c["name"] == "66 000 records with one insertion each")
    assert io.as_tuples(g[4]) == [(3, 500, 0, io.INS, 2, 66_000, 44_000, 22_000, 0), (3, 500, 1, io.INS, 2, 66_000, 44_000, 22_000, 2)] and g[5] == b"GTGT"


def test_every_refusal_names_its_slot_and_kind(ran):
    _, _, refusals, got = ran
    kinds = set()
    for c, (rcode, bad, n_events, n_seq, events, seq, event_off) in zip(refusals, got):
        status, slot = c["want"]
        assert (rcode, bad, n_events, n_seq, events) == (status, io.NONE if slot is None else slot, 0, 0, None), c["name"]
        with pytest.raises(io.Refused) as e:
            ic.want_of(c)
        assert (e.value.status, e.value.slot) == (status, slot), c["name"]
        kinds.add((status, slot is None))
    assert kinds == {(io.INVALID_ARG, False), (io.UNSUPPORTED, False), (io.INVALID_ARG, True)}

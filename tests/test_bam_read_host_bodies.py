"""The `__host__ __device__` bodies behind reading BAM (csrc/bam_read_rule.h: the verdict on a position, the slot check, a lane's
share of a read's bases and qualities, the FASTQ record, the key; csrc/bam_index_rule.h: the virtual offset in any framing) run
on the CPU by a stand-alone program (tests/bam_read_host_bodies.cpp: the kernels' steps, lanes 0 .. 15 in turn; every stream,
table and column an exact-size heap buffer) built with AddressSanitizer and UBSan.  Nothing is loaded into Python.  Everything
is held to the Python restatement (tests/bam_read_oracle.py), which shares no code with the product."""
import pytest

import bam_read_cases as rc
import bam_read_oracle as ro


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bamread")
    exe = rc.build_program(str(tmp / "bodies"), sanitize=True)
    corpus, reads, voffs = rc.corpus(), rc.reads_cases(), rc.voff_cases()
    cases = [dict(stream=s, body_off=rc.BODY, n_ref=n_ref, contigs=rc.CONTIGS[:n_ref]) for _, s, n_ref in corpus]
    cases += [dict(stream=s, body_off=rc.BODY, n_ref=rc.N_REF, contigs=rc.CONTIGS, flags=fl, require=rq, exclude=ex) for _, s, fl, rq, ex in reads]
    cases += [dict(stream=rc.HEADER, body_off=rc.BODY, n_ref=rc.N_REF, tables=(bo, oo), ask=ask) for _, bo, oo, ask in voffs]
    good = rc.HEADER + b"".join(rc.seq_rec(i, 10 + i, ref=1, pos=i) for i in range(4))
    off = ro.walk(good, rc.BODY, rc.N_REF)
    tables = [off[:2] + off[3:], off[:1] + [off[1] - 1] + off[2:], off[:3] + [off[3]] + off[3:], [off[0] + 1] + off[1:]]
    cases += [dict(stream=good, body_off=rc.BODY, n_ref=rc.N_REF, contigs=rc.CONTIGS, off=t) for t in tables]
    got = rc.run_program(exe, tmp, cases)
    a, b, c = len(corpus), len(corpus) + len(reads), len(corpus) + len(reads) + len(voffs)
    return dict(corpus=corpus, reads=reads, voffs=voffs, tables=tables, good=good, got_corpus=got[:a], got_reads=got[a:b], got_voffs=got[b:c],
                got_tables=got[c:])


def test_the_close_pair_exists():
    pair = rc.close_pair()
    assert pair is not None
    assert ro.verdict(pair, 0, rc.N_REF) == len(pair) and ro.verdict(pair, 4, rc.N_REF) is not None
    assert any(name == "two accepted positions 4 bytes apart" for name, _, _ in rc.corpus())


def test_the_table_is_the_walks(ran):
    refused = set()
    for (name, s, n_ref), g in zip(ran["corpus"], ran["got_corpus"]):
        rcode, n, n_cand, bad, off = g["table"]
        assert n_cand == len(ro.candidates(s, rc.BODY, n_ref)), name
        try:
            want = ro.walk(s, rc.BODY, n_ref)
        except ro.Refused as e:
            assert (rcode, n, bad) == (ro.INVALID_ARG, e.first_bad, e.first_bad), name
            refused.add(name)
            continue
        assert (rcode, n, bad, off) == (0, len(want) - 1, ro.NONE, want), name
        assert n_cand >= n, name
    assert refused == {"one byte short", "one byte long", "block_size into the middle of the next record", "refID == n_ref", "refID -2",
                       "next_refID == n_ref", "pos -2", "next_pos -2", "l_read_name 0", "a name without its NUL", "l_seq -1",
                       "block_size below what the fields need", "fewer than 36 bytes left"}


def test_fakes_are_candidates_and_never_records(ran):
    for (name, s, n_ref), g in zip(ran["corpus"], ran["got_corpus"]):
        if name in ("a record inside the qualities", "three linked fakes in a B:C tag", "two accepted positions 4 bytes apart"):
            assert g["table"][0] == 0 and g["table"][2] > g["table"][1], name
    by = {name: g for (name, _, _), g in zip(ran["corpus"], ran["got_corpus"])}
    assert by["three linked fakes in a B:C tag"]["table"][2] == by["three linked fakes in a B:C tag"]["table"][1] + 3


def test_reads_and_keys_of_the_corpus(ran):
    for (name, s, n_ref), g in zip(ran["corpus"], ran["got_corpus"]):
        if g["table"][0]:
            assert "reads" not in g
            continue
        off = g["table"][4]
        recs, seq, seq_off, qual, qual_off, src = ro.reads(s, off, n_ref)
        assert g["reads"][:2] == (0, ro.NONE), name
        assert rc.same_records(g["reads"][2], recs) and g["reads"][3:] == (seq, seq_off, qual, qual_off, src), name
        assert g["keys"] == (0, ro.NONE, ro.keys(s, off, rc.CONTIGS[:n_ref])), name


def test_reads_under_the_filter_and_as_sequenced(ran):
    seen = set()
    for (name, s, fl, rq, ex), g in zip(ran["reads"], ran["got_reads"]):
        off = ro.walk(s, rc.BODY, rc.N_REF)
        recs, seq, seq_off, qual, qual_off, src = ro.reads(s, off, rc.N_REF, fl, rq, ex)
        assert g["reads"][:2] == (0, ro.NONE), name
        assert rc.same_records(g["reads"][2], recs) and g["reads"][3:] == (seq, seq_off, qual, qual_off, src), name
        assert len(src) < len(off) - 1 or not (rq or ex), name
        seen |= {r["check"] for r in recs}
    assert {ro.CHECK_OK, ro.CHECK_INVALID_SEQ, ro.CHECK_NONASCII_QUAL, ro.CHECK_UNEQUAL} <= seen
    s = rc.all_codes()
    recs, seq, *_ = ro.reads(s, ro.walk(s, rc.BODY, rc.N_REF), rc.N_REF, ro.ORIGINAL)
    assert seq[recs[0]["seq_off"]:recs[0]["seq_off"] + 16] == bytes(ro.COMPLEMENT[b] for b in reversed(ro.BASES))


def test_a_table_from_elsewhere_is_checked(ran):
    # two records in one slot; a slot cut short; an empty slot (skipped); a slot that starts late
    outcomes = []
    for t, g in zip(ran["tables"], ran["got_tables"]):
        try:
            recs, *_ = ro.reads(ran["good"], t, rc.N_REF)
        except ro.Refused as e:
            assert g["reads"][:2] == (ro.INVALID_ARG, e.first_bad) and g["keys"][:2] == (ro.INVALID_ARG, e.first_bad)
            outcomes.append(e.first_bad)
            continue
        assert g["reads"][:2] == (0, ro.NONE) and rc.same_records(g["reads"][2], recs)
        assert g["keys"] == (0, ro.NONE, ro.keys(ran["good"], t, rc.CONTIGS))
        outcomes.append(None)
    assert outcomes == [1, 0, None, 0]


def test_virtual_offsets_in_any_framing(ran):
    for (name, bo, oo, ask), g in zip(ran["voffs"], ran["got_voffs"]):
        voff = ro.blocks_voff(bo, oo)
        assert g["voff"] == [voff(o) for o in ask], name
    bo, oo = ran["voffs"][0][1:3]  # 100, 50, end-of-file
    v = ro.blocks_voff(bo, oo)
    assert v(100) == bo[1] << 16 and v(150) == bo[2] << 16 and v(149) == (bo[1] << 16) | 49
    bo, oo = ran["voffs"][1][1:3]  # no end-of-file member: the closing row
    assert ro.blocks_voff(bo, oo)(150) == bo[2] << 16
    bo, oo = ran["voffs"][3][1:3]  # two empty members are skipped
    assert ro.blocks_voff(bo, oo)(100) == bo[3] << 16

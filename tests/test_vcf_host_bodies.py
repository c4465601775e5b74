"""The `__host__ __device__` bodies behind the VCF writer (csrc/vcf_rule.h: the checks of an element with its predecessor, a
line's fields and length, the two binary searches that place a line, a lane's share of a line's bytes, the digit count and the
number writer, the two byte tables) run on the CPU by a stand-alone program (tests/vcf_host_bodies.cpp: the kernels' steps with
the elements and lanes taken backwards; every list, table, text, scratch array, stage and output an exact-size heap buffer)
built with AddressSanitizer and UBSan.  Nothing is loaded into Python.  Everything is held to the Python restatement
(tests/vcf_oracle.py), which shares no code with the product: the whole corpus, byte for byte, and every refusal."""
import subprocess

import pytest

import vcf_cases as vc
import vcf_oracle as vo


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("vcf")
    exe = vc.build_program(str(tmp / "bodies"), sanitize=True)
    corpus, refusals = vc.corpus(), vc.refusals()
    got = vc.run_program(exe, tmp, corpus + refusals)
    return exe, corpus, got[:len(corpus)], refusals, got[len(corpus):]


def test_digit_counts_numbers_and_byte_tables_at_every_power_of_ten(ran):
    assert subprocess.call([ran[0]]) == 0


def test_the_lines_of_the_corpus_are_the_oracles(ran):
    _, corpus, got, _, _ = ran
    lines, longest = 0, 0
    for c, (rcode, bad, n_lines, out_bytes, text, line_off) in zip(corpus, got):
        want, want_off = vc.want_of(c)
        assert (rcode, bad, n_lines, out_bytes, line_off) == (0, vo.NONE, len(want_off) - 1, len(want), want_off), c["name"]
        assert text == want, c["name"]
        lines += n_lines
        longest = max([longest] + [b - a for a, b in zip(want_off, want_off[1:])])
    assert lines > 700 and longest > 70_000


def test_every_refusal_names_the_smallest_index(ran):
    _, _, _, refusals, got = ran
    for c, (rcode, bad, n_lines, out_bytes, text, line_off) in zip(refusals, got):
        assert (rcode, bad, n_lines, out_bytes, text) == (vo.INVALID_ARG, c["want"], 0, 0, None), c["name"]
        with pytest.raises(vo.Refused) as e:
            vc.want_of(c)
        assert (e.value.status, e.value.first_bad) == (vo.INVALID_ARG, c["want"]), c["name"]
    assert len(refusals) > 50

"""`bam.indels_bam` on a file made on the CPU: sorted records from tests/bam_oracle.py's encoder, framed as BGZF blocks with
deflate-compressed payloads (zlib).  The events, sequences and offsets are the oracle's (tests/bam_indels_oracle.py) on the
file's records; regions are named through the file's header.  The input gives deletions, insertions seen more than once and
insertions that differ in one base at one anchor, under the oracle alone."""
import numpy as np
import pytest

import bam_indels_oracle as io
import bam_oracle as bo
import bam_pileup_cases as pc
from rust_bio_amd import bam
from test_gpu_bam_sites_file import LENS, NAMES, deflated

pytestmark = pytest.mark.gpu


def records():
    """reads at drawn places, every third with a deletion and an insertion, the insertion one of three that differ in their last base;
    a few of them stacked on one place"""
    rng = np.random.default_rng(31)
    out = []
    for ref in (0, 1):
        for k in range(90):
            pos = 200 if k % 9 == 0 else int(rng.integers(0, LENS[ref] - 60))
            if k % 3 == 0:
                ins = [1, 2, 4, 8, (1, 2, 15)[int(rng.integers(0, 3))]]
                codes = rng.choice([1, 2, 4, 8], 20).tolist() + rng.choice([1, 2, 4, 8], 10).tolist() + ins + rng.choice([1, 2, 4, 8], 15).tolist()
                out.append(pc.rec(ref, pos, b"20M2D10M5I15M", codes=codes, flag=0x10 * int(rng.integers(0, 2)), mapq=60, name=b"q%d_%d" % (ref, k)))
            else:
                out.append(pc.rec(ref, pos, b"48M", seed=k, flag=0x10 * int(rng.integers(0, 2)), mapq=int(rng.choice([0, 60])), name=b"q%d_%d" % (ref, k)))
    return pc.by_position(out)


@pytest.fixture(scope="module")
def made():
    contigs = pc.contigs_of(LENS, NAMES)
    slots = records()
    data = deflated(bo.header(b"@HD\tVN:1.6\tSO:coordinate\n", contigs) + b"".join(slots))
    return dict(contigs=contigs, slots=slots, data=data)


def test_the_files_events_are_the_oracles(made):
    contigs = made["contigs"]
    regions = [(0, 0, 700), (1, 100, 1200), (2, 0, 40), (1, 0, 1300), (0, 231, 232)]
    named = [("chrA", 0, 700), (1, 100, 1200), (b"tiny", 0, 40), ("chrB", 0, 1300), ("chrA", 231, 232)]
    for kw in (dict(), dict(min_depth=3, min_alt=2, min_alt_permille=200), dict(min_alt_strand=1, min_mapq=1), dict(exclude=0x10)):
        want, want_seq, want_off = io.indels(made["slots"], contigs, regions, **kw)
        if not kw:  # the condition, under the oracle alone
            assert {e[3] for e in want} == {io.DEL, io.INS} and max(e[6] + e[7] for e in want) > 1
            here = [s for e, s in zip(want, io.strings(want, want_seq)) if e[2] == 4 and e[3] == io.INS]
            assert len(here) == 3 and len({s[:-1] for s in here}) == 1  # (anchor 231: three insertions that differ in the last base)
        events, seq, event_off = bam.indels_bam(made["data"], named, **kw)
        assert io.as_tuples(events) == want and seq.tobytes() == want_seq and event_off.tolist() == want_off, kw
        assert bam.indel_sequences(events, seq) == io.strings(want, want_seq), kw


def test_a_region_the_header_does_not_name_is_refused_before_the_device(made):
    with pytest.raises(ValueError) as e:
        bam.indels_bam(made["data"], [("chrZ", 0, 10)])
    assert "chrZ" in str(e.value)
    with pytest.raises(ValueError):
        bam.indels_bam(made["data"], [("chrA", 0, 701)])

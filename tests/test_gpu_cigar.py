"""`bg_cigar_batch` (csrc/align_text.hip: bio-types `Alignment::cigar`) against the reference's own known answers and the
CPU oracle and the plain restatement of tests/align_text_oracle.py, on alignments of random reads in the three supported modes."""
import numpy as np
import pytest

import align_text_oracle as ato
import oracle_py as orc
from kat_util import load
from rust_bio_amd import _lib
from rust_bio_amd.pairwise import Aligner, Alignment, Scoring, cigar_batch

pytestmark = pytest.mark.gpu
K = load("fastq_kats.json")


def test_cigar_kats_and_batches_against_the_oracle():
    OPK = {"Match": "M", "Subst": "S", "Ins": "I", "Del": "D"}
    for c in K["cigar"]:
        a = Alignment(0, 0, c["xstart"], 0, c["xend"], 0, c["xlen"], [OPK[o] for o in c["ops"]], c["mode"].capitalize())
        assert a.cigar(False) == c["soft"] and a.cigar(True) == c["hard"]
        kinds = [["Match", "Subst", "Del", "Ins"].index(o) for o in c["ops"]]
        assert [ato.cigar(c["xstart"], c["xend"], c["xlen"], c["mode"], kinds, hard) for hard in (False, True)] == [c["soft"], c["hard"]]
    with pytest.raises(AssertionError):
        Alignment(0, 0, 0, 0, 1, 1, 1, ["M"], "Custom").cigar(False)
    assert Alignment(0, 0, 0, 0, 0, 0, 4, [], "Local").cigar(False) == ""
    # alignments of random reads in the three supported modes
    from rust_bio_amd import synth
    xs, ys = synth.ragged_pairs(500, 120, seed=9, min_len=1)
    x, xo = _lib.concat(xs)
    y, yo = _lib.concat(ys)
    al = Aligner.with_scoring(Scoring.from_scores(-5, -1, 1, -1))
    for mode in (1, 2, 3):
        out, ops = al.align_arrays(mode, x, xo, y, yo)
        for hard in (False, True):
            got = cigar_batch(out, ops, hard)
            for p in range(len(out)):
                o = ops[int(out["ops_off"][p]):int(out["ops_off"][p]) + int(out["n_ops"][p])].astype(np.uint64)
                want = orc.cigar({"xstart": int(out["xstart"][p]), "xend": int(out["xend"][p]), "xlen": int(out["xlen"][p]), "mode": mode}, o, hard)
                assert got[p] == want, (mode, p, got[p], want)
                assert got[p] == ato.cigar(int(out["xstart"][p]), int(out["xend"][p]), int(out["xlen"][p]), mode, o, hard), (mode, p)

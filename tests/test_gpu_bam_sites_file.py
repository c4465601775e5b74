"""`bam.sites_bam` on a file made on the CPU: sorted records from tests/bam_oracle.py's encoder, framed as BGZF blocks with
deflate-compressed payloads (zlib), against FASTA text of several lines a record with soft-masked and N bases.  The sites, offsets
and summaries are the oracle's (tests/bam_sites_oracle.py) on the file's records and on the text put together in plain Python;
the reference may also come as the ready index text.  The input gives at least one site of each kind and at least one unjudged
position under the oracle alone.  A header whose contig length differs from the FASTA's raises ValueError."""
import struct
import zlib

import numpy as np
import pytest

import bam_oracle as bo
import bam_pileup_cases as pc
import bam_sites_oracle as so
from rust_bio_amd import bam

pytestmark = pytest.mark.gpu
LENS = [700, 1300, 40]
NAMES = [b"chrA", b"chrB", b"tiny"]


def sequences():
    rng = np.random.default_rng(21)
    out = []
    for ln in LENS:
        s = rng.choice(np.frombuffer(b"ACGT", np.uint8), ln)
        s = np.where(rng.integers(0, 10, ln) == 0, s + 32, s)
        s = np.where(rng.integers(0, 25, ln) == 0, ord("N"), s).astype(np.uint8)
        out.append(s.tobytes())
    return out


def fasta_text(seqs, width=60):
    out = b""
    for name, s in zip(NAMES, seqs):
        out += b">" + name + b" made up\n" + b"".join(s[i:i + width] + b"\n" for i in range(0, len(s), width))
    return out


def records(seqs, contigs):
    """reads that copy the reference with one base in ten changed, every sixth with a deletion and an insertion"""
    rng = np.random.default_rng(22)
    code = {65: 1, 67: 2, 71: 4, 84: 8}
    out = []
    for ref, s in enumerate(seqs[:2]):
        for k in range(60):
            pos = int(rng.integers(0, len(s) - 50))
            cigar = b"20M2D10M3I15M" if k % 6 == 0 else b"48M"
            n = pc.query_len(cigar)
            codes = [code.get(so.fold(b), 15) for b in s[pos:pos + n]]
            codes = [int(rng.choice([1, 2, 4, 8])) if rng.integers(0, 10) == 0 else c for c in codes]
            out.append(pc.rec(ref, pos, cigar, codes=codes, flag=0x10 * int(rng.integers(0, 2)), mapq=60, name=b"q%d_%d" % (ref, k)))
    return pc.by_position(out)


def deflated(data, eof=True):
    """BGZF blocks with compressed payloads"""
    out = b""
    for i in range(0, len(data), 60_000):
        payload = data[i:i + 60_000]
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        cdata = z.compress(payload) + z.flush()
        out += (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(cdata) + 25) + cdata +
                struct.pack("<II", zlib.crc32(payload), len(payload)))
    return out + (bo.EOF_BLOCK if eof else b"")


@pytest.fixture(scope="module")
def made():
    seqs = sequences()
    contigs = pc.contigs_of(LENS, NAMES)
    slots = records(seqs, contigs)
    data = deflated(bo.header(b"@HD\tVN:1.6\tSO:coordinate\n", contigs) + b"".join(slots))
    return dict(seqs=seqs, contigs=contigs, slots=slots, data=data, text=b"".join(s + b"$" for s in seqs))


def test_the_files_sites_are_the_oracles(made):
    contigs, text = made["contigs"], made["text"]
    regions = [(0, 0, 700), (1, 100, 1200), (2, 0, 40), (1, 0, 1300)]
    named = [("chrA", 0, 700), (1, 100, 1200), (b"tiny", 0, 40), ("chrB", 0, 1300)]
    for kw in (dict(), dict(min_depth=3, min_alt=2, min_alt_permille=200, cover=(1, 3, 5, 8)), dict(min_alt_strand=1, exclude=0x10)):
        want, want_off, want_sum = so.sites(made["slots"], contigs, text, regions, **kw)
        if not kw:  # the condition, under the oracle alone
            assert {s[3] for s in want} == {so.SNV, so.DEL, so.INS} and sum(s["n_ref_other"] for s in want_sum) > 0
            assert any(s[4] != text[contigs[s[0]][1] + s[1]] for s in want)  # (a site on a soft-masked base)
        for reference in (fasta_text(made["seqs"]), text):
            sites, site_off, summary = bam.sites_bam(made["data"], reference, named, **kw)
            assert so.as_tuples(sites) == want and site_off.tolist() == want_off and so.as_dicts(summary) == want_sum, kw


def test_a_header_that_disagrees_with_the_reference_is_named(made):
    seqs = made["seqs"]
    for reference in (fasta_text([seqs[0], seqs[1][:-1], seqs[2]]), seqs[0] + b"$" + seqs[1][:-1] + b"$" + seqs[2] + b"$"):
        with pytest.raises(ValueError) as e:
            bam.sites_bam(made["data"], reference, [("chrA", 0, 10)])
        assert "chrB" in str(e.value) and "1300" in str(e.value) and "1299" in str(e.value)
    with pytest.raises(ValueError) as e:
        bam.sites_bam(made["data"], fasta_text(seqs[:2]), [("chrA", 0, 10)])
    assert "tiny" in str(e.value)
    with pytest.raises(ValueError) as e:
        bam.sites_bam(made["data"], fasta_text(seqs), [("chrZ", 0, 10)])
    assert "chrZ" in str(e.value)

"""The chain records -> candidate sites and indel events -> VCF text on the GPU, with nothing copied to the host in between: for a
handful of cases of tests/bam_sites_cases.py and tests/bam_indels_cases.py that have a reference text, CPU-made records go
through `bam.sites_dev`, `bam.indels_dev` and `vcf.emit_dev`, each reading what the one before left in HBM, and the bytes are
what the VCF oracle (tests/vcf_oracle.py) makes of the sites oracle's and the indels oracle's output.  Then `vcf.vcf_bam` on a
BAM file made on the CPU with deflate-compressed blocks: plain, and with compress=True, where zlib on the host inflates the
members to header plus body, byte for byte."""
import zlib

import numpy as np
import pytest
import torch

import bam_indels_cases as ic
import bam_indels_oracle as io
import bam_oracle as bo
import bam_pileup_cases as pc
import bam_sites_cases as sc
import bam_sites_oracle as so
import vcf_cases as vc
import vcf_oracle as vo
from rust_bio_amd import bam, sam, vcf
from test_gpu_bam_sites_file import LENS, NAMES, deflated, records, sequences

pytestmark = pytest.mark.gpu
SHARED = ("require", "exclude", "min_mapq", "min_baseq", "min_depth", "min_alt", "min_alt_permille", "min_alt_strand")


def stream():
    return torch.cuda.current_stream().cuda_stream


def on_device(a):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy() if len(a) else np.zeros(16, np.uint8)).cuda()


def expected(slots, contigs, text, regions, kw):
    """the VCF oracle on the two oracles' lists: (text, line_off, n_sites, n_events)"""
    sites, _, _ = so.sites(slots, contigs, text, regions, **kw)
    events, seq, _ = io.indels(slots, contigs, regions, **kw)
    s = np.array([t[:6] + (0,) + t[6:] for t in sites], dtype=vc.SITE) if sites else np.zeros(0, vc.SITE)
    e = np.array([t[:4] + ((0, 0, 0),) + t[4:] for t in events], dtype=vc.EVENT) if events else np.zeros(0, vc.EVENT)
    return vo.emit(s, e, seq, contigs, text) + (len(s), len(e))


def cases():
    by_sites = {c["name"]: c for c in sc.corpus(with_deep=False)}
    picked = [by_sites[n] for n in ("a tile whose 512 positions all give 5 sites", "sites across a tile border", "random records, strict",
                                    "the threshold pile, {}")]
    out = [dict(name=c["name"], slots=c["slots"], contigs=c["contigs"], text=c["text"], regions=c["regions"], kw={k: c["params"][k] for k in SHARED})
           for c in picked]
    for c in ic.corpus(with_deep=False):
        if c["name"] in ("everything, region shapes", "insertions that differ in the last base or in base 17", "N, = and every code inside an insertion"):
            assert c["contigs"] is sc.CONTIGS
            out.append(dict(name=c["name"], slots=c["slots"], contigs=c["contigs"], text=sc.TEXT, regions=c["regions"], kw={k: c["params"][k] for k in SHARED}))
    assert len(out) == 7
    return out


def test_records_to_vcf_text_without_a_host_copy_in_between():
    lines = kinds = 0
    for c in cases():
        slots, contigs, text, regions, kw = c["slots"], c["contigs"], c["text"], c["regions"], c["kw"]
        want, want_off, n_sites_want, n_events_want = expected(slots, contigs, text, regions, kw)
        table = sam.Contigs(contigs)
        d_recs, d_off, d_contigs, d_names = on_device(b"".join(slots) or b"\0"), on_device(bo.offsets(slots)), on_device(table.table), on_device(table.names)
        d_text, d_regions = on_device(np.frombuffer(text, np.uint8)), on_device(bam.pileup_regions(regions))
        front = (len(slots), d_recs.data_ptr(), d_off.data_ptr(), d_contigs.data_ptr(), len(contigs))
        regs = (d_regions.data_ptr(), len(regions))
        n_sites = bam.sites_dev(*front, d_text.data_ptr(), len(text), *regs, stream=stream(), **kw)
        d_sites = torch.zeros(32 * max(n_sites, 1), dtype=torch.uint8, device="cuda")
        bam.sites_dev(*front, d_text.data_ptr(), len(text), *regs, d_sites.data_ptr(), n_sites, stream=stream(), **kw)
        n_events, n_seq = bam.indels_dev(*front, *regs, stream=stream(), **kw)
        d_events, d_seq = torch.zeros(40 * max(n_events, 1), dtype=torch.uint8, device="cuda"), torch.zeros(max(n_seq, 1), dtype=torch.uint8, device="cuda")
        bam.indels_dev(*front, *regs, d_events.data_ptr(), n_events, d_seq.data_ptr(), n_seq, stream=stream(), **kw)
        assert (n_sites, n_events) == (n_sites_want, n_events_want), c["name"]
        lists = (n_sites, d_sites.data_ptr(), n_events, d_events.data_ptr(), d_seq.data_ptr(), n_seq, d_contigs.data_ptr(), len(contigs), d_names.data_ptr(),
                 d_text.data_ptr(), len(text))
        n_lines, total = vcf.emit_dev(*lists, stream=stream())
        assert (n_lines, total) == (len(want_off) - 1, len(want)), c["name"]
        d_out = torch.full((total + 7,), 0xA5, dtype=torch.uint8, device="cuda")
        d_line_off = torch.zeros(n_lines + 1, dtype=torch.int64, device="cuda")
        assert vcf.emit_dev(*lists, d_out.data_ptr(), total, d_line_off.data_ptr(), stream=stream()) == (n_lines, total)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert got[:total].tobytes() == want and (got[total:] == 0xA5).all() and d_line_off.cpu().numpy().tolist() == want_off, c["name"]
        lines += n_lines
        kinds |= (b"TYPE=snp" in want) | 2 * (b"TYPE=del" in want) | 4 * (b"TYPE=ins" in want)
    assert lines > 1000 and kinds == 7


def inflate_members(data):
    out, at = b"", 0
    while at < len(data):
        z = zlib.decompressobj(31)
        out += z.decompress(data[at:])
        assert z.eof
        at = len(data) - len(z.unused_data)
    return out


@pytest.fixture(scope="module")
def made():
    seqs = sequences()
    contigs = pc.contigs_of(LENS, NAMES)
    slots = records(seqs, contigs)
    data = deflated(bo.header(b"@HD\tVN:1.6\tSO:coordinate\n", contigs) + b"".join(slots))
    return dict(contigs=contigs, slots=slots, data=data, text=b"".join(s + b"$" for s in seqs))


def test_a_bam_file_to_a_vcf_file_plain_and_compressed(made):
    contigs, text = made["contigs"], made["text"]
    whole = [(r, 0, ln) for r, ln in enumerate(LENS)]
    for regions, named, kw in ((whole, None, dict()), ([(1, 100, 1200), (0, 0, 700)], [("chrB", 100, 1200), (0, 0, 700)], dict(min_depth=3, min_alt=2)),
                               ([(2, 0, 40)], [(b"tiny", 0, 40)], dict(exclude=0x10))):
        body, _, n_sites, n_events = expected(made["slots"], contigs, text, regions, {k: dict(io.DEFAULT, **kw)[k] for k in SHARED})
        want = vo.header(contigs) + body
        if named is None:
            assert n_sites > 10 and n_events > 5 and b"TYPE=del" in body and b"TYPE=ins" in body  # the condition, under the oracles alone
        assert vcf.vcf_bam(made["data"], text, named, **kw) == want, kw
        packed = vcf.vcf_bam(made["data"], text, named, compress=True, **kw)
        assert packed.endswith(bo.EOF_BLOCK) and len(packed) < len(want) + 28 and inflate_members(packed) == want, kw
    with pytest.raises(ValueError):
        vcf.vcf_bam(made["data"], text, [("chrZ", 0, 10)])
    with pytest.raises(TypeError):
        vcf.vcf_bam(made["data"], text, cover=(1, 2, 3, 4))

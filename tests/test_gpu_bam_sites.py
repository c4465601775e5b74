"""bg_bam_sites[_dev] on the GPU against tests/bam_sites_oracle.py, record for record, and against `from_rows` applied to what
bg_bam_pileup_dev returns for the same inputs (a second derivation, through code that is not under test): the corpus of
tests/bam_sites_cases.py — the pileup's corpus (regions of 0, 1, T - 1, T, T + 1 positions, an empty tile between populated
ones, 66 000 records at one position, 1 000 small regions that overlap, repeat and come unordered, contigs with a non-zero
start) against a text with lower-case, N and IUPAC bytes; a site on the last position of a tile and on the first of the next;
a tile whose 512 positions all give 5 sites; every threshold one below and at its value — in the device and the host flavour.
Sites, offsets and summaries are pre-filled and lie between guard bytes; once more with d_sites at byte offsets 0, 4, 8, 12 and
d_text and d_recs at every residue 0 .. 15.  Sizing, a capacity one short and every refusal (a contig past n_text among them)
leave everything untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import bam_oracle as bo
import bam_sites_cases as sc
import bam_sites_oracle as so
from dev_shift import guards_intact, shifted, shifted_from
from rust_bio_amd import _lib, bam, sam

pytestmark = pytest.mark.gpu
NONE = 2**64 - 1
FILL = 0xA5
SLACK = 3  # records behind n_sites that must stay as they were
SITE, SUMMARY = _lib.BAM_SITE_DTYPE, _lib.BAM_REGION_SUMMARY_DTYPE


def stream():
    return torch.cuda.current_stream().cuda_stream


def on_device(a):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy() if len(a) else np.zeros(16, np.uint8)).cuda()


@pytest.fixture(scope="module")
def corpus():
    """[(case, sites, site_off, summaries)]: the oracle once for every case"""
    return [(c,) + sc.want_of(c) for c in sc.corpus()]


class Dev:
    """a case's arguments in HBM; the records at residue r_in, the text at residue r_text"""

    def __init__(self, c, r_in=0, r_text=0):
        slots = c["slots"]
        self.c, self.n, self.n_contigs, self.n_regions = c, len(slots), len(c["contigs"]), len(c["regions"])
        self.n_text = c.get("n_text", len(c["text"]))
        self.recs = shifted_from(b"".join(slots) or b"\0", r_in)
        self.text = shifted_from(bytes(c["text"]) or b"\0", r_text)
        self.off = on_device(bo.offsets(slots))
        self.contigs = on_device(sam.Contigs(c["contigs"]).table)
        self.regions = on_device(bam.pileup_regions(c["regions"]))

    def head(self):
        return (self.n, self.recs.data_ptr() if self.n else 0, self.off.data_ptr() if self.n else 0, self.contigs.data_ptr() if self.n_contigs else 0,
                self.n_contigs)

    def tail(self):
        return (self.regions.data_ptr() if self.n_regions else 0, self.n_regions)

    def call(self, d_sites=0, cap=0, d_site_off=0, d_summary=0):
        return bam.sites_dev(*self.head(), self.text.data_ptr() if self.n_text else 0, self.n_text, *self.tail(), d_sites, cap, d_site_off, d_summary,
                             stream=stream(), **self.c["params"])

    def rows16(self):
        """what bg_bam_pileup_dev gives for the same records, regions and filters: (rows, row_off)"""
        p = self.c["params"]
        kw = dict(flags=bam.PILEUP_STRANDS, require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"], min_baseq=p["min_baseq"], stream=stream())
        n = bam.pileup_dev(*self.head(), *self.tail(), **kw)
        d_rows = torch.zeros(max(n, 1) * 16, dtype=torch.int32, device="cuda")
        d_row_off = torch.zeros(self.n_regions + 1, dtype=torch.int64, device="cuda")
        assert bam.pileup_dev(*self.head(), *self.tail(), d_rows.data_ptr(), n, d_row_off.data_ptr(), **kw) == n
        torch.cuda.synchronize()
        return d_rows.cpu().numpy().view(np.uint32).reshape(-1, 16)[:n], d_row_off.cpu().numpy().tolist()


def sites_dev(c, r_in=0, r_text=0, r_out=0):
    """the device flavour between guards: (sites, site_off, summaries) as the oracle writes them"""
    d = Dev(c, r_in, r_text)
    n = d.call()  # the sizing call
    d_sites = shifted(32 * (n + SLACK), r_out, fill=FILL)
    d_site_off = shifted(8 * (d.n_regions + 1), 8, fill=FILL)
    d_summary = shifted(48 * d.n_regions, r_out, fill=FILL)
    assert d.call(d_sites.data_ptr(), n + SLACK, d_site_off.data_ptr(), d_summary.data_ptr()) == n
    assert guards_intact(d_sites) and guards_intact(d_site_off) and guards_intact(d_summary) and guards_intact(d.recs) and guards_intact(d.text)
    got = d_sites.cpu().numpy()
    assert (got[32 * n:] == FILL).all()  # nothing behind record n_sites
    return (so.as_tuples(got[:32 * n].view(SITE)), d_site_off.cpu().numpy().view(np.uint64).tolist(),
            so.as_dicts(d_summary.cpu().numpy().view(SUMMARY)))


def sites_host(c):
    slots = c["slots"]
    sites, site_off, summary = bam.sites_arrays(b"".join(slots), bo.offsets(slots), sam.Contigs(c["contigs"]), c["text"], c["regions"], **c["params"])
    return so.as_tuples(sites), site_off.tolist(), so.as_dicts(summary)


def test_the_corpus_in_the_device_flavour(corpus):
    for c, want, want_off, want_sum in corpus:
        assert sites_dev(c) == (want, want_off, want_sum), c["name"]


def test_the_sites_are_what_the_pileups_rows_give(corpus):
    for c, want, want_off, want_sum in corpus:
        rows, row_off = Dev(c).rows16()
        assert so.from_rows(rows, row_off, c["regions"], c["contigs"], c["text"], c["params"]) == (want, want_off, want_sum), c["name"]


def test_the_host_flavour_gives_the_device_flavours_sites(corpus):
    for c, want, want_off, want_sum in corpus:
        assert sites_host(c) == (want, want_off, want_sum), c["name"]


def test_a_tile_of_2560_sites_and_a_deep_pile(corpus):
    by = {c["name"]: (c, want, s) for c, want, _, s in corpus}
    c, want, _ = by["a tile whose 512 positions all give 5 sites"]
    got = sites_dev(c)[0]
    assert len(got) == 5 * sc.T and got == want and [s[3] for s in got[:5]] == [so.SNV, so.SNV, so.SNV, so.DEL, so.INS]
    c, want, want_sum = by["66 000 records at one position, strands"]
    got, _, summary = sites_dev(c)
    assert got == want and summary == want_sum and summary[0]["max_depth"] == 66_000 > 0xFFFF and len(got) == 3


def test_pointers_off_16_byte_alignment(corpus):
    by = {c["name"]: (c, want, off, s) for c, want, off, s in corpus}
    for name in ("every op kind", "all 16 codes, strands"):
        c, *want = by[name]
        for r in range(16):
            assert list(sites_dev(c, r_in=r, r_text=(5 * r + 3) % 16, r_out=4 * (r % 4))) == want, (name, r)
    for name in ("tile borders", "a tile whose 512 positions all give 5 sites", "region shapes"):
        c, *want = by[name]
        for r_out in (0, 4, 8, 12):
            assert list(sites_dev(c, r_in=(3 * r_out + 1) % 16, r_text=(r_out + 1) % 16, r_out=r_out)) == want, (name, r_out)


def test_the_optional_outputs_may_be_absent_and_calls_repeat(corpus):
    c, want, want_off, want_sum = next(t for t in corpus if t[0]["name"] == "random records, strict")
    d, n = Dev(c), len(want)
    side = torch.cuda.Stream()
    for k in range(3):
        d_sites = torch.full((32 * max(n, 1),), FILL, dtype=torch.uint8, device="cuda")
        d_summary = shifted(48 * d.n_regions, 0, fill=FILL)
        with torch.cuda.stream(side if k == 1 else torch.cuda.current_stream()):
            assert bam.sites_dev(*d.head(), d.text.data_ptr(), d.n_text, *d.tail(), d_sites.data_ptr(), n, 0, d_summary.data_ptr() if k else 0,
                                 stream=torch.cuda.current_stream().cuda_stream, **c["params"]) == n
        torch.cuda.synchronize()
        assert so.as_tuples(d_sites.cpu().numpy()[:32 * n].view(SITE)) == want, k
        if k:
            assert so.as_dicts(d_summary.cpu().numpy().view(SUMMARY)) == want_sum, k
        else:
            assert (d_summary.cpu().numpy() == FILL).all()


def host_call(c, sites, cap, site_off, summary):
    slots = c["slots"]
    body = np.frombuffer(b"".join(slots) or b"\0", dtype=np.uint8)
    text = np.frombuffer(bytes(c["text"]) or b"\0", dtype=np.uint8)
    n_text = c.get("n_text", len(c["text"]))
    off, table, reg, prm = bo.offsets(slots), sam.Contigs(c["contigs"]).table, bam.pileup_regions(c["regions"]), bam.sites_params(**c["params"])
    total, bad = C.c_uint64(0), C.c_uint64(0)
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    rc = _lib.lib().bg_bam_sites(_lib.default_context().h, prm.ctypes.data, len(slots), body.ctypes.data, off.ctypes.data, table.ctypes.data if len(table) else None,
                                 len(table), text.ctypes.data if n_text else None, n_text, reg.ctypes.data if len(reg) else None, len(reg), ptr(sites), cap,
                                 ptr(site_off), ptr(summary), C.byref(total), C.byref(bad))
    return rc, total.value, bad.value


def test_refusals_leave_everything_untouched():
    for c in sc.refusals():
        name, (status, slot) = c["name"], c["want"]
        if c["n_text"] != len(c["text"]):  # (a text the call is only told of: the device flavour alone, which copies nothing)
            c = dict(c, host=False)
        d = Dev(c)
        d_sites, d_site_off = shifted(4096, 4, fill=0xC3), shifted(8 * (d.n_regions + 1), 8, fill=0xC3)
        d_summary = shifted(48 * d.n_regions, 4, fill=0xC3)
        for out, cap, soff, summ in ((0, 0, 0, 0), (d_sites.data_ptr(), 4096 // 32, d_site_off.data_ptr(), d_summary.data_ptr())):
            with pytest.raises(bam.BamPileupError) as e:
                d.call(out, cap, soff, summ)
            assert (e.value.status, e.value.slot) == (status, slot), name
        for buf in (d_sites, d_site_off, d_summary):
            assert guards_intact(buf) and (buf.cpu().numpy() == 0xC3).all(), name
        if c.get("host", True):
            canary, canary_off = np.full(128, 0xC3, dtype=np.uint8).repeat(32).view(SITE), np.full(d.n_regions + 1, 0xC3, dtype=np.uint64)
            canary_sum = np.full(48 * max(d.n_regions, 1), 0xC3, dtype=np.uint8).view(SUMMARY)
            first = NONE if slot is None else slot
            assert host_call(c, canary, 128, canary_off, canary_sum) == (status, 0, first), name
            assert host_call(c, None, 0, None, None) == (status, 0, first), name
            assert (canary.view(np.uint8) == 0xC3).all() and (canary_off == 0xC3).all() and (canary_sum.view(np.uint8) == 0xC3).all(), name
            with pytest.raises(bam.BamPileupError) as e:
                sites_host(c)
            assert (e.value.status, e.value.slot) == (status, slot), name


def test_sizing_and_a_capacity_one_record_short(corpus):
    by = {c["name"]: (c, want) for c, want, _, _ in corpus}
    for name in ("every op kind", "region shapes", "1 000 regions of 1 .. 3 positions", "a tile whose 512 positions all give 5 sites"):
        c, want = by[name]
        d, n = Dev(c), len(want)
        assert n > 0 and d.call() == n
        d_sites, d_site_off, d_summary = shifted(32 * n, 0, fill=0xC3), shifted(8 * (d.n_regions + 1), 0, fill=0xC3), shifted(48 * d.n_regions, 0, fill=0xC3)
        with pytest.raises(_lib.BiogpuError) as e:
            d.call(d_sites.data_ptr(), n - 1, d_site_off.data_ptr(), d_summary.data_ptr())
        assert e.value.status == so.OPS_CAP and not isinstance(e.value, bam.BamPileupError), name
        for buf in (d_sites, d_site_off, d_summary):
            assert guards_intact(buf) and (buf.cpu().numpy() == 0xC3).all(), name
        canary = np.full(32 * n, 0xC3, dtype=np.uint8).view(SITE)
        assert host_call(c, canary, n - 1, None, None) == (so.OPS_CAP, n, NONE) and (canary.view(np.uint8) == 0xC3).all(), name
        assert host_call(c, canary, n, None, None) == (0, n, NONE) and so.as_tuples(canary) == want, name
    with pytest.raises(bam.BamPileupError):  # the sizing call makes every check
        Dev(sc.refusals()[0]).call()
    with pytest.raises(bam.BamPileupError):
        Dev(dict(by["every op kind"][0], params=so.params(min_alt_permille=1001))).call()


def test_2_32_positions_are_too_large():
    big = sc.pc.contigs_of([2**31 - 1], [b"big"])
    whole = (0, 0, 2**31 - 1)
    c = dict(slots=[], contigs=big, text=b"ACGT", n_text=2**31, regions=[whole, whole, (0, 5, 7)], params=so.params())
    with pytest.raises(_lib.BiogpuError) as e:  # (refused before a byte of the text is read)
        Dev(c).call()
    assert e.value.status == so.TOO_LARGE and not isinstance(e.value, bam.BamPileupError)


def test_results_do_not_depend_on_the_tile(corpus):
    """a region cut at arbitrary places gives the sites of the whole, renumbered, and summaries that add up"""
    c, want, _, want_sum = next(t for t in corpus if t[0]["name"] == "the full tile in the middle of a region, and cut")
    T = bam.PILEUP_TILE
    cuts = [0, 1, T - 7, T - 1, T, T + 1, 2 * T - 3, 2 * T + 100, 3 * T + 5, sc.CONTIGS[0][2]]
    pieces = dict(c, regions=[(0, a, b) for a, b in zip(cuts, cuts[1:])])
    got, site_off, summary = sites_dev(pieces)
    whole = [s for s in want if s[2] == 0]
    assert [s[:2] + s[3:] for s in got] == [s[:2] + s[3:] for s in whole]
    assert [s[2] for s in got] == [next(k for k in range(len(cuts) - 1) if cuts[k] <= s[1] < cuts[k + 1]) for s in got]
    assert site_off[-1] == len(whole) and site_off == sorted(site_off)
    for key in ("sum_depth", "match", "mismatch", "n_ref_other"):
        assert sum(s[key] for s in summary) == want_sum[0][key], key
    assert max(s["max_depth"] for s in summary) == want_sum[0]["max_depth"]
    assert [sum(s["covered"][k] for s in summary) for k in range(4)] == want_sum[0]["covered"]

"""bg_bam_indels_left[_dev] on the GPU against tests/bam_indels_left_oracle.py, record for record and byte for byte: the corpus of
tests/bam_indels_left_cases.py — raw anchors that shift over a tile's edge, a deletion that lands two tiles in front of its raw
anchor, regions that hold only the raw or only the shifted anchor, insertions of 1, 15, 16, 17 and 33 bases with k below, at
and above their length, spellings that meet only behind the shift, 1 100 records on one event, and the corpus of
tests/bam_indels_cases.py with max_shift 0 — in the device and the host flavour.  Where max_shift is 0 the bytes are those of
bg_bam_indels_dev on the same inputs; the depths are what bg_bam_pileup_dev's rows give at the shifted anchors.  Events,
sequences and offsets are pre-filled and lie between guard bytes; d_events at every 8-byte-aligned residue of 64, d_seq, d_text
and d_recs at odd addresses.  Sizing, each capacity one short and every refusal leave everything untouched; a call repeated
gives the same bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import bam_indels_left_cases as lc
import bam_indels_left_oracle as lo
import bam_indels_oracle as io
import bam_oracle as bo
from dev_shift import guards_intact, shifted, shifted_from
from rust_bio_amd import _lib, bam, sam

pytestmark = pytest.mark.gpu
NONE = 2**64 - 1
FILL = 0xA5
SLACK = 3  # records and bytes behind the totals that must stay as they were
EVENT = _lib.BAM_INDEL_DTYPE


def stream():
    return torch.cuda.current_stream().cuda_stream


def on_device(a):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy() if len(a) else np.zeros(16, np.uint8)).cuda()


@pytest.fixture(scope="module")
def corpus():
    """[(case, events, seq, event_off)]: the oracle once for every case"""
    return [(c,) + lc.want_of(c) for c in lc.corpus()]


class Dev:
    """a case's arguments in HBM; the records at residue r_in, the text at residue r_text"""

    def __init__(self, c, r_in=0, r_text=0):
        slots = c["slots"]
        self.c, self.n, self.n_contigs, self.n_regions, self.n_text = c, len(slots), len(c["contigs"]), len(c["regions"]), c["n_text"]
        self.recs = shifted_from(b"".join(slots) or b"\0", r_in)
        self.off = on_device(bo.offsets(slots))
        self.contigs = on_device(sam.Contigs(c["contigs"]).table)
        self.text = shifted_from(c["text"][:c["n_text"]] or b"\0", r_text)  # not a byte behind n_text
        self.regions = on_device(bam.pileup_regions(c["regions"]))

    def head(self):
        return (self.n, self.recs.data_ptr() if self.n else 0, self.off.data_ptr() if self.n else 0, self.contigs.data_ptr() if self.n_contigs else 0,
                self.n_contigs)

    def regs(self):
        return (self.regions.data_ptr() if self.n_regions else 0, self.n_regions)

    def call(self, d_events=0, cap=0, d_seq=0, seq_cap=0, d_event_off=0, null_text=False):
        return bam.indels_left_dev(*self.head(), 0 if null_text or not self.n_text else self.text.data_ptr(), self.n_text, *self.regs(), d_events, cap, d_seq,
                                   seq_cap, d_event_off, stream=stream(), **self.c["params"])

    def plain(self, d_events=0, cap=0, d_seq=0, seq_cap=0, d_event_off=0):
        """bg_bam_indels_dev on the same inputs"""
        return bam.indels_dev(*self.head(), *self.regs(), d_events, cap, d_seq, seq_cap, d_event_off, stream=stream(),
                              **{f: self.c["params"][f] for f in io.DEFAULT})

    def rows16(self):
        """what bg_bam_pileup_dev gives for the same records, regions and filters: (rows, row_off)"""
        p = self.c["params"]
        kw = dict(flags=bam.PILEUP_STRANDS, require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"], min_baseq=p["min_baseq"], stream=stream())
        n = bam.pileup_dev(*self.head(), *self.regs(), **kw)
        d_rows = torch.zeros(max(n, 1) * 16, dtype=torch.int32, device="cuda")
        d_row_off = torch.zeros(self.n_regions + 1, dtype=torch.int64, device="cuda")
        assert bam.pileup_dev(*self.head(), *self.regs(), d_rows.data_ptr(), n, d_row_off.data_ptr(), **kw) == n
        torch.cuda.synchronize()
        return d_rows.cpu().numpy().view(np.uint32).reshape(-1, 16)[:n], d_row_off.cpu().numpy().tolist()


def between_guards(d, fn, r_events=0, r_seq=0, raw=False):
    """fn (Dev.call or Dev.plain) between guards: (events, seq, event_off) as the oracle writes them; raw: the bytes of all three"""
    n, n_seq = fn()  # the sizing call
    assert r_events % 8 == 0
    wide = shifted(40 * (n + SLACK) + 64, 0, fill=FILL)  # a residue of 64 inside an allocation whose view begins at a multiple of 16
    skip = (r_events - wide.data_ptr()) % 64
    d_events = wide[skip:skip + 40 * (n + SLACK)]
    assert d_events.data_ptr() % 64 == r_events
    d_seq = shifted(n_seq + SLACK, r_seq, fill=FILL)
    d_event_off = shifted(8 * (d.n_regions + 1), 8, fill=FILL)
    assert fn(d_events.data_ptr(), n + SLACK, d_seq.data_ptr(), n_seq + SLACK, d_event_off.data_ptr()) == (n, n_seq)
    assert guards_intact(wide) and guards_intact(d_seq) and guards_intact(d_event_off) and guards_intact(d.recs) and guards_intact(d.text)
    everything, got_seq = wide.cpu().numpy(), d_seq.cpu().numpy()
    got = everything[skip:skip + 40 * (n + SLACK)]
    assert (everything[:skip] == FILL).all() and (everything[skip + 40 * n:] == FILL).all() and (got_seq[n_seq:] == FILL).all()  # nothing around the totals
    if raw:
        return got.tobytes(), got_seq.tobytes(), d_event_off.cpu().numpy().tobytes()
    return io.as_tuples(got[:40 * n].view(EVENT)), got_seq[:n_seq].tobytes(), d_event_off.cpu().numpy().view(np.uint64).tolist()


def left_dev(c, r_in=0, r_text=0, r_events=0, r_seq=0, raw=False):
    d = Dev(c, r_in, r_text)
    return between_guards(d, d.call, r_events, r_seq, raw)


def left_host(c):
    slots = c["slots"]
    events, seq, event_off = bam.indels_left_arrays(b"".join(slots), bo.offsets(slots), sam.Contigs(c["contigs"]), c["text"][:c["n_text"]], c["regions"],
                                                    **c["params"])
    assert not events["reserved"].any()
    return io.as_tuples(events), seq.tobytes(), event_off.tolist()


def test_the_corpus_in_the_device_flavour(corpus):
    for c, want, want_seq, want_off in corpus:
        assert left_dev(c) == (want, want_seq, want_off), c["name"]


def test_max_shift_0_gives_the_bytes_of_the_unshifted_call(corpus):
    seen = 0
    for c, want, want_seq, want_off in corpus:
        if c["params"]["max_shift"]:
            continue
        d = Dev(c)
        assert between_guards(d, d.call, raw=True) == between_guards(d, d.plain, raw=True), c["name"]
        seen += 1
    assert seen > len(lc.ic.corpus())


def test_the_depths_are_what_the_pileups_rows_give_at_the_shifted_anchors(corpus):
    for c, want, want_seq, want_off in corpus:
        rows, row_off = Dev(c).rows16()
        assert lo.from_rows(c["slots"], c["contigs"], c["text"], rows, row_off, c["regions"], **c["params"]) == (want, want_seq, want_off), c["name"]


def test_the_host_flavour_gives_the_device_flavours_events(corpus):
    for c, want, want_seq, want_off in corpus:
        assert left_host(c) == (want, want_seq, want_off), c["name"]


def test_events_at_every_aligned_residue_and_the_rest_at_odd_addresses(corpus):
    by = {c["name"]: (c, want, seq, off) for c, want, seq, off in corpus}
    for name in ("insertions of 1, 15, 16, 17 and 33 bases with k below, at and above their length", "raw anchors at T - 1, T and T + 1 of a tile that shift by one"):
        c, *want = by[name]
        for k, r_events in enumerate(range(0, 64, 8)):
            assert list(left_dev(c, r_in=(2 * k + 1) % 16, r_text=(2 * k + 3) % 16, r_events=r_events, r_seq=(2 * k + 5) % 16)) == want, (name, r_events)
    for name in ("a deletion that lands two tiles in front of its raw anchor", "everything, region shapes, against a random text"):
        c, *want = by[name]
        for r in (1, 7, 15):
            assert list(left_dev(c, r_in=(3 * r) % 16, r_text=r, r_events=8 * (r % 8), r_seq=(5 * r) % 16)) == want, (name, r)


def test_a_call_repeated_gives_identical_bytes_and_offsets_may_be_absent(corpus):
    c, want, want_seq, want_off = next(t for t in corpus if t[0]["name"] == "everything, region shapes, against a random text")
    first = left_dev(c, raw=True)
    assert left_dev(c, raw=True) == first
    d, n, n_seq = Dev(c), len(want), len(want_seq)
    side = torch.cuda.Stream()
    for k in range(2):
        d_events = torch.full((40 * n,), FILL, dtype=torch.uint8, device="cuda")
        d_seq = torch.full((max(n_seq, 1),), FILL, dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(side if k else torch.cuda.current_stream()):
            assert bam.indels_left_dev(*d.head(), d.text.data_ptr(), d.n_text, *d.regs(), d_events.data_ptr(), n, d_seq.data_ptr(), n_seq, 0,
                                       stream=torch.cuda.current_stream().cuda_stream, **c["params"]) == (n, n_seq)
        torch.cuda.synchronize()
        assert d_events.cpu().numpy().tobytes() == first[0][:40 * n] and d_seq.cpu().numpy()[:n_seq].tobytes() == want_seq, k


def host_call(c, events, cap, seq, seq_cap, event_off, null_text=False):
    slots = c["slots"]
    body = np.frombuffer(b"".join(slots) or b"\0", dtype=np.uint8)
    text = np.frombuffer(c["text"][:c["n_text"]] or b"\0", dtype=np.uint8)
    off, table, reg, prm = bo.offsets(slots), sam.Contigs(c["contigs"]).table, bam.pileup_regions(c["regions"]), bam.indels_left_params(**c["params"])
    total, n_seq, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    rc = _lib.lib().bg_bam_indels_left(_lib.default_context().h, prm.ctypes.data, len(slots), body.ctypes.data, off.ctypes.data,
                                       table.ctypes.data if len(table) else None, len(table), None if null_text or not c["n_text"] else text.ctypes.data,
                                       c["n_text"], reg.ctypes.data if len(reg) else None, len(reg), ptr(events), cap, ptr(seq), seq_cap, ptr(event_off),
                                       C.byref(total), C.byref(n_seq), C.byref(bad))
    return rc, total.value, n_seq.value, bad.value


def test_refusals_leave_everything_untouched():
    for c in lc.refusals():
        name, (status, slot) = c["name"], c["want"]
        d = Dev(c)
        d_events, d_seq, d_event_off = shifted(4000, 8, fill=0xC3), shifted(333, 5, fill=0xC3), shifted(8 * (d.n_regions + 1), 8, fill=0xC3)
        for args in ((0, 0, 0, 0, 0), (d_events.data_ptr(), 100, d_seq.data_ptr(), 333, d_event_off.data_ptr())):
            with pytest.raises(bam.BamPileupError) as e:
                d.call(*args)
            assert (e.value.status, e.value.slot) == (status, slot), name
        for buf in (d_events, d_seq, d_event_off):
            assert guards_intact(buf) and (buf.cpu().numpy() == 0xC3).all(), name
        if c["n_text"] > len(c["text"]):  # (a text the call is only told of: the device flavour alone, which copies nothing)
            continue
        canary, canary_seq = np.full(100 * 40, 0xC3, dtype=np.uint8).view(EVENT), np.full(64, 0xC3, dtype=np.uint8)
        canary_off = np.full(d.n_regions + 1, 0xC3, dtype=np.uint64)
        first = NONE if slot is None else slot
        assert host_call(c, canary, 100, canary_seq, 64, canary_off) == (status, 0, 0, first), name
        assert host_call(c, None, 0, None, 0, None) == (status, 0, 0, first), name
        assert (canary.view(np.uint8) == 0xC3).all() and (canary_seq == 0xC3).all() and (canary_off == 0xC3).all(), name
        with pytest.raises(bam.BamPileupError) as e:
            left_host(c)
        assert (e.value.status, e.value.slot) == (status, slot), name


def test_a_null_text_is_refused_in_both_flavours(corpus):
    c = corpus[0][0]
    d = Dev(c)
    d_events, d_seq = shifted(4000, 8, fill=0xC3), shifted(333, 5, fill=0xC3)
    for args in ((0, 0, 0, 0, 0), (d_events.data_ptr(), 100, d_seq.data_ptr(), 333, 0)):
        with pytest.raises(bam.BamPileupError) as e:
            d.call(*args, null_text=True)
        assert (e.value.status, e.value.slot) == (lo.INVALID_ARG, None)
    assert (d_events.cpu().numpy() == 0xC3).all() and (d_seq.cpu().numpy() == 0xC3).all()
    assert host_call(c, None, 0, None, 0, None, null_text=True) == (lo.INVALID_ARG, 0, 0, NONE)


def test_sizing_and_each_capacity_one_short(corpus):
    by = {c["name"]: (c, want, seq) for c, want, seq, _ in corpus}
    for name in ("insertions of 1, 15, 16, 17 and 33 bases with k below, at and above their length", "everything, region shapes, against a random text",
                 "everything, 1 000 regions of 1 .. 3 positions, max_shift 0"):
        c, want, want_seq = by[name]
        d, n, n_seq = Dev(c), len(want), len(want_seq)
        assert n > 0 and n_seq > 0 and d.call() == (n, n_seq)
        d_events, d_seq, d_event_off = shifted(40 * n, 0, fill=0xC3), shifted(n_seq, 3, fill=0xC3), shifted(8 * (d.n_regions + 1), 0, fill=0xC3)
        for cap, seq_cap in ((n - 1, n_seq), (n, n_seq - 1), (0, 0)):
            with pytest.raises(_lib.BiogpuError) as e:
                d.call(d_events.data_ptr(), cap, d_seq.data_ptr(), seq_cap, d_event_off.data_ptr())
            assert e.value.status == io.OPS_CAP and not isinstance(e.value, bam.BamPileupError) and e.value.totals == (n, n_seq), name
            for buf in (d_events, d_seq, d_event_off):
                assert guards_intact(buf) and (buf.cpu().numpy() == 0xC3).all(), name
        canary, canary_seq = np.full(40 * n, 0xC3, dtype=np.uint8).view(EVENT), np.full(n_seq, 0xC3, dtype=np.uint8)
        for cap, seq_cap in ((n - 1, n_seq), (n, n_seq - 1)):
            assert host_call(c, canary, cap, canary_seq, seq_cap, None) == (io.OPS_CAP, n, n_seq, NONE), name
            assert (canary.view(np.uint8) == 0xC3).all() and (canary_seq == 0xC3).all(), name
        assert host_call(c, canary, n, canary_seq, n_seq, None) == (0, n, n_seq, NONE) and io.as_tuples(canary) == want, name
        assert canary_seq.tobytes() == want_seq, name
    with pytest.raises(bam.BamPileupError):  # the sizing call makes every check
        Dev(lc.refusals()[0]).call()


def test_results_do_not_depend_on_the_tile(corpus):
    """a contig cut at arbitrary places gives the events of the whole, the region index aside: an event belongs to the piece that
    holds its SHIFTED anchor, wherever the raw one lay"""
    T = bam.PILEUP_TILE
    for name, ref, ln in (("a deletion that lands two tiles in front of its raw anchor", 1, 3 * T),
                          ("everything, region shapes, against a random text", 0, lc.CONTIGS[0][2])):
        c = next(t[0] for t in corpus if t[0]["name"] == name)
        cuts = [0, 1, 49, 50, T - 7, T - 1, T, T + 1, 2 * T - 3, 2 * T - 1, 2 * T + 100, ln]
        one, one_seq, _ = left_dev(dict(c, regions=[(ref, 0, ln)]))
        got, got_seq, event_off = left_dev(dict(c, regions=[(ref, a, b) for a, b in zip(cuts, cuts[1:])]))
        assert len(one) >= 1 and [e[:2] + e[3:] for e in got] == [e[:2] + e[3:] for e in one] and got_seq == one_seq, name
        assert [e[2] for e in got] == [next(k for k in range(len(cuts) - 1) if cuts[k] <= e[1] < cuts[k + 1]) for e in got], name
        assert event_off[-1] == len(one) and event_off == sorted(event_off), name

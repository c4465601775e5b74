"""bg_bam_indels[_dev] on the GPU against tests/bam_indels_oracle.py, record for record and byte for byte, and with the depth
taken from what bg_bam_pileup_dev returns for the same inputs (a second derivation, through code that is not under test): the
corpus of tests/bam_indels_cases.py — the pileup's corpus, anchors at T - 1 and T, a deletion that reaches into the next tile,
regions one behind an anchor and of the anchor alone, insertions of 1, 15, 16, 17 and 33 bases that differ in one base, at both
parities, every dropped operation, 66 000 records with one insertion each — in the device and the host flavour.  Events,
sequences and offsets are pre-filled and lie between guard bytes; once more with d_recs at every residue 0 .. 15 and d_seq at
odd addresses.  Sizing, each capacity one short and every refusal leave everything untouched; a call repeated gives the same
bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import bam_indels_cases as ic
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
    return [(c,) + ic.want_of(c) for c in ic.corpus()]


class Dev:
    """a case's arguments in HBM; the records at residue r_in"""

    def __init__(self, c, r_in=0):
        slots = c["slots"]
        self.c, self.n, self.n_contigs, self.n_regions = c, len(slots), len(c["contigs"]), len(c["regions"])
        self.recs = shifted_from(b"".join(slots) or b"\0", r_in)
        self.off = on_device(bo.offsets(slots))
        self.contigs = on_device(sam.Contigs(c["contigs"]).table)
        self.regions = on_device(bam.pileup_regions(c["regions"]))

    def head(self):
        return (self.n, self.recs.data_ptr() if self.n else 0, self.off.data_ptr() if self.n else 0, self.contigs.data_ptr() if self.n_contigs else 0,
                self.n_contigs, self.regions.data_ptr() if self.n_regions else 0, self.n_regions)

    def call(self, d_events=0, cap=0, d_seq=0, seq_cap=0, d_event_off=0):
        return bam.indels_dev(*self.head(), d_events, cap, d_seq, seq_cap, d_event_off, stream=stream(), **self.c["params"])

    def rows16(self):
        """what bg_bam_pileup_dev gives for the same records, regions and filters: (rows, row_off)"""
        p = self.c["params"]
        kw = dict(flags=bam.PILEUP_STRANDS, require=p["require"], exclude=p["exclude"], min_mapq=p["min_mapq"], min_baseq=p["min_baseq"], stream=stream())
        n = bam.pileup_dev(*self.head(), **kw)
        d_rows = torch.zeros(max(n, 1) * 16, dtype=torch.int32, device="cuda")
        d_row_off = torch.zeros(self.n_regions + 1, dtype=torch.int64, device="cuda")
        assert bam.pileup_dev(*self.head(), d_rows.data_ptr(), n, d_row_off.data_ptr(), **kw) == n
        torch.cuda.synchronize()
        return d_rows.cpu().numpy().view(np.uint32).reshape(-1, 16)[:n], d_row_off.cpu().numpy().tolist()


def indels_dev(c, r_in=0, r_seq=0, raw=False):
    """the device flavour between guards: (events, seq, event_off) as the oracle writes them; raw: the bytes of all three"""
    d = Dev(c, r_in)
    n, n_seq = d.call()  # the sizing call
    d_events = shifted(40 * (n + SLACK), 8 * (r_in % 2), fill=FILL)
    d_seq = shifted(n_seq + SLACK, r_seq, fill=FILL)
    d_event_off = shifted(8 * (d.n_regions + 1), 8, fill=FILL)
    assert d.call(d_events.data_ptr(), n + SLACK, d_seq.data_ptr(), n_seq + SLACK, d_event_off.data_ptr()) == (n, n_seq)
    assert guards_intact(d_events) and guards_intact(d_seq) and guards_intact(d_event_off) and guards_intact(d.recs)
    got, got_seq = d_events.cpu().numpy(), d_seq.cpu().numpy()
    assert (got[40 * n:] == FILL).all() and (got_seq[n_seq:] == FILL).all()  # nothing behind the totals
    if raw:
        return got.tobytes(), got_seq.tobytes(), d_event_off.cpu().numpy().tobytes()
    return io.as_tuples(got[:40 * n].view(EVENT)), got_seq[:n_seq].tobytes(), d_event_off.cpu().numpy().view(np.uint64).tolist()


def indels_host(c):
    slots = c["slots"]
    events, seq, event_off = bam.indels_arrays(b"".join(slots), bo.offsets(slots), sam.Contigs(c["contigs"]), c["regions"], **c["params"])
    assert not events["reserved"].any()
    return io.as_tuples(events), seq.tobytes(), event_off.tolist()


def test_the_corpus_in_the_device_flavour(corpus):
    for c, want, want_seq, want_off in corpus:
        assert indels_dev(c) == (want, want_seq, want_off), c["name"]


def test_the_depths_are_what_the_pileups_rows_give(corpus):
    for c, want, want_seq, want_off in corpus:
        rows, row_off = Dev(c).rows16()
        assert io.from_rows(c["slots"], rows, row_off, c["regions"], **c["params"]) == (want, want_seq, want_off), c["name"]


def test_the_host_flavour_gives_the_device_flavours_events(corpus):
    for c, want, want_seq, want_off in corpus:
        assert indels_host(c) == (want, want_seq, want_off), c["name"]


def test_the_deep_pile_is_one_event_and_strings_come_back(corpus):
    by = {c["name"]: (c, want, seq) for c, want, seq, _ in corpus}
    c, want, want_seq = by["66 000 records with one insertion each"]
    got, seq, _ = indels_dev(c)
    assert got == want and len(got) == 2 and got[0][5:8] == (66_000, 44_000, 22_000) and seq == b"GTGT"
    c, want, want_seq = by["insertions that differ in the last base or in base 17"]
    slots = c["slots"]
    events, seq, _ = bam.indels_arrays(b"".join(slots), bo.offsets(slots), sam.Contigs(c["contigs"]), c["regions"], **c["params"])
    strings = bam.indel_sequences(events, seq)
    assert strings == io.strings(want, want_seq) and {len(s) for s in strings} == {1, 15, 16, 17, 33}
    first = [s for e, s in zip(want, strings) if e[2] == 0]
    assert len(first) == len(set(first)) == 11  # every variant its own event, however late the difference


def test_records_at_every_residue_and_sequences_at_odd_addresses(corpus):
    by = {c["name"]: (c, want, seq, off) for c, want, seq, off in corpus}
    for name in ("insertions that differ in the last base or in base 17", "N, = and every code inside an insertion"):
        c, *want = by[name]
        for r in range(16):
            assert list(indels_dev(c, r_in=r, r_seq=(2 * r + 1) % 16)) == want, (name, r)
    for name in ("dropped operations, shared anchors, rows of I and of D", "everything, region shapes"):
        c, *want = by[name]
        for r_seq in (1, 7, 15):
            assert list(indels_dev(c, r_in=(3 * r_seq) % 16, r_seq=r_seq)) == want, (name, r_seq)


def test_a_call_repeated_gives_identical_bytes_and_offsets_may_be_absent(corpus):
    c, want, want_seq, want_off = next(t for t in corpus if t[0]["name"] == "everything, region shapes")
    first = indels_dev(c, raw=True)
    assert indels_dev(c, raw=True) == first
    d, n, n_seq = Dev(c), len(want), len(want_seq)
    side = torch.cuda.Stream()
    for k in range(2):
        d_events = torch.full((40 * n,), FILL, dtype=torch.uint8, device="cuda")
        d_seq = torch.full((max(n_seq, 1),), FILL, dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(side if k else torch.cuda.current_stream()):
            assert bam.indels_dev(*d.head(), d_events.data_ptr(), n, d_seq.data_ptr(), n_seq, 0, stream=torch.cuda.current_stream().cuda_stream,
                                  **c["params"]) == (n, n_seq)
        torch.cuda.synchronize()
        assert d_events.cpu().numpy().tobytes() == first[0][:40 * n] and d_seq.cpu().numpy()[:n_seq].tobytes() == want_seq, k


def host_call(c, events, cap, seq, seq_cap, event_off):
    slots = c["slots"]
    body = np.frombuffer(b"".join(slots) or b"\0", dtype=np.uint8)
    off, table, reg, prm = bo.offsets(slots), sam.Contigs(c["contigs"]).table, bam.pileup_regions(c["regions"]), bam.indels_params(**c["params"])
    total, n_seq, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    rc = _lib.lib().bg_bam_indels(_lib.default_context().h, prm.ctypes.data, len(slots), body.ctypes.data, off.ctypes.data, table.ctypes.data if len(table) else None,
                                  len(table), reg.ctypes.data if len(reg) else None, len(reg), ptr(events), cap, ptr(seq), seq_cap, ptr(event_off),
                                  C.byref(total), C.byref(n_seq), C.byref(bad))
    return rc, total.value, n_seq.value, bad.value


def test_refusals_leave_everything_untouched():
    for c in ic.refusals():
        name, (status, slot) = c["name"], c["want"]
        d = Dev(c)
        d_events, d_seq, d_event_off = shifted(4000, 8, fill=0xC3), shifted(333, 5, fill=0xC3), shifted(8 * (d.n_regions + 1), 8, fill=0xC3)
        for args in ((0, 0, 0, 0, 0), (d_events.data_ptr(), 100, d_seq.data_ptr(), 333, d_event_off.data_ptr())):
            with pytest.raises(bam.BamPileupError) as e:
                d.call(*args)
            assert (e.value.status, e.value.slot) == (status, slot), name
        for buf in (d_events, d_seq, d_event_off):
            assert guards_intact(buf) and (buf.cpu().numpy() == 0xC3).all(), name
        canary, canary_seq = np.full(100 * 40, 0xC3, dtype=np.uint8).view(EVENT), np.full(64, 0xC3, dtype=np.uint8)
        canary_off = np.full(d.n_regions + 1, 0xC3, dtype=np.uint64)
        first = NONE if slot is None else slot
        assert host_call(c, canary, 100, canary_seq, 64, canary_off) == (status, 0, 0, first), name
        assert host_call(c, None, 0, None, 0, None) == (status, 0, 0, first), name
        assert (canary.view(np.uint8) == 0xC3).all() and (canary_seq == 0xC3).all() and (canary_off == 0xC3).all(), name
        with pytest.raises(bam.BamPileupError) as e:
            indels_host(c)
        assert (e.value.status, e.value.slot) == (status, slot), name


def test_sizing_and_each_capacity_one_short(corpus):
    by = {c["name"]: (c, want, seq) for c, want, seq, _ in corpus}
    for name in ("every op kind", "everything, region shapes", "everything, 1 000 regions of 1 .. 3 positions",
                 "insertions that differ in the last base or in base 17"):
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
        Dev(ic.refusals()[0]).call()
    with pytest.raises(bam.BamPileupError):
        Dev(dict(by["every op kind"][0], params=io.params(min_alt_permille=1001))).call()


def test_2_32_positions_are_too_large():
    big = ic.pc.contigs_of([2**31 - 1], [b"big"])
    whole = (0, 0, 2**31 - 1)
    c = dict(slots=[], contigs=big, regions=[whole, whole, (0, 5, 7)], params=io.params())
    with pytest.raises(_lib.BiogpuError) as e:
        Dev(c).call()
    assert e.value.status == io.TOO_LARGE and not isinstance(e.value, bam.BamPileupError)


def test_results_do_not_depend_on_the_tile(corpus):
    """a contig cut at arbitrary places gives the events of the whole, the region index aside"""
    c, want, want_seq, _ = next(t for t in corpus if t[0]["name"] == "everything, region shapes")
    T = bam.PILEUP_TILE
    cuts = [0, 1, T - 7, T - 1, T, T + 1, 2 * T - 3, 2 * T - 1, 2 * T + 100, 3 * T + 5, ic.CONTIGS[0][2]]
    whole = dict(c, regions=[(0, 0, ic.CONTIGS[0][2])])
    pieces = dict(c, regions=[(0, a, b) for a, b in zip(cuts, cuts[1:])])
    one, one_seq, _ = indels_dev(whole)
    got, got_seq, event_off = indels_dev(pieces)
    assert len(one) > 20 and [e[:2] + e[3:] for e in got] == [e[:2] + e[3:] for e in one] and got_seq == one_seq
    assert [e[2] for e in got] == [next(k for k in range(len(cuts) - 1) if cuts[k] <= e[1] < cuts[k + 1]) for e in got]
    assert event_off[-1] == len(one) and event_off == sorted(event_off)


def test_the_call_may_be_ended_behind_a_pass_for_timing(corpus):
    """indels_stop_after (A/B: the timing tool tells the passes apart with it) ends the call with no event and nothing written;
    the next call without it is whole again"""
    c, want, want_seq, want_off = next(t for t in corpus if t[0]["name"] == "everything, region shapes")
    ctx = _lib.default_context()
    d, n, n_seq = Dev(c), len(want), len(want_seq)
    d_events, d_seq = shifted(40 * n, 0, fill=0xC3), shifted(n_seq, 1, fill=0xC3)
    try:
        for stop in (1, 2, 3):
            ctx.set_option("indels_stop_after", stop)
            assert d.call() == (0, 0) and d.call(d_events.data_ptr(), n, d_seq.data_ptr(), n_seq) == (0, 0), stop
            assert (d_events.cpu().numpy() == 0xC3).all() and (d_seq.cpu().numpy() == 0xC3).all(), stop
        with pytest.raises(_lib.BiogpuError):
            ctx.set_option("indels_stop_after", 4)
    finally:
        ctx.set_option("indels_stop_after", 0)
    assert indels_dev(c) == (want, want_seq, want_off)

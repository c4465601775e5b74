"""bg_vcf_emit[_dev] on the GPU against tests/vcf_oracle.py, byte for byte: the corpus of tests/vcf_cases.py — digit boundaries of
POS and the counters, contig names of 1, 15, 16, 17 and 255 bytes, every kind at one position, runs of 300 elements of one list
between two of the other, regions in any order, bytes that fold, deletions at a contig's end, around the stage size and of
70 000 bases, insertions of 1 .. 33 bases — in the device and the host flavour.  The output and the line offsets are
pre-filled and lie between guard bytes, with SLACK bytes behind the totals that must stay as they were; once more with d_out
at every residue 0 .. 15 and d_text, d_seq and d_names at odd addresses.  Sizing, a capacity one short and every refusal leave
everything untouched; a call repeated gives the same bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import vcf_cases as vc
import vcf_oracle as vo
from dev_shift import guards_intact, shifted, shifted_from
from rust_bio_amd import _lib, sam, vcf

pytestmark = pytest.mark.gpu
NONE = 2**64 - 1
FILL = 0xA5
SLACK = 19  # bytes behind the text, and 8-byte words behind the offsets, that must stay as they were


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def corpus():
    """[(case, text, line_off)]: the oracle once for every case"""
    return [(c,) + vc.want_of(c) for c in vc.corpus()]


class Dev:
    """a case's arguments in HBM: the sites at a 4-byte, the events at an 8-byte address, text, bases and names at residue r"""

    def __init__(self, c, r=0):
        table, names = vc.contig_arrays(c["contigs"])
        self.c, self.ns, self.ne, self.n_seq, self.n_contigs, self.n_text = c, len(c["sites"]), len(c["events"]), len(c["seq"]), len(table), c["n_text"]
        held = lambda data, residue: shifted_from(data, residue) if len(data) else shifted(16, residue)  # noqa: E731 (an empty list: never read)
        self.sites = held(c["sites"], 4 * (r % 4))
        self.events = held(c["events"], 8 * (r % 2))
        self.seq = held(c["seq"], r)
        self.contigs = held(table, 0)
        self.names = held(names, (r + 2) % 16 if r else 0)
        self.text = held(c["text"][:c["n_text"]], (3 * r) % 16)
        self.inputs = (self.sites, self.events, self.seq, self.contigs, self.names, self.text)

    def call(self, d_out=0, cap=0, d_line_off=0):
        ptr = lambda buf, n: buf.data_ptr() if n else 0  # noqa: E731
        return vcf.emit_dev(self.ns, ptr(self.sites, self.ns), self.ne, ptr(self.events, self.ne), ptr(self.seq, self.n_seq), self.n_seq,
                            ptr(self.contigs, self.n_contigs), self.n_contigs, ptr(self.names, self.n_contigs), ptr(self.text, self.n_text), self.n_text,
                            d_out, cap, d_line_off, stream=stream())


def emit_dev(c, r_out=0, r=0, raw=False):
    """the device flavour between guards: (text, line_off) as the oracle gives them; raw: every byte of both buffers"""
    d = Dev(c, r)
    n_lines, total = d.call()  # the sizing call
    d_out = shifted(total + SLACK, r_out, fill=FILL)
    d_line_off = shifted(8 * (n_lines + 1 + SLACK), 8 * (r_out % 2), fill=FILL)
    assert d.call(d_out.data_ptr(), total + (r_out % 3), d_line_off.data_ptr()) == (n_lines, total)
    assert guards_intact(d_out) and guards_intact(d_line_off) and all(guards_intact(b) for b in d.inputs)
    got, got_off = d_out.cpu().numpy(), d_line_off.cpu().numpy()
    assert (got[total:] == FILL).all() and (got_off[8 * (n_lines + 1):] == FILL).all()  # nothing behind the totals
    if raw:
        return got.tobytes(), got_off.tobytes()
    return got[:total].tobytes(), got_off[:8 * (n_lines + 1)].view(np.uint64).tolist()


def emit_host(c):
    text, line_off = vcf.emit_arrays(c["sites"], c["events"], c["seq"], sam.Contigs(c["contigs"]), c["text"][:c["n_text"]])
    return text, line_off.tolist()


def test_the_corpus_in_the_device_flavour(corpus):
    for c, want, want_off in corpus:
        assert emit_dev(c) == (want, want_off), c["name"]


def test_the_host_flavour_gives_the_same_bytes(corpus):
    for c, want, want_off in corpus:
        assert emit_host(c) == (want, want_off), c["name"]


def test_the_output_at_every_residue_and_the_inputs_at_odd_addresses(corpus):
    by = {c["name"]: (c, want, off) for c, want, off in corpus}
    for name in ("contig names of 1, 15, 16, 17 and 255 bytes", "deletions whose line is one under, at and one over the stage size",
                 "inserted bytes =, N, M and more; insertions of 1, 15, 16, 17 and 33 bases", "three SNV alleles, a DEL and two INS at one position"):
        c, *want = by[name]
        for r in range(16):
            assert list(emit_dev(c, r_out=r, r=(2 * r + 1) % 16)) == want, (name, r)
    for name in ("a deletion of 70 000 bases, one more that ends on the contig's last base", "a run of 300 events between two sites"):
        c, *want = by[name]
        for r in (1, 7, 15):
            assert list(emit_dev(c, r_out=r, r=(r + 4) % 16 + 1 - (r + 4) % 2)) == want, (name, r)


def test_a_call_repeated_gives_identical_bytes_and_offsets_may_be_absent(corpus):
    c, want, want_off = next(t for t in corpus if t[0]["name"].startswith("regions that overlap"))
    first = emit_dev(c, raw=True)
    assert emit_dev(c, raw=True) == first
    d, side = Dev(c), torch.cuda.Stream()
    for k in range(2):
        d_out = torch.full((len(want),), FILL, dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(side if k else torch.cuda.current_stream()):
            assert d.call(d_out.data_ptr(), len(want)) == (len(want_off) - 1, len(want))
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == want, k


def test_sizing_and_a_capacity_one_short(corpus):
    by = {c["name"]: (c, want, off) for c, want, off in corpus}
    for name in ("three SNV alleles, a DEL and two INS at one position", "a run of 300 sites between two events",
                 "a deletion of 70 000 bases, one more that ends on the contig's last base"):
        c, want, want_off = by[name]
        d, n, total = Dev(c), len(want_off) - 1, len(want)
        assert d.call() == (n, total)
        d_out, d_line_off = shifted(total, 5, fill=0xC3), shifted(8 * (n + 1), 8, fill=0xC3)
        for cap in (total - 1, 1, 0):
            with pytest.raises(_lib.BiogpuError) as e:
                d.call(d_out.data_ptr(), cap, d_line_off.data_ptr())
            assert e.value.status == vo.OPS_CAP and not isinstance(e.value, vcf.VcfError) and e.value.totals == (n, total), (name, cap)
            for buf in (d_out, d_line_off):
                assert guards_intact(buf) and (buf.cpu().numpy() == 0xC3).all(), (name, cap)
        canary, canary_off = np.full(total, 0xC3, dtype=np.uint8), np.full(n + 1, 0xC3C3C3C3C3C3C3C3, dtype=np.uint64)
        assert host_call(c, canary, total - 1, canary_off) == (vo.OPS_CAP, n, total, NONE), name
        assert (canary == 0xC3).all() and (canary_off.view(np.uint8) == 0xC3).all(), name
        assert host_call(c, None, 0, canary_off) == (0, n, total, NONE) and (canary_off.view(np.uint8) == 0xC3).all(), name  # sizing writes no offset
        assert host_call(c, canary, total, canary_off) == (0, n, total, NONE) and canary.tobytes() == want and canary_off.tolist() == want_off, name


def host_call(c, out, cap, line_off):
    table, names = vc.contig_arrays(c["contigs"])
    names = np.frombuffer(names + b"\0", dtype=np.uint8)
    text, seq = np.frombuffer(c["text"][:c["n_text"]] + b"\0", dtype=np.uint8), np.frombuffer(c["seq"] + b"\0", dtype=np.uint8)
    prm = vcf.params()
    n_lines, total, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    ptr = lambda a, n=1: a.ctypes.data if a is not None and n else None  # noqa: E731
    rc = _lib.lib().bg_vcf_emit(_lib.default_context().h, prm.ctypes.data, ptr(c["sites"], len(c["sites"])), len(c["sites"]), ptr(c["events"], len(c["events"])),
                                len(c["events"]), ptr(seq, len(c["seq"])), len(c["seq"]), ptr(table, len(table)), len(table), ptr(names, len(table)),
                                ptr(text, c["n_text"]), c["n_text"], ptr(out), cap, ptr(line_off), C.byref(n_lines), C.byref(total), C.byref(bad))
    return rc, n_lines.value, total.value, bad.value


def test_empty_lists_and_the_nulls_that_go_with_them():
    assert vcf.emit_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, stream=stream()) == (0, 0)
    d_out, d_line_off = shifted(32, 3, fill=0xC3), shifted(16, 8, fill=0xC3)
    assert vcf.emit_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, d_out.data_ptr(), 32, d_line_off.data_ptr(), stream=stream()) == (0, 0)
    assert (d_out.cpu().numpy() == 0xC3).all() and d_line_off.cpu().numpy().view(np.uint64).tolist() == [0, 0xC3C3C3C3C3C3C3C3]
    text, line_off = vcf.emit_arrays(np.zeros(0, vc.SITE), np.zeros(0, vc.EVENT), b"", sam.Contigs([]), b"")
    assert text == b"" and line_off.tolist() == [0]
    c = vc.base_case()
    d = Dev(c)
    args = [d.ns, d.sites.data_ptr(), d.ne, d.events.data_ptr(), d.seq.data_ptr(), d.n_seq, d.contigs.data_ptr(), d.n_contigs, d.names.data_ptr(), d.text.data_ptr(),
            d.n_text]
    for null in (1, 3, 4, 6, 8, 9):  # a null array with a count
        with pytest.raises(vcf.VcfError) as e:
            vcf.emit_dev(*[0 if k == null else v for k, v in enumerate(args)], stream=stream())
        assert e.value.status == vo.INVALID_ARG and e.value.first_bad is None, null
    for shift, null in ((2, 1), (4, 3)):  # sites off 4 bytes, events off 8
        with pytest.raises(vcf.VcfError):
            vcf.emit_dev(*[v + shift if k == null else v for k, v in enumerate(args)], stream=stream())
    with pytest.raises(vcf.VcfError):  # a null out with a capacity
        vcf.emit_dev(*args, 0, 10, stream=stream())
    n = [C.c_uint64(0) for _ in range(3)]
    for prm in (np.array([(1, 0)], dtype=_lib.VCF_PARAMS_DTYPE), np.array([(0, 1)], dtype=_lib.VCF_PARAMS_DTYPE)):
        assert _lib.lib().bg_vcf_emit_dev(_lib.default_context().h, prm.ctypes.data, *args, None, 0, None, C.byref(n[0]), C.byref(n[1]), C.byref(n[2]),
                                          stream()) == vo.INVALID_ARG


def test_refusals_name_the_smallest_index_and_leave_everything_untouched():
    for c in vc.refusals():
        d = Dev(c)
        d_out, d_line_off = shifted(4000, 5, fill=0xC3), shifted(8 * 40, 8, fill=0xC3)
        for args in ((0, 0, 0), (d_out.data_ptr(), 4000, d_line_off.data_ptr())):
            with pytest.raises(vcf.VcfError) as e:
                d.call(*args)
            assert (e.value.status, e.value.first_bad) == (vo.INVALID_ARG, c["want"]), c["name"]
        for buf in (d_out, d_line_off):
            assert guards_intact(buf) and (buf.cpu().numpy() == 0xC3).all(), c["name"]
    for c in vc.refusals()[::5]:
        canary, canary_off = np.full(4000, 0xC3, dtype=np.uint8), np.full(40, 0xC3C3C3C3C3C3C3C3, dtype=np.uint64)
        assert host_call(c, canary, 4000, canary_off) == (vo.INVALID_ARG, 0, 0, c["want"]), c["name"]
        assert (canary == 0xC3).all() and (canary_off.view(np.uint8) == 0xC3).all(), c["name"]
        with pytest.raises(vcf.VcfError) as e:
            emit_host(c)
        assert e.value.first_bad == c["want"], c["name"]

"""K7 (csrc/fmd_smems.hip: FMDIndex::smems / all_smems, fmindex.rs:363-501) where its state machine and its limits can go wrong,
against the CPU oracle, exactly: the six fields of every record and every read's count.  The corpus is tests/fmd_cases.py;
tests/test_oracle_fmd_edges.py holds it to the properties it claims.  What this file reaches that the random-read tests do not:
a quad's second and third read (more reads than the launch has quad slots), reads kept in LDS next to reads read in place
(248 / 249 symbols), the three extension flavours on one index, every panic of the reference as count 0xFFFFFFFF beside clean
reads, size-0 records, the '$' step, reads at the 65 534-symbol limit, caps, sizing calls and refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fmd_cases as fc
import oracle_py as orc
from rust_bio_amd import _lib
from rust_bio_amd.bwt import Occ
from rust_bio_amd.fmindex import FMDIndex, FMIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, INVALID_ARG, OUT_OF_ALPHABET, TOO_LARGE, OPS_CAP, UNSUPPORTED = 0, -1, -7, -8, -9, -11
CASES = fc.cases()
TEXTS = sorted({c["name"].split("/")[0] for c in CASES})
FLAVOURS = ["u64_k3", "u32_k3", "wide_k3", "u64_k1", "u64_k64"]


@functools.lru_cache(maxsize=None)
def tables(fwd, alphabet):
    text = fc.full_text(fwd)
    sa = orc.suffix_array(text)
    b = np.frombuffer(bytes(orc.bwt(text, sa)), np.uint8)
    ls = np.asarray(orc.less(b, alphabet), np.uint64)
    return b, ls, orc.FMDIndex(b, ls, orc.Occ(b, 3, alphabet))


@functools.lru_cache(maxsize=None)
def wide_ctx():
    ctx = _lib.Context(0)  # the 64-bit layout forced onto small texts, as in tests/test_gpu_fm_wide.py
    ctx.set_option("fm_wide_from", 1)
    ctx.set_option("fm_wide_sb_shift", 2)
    return ctx


def device_index(fwd, alphabet, flavour="u64_k3"):
    b, ls, _ = tables(fwd, alphabet)
    kind, k = flavour.split("_k")
    fm = FMIndex(b, ls, Occ(b, int(k), alphabet), ctx=wide_ctx() if kind == "wide" else None)
    return fm, FMDIndex(fm, records32=kind == "u32")


@functools.lru_cache(maxsize=None)
def expected(name):
    case = next(c for c in CASES if c["name"] == name)
    _, _, ofmd = tables(case["text"], case["alphabet"])
    buf, off = fc.concat(case["reads"])
    return (buf, off) + fc.oracle_batch(orc, ofmd, buf, off, case["positions"], case["min_len"])


def same(cnt, out, want_cnt, want_flat, what):
    """counts (0xFFFFFFFF where the oracle raises) and every record of every read: nothing is left out"""
    bad = np.nonzero(cnt != want_cnt)[0]
    assert len(bad) == 0, (what, "count of read", int(bad[0]), int(cnt[bad[0]]), int(want_cnt[bad[0]]), len(bad))
    got = out[fc.valid_mask(cnt, out.shape[1])].astype(np.uint64)
    assert got.shape == want_flat.shape, what
    bad = np.nonzero((got != want_flat).any(axis=1))[0]
    assert len(bad) == 0, (what, "record", int(bad[0]), got[bad[0]].tolist(), want_flat[bad[0]].tolist(), len(bad))


def run_case(fmd, case, cap=None):
    buf, off, want_cnt, want_flat = expected(case["name"])
    if cap is None:
        cap = max(1, int(np.where(want_cnt == fc.PANIC, 0, want_cnt).max()))
    cnt, out = fmd.smems_arrays(buf, off, case["positions"], case["min_len"], all_=case["positions"] is None, cap=cap, keep_panics=True)
    return cnt, out, want_cnt, want_flat


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("text", TEXTS)
def test_corpus_equals_the_oracle(text, flavour):
    """every case of the corpus on a host-built index: uint64 and uint32 records, the forced 64-bit layout, Occ sampling rates
    1, 3 and 64"""
    mine = [c for c in CASES if c["name"].split("/")[0] == text]
    if flavour.startswith("wide") and not mine[0]["wide"]:
        # N in rank bit vectors: the 64-bit layout keeps none and says so when it is built — there is no such index to ask
        with pytest.raises(_lib.BiogpuError) as e:
            device_index(mine[0]["text"], mine[0]["alphabet"], flavour)
        assert e.value.status == UNSUPPORTED
        return
    fm, fmd = device_index(mine[0]["text"], mine[0]["alphabet"], flavour)
    for case in mine:
        cnt, out, want_cnt, want_flat = run_case(fmd, case)
        same(cnt, out, want_cnt, want_flat, case["name"])
        assert len(cnt) == len(case["reads"])
    fm.close()


def is_plain(t):
    return t["alphabet"] == fc.ALPHA and all(c in b"ACGT$" for c in set(t["text"]))


@pytest.mark.parametrize("text", [k for k, t in fc.texts().items() if is_plain(t)])
def test_the_three_extension_flavours_agree(text, monkeypatch):
    """a plain index (ACGT and '$' alone in the BWT) through the flavour the host picks for it, through the plain one that ranks
    '$' in its list (BG_K7_PLAIN1) and through the general one (BG_K7_GENERAL): identical arrays, equal to the oracle"""
    mine = [c for c in CASES if c["name"].split("/")[0] == text]
    fm, fmd = device_index(mine[0]["text"], mine[0]["alphabet"])
    for case in mine:
        got = {}
        for env in (None, "BG_K7_PLAIN1", "BG_K7_GENERAL"):
            monkeypatch.delenv("BG_K7_PLAIN1", raising=False)
            monkeypatch.delenv("BG_K7_GENERAL", raising=False)
            if env:
                monkeypatch.setenv(env, "1")
            cnt, out, want_cnt, want_flat = run_case(fmd, case)
            same(cnt, out, want_cnt, want_flat, (case["name"], env))
            keep = fc.valid_mask(cnt, out.shape[1])
            got[env] = (cnt, out[keep])
        for env in ("BG_K7_PLAIN1", "BG_K7_GENERAL"):
            assert (got[env][0] == got[None][0]).all() and np.array_equal(got[env][1], got[None][1]), (case["name"], env)
    fm.close()


def test_every_quad_walks_a_second_read_and_some_a_third():
    """300 000 reads in one call: the launch has at most 256 CUs x 8 blocks x 64 quads = 131 072 quad slots, so the edge
    PH_FINISH -> q += n_slots -> PH_LOAD runs on every quad, with everything it has to reset — the panic flag (panicking and clean
    reads alternate on a slot), the record count, the lists' roles, the look-ahead entry, and the read's bytes in LDS or in place
    (1 % of the reads are 249 - 400 symbols long).  all_smems, then smems with empty reads and i >= len; all reads compared."""
    bb = fc.big_batch()
    n = len(bb["off"]) - 1
    b, ls, ofmd = tables(bb["text"], bb["alphabet"])
    fm, fmd = device_index(bb["text"], bb["alphabet"], "u32_k64")
    for pos, min_len in ((None, 0), (bb["positions"], 5)):
        want_cnt, want_flat = fc.oracle_batch(orc, ofmd, bb["buf"], bb["off"], pos, min_len)
        cap = int(np.where(want_cnt == fc.PANIC, 0, want_cnt).max())
        cnt, out = fmd.smems_arrays(bb["buf"], bb["off"], pos, min_len, all_=pos is None, cap=cap, keep_panics=True)
        assert len(cnt) == n == 300_000
        panics = int((want_cnt == fc.PANIC).sum())
        assert panics >= (1500 if pos is None else 3000)
        same(cnt, out, want_cnt, want_flat, "all_smems" if pos is None else "smems")
    fm.close()


def clean_case():
    """the reads of random/all the reference does not panic on, and their oracle answer"""
    case = next(c for c in CASES if c["name"] == "random/all")
    _, _, want_cnt, _ = expected(case["name"])
    reads = [r for r, c in zip(case["reads"], want_cnt) if c != fc.PANIC]
    _, _, ofmd = tables(case["text"], case["alphabet"])
    buf, off = fc.concat(reads)
    cnt, flat = fc.oracle_batch(orc, ofmd, buf, off, None, 0)
    return case, buf, off, cnt, flat


def first_records(cnt, flat, cap):
    """the oracle's first `cap` records of every read"""
    start = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))[:-1]])
    rank = np.arange(len(flat)) - np.repeat(start, cnt.astype(np.int64))
    return flat[rank < cap]


def test_cap_below_the_count_truncates_and_says_so():
    case, buf, off, want_cnt, want_flat = clean_case()
    n, cap, guard, mark = len(off) - 1, 3, 4096, 0xA5A5A5A5A5A5A5A5
    assert (want_cnt > cap).sum() > 10 and (want_cnt < cap).sum() > 10
    fm, fmd = device_index(case["text"], case["alphabet"])
    L = _lib.lib()
    # host buffers: the status, the true counts, the first `cap` records, nothing behind the buffer's n * cap records
    cnt = np.zeros(n, np.uint32)
    out = np.full(n * cap * 6 + guard, mark, np.uint64)
    rc = L.bg_fmd_smems_batch64(fm.h, 1, n, buf.ctypes.data, off.ctypes.data, None, 0, cap, cnt.ctypes.data, out.ctypes.data)
    assert rc == OPS_CAP
    assert (cnt == want_cnt).all()
    recs = out[:n * cap * 6].reshape(n, cap, 6)
    assert np.array_equal(recs[fc.valid_mask(np.minimum(cnt, cap), cap)], first_records(want_cnt, want_flat, cap))
    assert (out[n * cap * 6:] == mark).all()
    # device buffers: every slot the kernel has no record for keeps what was there, and so does the guard behind the last read
    d_pat, d_off = torch.from_numpy(buf.copy()).to(DEV), torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_cnt = torch.zeros(n, dtype=torch.int32, device=DEV)
    d_out = torch.full((n * cap * 6 + guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    rc = L.bg_fmd_smems_batch64_dev(fm.h, 1, n, d_pat.data_ptr(), d_off.data_ptr(), None, 0, int(np.diff(off).max()), cap,
                                    d_cnt.data_ptr(), d_out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == OK
    assert (d_cnt.cpu().numpy().view(np.uint32) == want_cnt).all()
    o = d_out.cpu().numpy().view(np.uint64)
    recs, keep = o[:n * cap * 6].reshape(n, cap, 6), fc.valid_mask(np.minimum(want_cnt, cap), cap)
    assert np.array_equal(recs[keep], first_records(want_cnt, want_flat, cap))
    assert (recs[~keep] == 0x5A5A5A5A5A5A5A5A).all() and (o[n * cap * 6:] == 0x5A5A5A5A5A5A5A5A).all()
    # cap == 0 with no output buffer: a sizing call, the counts alone (and the status that says they exceed the cap)
    cnt0 = np.full(n, 7, np.uint32)
    rc = L.bg_fmd_smems_batch64(fm.h, 1, n, buf.ctypes.data, off.ctypes.data, None, 0, 0, cnt0.ctypes.data, None)
    assert rc == OPS_CAP and (cnt0 == want_cnt).all()
    cnt0[:] = 7
    rc = L.bg_fmd_smems_batch(fm.h, 1, n, buf.ctypes.data, off.ctypes.data, None, 0, 0, cnt0.ctypes.data, None)
    assert rc == OPS_CAP and (cnt0 == want_cnt).all()
    fm.close()


def test_refusals():
    t, too_long = fc.refused_read()
    fm, fmd = device_index(t["text"], t["alphabet"])
    L = _lib.lib()
    # a read of 65 535 symbols: the host entry points refuse the call
    buf, off = fc.concat([too_long])
    cnt = np.full(1, 7, np.uint32)
    out = np.zeros(6 * 4, np.uint64)
    for all_ in (1, 0):
        ip = np.zeros(1, np.uint32)
        assert L.bg_fmd_smems_batch64(fm.h, all_, 1, buf.ctypes.data, off.ctypes.data, ip.ctypes.data, 20, 4, cnt.ctypes.data, out.ctypes.data) == TOO_LARGE
        assert L.bg_fmd_smems_batch(fm.h, all_, 1, buf.ctypes.data, off.ctypes.data, ip.ctypes.data, 20, 4, cnt.ctypes.data, out.ctypes.data) == TOO_LARGE
    with pytest.raises(_lib.BiogpuError) as e:
        fmd.all_smems(too_long, 20)
    assert e.value.status == TOO_LARGE
    # ... and the device entry points on max_pattern_len alone, the count buffer left as it was
    d_pat, d_off = torch.from_numpy(buf.copy()).to(DEV), torch.from_numpy(off.astype(np.int64)).to(DEV)
    d_cnt = torch.full((1,), 0x7777, dtype=torch.int32, device=DEV)
    d_out = torch.zeros(6 * 4, dtype=torch.int64, device=DEV)
    for fn in (L.bg_fmd_smems_batch64_dev, L.bg_fmd_smems_batch_dev):
        assert fn(fm.h, 1, 1, d_pat.data_ptr(), d_off.data_ptr(), None, 20, 65_535, 4, d_cnt.data_ptr(), d_out.data_ptr(), None) == TOO_LARGE
        torch.cuda.synchronize()
        assert int(d_cnt.cpu()[0]) == 0x7777
    # no patterns: accepted, whatever the other pointers are
    assert L.bg_fmd_smems_batch64(fm.h, 1, 0, None, None, None, 0, 4, None, None) == OK
    assert L.bg_fmd_smems_batch(fm.h, 0, 0, None, None, None, 0, 4, None, None) == OK
    assert L.bg_fmd_smems_batch64_dev(fm.h, 1, 0, None, None, None, 0, 100, 4, None, None, None) == OK
    assert L.bg_fmd_smems_batch_dev(fm.h, 0, 0, None, None, None, 0, 100, 4, None, None, None) == OK
    # the null pointers the entry points check
    one, ooff = fc.concat([b"ACGTACGT"])
    ip = np.zeros(1, np.uint32)
    out, d_out = np.zeros(6 * 8, np.uint64), torch.zeros(6 * 8, dtype=torch.int64, device=DEV)  # (at most one record per base)
    p, o, i, c, r = one.ctypes.data, ooff.ctypes.data, ip.ctypes.data, cnt.ctypes.data, out.ctypes.data
    for fn in (L.bg_fmd_smems_batch64, L.bg_fmd_smems_batch):
        assert fn(None, 1, 1, p, o, i, 0, 8, c, r) == INVALID_ARG
        assert fn(fm.h, 1, 1, p, None, i, 0, 8, c, r) == INVALID_ARG
        assert fn(fm.h, 1, 1, p, o, i, 0, 8, None, r) == INVALID_ARG
        assert fn(fm.h, 1, 1, p, o, i, 0, 8, c, None) == INVALID_ARG
        assert fn(fm.h, 0, 1, p, o, None, 0, 8, c, r) == INVALID_ARG
        assert fn(fm.h, 1, 1, p, o, None, 0, 8, c, r) == OK  # (all_smems needs no positions)
    d_one, d_ooff = torch.from_numpy(one.copy()).to(DEV), torch.from_numpy(ooff.astype(np.int64)).to(DEV)
    d_ip = torch.zeros(1, dtype=torch.int32, device=DEV)
    p, o, i, c, r = d_one.data_ptr(), d_ooff.data_ptr(), d_ip.data_ptr(), d_cnt.data_ptr(), d_out.data_ptr()
    for fn in (L.bg_fmd_smems_batch64_dev, L.bg_fmd_smems_batch_dev):
        assert fn(None, 1, 1, p, o, i, 0, 8, 8, c, r, None) == INVALID_ARG
        assert fn(fm.h, 1, 1, p, None, i, 0, 8, 8, c, r, None) == INVALID_ARG
        assert fn(fm.h, 1, 1, p, o, i, 0, 8, 8, None, r, None) == INVALID_ARG
        assert fn(fm.h, 1, 1, p, o, i, 0, 8, 8, c, None, None) == INVALID_ARG
        assert fn(fm.h, 0, 1, p, o, None, 0, 8, 8, c, r, None) == INVALID_ARG
    torch.cuda.synchronize()
    fm.close()


@pytest.mark.parametrize("name", ["five_sequences/smems", "few_n/all"])
def test_device_entry_point_on_a_stream_of_its_own(name):
    """bg_fmd_smems_batch64_dev on torch tensors and a non-default stream: the host-buffer call's arrays"""
    case = next(c for c in CASES if c["name"] == name)
    fm, fmd = device_index(case["text"], case["alphabet"])
    cnt, out, want_cnt, want_flat = run_case(fmd, case)
    same(cnt, out, want_cnt, want_flat, name)
    buf, off = fc.concat(case["reads"])
    n, cap = len(off) - 1, out.shape[1]
    st = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(st):
        d_pat, d_off = torch.from_numpy(buf.copy()).to(DEV), torch.from_numpy(off.astype(np.int64)).to(DEV)
        d_ip = None if case["positions"] is None else torch.tensor(case["positions"], dtype=torch.int32, device=DEV)
        d_cnt = torch.zeros(n, dtype=torch.int32, device=DEV)
        d_out = torch.zeros(n * cap * 6, dtype=torch.int64, device=DEV)
        rc = _lib.lib().bg_fmd_smems_batch64_dev(fm.h, 1 if d_ip is None else 0, n, d_pat.data_ptr(), d_off.data_ptr(),
                                                 None if d_ip is None else d_ip.data_ptr(), case["min_len"], int(np.diff(off).max()),
                                                 cap, d_cnt.data_ptr(), d_out.data_ptr(), C.c_void_p(st.cuda_stream))
        assert rc == OK
    st.synchronize()
    dc = d_cnt.cpu().numpy().view(np.uint32)
    do = d_out.cpu().numpy().view(np.uint64).reshape(n, cap, 6)
    keep = fc.valid_mask(cnt, cap)
    assert (dc == cnt).all() and np.array_equal(do[keep], out[keep])
    fm.close()

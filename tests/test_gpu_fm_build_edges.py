"""The FM index builder (csrc/fm_build.hip: one device builder behind bg_fm_build and bg_fm_build_dev, for the 32-bit and
the 64-bit layout) where it can go wrong: text lengths either side of a 2-bit block (192 symbols), a bit-vector block (480),
their common multiple (960) and a superblock (768 with fm_wide_sb_shift = 2); alphabets with fewer than four letters, with
exactly as many symbols beyond the top four as the exception list holds (1024) and one more, with several dense symbols; a
caller's `less` that is not the BWT's own; and the order of bg_fm_build's errors.  Texts are real (random letters + '$',
host suffix array / BWT / less); every index built through both entry points is compared with the oracle's
backward_search over a few hundred short patterns and with the suffix array through a rate-4 sampled one."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_py as orc
from rust_bio_amd import _lib, pack2
from rust_bio_amd.bwt import Occ, bwt, less
from rust_bio_amd.fmindex import FMIndex
from rust_bio_amd.suffix_array import SampledSuffixArray, suffix_array

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DNA = b"ACGTNacgtn"
PROTEIN = bytes(sorted(b"ARNDCQEGHILKMFPSTWYV"))
INVALID_ARG, OUT_OF_ALPHABET, UNSUPPORTED = -1, -7, -11
NARROW_N = [1, 2, 191, 192, 193, 479, 480, 481, 960, 961]  # kSymPerBlock, kBvBits and their lcm
WIDE_N = NARROW_N + [767, 768, 769]                        # + a superblock of 4 blocks


def make_ctx(layout):
    ctx = _lib.Context(0)
    if layout == "wide":
        ctx.set_option("fm_wide_from", 1)
        ctx.set_option("fm_wide_sb_shift", 2)
    return ctx


def random_text(n, letters, seed, weights=None):
    """n symbols, the sentinel included"""
    rng = np.random.default_rng(seed)
    al = np.frombuffer(letters, dtype=np.uint8)
    p = None if weights is None else np.asarray(weights, dtype=float) / np.sum(weights)
    return np.append(al[rng.choice(len(al), size=n - 1, p=p)], np.uint8(ord("$")))


def short_patterns(t, letters, seed, n_q=300):
    """1-8 symbols: half of them substrings of the text, half random over `letters`; plus the empty pattern and '$'"""
    rng = np.random.default_rng(seed)
    al = np.frombuffer(letters, dtype=np.uint8)
    body = t[:-1]
    pats = [b"", b"$"]
    for _ in range(n_q):
        L = int(rng.integers(1, 9))
        if rng.random() < 0.5 and len(body) >= L:
            s = int(rng.integers(0, len(body) - L + 1))
            pats.append(body[s:s + L].tobytes())
        else:
            pats.append(al[rng.integers(0, len(al), size=L)].tobytes())
    return _lib.concat(pats)


def oracle_search(b, ls, alphabet, pat, off):
    otag, olo, ohi, oml = orc.backward_search_batch(b, ls, orc.Occ(b, 3, alphabet), pat, off, threads=2)
    assert not (otag == 3).any()  # (checked on the CPU: none of the chosen patterns panics)
    return otag, olo, ohi, oml


def build_both(b, ls, alphabet, layout):
    """(name, index) through bg_fm_build with `ls` and through bg_fm_build_dev, which derives its own"""
    ctx = make_ctx(layout)
    yield "bg_fm_build", FMIndex(b, ls, Occ(b, 3, alphabet), ctx=ctx)
    dev = FMIndex.from_device(torch.from_numpy(np.array(b)).to(DEV), 3, alphabet, ctx=ctx)
    assert (dev._less == less(b, alphabet)).all()
    yield "bg_fm_build_dev", dev


def check_index(fm, want, pat, off, sa=None, t=None, b=None):
    tag, lo, hi, ml = fm.backward_search_arrays(pat, off)
    otag, olo, ohi, oml = want
    assert (tag == otag).all() and (lo == olo).all() and (hi == ohi).all() and (ml.astype(np.uint64) == oml).all()
    if sa is not None:
        SampledSuffixArray(sa, t, b, 4, fmindex=fm)
        rows = np.arange(len(sa), dtype=np.uint64)
        assert (fm.interval_occ_arrays(rows, rows + np.uint64(1))[1] == sa).all()


def check_text(t, alphabet, letters, layout, seed=1):
    """both entry points on one text against the oracle and the suffix array; yields each handle for further checks and
    compares what the two report as their sizes"""
    sa = suffix_array(t)
    b = bwt(t, sa)
    ls = less(b, alphabet)
    pat, off = short_patterns(t, letters, seed)
    want = oracle_search(b, ls, alphabet, pat, off)
    sizes = []
    for name, fm in build_both(b, ls, alphabet, layout):
        assert len(fm) == len(t), name
        check_index(fm, want, pat, off, sa, t, b)
        sizes.append((fm.device_bytes(), fm.step2_bytes()))
        yield name, fm, b, ls, (pat, off, want)
        fm.close()
    assert sizes[0] == sizes[1]


@pytest.mark.parametrize("layout,n", [("narrow", n) for n in NARROW_N] + [("wide", n) for n in WIDE_N])
def test_lengths_at_the_block_boundaries(layout, n):
    t = random_text(n, b"ACGT", seed=n)
    for _ in check_text(t, DNA, b"ACGT", layout, seed=n + 1):
        pass


@pytest.mark.parametrize("layout", ["narrow", "wide"])
@pytest.mark.parametrize("letters", [b"A", b"AC", b"ACG"])
def test_fewer_than_four_letters(layout, letters):
    """'$' takes a 2-bit code of its own next to the letters: with one or two letters n_codes < 4 (no packed patterns, no
    2-step blocks); with three the four codes are '$' and the letters"""
    t = random_text(700, letters, seed=len(letters))
    for name, fm, b, ls, _ in check_text(t, DNA, letters + b"T", layout):
        codes = (C.c_uint8 * 4)()
        rc = _lib.lib().bg_fm_pattern_codes(fm.h, codes)
        if len(letters) < 3:
            assert rc == UNSUPPORTED and fm.step2_bytes() == 0, name
        else:
            assert rc == 0 and sorted(bytes(codes)) == sorted(b"$" + letters), name


def dna_with_n(beyond4):
    """ACGT with N: `beyond4` BWT symbols beyond the four most frequent (beyond4 - 1 N and the sentinel)"""
    t = random_text(6000, b"ACGT", seed=beyond4)
    t[np.random.default_rng(beyond4).choice(5999, size=beyond4 - 1, replace=False)] = ord("N")
    assert np.sort(np.bincount(t, minlength=256))[:-4].sum() == beyond4
    return t


def packed_search_equals(fm, ctx, pat, off, want):
    """the patterns made of the index's four coded letters, as one 2-bit stream"""
    codes = fm.pattern_codes()
    pats = [pat[int(a):int(e)].tobytes() for a, e in zip(off[:-1], off[1:])]
    keep = [q for q, p in enumerate(pats) if p and all(c in codes for c in p)]
    assert len(keep) > 50
    cbuf, coff = _lib.concat([pats[q] for q in keep])
    d_pat, d_off = torch.from_numpy(cbuf.copy()).to(DEV), torch.from_numpy(coff.astype(np.int64)).to(DEV)
    pk, bad = pack2.pack_dev(d_pat, codes=codes, ctx=ctx)
    assert bad == 0
    nq = len(keep)
    d_tag = torch.full((nq,), 9, dtype=torch.uint8, device=DEV)
    d_lo, d_hi = torch.zeros(nq, dtype=torch.int64, device=DEV), torch.zeros(nq, dtype=torch.int64, device=DEV)
    d_ml = torch.zeros(nq, dtype=torch.int32, device=DEV)
    fm.backward_search_packed_dev(nq, pk.data_ptr(), d_off.data_ptr(), d_tag.data_ptr(), d_lo.data_ptr(), d_hi.data_ptr(), d_ml.data_ptr())
    torch.cuda.synchronize()
    otag, olo, ohi, oml = (w[keep] for w in want)
    assert (d_tag.cpu().numpy() == otag).all() and (d_lo.cpu().numpy().astype(np.uint64) == olo).all()
    assert (d_hi.cpu().numpy().astype(np.uint64) == ohi).all() and (d_ml.cpu().numpy().astype(np.uint64) == oml).all()


@pytest.mark.parametrize("layout", ["narrow", "wide"])
def test_exactly_as_many_exceptions_as_the_list_holds(layout):
    """1024 symbols beyond the top four: still sorted lists, no dense symbols (packed patterns are accepted)"""
    t = dna_with_n(1024)
    for name, fm, b, ls, (pat, off, want) in check_text(t, DNA, b"ACGTN", layout):
        assert sorted(fm.pattern_codes()) == sorted(b"ACGT"), name
        packed_search_equals(fm, fm.ctx, pat, off, want)


def test_one_exception_more_gets_dense_symbols_on_the_narrow_layout():
    t = dna_with_n(1025)
    for name, fm, b, ls, _ in check_text(t, DNA, b"ACGTN", "narrow"):
        codes = (C.c_uint8 * 4)()
        assert _lib.lib().bg_fm_pattern_codes(fm.h, codes) == UNSUPPORTED, name
        assert fm.step2_bytes() == 0, name


def raw_build(ctx, b, ls, less_len, k, alphabet):
    b, al = _lib.as_u8(b), _lib.as_u8(alphabet)
    h = C.c_void_p()
    rc = _lib.lib().bg_fm_build(ctx.h, b.ctypes.data, len(b), None if ls is None else ls.ctypes.data, less_len, k,
                                al.ctypes.data, len(al), C.byref(h))
    assert (rc == 0) == bool(h)
    if h:
        _lib.lib().bg_fm_free(h)
    return rc


def raw_build_dev(ctx, b, k, alphabet):
    d_b, al = torch.from_numpy(np.array(b)).to(DEV), _lib.as_u8(alphabet)
    h = C.c_void_p()
    rc = _lib.lib().bg_fm_build_dev(ctx.h, d_b.data_ptr(), d_b.numel(), k, al.ctypes.data, len(al), None, C.byref(h), 0)
    assert (rc == 0) == bool(h)
    if h:
        _lib.lib().bg_fm_free(h)
    return rc


@pytest.mark.parametrize("kind", ["dna_n_1025", "protein"])
def test_dense_symbols_are_refused_on_the_wide_layout(kind):
    t, alphabet = (dna_with_n(1025), DNA) if kind == "dna_n_1025" else (random_text(2000, PROTEIN, seed=20), PROTEIN)
    b = bwt(t, suffix_array(t))
    ls = less(b, alphabet)
    ctx = make_ctx("wide")
    assert raw_build(ctx, b, ls, len(ls), 3, alphabet) == UNSUPPORTED
    assert raw_build_dev(ctx, b, 3, alphabet) == UNSUPPORTED


def test_twenty_letters_with_several_dense_symbols():
    t = random_text(2000, PROTEIN, seed=20)
    hist = np.sort(np.bincount(t, minlength=256))[::-1]
    # the rarest symbols stay lists while they sum to at most 1024; what is left beyond the three coded ones is dense
    n_sparse = int((np.cumsum(hist[hist > 0][::-1]) <= 1024).sum())
    assert int((hist > 0).sum()) - 3 - n_sparse >= 3
    for _ in check_text(t, PROTEIN, PROTEIN, "narrow"):
        pass


@pytest.mark.parametrize("layout", ["narrow", "wide"])
def test_a_less_that_is_not_the_bwts_own_keeps_single_steps(layout):
    """The entry of the largest occurring symbol (T) lowered to the entry of the occurring symbol before it (G: the entry
    right before T's, less['S'], equals T's own — no 'S' occurs): T's rows then land in G's, every interval stays inside
    [0, n), and the index must reproduce the reference's arithmetic on that less — through single steps, since 2-step rank
    blocks lean on LF."""
    t = random_text(1500, b"ACGT", seed=77)
    n = len(t)
    b = bwt(t, suffix_array(t))
    own = less(b, DNA)
    bent = own.copy()
    bent[ord("T")] = own[ord("G")]
    assert bent[ord("T")] < own[ord("T")]
    pat, off = short_patterns(t, b"ACGT", seed=78)
    want = oracle_search(b, bent, DNA, pat, off)
    found = want[0] != 2
    assert (want[2][found] <= n).all() and (want[1][found] < want[2][found]).all()
    assert (want[1] != oracle_search(b, own, DNA, pat, off)[1]).any()  # (the bent entry matters to these patterns)
    ctx = make_ctx(layout)
    fm = FMIndex(b, bent, Occ(b, 3, DNA), ctx=ctx)
    assert fm.step2_bytes() == 0
    check_index(fm, want, pat, off)
    fm.close()
    fm = FMIndex(b, own, Occ(b, 3, DNA), ctx=ctx)
    assert fm.step2_bytes() > 0
    check_index(fm, oracle_search(b, own, DNA, pat, off), pat, off)
    fm.close()


@pytest.mark.parametrize("layout", ["narrow", "wide"])
def test_bg_fm_build_error_order(layout):
    ctx = make_ctx(layout)
    t = random_text(500, b"ACGT", seed=5)
    b = bwt(t, suffix_array(t))
    ls = np.zeros(300, dtype=np.uint64)
    ls[:86] = less(b, b"ACGT")
    assert raw_build(ctx, b, ls, 86, 3, b"ACGT") == 0
    assert raw_build(ctx, b, None, 86, 3, b"ACGT") == INVALID_ARG
    assert raw_build(ctx, b, ls, 86, 0, b"ACGT") == INVALID_ARG
    foreign = b.copy()
    foreign[250] = ord("a")  # beyond max_symbol = 'T'
    for bw in (b, foreign):
        assert raw_build(ctx, bw, ls, 85, 3, b"ACGT") == INVALID_ARG
        assert raw_build(ctx, bw, ls, 87, 3, b"ACGT") == INVALID_ARG
    assert raw_build(ctx, foreign, ls, 86, 3, b"ACGT") == OUT_OF_ALPHABET
    assert raw_build_dev(ctx, foreign, 3, b"ACGT") == OUT_OF_ALPHABET

"""One SHA-256 per case over what an FM index answers, for comparing two builds of the library bit by bit:
python tools/exp/fm_build_identity.py <lib.so>
Cases: DNA 1 M, DNA with 5 % N 1 M, protein 300 k, IUPAC 800 k and the 22-symbol KAT text x bg_fm_build / bg_fm_build_dev x the
narrow layout / the 64-bit one forced (fm_wide_from = 1; a text that needs dense symbols prints the refusal) x the BWT's own
`less` / one that is not (bg_fm_build only: the entry of the largest occurring symbol lowered to that of the occurring symbol
before it, so every interval stays inside [0, n)).  Hashed per case: tags, lowers, uppers and matched lengths of 20 000
patterns and, with the BWT's own `less`, the located positions of 5 000 rows through a rate-4 sampled suffix array; printed next
to it: device_bytes, step2_bytes, pattern_codes."""
import ctypes as C, hashlib, os, sys
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
import numpy as np
import torch
torch.cuda.init()
from rust_bio_amd import _lib
_lib.SO_PATH = os.path.abspath(sys.argv[1])
from rust_bio_amd import synth
from rust_bio_amd.bwt import Occ, less
from rust_bio_amd.fmindex import FMIndex
from rust_bio_amd.suffix_array import SampledSuffixArray, bwt_dev, suffix_array_dev

DEV = "cuda:0"
DNA = b"ACGTNacgtn"
PROTEIN = b"ARNDCQEGHILKMFPSTWYV"
IUPAC = b"ACGTRYSWKMBDHVNacgtryswkmbdhvn"


def with_sentinel(letters, n, seed, p=None):
    rng = np.random.default_rng(seed)
    al = np.frombuffer(letters, dtype=np.uint8)
    return np.append(al[rng.choice(len(al), size=n, p=None if p is None else np.asarray(p) / np.sum(p))], np.uint8(ord("$")))


def texts():
    yield "dna_1m", synth.genome(1_000_000, 5), DNA, b"ACGT"
    g = synth.genome(1_000_000, 6).copy()
    rng = np.random.default_rng(6)
    g[:-1][rng.random(len(g) - 1) < 0.025] = ord("N")
    for s in rng.integers(0, len(g) - 600, size=50):
        g[s:s + 500] = ord("N")
    yield "dna_n_1m", g, DNA, b"ACGTN"
    yield "protein_300k", with_sentinel(PROTEIN, 300_000, 7), bytes(sorted(PROTEIN)), PROTEIN
    yield "iupac_800k", with_sentinel(IUPAC, 800_000, 8, [20.0] * 4 + [1.0] * 11 + [2.0] * 4 + [0.0005] * 11), IUPAC, IUPAC[:19]
    yield "kat_22", np.frombuffer(b"GCCTTAACATTATTACGCCTA$", dtype=np.uint8), DNA, b"ACGT"


def patterns(t, letters, n_q, seed):
    rng = np.random.default_rng(seed)
    al = np.frombuffer(letters, dtype=np.uint8)
    plen = 12 if len(t) > 100 else 3
    starts = rng.integers(0, len(t) - 1 - plen, size=n_q)
    pats = t[starts[:, None] + np.arange(plen)[None, :]].copy()
    mut = rng.random(n_q) < 0.3
    cols = rng.integers(0, plen, size=n_q)
    pats[mut, cols[mut]] = al[rng.integers(0, len(al), size=int(mut.sum()))]
    return np.ascontiguousarray(pats.reshape(-1)), np.arange(n_q + 1, dtype=np.uint64) * np.uint64(plen)


def report(name, fm, pat, off, locate):
    h = hashlib.sha256()
    for a in fm.backward_search_arrays(pat, off):
        h.update(np.ascontiguousarray(a).tobytes())
    if locate is not None:
        sa, t, b = locate
        SampledSuffixArray(sa, t, b, 4, fmindex=fm)
        rows = np.random.default_rng(3).integers(0, len(sa), size=min(5000, len(sa))).astype(np.uint64)
        h.update(fm.interval_occ_arrays(rows, rows + np.uint64(1))[1].tobytes())
    cb = (C.c_uint8 * 4)()
    rc = _lib.lib().bg_fm_pattern_codes(fm.h, cb)
    print("%-44s %s device_bytes=%d step2_bytes=%d pattern_codes=%s" % (name, h.hexdigest(), fm.device_bytes(), fm.step2_bytes(),
                                                                     bytes(cb).decode() if rc == 0 else rc), flush=True)
    fm.close()


for tname, t, alpha, letters in texts():
    d_t = torch.from_numpy(np.array(t)).to(DEV)
    d_sa = suffix_array_dev(d_t)
    d_b = bwt_dev(d_t, d_sa)
    sa, b = d_sa.cpu().numpy().astype(np.uint64), d_b.cpu().numpy()
    own = less(b, alpha)
    bent = own.copy()
    occurring = np.nonzero(np.bincount(b, minlength=256))[0]
    bent[occurring[-1]] = own[occurring[-2]]
    pat, off = patterns(t, letters, 20_000, 9)
    for layout in ("narrow", "wide"):
        ctx = _lib.Context(0)
        if layout == "wide":
            ctx.set_option("fm_wide_from", 1)
        for entry, ls in (("build", own), ("build", bent), ("build_dev", own)):
            name = "%s %s %s %s" % (tname, layout, entry, "own" if ls is own else "bent")
            try:
                fm = FMIndex(b, ls, Occ(b, 64, alpha), ctx=ctx) if entry == "build" else FMIndex.from_device(d_b, 64, alpha, ctx=ctx)
            except _lib.BiogpuError as e:
                print("%-44s refused: %d" % (name, e.status), flush=True)
                continue
            report(name, fm, pat, off, (sa, t, b) if ls is own else None)

"""The corpus of the FMD SMEM edge tests (K7: csrc/fmd_smems.hip), for tests/test_gpu_fmd_edges.py and its CPU companion
tests/test_oracle_fmd_edges.py, which holds every case to the properties it claims.  numpy only: no torch, no device library.

A case: name, text (the forward strand; `full_text` appends '$', the reverse complement and '$'), alphabet, reads, positions
(None: all_smems; else one per read: smems), min_len, claims (what the oracle must show on it, see CLAIMS) and wide (False
where the 64-bit layout has no such index: it keeps no rank bit vectors).  Everything is seeded.

The texts stay under 60 kb so that the host builders stay fast, with one exception: the reads at the engine's length limit
(65 534 symbols) need a text they occur in, `limit` has 66 000 bases."""
import numpy as np

ALPHA = b"ACGTNacgtn"  # dna::n_alphabet(); '$' is tabulated by itself
COMP = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")
PANIC = 0xFFFFFFFF     # out_count of a read the reference panics on (include/biogpu.h)
MAX_LEN = 65_534       # the longest read the engine takes (msz << 16 | mlen in its list entries)

CLAIMS = {
    "size0": "a record whose interval has size 0",
    "dollar_step": "a record at pattern position 0 that only the '$' step emits (the extension by '$' is not empty)",
    "palindrome": "a record whose interval has lower == lower_rev",
    "many_records": "a read with at least 20 records",
    "long_forward": "a read whose forward pass changes interval size at 100 steps or more",
    "dedup": "a backward pass in which two neighbouring list entries extend to the same size (the second is dropped)",
    "mixed_block": "reads up to 248 symbols and longer ones in the same block of 64 reads",
    "panic_empty": "the empty pattern in smems mode panics",
    "panic_i": "i >= len panics",
    "panic_less": "a byte beyond `less` panics",
    "panic_class": "a symbol of the extension order outside the index's alphabet panics",
    "panic_underflow": "lower + size == 0 panics",
    "x_no_panic": "a read with X (outside the alphabet, below len(less)) does not panic",
    "empty_all": "the empty pattern in all_smems mode gives no records",
}


def revcomp(s):
    return s.translate(COMP)[::-1]


def full_text(fwd):
    return fwd + b"$" + revcomp(fwd) + b"$"


def random_dna(n, seed):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, size=n)].tobytes()


def other_base(c):
    return {65: 67, 67: 71, 71: 84, 84: 65}.get(c, 65)


def substituted(read, every, start=None):
    """a different base every `every` symbols"""
    r = bytearray(read)
    for p in range(every // 2 if start is None else start, len(r), every):
        r[p] = other_base(r[p])
    return bytes(r)


def with_byte(read, pos, byte):
    r = bytearray(read)
    r[pos] = byte
    return bytes(r)


# ---- texts
def texts():
    base = random_dna(20_000, 1)
    rng = np.random.default_rng(2)
    t = {}
    t["random"] = dict(text=base)
    g = bytearray(base)
    for p in rng.integers(0, len(g), size=8):
        g[int(p)] = ord("N")
    t["few_n"] = dict(text=bytes(g))
    g = bytearray(base)
    g[5_000:5_150] = bytes(g[5_000:5_150]).lower()
    for p in (100, 7_000, 7_001):
        g[p] = ord("N")
    t["soft_masked"] = dict(text=bytes(g))
    t["two_sequences"] = dict(text=base[:9_000] + b"$" + base[9_000:16_000])
    t["five_sequences"] = dict(text=b"$".join(base[s:s + 2_500 + 100 * k] for k, s in enumerate(range(0, 15_000, 3_000))))
    t["homopolymer"] = dict(text=base[:6_000] + b"A" * 300 + base[6_000:12_000])
    t["tandem"] = dict(text=base[:3_000] + b"AC" * 400 + base[3_000:6_000] + b"ACG" * 300 + base[6_000:9_000] + b"ACGTTGA" * 150 + base[9_000:12_000])
    seg = base[13_000:13_500]
    copies = b""
    for k in range(4):
        copies += base[1_000 * k:1_000 * k + 1_000] + with_byte(seg, 100 + 90 * k, other_base(seg[100 + 90 * k]))
    t["four_copies"] = dict(text=copies)
    x = base[:5_000]
    t["own_revcomp"] = dict(text=x + revcomp(x))
    # N in the dense classes (rank bit vectors), like text_with_n of tests/test_gpu_fm_alphabets.py: 5 % N, half of it isolated
    # bases, half in runs of 500
    g = np.frombuffer(random_dna(60_000, 3), np.uint8).copy()
    rn = np.random.default_rng(21)
    g[rn.random(len(g)) < 0.025] = ord("N")
    for s in rn.integers(0, len(g) - 600, size=3):
        g[int(s):int(s) + 500] = ord("N")
    t["dense_n"] = dict(text=g.tobytes(), wide=False)
    # an index over ACGT alone: N and the lower-case letters of the extension order are outside its alphabet
    t["acgt_alphabet"] = dict(text=random_dna(5_000, 4), alphabet=b"ACGT")
    t["limit"] = dict(text=random_dna(66_000, 5))
    for v in t.values():
        v.setdefault("alphabet", ALPHA)
        v.setdefault("wide", True)
    return t


# ---- read families
def cut(fwd, rng, length):
    """`length` symbols of one of the text's sequences (no '$'), where one is long enough; else of the text with '$' as A"""
    seqs = [(s, e) for s, e in sequences(fwd) if e - s >= length]
    if not seqs:
        return fwd.replace(b"$", b"A")[:length].ljust(length, b"C")
    s, e = seqs[int(rng.integers(0, len(seqs)))]
    a = int(rng.integers(s, e - length + 1))
    return fwd[a:a + length]


def sequences(fwd):
    out, s = [], 0
    for part in fwd.split(b"$"):
        out.append((s, s + len(part)))
        s += len(part) + 1
    return out


def family_lengths(fwd, rng):
    """(a) lengths around the 248 symbols a quad keeps in LDS, and far beyond: exact, with substitutions, reverse complemented"""
    reads = []
    for rep in range(3):
        for length in (1, 2, 247, 248, 249, 250, 1_000, 2_000):
            r = cut(fwd, rng, length)
            if rep == 1:
                r = substituted(r, 47)
            if rep == 2:
                r = revcomp(substituted(r, 301, start=length - 1))  # (the last base: the revcomp's first)
            reads.append(r)
    return reads


def family_ends(fwd):
    """(c) prefixes and suffixes of the text and of every '$'-separated sequence, on both strands"""
    reads = []
    for s, e in sequences(fwd)[:5]:
        for r in (fwd[s:s + 30], fwd[e - 30:e], fwd[s:s + 1], fwd[e - 1:e], fwd[s:s + 260], fwd[e - 260:e]):
            reads += [r, revcomp(r)]
    return reads


def family_repeats(fwd, rng):
    """(d) homopolymers longer than any run, periodic reads with one phase break, reverse-palindromic reads"""
    reads = [b"A" * 400, b"T" * 40, b"A" * 250, b"AC" * 150, b"AC" * 30 + b"C" + b"AC" * 30, b"ACG" * 50 + b"CG" + b"ACG" * 40,
             b"ACGTTGA" * 20 + b"CGTTGA" + b"ACGTTGA" * 12, b"GT" * 200, b"ACGT", b"AATT", b"GAATTC", b"AT", b"CG" * 6]
    for length in (12, 40):
        s = cut(fwd, rng, length)
        reads.append(s + revcomp(s))
    return reads


def family_absent(fwd, rng):
    """(e) reads with no occurrence, reads whose first symbol does not occur in the text (N, n), or lies below '$' (#)"""
    r = cut(fwd, rng, 40)
    return [random_dna(40, 900), random_dna(300, 901), b"N" + r, b"n" + r, b"N", b"NN", b"a", b"#" + r, b"#", b"\x00" + r, r + b"#"]


def family_foreign(fwd, rng):
    """(f) N, lower case, X (outside the alphabet, below len(less)), 0xFF and z (above it), '$': first, inside, last"""
    reads = []
    for byte in (ord("N"), ord("a"), ord("t"), ord("g"), ord("c"), ord("n"), ord("X"), 0xFF, ord("z"), ord("$"), ord("Y"), ord("R")):
        r = cut(fwd, rng, 60)
        reads += [with_byte(r, 0, byte), with_byte(r, 20, byte), with_byte(r, 59, byte)]
    r = cut(fwd, rng, 300)
    reads += [with_byte(r, 270, ord("X")), with_byte(r, 270, 0xFF), r.lower(), r[:100] + r[100:200].lower() + r[200:]]
    return reads


def common_reads(fwd, seed):
    rng = np.random.default_rng(seed)
    reads = family_lengths(fwd, rng) + family_ends(fwd) + family_repeats(fwd, rng) + family_absent(fwd, rng) + family_foreign(fwd, rng)
    reads += [b""]  # (i)
    order = rng.permutation(len(reads))
    return [reads[int(k)] for k in order]


def smems_positions(reads, seed):
    """(h) i at 0, at len - 1, inside — and at len for every 13th read (the reference indexes pattern[i]); at 0 where the first
    byte lies below '$' (its empty interval at row 0 is the lower + size == 0 panic)"""
    rng = np.random.default_rng(seed)
    pos = []
    for q, r in enumerate(reads):
        n = len(r)
        pick = q % 13
        pos.append(0 if n == 0 or pick < 4 or r[0] < ord("$") else n - 1 if pick < 7 else n if pick == 12 else int(rng.integers(0, n)))
    return pos


def cases():
    out = []
    tx = texts()
    common = {"size0", "dollar_step", "palindrome", "many_records", "mixed_block", "x_no_panic", "panic_less", "panic_underflow"}
    for k, (name, t) in enumerate(tx.items()):
        if name == "limit":
            continue
        reads = common_reads(t["text"], 50 + k)
        claims = set(common)
        if name == "acgt_alphabet":  # (nearly every extension passes N in the order: most reads panic)
            claims = {"panic_class", "panic_less"}
            reads += [b"GGCCGC", b"CCGG", b"G", b"C" * 30, b"GC" * 20]
        if name in ("homopolymer", "tandem"):
            claims |= {"long_forward"}
        base = dict(text=t["text"], alphabet=t["alphabet"], wide=t["wide"], reads=reads)
        out.append(dict(base, name=name + "/all", positions=None, min_len=0, claims=claims | ({"empty_all"} if name != "acgt_alphabet" else set())))
        out.append(dict(base, name=name + "/smems", positions=smems_positions(reads, 70 + k), min_len=0,
                        claims=(claims - {"many_records", "long_forward"}) | {"panic_empty", "panic_i"} | ({"dedup"} if name != "acgt_alphabet" else set())))
    # (g) one set of 60-base reads under min_len 0, 1, the reads' length and one more
    for name in ("random", "few_n", "two_sequences"):
        t = tx[name]
        rng = np.random.default_rng(91)
        reads = []
        for k in range(40):
            r = cut(t["text"], rng, 60)
            reads.append(r if k % 4 == 0 else substituted(r, 25) if k % 4 == 1 else revcomp(r) if k % 4 == 2 else with_byte(r, 30, ord("N")))
        reads += [random_dna(60, 77), b"N" + cut(t["text"], rng, 59)]
        for min_len in (0, 1, 60, 61):
            base = dict(text=t["text"], alphabet=t["alphabet"], wide=t["wide"], reads=reads, min_len=min_len, claims=set())
            out.append(dict(base, name="%s/all/min_len_%d" % (name, min_len), positions=None))
            out.append(dict(base, name="%s/smems/min_len_%d" % (name, min_len), positions=[(7 * q) % 60 for q in range(len(reads))]))
    # (b) reads at the limit, each a call of its own (the lists' scratch is per quad slot and grows with the longest read)
    t = tx["limit"]
    exact = t["text"][300:300 + MAX_LEN]
    base = dict(text=t["text"], alphabet=t["alphabet"], wide=t["wide"], min_len=20)
    out.append(dict(base, name="limit/exact/all", reads=[exact], positions=None, claims=set()))
    out.append(dict(base, name="limit/exact/smems_first", reads=[exact], positions=[0], claims=set()))
    out.append(dict(base, name="limit/exact/smems_last", reads=[exact], positions=[MAX_LEN - 1], claims=set()))
    out.append(dict(base, name="limit/substituted/all", reads=[substituted(exact, 50)], positions=None, claims={"many_records"}))
    out.append(dict(base, name="limit/substituted/smems", reads=[substituted(exact, 50)], positions=[MAX_LEN // 2], claims=set()))
    return out


def refused_read():
    """(b) a read of 65 535 bases: the engine refuses the call (BG_ERR_TOO_LARGE)"""
    t = texts()["limit"]
    return t, t["text"][100:100 + MAX_LEN + 1]


# ---- the large batch: more reads than the launch has quad slots
def big_batch(n=300_000, seed=5):
    """(text, reads as (buffer, offsets), smems positions): `n` reads of 12 - 40 bases cut from the read families on a 50 kb
    text with a homopolymer run, a tandem repeat and a repeated segment; about 1 % are 249 - 400 bases long; between 0.5 % and
    1 % hold a byte beyond `less` (0xFF, z) and panic; in the positions, a further 0.3 % have i >= len, and 0.3 % of the reads
    are empty (a panic in smems mode only).  Shuffled by construction: every kind is drawn per read."""
    rng = np.random.default_rng(seed)
    base = random_dna(50_000, 6)
    fwd = base[:20_000] + b"A" * 60 + base[20_000:30_000] + b"AC" * 50 + base[30_000:40_000] + base[1_000:1_400] + base[40_000:49_440]
    assert len(fwd) == 50_000
    t = np.frombuffer(fwd, np.uint8)
    comp = np.frombuffer(COMP, np.uint8)
    kind = rng.random(n)
    lens = rng.integers(12, 41, size=n)
    long_ = kind < 0.01
    lens[long_] = rng.integers(249, 401, size=int(long_.sum()))
    empty = (kind >= 0.01) & (kind < 0.013)
    lens[empty] = 0
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    starts = rng.integers(0, len(fwd) - 400, size=n)
    read_of = np.repeat(np.arange(n), lens)
    within = np.arange(int(off[-1])) - off[:-1].astype(np.int64)[read_of]
    buf = t[starts[read_of] + within].copy()
    # substitutions: 0 - 2 per read, at random places
    for _ in range(2):
        hit = (rng.random(n) < 0.4) & (lens > 0)
        at = off[:-1].astype(np.int64)[hit] + rng.integers(0, 1 << 30, size=int(hit.sum())) % lens[hit]
        buf[at] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=len(at))]
    # reverse complements (read by read: reverse the read's span, complement its bytes)
    rc = (rng.random(n) < 0.5)[read_of]
    mirror = off[:-1].astype(np.int64)[read_of] + lens[read_of] - 1 - within
    buf = np.where(rc, comp[buf[mirror]], buf)
    # foreign bytes that do not panic (N, X, lower case, '$'), and the ones that do
    mild = (rng.random(n) < 0.05) & (lens > 0)
    at = off[:-1].astype(np.int64)[mild] + rng.integers(0, 1 << 30, size=int(mild.sum())) % lens[mild]
    buf[at] = np.frombuffer(b"NXacgtn$", np.uint8)[rng.integers(0, 8, size=len(at))]
    bad = (rng.random(n) < 0.0075) & (lens > 0)
    at = off[:-1].astype(np.int64)[bad] + rng.integers(0, 1 << 30, size=int(bad.sum())) % lens[bad]
    buf[at] = np.frombuffer(b"\xffz", np.uint8)[rng.integers(0, 2, size=len(at))]
    # smems positions: inside the read; at len (or beyond) for 0.3 %
    pos = (rng.integers(0, 1 << 30, size=n) % np.maximum(lens, 1)).astype(np.uint32)
    beyond = rng.random(n) < 0.003
    pos[beyond] = (lens[beyond] + rng.integers(0, 3, size=int(beyond.sum()))).astype(np.uint32)
    return dict(text=fwd, alphabet=ALPHA, buf=np.ascontiguousarray(buf), off=off, positions=pos, bad=bad, empty=empty, beyond=beyond,
                long=long_)


# ---- the oracle on a batch (oracle_py.FMDIndex, one call per read)
def concat(reads):
    off = np.zeros(len(reads) + 1, np.uint64)
    if reads:
        off[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), np.uint8), off


def oracle_batch(orc, ofmd, buf, off, positions, min_len):
    """-> (counts: uint32, PANIC where the reference panics; records [sum of counts, 6] uint64 in read order).  positions None:
    all_smems.  Straight on the oracle's C entry point with one output buffer: a few microseconds per short read."""
    fn = orc.lib().orc_fmd_smems
    n = len(off) - 1
    counts = np.zeros(n, np.uint32)
    cap = 4 * int(np.diff(off).max() if n else 0) + 8
    out = np.zeros(6 * cap, np.uint64)
    keep = np.ascontiguousarray(buf, np.uint8)
    if len(keep) == 0:
        keep = np.zeros(1, np.uint8)
    p0, o, recs = keep.ctypes.data, out.ctypes.data, []
    bwt, less, occ = ofmd.bwt, ofmd.less, ofmd.occ.h
    for q in range(n):
        a, e = int(off[q]), int(off[q + 1])
        r = fn(bwt.ctypes.data, len(bwt), less.ctypes.data, len(less), occ, p0 + a, e - a,
               0 if positions is None else int(positions[q]), min_len, 1 if positions is None else 0, o, cap)
        if r < 0:
            counts[q] = PANIC
        else:
            assert r <= cap
            counts[q] = r
            if r:
                recs.append(out[:6 * r].copy())
    flat = np.concatenate(recs).reshape(-1, 6) if recs else np.zeros((0, 6), np.uint64)
    return counts, flat


def valid_mask(counts, cap):
    """[n, cap] bool: the record slots a count vector fills"""
    c = np.where(counts == PANIC, 0, counts).astype(np.int64)
    return np.arange(cap)[None, :] < c[:, None]

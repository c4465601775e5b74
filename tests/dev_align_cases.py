"""Inputs for tests/test_gpu_dev_pointer_alignment.py: the smallest batches at which the `_dev` entry points take the code
paths they choose from the ADDRESS of a caller's byte pointer (16-byte vector loads and stores, 8-byte header words, dword
stores, the head / body / tail split of a copy), and the residues mod 16 every pointer is put at.

Generators only: numpy and the other case files, nothing of the GPU, deterministic by seed.  tests/test_dev_align_cases.py
shows with the CPU oracles that every input holds what it is for and that the copies of the kernels' constants below still
equal the sources; the GPU module runs the inputs."""
import functools
import random

import numpy as np

import band_edge_cases as bec
import fmd_cases as fc

# ---- copies of the kernels' constants (compared with the sources by test_dev_align_cases.py) -----------------------------
FQ_TILE = 16384      # fastq_ingest.hip: kTile, the one-pass kernel's tile
FQ_HALO = 1024       # kHaloBytes, the bytes in front of a tile kept in LDS and the window of the search in front of it
FQ_CHUNK = 4096      # kChunk, the general kernels' chunk
FA_TILE = 8192       # fasta_ingest.hip: BG_FASTA_TILE
SAM_STAGE = 1040     # sam_emit.hip: kStageBuf, a line with (offset mod 16) + length up to this is staged in LDS
SAM_LONG_LINE = 16384  # sam_rule.h: a longer record goes to the block kernel of the sort's copy

# ---- residues (mod 16) ------------------------------------------------------------------------------------------------------
FQ_TEXT_RES, FQ_SEQ_RES, FQ_QUAL_RES = (1, 4, 8, 12, 15), (0, 5), (0, 11)
PACK_RES = tuple(range(16))
REF_OUT_RES, REF_IN_RES = (0, 1, 8, 15), (0, 3)
SW_SEQ_RES, SW_OPS_RES = (0, 1, 7), (0, 1, 2, 3)
BAND_RES = (0, 1, 9, 15)
SEED_READS_RES, SEED_OPS_RES, SEED_TEXT_RES = (0, 3, 8, 13), (0, 5), (0, 6)
SAM_OUT_RES, SAM_IN_RES = (0, 1, 15), (0, 7)
TEXT_RES = (0, 1, 15)  # revcomp and CIGAR: input and output
COL_RES = (0, 9)       # the FASTQ column calls: sequences, qualities, their outputs

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---- bg_fastq_parse_dev -------------------------------------------------------------------------------------------------------
SPACE_OFFSETS = tuple(range(18))  # id lengths: the header's first space 0 .. 17 bytes behind the '@' + 1


def fq_record(rng, k, n_bases, nl=b"\n", id_len=None):
    """a four-line record; id_len bytes of id, then a space and a description — id_len None: an id of 20 bytes and no space"""
    seq = _ACGT[rng.integers(0, 4, size=n_bases)].tobytes()
    qual = rng.integers(33, 75, size=n_bases).astype(np.uint8).tobytes()
    if id_len is None:
        hdr = b"@" + (b"nospace%013d" % k)
    else:
        hdr = b"@" + (b"%017d" % k)[17 - id_len:] + b" d%d" % k
    return hdr + nl + seq + nl + b"+" + nl + qual + nl


def fq_short_reads(nl=b"\n", total=int(3.2 * FQ_TILE), seed=1):
    """about 3.2 tiles of 150-base records; record k's id has k % 19 bytes (18: no space at all)"""
    rng = np.random.default_rng([201, seed])
    parts, size, k = [], 0, 0
    while size < total:
        parts.append(fq_record(rng, k, 150, nl, None if k % 19 == 18 else k % 19))
        size += len(parts[-1])
        k += 1
    return b"".join(parts), k


@functools.lru_cache(maxsize=None)
def fastq_texts():
    """name -> (text, records): four-line ASCII records, CRLF, no final newline, 20 KB lines, 9 - 14 KB lines, a non-ASCII byte"""
    out = {}
    lf, n = fq_short_reads()
    out["lf"] = (lf, n)
    out["crlf"] = fq_short_reads(b"\r\n", seed=2)
    out["no-final-newline"] = (lf[:-1], n)
    rng = np.random.default_rng([202])
    # lines longer than a tile: the search for the four newlines in front of a tile runs through all its windows and gives up
    # (a record of 40 KB begins too far in front of the tile it ends in): the general kernels take the text, their gather with
    # a wavefront per record; ids of 3 and 12 bytes: the first space in the first and in the second 8-byte word
    longs = [fq_record(rng, 0, 20_000, id_len=3), fq_record(rng, 1, 20_011, id_len=12)]
    tail = [fq_record(rng, 2 + k, 150, id_len=k % 18) for k in range(20)]
    out["long-lines"] = (b"".join(longs + tail), 22)
    # lines of 9 - 14 KB: such a record stays with the one-pass kernel (every tile finds its four newlines within the 31 windows),
    # and its header lies more than the halo in front of the tile it ends in: the header's words are read from memory
    mids = [fq_record(rng, 30 + k, n, id_len=None if k == 3 else (5 * k) % 18) for k, n in enumerate((9_000, 14_000, 12_001, 10_007, 13_500, 9_500))]
    mixed = [r for k, m in enumerate(mids) for r in (m, fq_record(rng, 40 + k, 150, id_len=(7 * k) % 18))]
    out["mid-lines"] = (b"".join(mixed), 12)
    # a byte >= 0x80 in the second tile: the one-pass kernel raises its flag and the general kernels take the whole text
    cut = lf.index(b"\n@", FQ_TILE + 2000) + 1
    out["non-ascii"] = (lf[:cut] + "@id é desc\nACGT\n+\nIIII\n".encode() + lf[cut:], n + 1)
    return out


FQ_WINDOWS = 31  # fastq_ingest.hip: kHaloWindows


def one_pass_finds_its_lines(text):
    """the one-pass kernel's search in front of every tile ends within its windows: the four newlines in front of the tile lie
    at most FQ_WINDOWS * FQ_HALO bytes back, or the search reaches the start of the text"""
    reach = FQ_WINDOWS * FQ_HALO
    for t0 in range(FQ_TILE, len(text), FQ_TILE):
        at, found = t0, 0
        while found < 4 and at > 0:
            at = text.rfind(b"\n", 0, at)
            if at < 0:
                break
            found += 1
        if (found == 4 and at < t0 - reach) or (found < 4 and t0 > reach):
            return False
    return True


def record_spans(text):
    """[(start, end)] of the four-line records of a text made by the generators above"""
    starts = [0]
    at, lines = 0, 0
    while True:
        nl = text.find(b"\n", at)
        if nl < 0:
            break
        at = nl + 1
        lines += 1
        if lines % 4 == 0 and at < len(text):
            starts.append(at)
    return list(zip(starts, starts[1:] + [len(text)]))


# ---- bg_pack2_dev / bg_unpack2_dev ------------------------------------------------------------------------------------------
PACK_N = (1, 15, 16, 17, 31, 32, 33, 4096 + 5)
INVALID = ord("N")


def pack_inputs(n):
    """[(name, bytes, number of invalid bytes)]: random ACGT that does not begin a word with 'A' (code 0: a dropped byte would
    not show), and the same with one 'N' in the first word, in the last whole word and in the tail (where n has them)"""
    rng = np.random.default_rng([203, n])
    base = _ACGT[rng.integers(0, 4, size=n)].copy()
    base[::16] = _ACGT[1 + rng.integers(0, 3, size=len(base[::16]))]
    out = [("valid", base.tobytes(), 0)]
    places = {"first-word": 0}
    if n >= 32:
        places["last-whole-word"] = 16 * (n // 16) - 1
    if n % 16 and n > 16:
        places["tail"] = n - 1
    for name, at in places.items():
        b = base.copy()
        b[at] = INVALID
        out.append((name, b.tobytes(), 1))
    return out


# ---- bg_align_batch_dev, bg_cigar_batch_dev ---------------------------------------------------------------------------------
SW_PAIRS, SW_M, SW_N = 37, 150, 160
SW_STRIDES = (2 * SW_N + 4, 2 * SW_N + 5)
SW_SCORES = dict(gap_open=-5, gap_extend=-1, match=1, mismatch=-1)


@functools.lru_cache(maxsize=None)
def sw_pairs():
    """37 pairs of 150 x 160 (a partial wavefront), x a mutated window of y or unrelated"""
    from test_gpu_pk16 import related_pairs  # (a generator that lives in a GPU module; importing it runs nothing)
    return related_pairs(np.random.default_rng(204), SW_PAIRS, lambda p: SW_M, lambda p: SW_N)


def dword_ok(ops_res, stride, p):
    """sw_traceback.hip: pair p stores its operations a dword at a time when the end of its slot is 4-byte aligned"""
    return (ops_res + (p + 1) * stride) % 4 == 0


# ---- bg_revcomp_batch_dev -------------------------------------------------------------------------------------------------------
def revcomp_seqs():
    """70 sequences of 0 .. 40 bytes over the n-alphabet in both cases"""
    rng = random.Random(205)
    return [bytes(rng.choice(fc.ALPHA) for _ in range((7 * i) % 41)) for i in range(70)]


# ---- bg_align_banded_batch_dev ------------------------------------------------------------------------------------------------
BAND_TILE_N = (2047, 2048, 2049, 4097)


def band_pairs():
    """eight pairs around the builder's 2048-column raster tile: identical and mutated, from tests/band_edge_cases.py"""
    return [bec.tile_pair(n, mutated) for n in BAND_TILE_N for mutated in (False, True)]


# ---- bg_seed_extend_strands_batch_dev, bg_seed_extend_tiered_batch_dev --------------------------------------------------------
SEED_READS, SEED_LEN, SEED_PAD = 64, 100, 25
SEED_STRIDE = 2 * SEED_LEN + 2 * SEED_PAD + 4
SEED_BELOW = 60  # below every exact read's score (100), above a read without a tier-1 hit


@functools.lru_cache(maxsize=None)
def seed_genome():
    return fc.random_dna(20_000, 206)


@functools.lru_cache(maxsize=None)
def seed_reads():
    """(buf, off, planted): 64 reads of 100 bases of the genome; the planted half carries a substitution in every window of
    tier 1 (at 15, 35, ...), so that tier 1 finds nothing and the SMEMs of tier 2 do; every third read reverse complemented.
    Which reads are planted is irregular, so that read r and its index among the re-seeded ones differ by changing amounts."""
    rng = np.random.default_rng(207)
    g = seed_genome()
    reads, planted = [], []
    for r in range(SEED_READS):
        s = int(rng.integers(0, len(g) - SEED_LEN))
        piece = g[s:s + SEED_LEN]
        is_planted = (r % 8) in (1, 2, 4, 7)
        if is_planted:
            piece = fc.substituted(piece, 20, start=15)
        reads.append(fc.revcomp(piece) if r % 3 == 1 else piece)
        planted.append(is_planted)
    buf, off = fc.concat(reads)
    return buf, off, np.array(planted)


def copy_wave_kinds(tier2_winners, reseeded, ops_res, n_ops, stride=SEED_STRIDE):
    """seed_tiered.hip, copy_wave: for every read whose tier-2 hit wins, 'vector' when the operations' address in the caller's
    slot and in the call's scratch slot (an allocation of its own: residue 0) agree mod 16, else 'bytes'.  reseeded: the reads
    of tier 2 in order (read r is compact read j = its index there)."""
    compact = {int(r): j for j, r in enumerate(reseeded)}
    kinds = {}
    for r in tier2_winners:
        r = int(r)
        dst = ops_res + (r + 1) * stride - int(n_ops[r])
        src = (compact[r] + 1) * stride - int(n_ops[r])
        kinds[r] = "vector" if (dst - src) % 16 == 0 else "bytes"
    return kinds


# ---- bg_sam_emit_batch_dev, bg_sam_sort_dev -----------------------------------------------------------------------------------
def sam_case():
    """40 reads, K = 1, NM and MD: unplaced reads without an id (22 bytes, the shortest line there is: at most residues no
    16-byte store at all), unplaced reads whose line is exactly 32 bytes, placed lines of a few hundred bytes on both strands
    (staged in LDS) and placed lines beyond the staging limit (written in place)"""
    import sam_edge_cases as ec
    at = ec.MD_CONTIGS[1][1] + 40
    reads, hits = [], []
    for i in range(40):
        kind = i % 5
        if kind == 0:
            reads.append(ec.read(b"", 0))
            hits.append(None)
        elif kind == 1:
            reads.append(ec.read(b"f" * 11, 0))
            hits.append(None)
        elif kind == 2:
            n = 25 + i  # (25: the lines then begin at every residue of the output)
            reads.append(ec.read(b"s%d" % i, n, i))
            hits.append(ec.hit(at + 3 * i, "=" * (n - 3) + "X==", i % 2, score=n - 5))
        elif kind == 3:
            n = 130 + 3 * i
            reads.append(ec.read(b"m%d" % i, n, i))
            hits.append(ec.hit(at + 5 * i, "=" * 50 + "XD" + "=" * (n - 51), (i // 5) % 2, score=n - 9))
        else:
            n = 560 + 7 * i
            reads.append(ec.read(b"long%d" % i, n, i))
            hits.append(ec.hit(at + 7 * i, "=" * 100 + "I" + "=" * (n - 101), (i // 5) % 2, score=n - 7))
    kat = {"flags": ["NM", "MD"], "K": 1, "reads": reads, "hits": hits}
    return ec.EmitCase("pointer_alignment", "lines of 22 and 32 bytes, staged and unstaged placed lines", ec.MD_CONTIGS, kat, ec.md_text())


SORT_LENS = (0, 1, 15, 16, 17, 22, 32, 33, 47, 48, 300, 1041, SAM_LONG_LINE, SAM_LONG_LINE + 1, 20_000)


def sort_batch(seed=11):
    """40 records: every length of SORT_LENS (shorter than a vector, exactly one, long ones for both copy kernels), keys
    that move them about"""
    import sam_edge_cases as ec
    rng = random.Random(seed)  # (the default: a seed under which, at every pair of residues, some vectors have an aligned source: the CPU test)
    lens = list(SORT_LENS) + [rng.choice((1, 15, 16, 17, 23, 40, 77, 300)) for _ in range(40 - len(SORT_LENS))]
    rng.shuffle(lens)
    keys = [rng.choice((rng.randrange(1990), rng.randrange(30), ec.TOP)) for _ in lens]
    return ec.SortBatch("pointer_alignment", "records of 0 ... 20 000 bytes", lens, keys)


def copy_plan(dst_res, length):
    """sam_rule.h, sam_copy_plan: (head, body, tail) of a line of `length` bytes whose destination has residue dst_res"""
    head = min(length, (16 - dst_res) % 16)
    return head, (length - head) // 16, (length - head) % 16


# ---- bg_fastq_trim_dev, bg_fastq_filter_dev, bg_fastq_demux_split_dev, bg_fastq_qual_cut_dev -----------------------------------
def column_records():
    """40 records of 0 .. 40 bases from tests/fastq_write_cases.py, some with unequal sequence and quality lengths"""
    from fastq_write_cases import random_records
    return random_records(random.Random(209), 40, 0, 40)


def qual_records():
    """40 records of tests/fastq_qual_cases.py: lengths around 16 and 32, low stretches at the ends"""
    from fastq_qual_cases import random_records
    return random_records(random.Random(210), 40, hi=120)


def trim_hits(records, n_pat=2):
    """hand-made records of a best call (score, ystart, yend): about half of the reads have a hit in one pattern"""
    from fastq_demux_cases import blank_hits, set_hit
    rng = random.Random(211)
    hits = blank_hits(len(records), n_pat)
    for r, (_, _, s, _) in enumerate(records):
        hits["ylen"][r * n_pat:(r + 1) * n_pat] = len(s)
        if len(s) >= 8 and rng.random() < 0.6:
            ys = rng.randint(0, len(s) - 8)
            set_hit(hits, n_pat, r, rng.randrange(n_pat), rng.randint(0, 3), ys, min(len(s), ys + rng.randint(4, 8)))
    return hits


def split_bins(n, n_bins=3):
    """a sample per read: the bins, unassigned (n_bins), ambiguous (n_bins + 1) and a value beyond them"""
    rng = random.Random(212)
    return np.array([rng.choice([0, 1, 2, 2, n_bins, n_bins + 1, 77]) for _ in range(n)], dtype=np.uint32)

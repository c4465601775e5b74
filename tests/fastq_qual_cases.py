"""Seeded random batches for the quality tests.  A quality string is a chain of stretches of four kinds, so that every branch
of the three rules is common: high, low, exactly at the cutoff, and bytes below the phred offset (quality 0)."""
import fastq_qual_oracle as qo

PHRED, CUTOFF = 33, 20
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33)
METHOD_PAIRS = [(m5, m3) for m5 in (qo.NONE, qo.RUNSUM) for m3 in (qo.NONE, qo.RUNSUM, qo.WINDOW)]
SELECT_FLAGS = (0, qo.PAIRED, qo.PAIRED | qo.PAIR_BOTH)


def qual_string(rng, n, p_low=0.4, cutoff=CUTOFF, phred=PHRED):
    out = bytearray()
    while len(out) < n:
        k = rng.random()
        run = rng.randint(1, 9)
        if k < p_low:
            out += bytes(phred + rng.randint(0, cutoff - 1) for _ in range(run))
        elif k < p_low + 0.12:
            out += bytes([phred + cutoff]) * run
        elif k < p_low + 0.2:
            out += bytes(rng.randint(phred - 19, phred - 2) for _ in range(run))  # 14 .. 31: no byte a FASTQ reader strips at a line's end
        else:
            out += bytes(phred + rng.randint(cutoff + 1, 41) for _ in range(run))
    return bytes(out[:n])


def random_records(rng, n, lengths=LENGTHS, hi=300, p_low=0.4, equal=0.85, tag=b"q"):
    """(id, desc, seq, qual): lengths from `lengths` or random up to hi; a few records whose two lengths differ"""
    out = []
    for r in range(n):
        ln = rng.choice(lengths) if rng.random() < 0.5 else rng.randint(0, hi)
        ql = ln if rng.random() < equal else rng.randint(0, hi)
        low = rng.choice([0.05, 0.05, p_low, 0.9])  # mostly good, mixed, mostly bad reads
        q = bytearray(qual_string(rng, ql, low))
        if r % 2 == 1:  # ... and good reads with a few low symbols at one end or both
            head, tail = rng.choice([(0, 6), (6, 0), (6, 6), (6, 6)])
            for i in range(min(ql, rng.randint(0, head))):
                q[i] = PHRED + rng.randint(0, 5)
            for i in range(min(ql, rng.randint(0, tail))):
                q[ql - 1 - i] = PHRED + rng.randint(0, 5)
        out.append((tag + b"%d" % r, None if r % 3 else b"d%d" % r, bytes(rng.choice(b"ACGTNacgtn") for _ in range(ln)), bytes(q)))
    return out


def cut_params(rng, m5, m3, window=None):
    return dict(method_5p=m5, method_3p=m3, cutoff_5p=rng.choice([CUTOFF, CUTOFF, 2, 300]), cutoff_3p=rng.choice([CUTOFF, CUTOFF, 3, 41]),
                window=window if window is not None else rng.choice([1, 2, 4, 5, 40]))


def select_params(rng, flags):
    return dict(flags=flags, min_mean_q=rng.choice([0, 15, CUTOFF, 25]), low_q=rng.choice([0, CUTOFF, CUTOFF + 1]),
                max_low_pct=rng.choice([0, 20, 40, 100, 250]))

"""Alphabets used to size Less/Occ (reference: src/alphabets/mod.rs:49-133, dna.rs:23-35) and the DNA complement
(dna.rs:37-92)."""
import numpy as np


class Alphabet:
    def __init__(self, symbols):
        self.symbols = bytes(sorted(set(bytes(symbols))))

    def is_word(self, text):
        s = set(self.symbols)
        return all(c in s for c in bytes(text))

    def max_symbol(self):
        return self.symbols[-1] if self.symbols else None

    def insert(self, a):
        self.symbols = bytes(sorted(set(self.symbols) | {a}))

    def __len__(self):
        return len(self.symbols)

    def __bytes__(self):
        return self.symbols


def _complement_table():
    t = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"AGCTYRWSKMDVHBN", b"TCGARYWSMKHBDVN"):  # dna.rs:37-50: upper case, and the same + 32 for lower case
        t[a], t[a + 32] = b, b + 32
    return t


_COMPLEMENT = _complement_table()


class dna:
    @staticmethod
    def alphabet():
        return Alphabet(b"ACGTacgt")  # dna.rs:23-25

    @staticmethod
    def n_alphabet():
        return Alphabet(b"ACGTNacgtn")  # dna.rs:29-31

    @staticmethod
    def iupac_alphabet():
        return Alphabet(b"ACGTRYSWKMBDHVNacgtryswkmbdhvn")  # dna.rs:33-35

    COMPLEMENT = _COMPLEMENT  # uint8[256]: the complement of every byte value (every byte outside the table is itself)

    @staticmethod
    def complement(a):
        """dna::complement: the complement of one byte value, case kept (N -> N)"""
        return int(_COMPLEMENT[a])

    @staticmethod
    def revcomp(text):
        """dna::revcomp: the reverse complement of a byte string (bytes in, bytes out; a uint8 array gives a uint8 array)"""
        if isinstance(text, np.ndarray):
            return _COMPLEMENT[np.ascontiguousarray(text, dtype=np.uint8)[::-1]]
        return _COMPLEMENT[np.frombuffer(bytes(text), dtype=np.uint8)[::-1]].tobytes()

"""Batches for the FASTQ filter and writer tests: records given as (id, desc or None, seq, qual) laid out as the columns
`bg_fastq_parse` leaves (a text that holds ids and descriptions, concatenated sequences and qualities with n + 1 offsets,
records that point into them), optionally behind prefixes so that every run starts at a chosen byte alignment."""
import numpy as np

from rust_bio_amd import _lib


class Batch:
    def __init__(self, records, a_text=0, a_seq=0, a_qual=0, checks=None):
        n = len(records)
        self.records = list(records)
        self.recs = np.zeros(n, dtype=_lib.FQREC_DTYPE)
        text, seq, qual = bytearray(b"#" * a_text), bytearray(b"#" * a_seq), bytearray(b"#" * a_qual)
        so, qo = [a_seq], [a_qual]
        for r, (id_, desc, s, q) in enumerate(records):
            c = self.recs[r]
            text += b"@"
            c["id_off"], c["id_len"] = len(text), len(id_)
            text += id_
            if desc is not None:
                text += b" "
                c["has_desc"], c["desc_off"], c["desc_len"] = 1, len(text), len(desc)
                text += desc
            text += b"\n"
            c["seq_off"], c["seq_len"], c["qual_off"], c["qual_len"] = len(seq), len(s), len(qual), len(q)
            if checks is not None:
                c["check"] = checks[r]
            seq += s
            qual += q
            so.append(len(seq))
            qo.append(len(qual))
        self.text, self.seq, self.qual = bytes(text), bytes(seq), bytes(qual)
        self.seq_off, self.qual_off = np.array(so, np.uint64), np.array(qo, np.uint64)

    def __len__(self):
        return len(self.recs)

    def columns(self):
        return self.recs, self.seq, self.seq_off, self.qual, self.qual_off

    def host(self):
        """(text, recs, seq, qual) for fastq.emit_arrays"""
        return self.text + b"#", self.recs, self.seq + b"#", self.qual + b"#"

    def to_dev(self, device="cuda:0"):
        """(d_text, d_recs, d_seq, d_seq_off, d_qual, d_qual_off) as torch tensors; no buffer is empty"""
        import torch

        def up(b):
            return torch.frombuffer(bytearray(b + b"#"), dtype=torch.uint8).to(device)

        return (up(self.text), up(self.recs.tobytes()), up(self.seq), torch.from_numpy(self.seq_off.astype(np.int64)).to(device), up(self.qual),
                torch.from_numpy(self.qual_off.astype(np.int64)).to(device))


def random_records(rng, n, lo=0, hi=40, alphabet=b"ACGTNn", equal=0.8, tag=b"r"):
    out = []
    for r in range(n):
        desc = None if rng.random() < 0.4 else bytes(rng.randint(48, 122) for _ in range(rng.randint(0, 12)))
        ln = rng.randint(lo, hi)
        ql = ln if rng.random() < equal else rng.randint(lo, hi)
        out.append((tag + b"%d" % r, desc, bytes(rng.choice(alphabet) for _ in range(ln)), bytes(rng.randint(33, 73) for _ in range(ql))))
    return out

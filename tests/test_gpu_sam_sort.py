"""bg_sam_sort[_dev] against the CPU statement (tests/sam_sort_oracle.py): the permutation, the offsets and the bytes.  The
records are synthetic lines (tests/sam_sort_cases.py) of every length around the 16-byte granule of the copy, one of 140 000
bytes among short ones (beyond the length at which a line is cut into chunks for blocks), at source offsets that cover all 16
residues against the destination's; the keys are all equal (stability), strictly descending, all UINT64_MAX, or differ only in
their high word."""
import random

import numpy as np
import pytest
import torch

import sam_oracle as so
import sam_sort_oracle as sso
from rust_bio_amd import _lib, sam
import sam_edge_cases as ec
from sam_sort_cases import LINE_LENGTHS, synthetic_lines

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPS_CAP = -9
POISON = 0x7e
TOP = 2**64 - 1


def dev(a, dtype=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(DEV) if a.size else torch.zeros(16, dtype=torch.uint8, device=DEV)


def check(key, recs, host=True):
    """both flavours against the oracle; the device flavour into a poisoned buffer with 64 bytes behind the text.
    Returns (perm, out_off) of the oracle."""
    key = np.asarray(key, dtype=np.uint64)
    text, off = b"".join(recs), so.offsets(recs)
    perm, out_off, want = sso.sort(key, recs)
    n, nbytes = len(recs), len(text)
    if host:
        got, got_off, got_perm = sam.sort_arrays(key, text, off)
        assert (got_perm == perm).all() and (got_off == out_off).all() and got == want
    d_key, d_in, d_off = dev(key), dev(np.frombuffer(text, np.uint8)), dev(off)
    d_out = torch.full((nbytes + 64,), POISON, dtype=torch.uint8, device=DEV)
    d_out_off = torch.full((n + 1,), -1, dtype=torch.int64, device=DEV)
    d_perm = torch.full((max(n, 1),), -1, dtype=torch.int64, device=DEV)
    args = (n, d_key.data_ptr(), d_in.data_ptr(), d_off.data_ptr(), nbytes, d_out.data_ptr())
    tail = (d_out_off.data_ptr(), d_perm.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    if nbytes:
        with pytest.raises(_lib.BiogpuError) as e:
            sam.sort_dev(*args, nbytes - 1, *tail, stream=stream)
        torch.cuda.synchronize()
        assert e.value.status == OPS_CAP and (d_out == POISON).all() and (d_out_off == -1).all() and (d_perm == -1).all()
    sam.sort_dev(*args, nbytes + 64, *tail, stream=stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (d_perm.cpu().numpy()[:n].astype(np.uint64) == perm).all()
    assert (d_out_off.cpu().numpy().astype(np.uint64) == out_off).all()
    assert (out[nbytes:] == POISON).all(), "bytes behind the text were touched"
    if out[:nbytes].tobytes() != want:  # name the first record that differs
        for j in range(n):
            a, b = int(out_off[j]), int(out_off[j + 1])
            assert out[a:b].tobytes() == want[a:b], (j, int(perm[j]), b - a, a % 16, int(off[int(perm[j])]) % 16)
    return perm, out_off


def test_every_length_and_every_residue():
    rng = random.Random(3)
    recs, text, off = synthetic_lines(rng, 600, long_at=311)
    key = [rng.randrange(40) for _ in recs]
    perm, out_off = check(key, recs)
    assert len(recs[311]) == 140_000
    # every length, and for the lines with a 16-byte body every residue of the source against the destination
    assert {len(r) for r in recs} == set(LINE_LENGTHS) | {140_000}
    residues = {(int(off[int(i)]) - int(out_off[j])) % 16 for j, i in enumerate(perm) if len(recs[int(i)]) >= 31}
    assert residues == set(range(16))
    heads = {int(out_off[j]) % 16 for j, i in enumerate(perm) if len(recs[int(i)]) >= 31}
    assert heads == set(range(16))
    # the long line at every residue pair is too much for one test: three more, at other offsets
    for extra in (1, 6, 11):
        recs2 = [b"x" * extra] + recs[300:320]
        check([5] + [rng.randrange(4) for _ in recs2[1:]], recs2, host=False)


@pytest.mark.parametrize("pattern", ["equal", "descending", "top", "high word"])
def test_key_patterns(pattern):
    rng = random.Random(5)
    recs, _, _ = synthetic_lines(rng, 1500, lengths=LINE_LENGTHS + (40, 77))
    n = len(recs)
    key = {"equal": [12345] * n, "descending": [10**12 - 3 * i for i in range(n)], "top": [TOP] * n,
           "high word": [((i * 7919) % 5 << 32) | 77 for i in range(n)]}[pattern]
    perm, _ = check(key, recs)
    if pattern in ("equal", "top"):
        assert perm.tolist() == list(range(n))
    if pattern == "descending":
        assert perm.tolist() == list(range(n))[::-1]


def test_many_short_lines():
    rng = random.Random(7)
    recs, _, _ = synthetic_lines(rng, 70_000, lengths=tuple(range(1, 41)))
    key = np.random.default_rng(7).integers(0, 2**40, size=len(recs), dtype=np.uint64)
    key[::9] = TOP
    check(key, recs, host=False)


@pytest.mark.parametrize("n", [0, 1])
def test_tiny(n):
    check([9] * n, [b"only line\n"] * n)
    if n:
        check([9], [b""])


# ---- the edges of the two copy kernels (the batches of tests/sam_edge_cases.py; tests/test_sam_edge_cases.py shows what they hold)
def test_lengths_around_the_switch_between_the_copy_kernels():
    b = ec.sort_switch()
    assert {(ln, res) for ln, res, _ in b.placed() if ln >= 16383} == {(ln, res) for ln in ec.SWITCH_LENGTHS for res in ec.RESIDUES}
    check(b.key, b.recs)


def test_lengths_around_a_chunk_and_the_column_wrap():
    b = ec.sort_chunk()
    assert {(ln >> 4) // 256 + 1 for ln, _, _ in b.placed()} == {5, 6, 32, 33, 34}  # chunks as the long-line kernel counts them
    check(b.key, b.recs)


@pytest.mark.parametrize("n_long", [255, 256, 257])
def test_row_wrap_of_the_long_line_kernel(n_long):
    b = ec.sort_rows(n_long)
    assert sum(len(r) > ec.LONG_LINE for r in b.recs) == n_long
    check(b.key, b.recs, host=n_long == 257)


@pytest.mark.parametrize("which", ["first", "last"])
def test_a_long_line_at_either_end_of_the_buffer(which):
    b = ec.sort_ends(which)
    perm, _ = check(b.key, b.recs, host=which == "last")  # (check() requires the 64 poisoned bytes behind the text intact)
    assert len(b.recs[int(perm[0 if which == "first" else -1])]) == 20_000


def test_several_long_lines_from_the_generator():
    rng = random.Random(13)
    longs = {3: 16_385, 40: 20_480, 41: 16_384, 99: 70_001}
    recs, _, _ = synthetic_lines(rng, 100, long_at=longs)
    assert all(len(recs[i]) == ln for i, ln in longs.items())
    check([rng.randrange(8) for _ in recs], recs, host=False)

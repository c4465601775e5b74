"""BGZF framing (`bg_bgzf_frame[_dev]`): the format is deterministic, so the output must equal `bam_oracle.frame` byte for byte
(gzip header, BC subfield, stored deflate block, zlib's CRC-32, ISIZE), and `gzip.decompress` must give the input back.  Sizes
around a payload (65 280 bytes), random and all-zero bytes, source and destination at every residue mod 16 between guard
bytes, with and without the end-of-file block, BG_ERR_OPS_CAP one byte short."""
import gzip

import numpy as np
import pytest
import torch

import bam_oracle as bo
from dev_shift import guards_intact, shifted, shifted_from
from rust_bio_amd import _lib, bam

pytestmark = pytest.mark.gpu
P = 65280
SIZES = [0, 1, 3, 4, P - 1, P, P + 1, 2 * P, 2 * P + 1, 300 * P + 12345]


def stream():
    return torch.cuda.current_stream().cuda_stream


def data_of(n, zero):
    return np.zeros(n, np.uint8) if zero else np.random.default_rng(n + 5).integers(0, 256, n, dtype=np.uint8)


def frame_dev(data, flags, r_in=0, r_out=0):
    d_in = shifted_from(data, r_in)
    need = bam.framed_bytes(len(data), flags)
    assert bam.bgzf_frame_dev(d_in.data_ptr(), len(data), 0, 0, flags, stream()) == need  # the sizing call
    d_out = shifted(need, r_out)
    assert bam.bgzf_frame_dev(d_in.data_ptr(), len(data), d_out.data_ptr(), need, flags, stream()) == need
    assert guards_intact(d_out) and guards_intact(d_in)
    return d_out.cpu().numpy().tobytes()


@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(n, zero):
    data = data_of(n, zero)
    raw = data.tobytes()
    want = bo.frame(raw, True)
    assert len(want) == n + 31 * ((n + P - 1) // P) + 28
    got = frame_dev(data, bam.BGZF_EOF, r_in=n % 16, r_out=(n * 7 + 3) % 16)
    assert got == want
    assert gzip.decompress(got) == raw
    assert frame_dev(data, 0) == want[:-28]
    assert bam.bgzf_frame_arrays(raw, bam.BGZF_EOF) == want and bam.bgzf_frame_arrays(raw) == want[:-28]


@pytest.mark.parametrize("r_out", range(16))
def test_every_residue(r_out):
    data = data_of(2 * P + 77, False)
    want = bo.frame(data.tobytes(), True)
    for r_in in range(16):
        assert frame_dev(data, bam.BGZF_EOF, r_in, r_out) == want, (r_in, r_out)


@pytest.mark.parametrize("flags", [0, bam.BGZF_EOF])
def test_ops_cap_one_byte_short_writes_nothing(flags):
    data = data_of(P + 9, False)
    need = bam.framed_bytes(len(data), flags)
    d_in, d_out = shifted_from(data, 3), shifted(need, 5, fill=0x5A)
    with pytest.raises(_lib.BiogpuError) as e:
        bam.bgzf_frame_dev(d_in.data_ptr(), len(data), d_out.data_ptr(), need - 1, flags, stream())
    torch.cuda.synchronize()
    assert e.value.status == -9 and bool((d_out == 0x5A).all()) and guards_intact(d_out)


def test_unknown_flag_bits():
    with pytest.raises(_lib.BiogpuError) as e:
        bam.bgzf_frame_arrays(b"abc", 2)
    assert e.value.status == -1

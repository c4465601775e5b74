"""bg_bgzf_deflate[_dev] on the GPU against the CPU run of the same bodies: tests/bgzf_deflate_host_bodies.cpp, built once for
this module without sanitizer flags, makes every block lane by lane, and the GPU must give exactly its bytes — for the payloads
of tests/bgzf_deflate_cases.py and for inputs of 65 281 and 2 * 65 280 + 77 bytes (zeros, random, text), with and without the
end-of-file block.  `gzip.decompress` gives the input back; `block_off` holds the block starts found by walking BSIZE; the
bytes are the same at the residues (0, 0), (7, 3), (15, 1), (1, 15) of source and destination between intact guard bytes and
on a second call; one byte short of the stored bound is status -9 with the output untouched; the host flavour gives the device
flavour's bytes; an empty input gives no block; FASTQ text leaves as .fastq.gz."""
import gzip
import random

import numpy as np
import pytest
import torch

import bam_oracle as bo
import bgzf_deflate_cases as dc
import fastq_write_cases as fw
from dev_shift import guards_intact, shifted, shifted_from
from rust_bio_amd import _lib, bam, fastq

pytestmark = pytest.mark.gpu
P = dc.P
RESIDUES = ((0, 0), (7, 3), (15, 1), (1, 15))  # (source, destination)


def stream():
    return torch.cuda.current_stream().cuda_stream


def cut(data):
    return [data[a:a + P] for a in range(0, len(data), P)]


def long_inputs():
    rng = np.random.default_rng(99)
    out = []
    for n in (P + 1, 2 * P + 77):
        out += [("zeros %d" % n, bytes(n)), ("random %d" % n, dc.rand(rng, n)), ("text %d" % n, dc.text_of(rng, n))]
    return out


@pytest.fixture(scope="module")
def want(tmp_path_factory):
    """name -> (input, the stream of blocks the CPU run gives for it)"""
    tmp = tmp_path_factory.mktemp("dfl_gpu")
    exe = dc.build_program(str(tmp / "bodies"), sanitize=False)
    inputs = dc.payloads() + long_inputs()
    parts = [cut(d) for _, d in inputs]
    _, blocks = dc.run_program(exe, tmp, [], [p for ps in parts for p in ps])
    out, at = {}, 0
    for (name, data), ps in zip(inputs, parts):
        out[name] = (data, b"".join(b for b, _, _ in blocks[at:at + len(ps)]))
        at += len(ps)
    return out


def deflate_dev(data, flags, r_in=0, r_out=0, fill=0xA5):
    """-> (bytes, block_off) of bg_bgzf_deflate_dev with the source and the destination at the given residues mod 16"""
    d_in = shifted_from(data, r_in)
    cap = bam.framed_bytes(len(data), flags)
    assert bam.bgzf_deflate_dev(d_in.data_ptr(), len(data), 0, 0, flags, stream()) == cap  # the sizing call
    d_out = shifted(cap, r_out, fill=fill)
    d_off = torch.full(((len(data) + P - 1) // P + 1,), -1, dtype=torch.int64, device="cuda")
    n = bam.bgzf_deflate_dev(d_in.data_ptr(), len(data), d_out.data_ptr(), cap, flags, stream(), d_block_off=d_off.data_ptr())
    assert n <= cap and guards_intact(d_out) and guards_intact(d_in)
    got = d_out.cpu().numpy()
    assert (got[n:] == fill).all()  # nothing behind the stream
    return got[:n].tobytes(), d_off.cpu().numpy().astype(np.uint64)


def test_gpu_bytes_are_the_cpu_bodies_bytes(want):
    for name, (data, blocks) in want.items():
        got, off = deflate_dev(data, bam.BGZF_EOF)
        assert got == blocks + bo.EOF_BLOCK, name
        assert gzip.decompress(got) == data, name
        starts = np.cumsum([0] + [len(b) for b in dc.split_blocks(blocks)])
        assert off.tolist() == starts.tolist(), name
        if len(data) > P or len(data) in (1, 259):
            got0, off0 = deflate_dev(data, 0)
            assert got0 == blocks and off0.tolist() == off.tolist(), name
            cap = bam.framed_bytes(len(data))
            assert bam.bgzf_deflate_dev(shifted_from(data, 0).data_ptr(), len(data), shifted(cap, 0).data_ptr(), cap, 0, stream()) == len(got0)  # no table


@pytest.mark.parametrize("name", ["text %d" % (2 * P + 77), "zeros %d" % (P + 1), "random %d" % (2 * P + 77), "text 259", "period 258"])
def test_residues_and_a_second_call(want, name):
    data, blocks = want[name]
    for r_in, r_out in RESIDUES:
        got, _ = deflate_dev(data, bam.BGZF_EOF, r_in, r_out)
        assert got == blocks + bo.EOF_BLOCK, (r_in, r_out)
    assert deflate_dev(data, bam.BGZF_EOF, 7, 3)[0] == blocks + bo.EOF_BLOCK


@pytest.mark.parametrize("flags", [0, bam.BGZF_EOF])
def test_one_byte_short_of_the_stored_bound_writes_nothing(flags):
    data = dc.text_of(np.random.default_rng(5), P + 9)  # compresses well: the bound is what counts, not the actual size
    cap = bam.framed_bytes(len(data), flags)
    d_in, d_out = shifted_from(data, 3), shifted(cap, 5, fill=0x5A)
    with pytest.raises(_lib.BiogpuError) as e:
        bam.bgzf_deflate_dev(d_in.data_ptr(), len(data), d_out.data_ptr(), cap - 1, flags, stream())
    torch.cuda.synchronize()
    assert e.value.status == -9 and bool((d_out == 0x5A).all()) and guards_intact(d_out)


def test_host_flavour_gives_the_device_flavours_bytes(want):
    for name in ("text %d" % (2 * P + 77), "random %d" % (P + 1), "zeros 4", "fibonacci counts"):
        data, blocks = want[name]
        for flags, tail in ((0, b""), (bam.BGZF_EOF, bo.EOF_BLOCK)):
            got, off = bam.bgzf_deflate_arrays(data, flags)
            assert got == blocks + tail, (name, flags)
            assert off.tolist() == np.cumsum([0] + [len(b) for b in dc.split_blocks(blocks)]).tolist()


def test_empty_input():
    # no block and no end-of-file block: nothing is written but the closing offset (a null d_out would be the sizing call)
    d_out, d_off = shifted(16, 5), torch.full((1,), -1, dtype=torch.int64, device="cuda")
    assert bam.bgzf_deflate_dev(0, 0, d_out.data_ptr(), 0, 0, stream(), d_block_off=d_off.data_ptr()) == 0
    assert d_off.tolist() == [0] and bool((d_out == 0xA5).all()) and guards_intact(d_out)
    got, off = deflate_dev(b"", bam.BGZF_EOF)
    assert got == bo.EOF_BLOCK and off.tolist() == [0]
    assert bam.bgzf_deflate_arrays(b"", bam.BGZF_EOF)[0] == bo.EOF_BLOCK and bam.bgzf_deflate_arrays(b"")[0] == b""


def test_fastq_text_leaves_as_fastq_gz():
    b = fw.Batch(fw.random_records(random.Random(3), 3000, lo=30, hi=151, equal=1.0))
    text, _ = fastq.emit_arrays(b.host())
    assert text.count(b"\n") == 4 * 3000 and len(text) > 2 * P
    got, off = bam.bgzf_deflate_arrays(text, bam.BGZF_EOF)
    # bases over 6 letters and qualities over 41 values: 2.6 and 5.4 bits a byte, half the text each, and the names on top
    assert gzip.decompress(got) == text and got.endswith(bo.EOF_BLOCK) and len(got) < 0.7 * len(text)
    assert len(off) == (len(text) + P - 1) // P + 1 and int(off[-1]) == len(got) - 28

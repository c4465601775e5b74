"""bg_bgzf_blocks[_dev] and bg_bgzf_inflate[_dev] on the GPU, on the cases of tests/bgzf_inflate_cases.py as files of a few
dozen blocks, against the CPU run of the same bodies (tests/bgzf_inflate_host_bodies.cpp, built once for this module without
sanitizer flags).

The block table of every file must be the Python walk over BSIZE; good members must come out as the bytes that went in;
statuses and first_bad must be the CPU program's, which the host-bodies test holds to zlib's verdict.  Bad members stand between
good ones whose payloads must be intact (the bytes on either side of a bad block's output range), between intact guard bytes
around the whole buffer.  d_in and d_out at every offset 0 .. 15 from 16-byte alignment; sizing calls, BG_ERR_OPS_CAP and the
refusals that leave everything unwritten; the host flavours and `bam.BgzfError`."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import bgzf_inflate_cases as ic
from dev_shift import guards_intact, shifted, shifted_from
from rust_bio_amd import _lib, bam

pytestmark = pytest.mark.gpu
FILE_BLOCKS = 60
CORRUPT_BLOCKS = 80


def stream():
    return torch.cuda.current_stream().cuda_stream


def table(values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint64).view(np.int64).copy()).cuda()


@pytest.fixture(scope="module")
def want(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("inf_gpu")
    exe = ic.build_program(str(tmp / "bodies"), sanitize=False)
    good, hand, corrupt = ic.good_members(), ic.hand_made(), ic.corruptions()
    files = [b"".join(m for _, m, _ in good[k:k + FILE_BLOCKS]) for k in range(0, len(good), FILE_BLOCKS)]
    pad = [good[3][1], good[40][1]]
    mixed = b"".join(pad[k & 1] + m for k, (_, m, _) in enumerate(hand)) + pad[len(hand) & 1]  # every hand-made member between two good ones
    empty = b"".join(m for _, m, _ in ic.empty_member_file())
    got_files, got_members = ic.run_program(exe, tmp, files + [mixed, empty], [(m, ic.range_of(m)) for m in corrupt])
    return dict(good=good, hand=hand, corrupt=corrupt, files=files, mixed=mixed, empty=empty, cpu_files=got_files[:-2], cpu_mixed=got_files[-2],
                cpu_empty=got_files[-1], cpu_members=got_members)


def blocks_dev(f, r_in=0):
    """-> (block_off, out_off) of bg_bgzf_blocks_dev: the sizing call, then the tables"""
    d_in = shifted_from(f, r_in)
    n, total = bam.bgzf_blocks_dev(d_in.data_ptr(), len(f), stream=stream())
    d_b, d_o = (torch.full((n + 2,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    assert bam.bgzf_blocks_dev(d_in.data_ptr(), len(f), d_b.data_ptr(), d_o.data_ptr(), n, stream=stream()) == (n, total)
    assert int(d_b[n + 1]) == -1 and int(d_o[n + 1]) == -1 and guards_intact(d_in)
    return d_b[:n + 1].cpu().numpy().astype(np.uint64).tolist(), d_o[:n + 1].cpu().numpy().astype(np.uint64).tolist()


def inflate_dev(f, block_off, out_off, r_in=0, r_out=0, fill=0xA5):
    """-> (the BgzfError or None, statuses, the output buffer's bytes) of bg_bgzf_inflate_dev"""
    n, total = len(block_off) - 1, int(out_off[-1])
    d_in, d_out = shifted_from(f, r_in), shifted(total, r_out, fill=fill)
    d_status = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    d_b, d_o = table(block_off), table(out_off)
    err = None
    try:
        bam.bgzf_inflate_dev(d_in.data_ptr(), len(f), n, d_b.data_ptr(), d_o.data_ptr(), d_out.data_ptr(), total,
                             d_status.data_ptr(), stream())
    except bam.BgzfError as e:
        err = e
    assert guards_intact(d_out) and guards_intact(d_in)
    return err, d_status[:n].cpu().tolist(), d_out.cpu().numpy().tobytes()


def test_good_files(want):
    good = want["good"]
    for k, f in enumerate(want["files"]):
        part = good[k * FILE_BLOCKS:(k + 1) * FILE_BLOCKS]
        rc, block_off, out_off, _ = ic.walk(f)
        assert rc == 0 and blocks_dev(f, (5 * k) % 16) == (block_off, out_off) == (want["cpu_files"][k][4], want["cpu_files"][k][5])
        err, status, out = inflate_dev(f, block_off, out_off, (3 * k + 1) % 16, (7 * k + 2) % 16)
        assert err is None and status == [0] * len(part)
        assert out == b"".join(d for _, _, d in part)


def test_empty_members_in_front_in_the_middle_and_at_the_end(want):
    f, cpu, part = want["empty"], want["cpu_empty"], ic.empty_member_file()
    rc, block_off, out_off, _ = ic.walk(f)
    assert rc == 0 and out_off[:3] == [0, 0, 0] and out_off[-3] == out_off[-1] and (block_off, out_off) == (cpu[4], cpu[5])
    for r in (0, 3, 8, 15):
        assert blocks_dev(f, r) == (block_off, out_off), r
        err, status, out = inflate_dev(f, block_off, out_off, (r + 5) % 16, (3 * r + 1) % 16)
        assert err is None and status == cpu[6] == [0] * len(part) and out == cpu[8] == b"".join(d for _, _, d in part), r
    # empty members only: nothing to write, and no output buffer is needed (a null d_out with out_cap 0)
    f = ic.EOF_BLOCK + part[1][1] + ic.EOF_BLOCK
    assert blocks_dev(f, 7) == ([0, 28, 59, 87], [0, 0, 0, 0]) and len(part[1][1]) == 31
    d_in, d_b, d_o = shifted_from(f, 7), table([0, 28, 59, 87]), table([0, 0, 0, 0])
    d_status = torch.full((3,), 0xEE, dtype=torch.uint8, device="cuda")
    bam.bgzf_inflate_dev(d_in.data_ptr(), len(f), 3, d_b.data_ptr(), d_o.data_ptr(), 0, 0, d_status.data_ptr(), stream())
    assert d_status.tolist() == [0, 0, 0] and guards_intact(d_in)
    with pytest.raises(bam.BgzfError):  # ... but a null d_out with bytes to write stays refused
        bam.bgzf_inflate_dev(d_in.data_ptr(), len(f), 3, d_b.data_ptr(), table([0, 0, 1, 1]).data_ptr(), 0, 1, d_status.data_ptr(), stream())


def test_every_offset_from_alignment(want):
    f = b"".join(m for _, m, _ in want["good"][:21])  # payloads of 1 .. 259 bytes at level 0: stored copies at every residue
    f += b"".join(m for name, m, d in want["good"] if len(d) <= 4000 and "level 6" in name)
    rc, block_off, out_off, _ = ic.walk(f)
    expect = b"".join(ic.verdict(f[a:b]) for a, b in zip(block_off, block_off[1:]))
    assert rc == 0 and len(block_off) < 100
    for r in range(16):
        assert blocks_dev(f, r) == (block_off, out_off), r
        err, status, out = inflate_dev(f, block_off, out_off, r, (11 * r + 3) % 16)
        assert err is None and not any(status) and out == expect, r


def test_hand_made_members_between_good_ones(want):
    f, cpu = want["mixed"], want["cpu_mixed"]
    rc, block_off, out_off, _ = ic.walk(f)
    assert rc == 0 and len(block_off) - 1 == 2 * len(want["hand"]) + 1 < 100
    assert blocks_dev(f, 9) == (block_off, out_off) == (cpu[4], cpu[5])
    err, status, out = inflate_dev(f, block_off, out_off, 6, 13)
    assert status == cpu[6] and status[1::2] == [s for _, _, s in want["hand"]] and not any(status[0::2])
    assert err is not None and err.status == -1 and err.block == cpu[7] == 0 + 1
    for b, s in enumerate(status):  # good blocks are written in full: the bytes either side of every bad block's range are intact
        if not s:
            assert out[out_off[b]:out_off[b + 1]] == cpu[8][out_off[b]:out_off[b + 1]] == ic.verdict(f[block_off[b]:block_off[b + 1]]), b


def test_single_byte_corruptions(want):
    corrupt, cpu = want["corrupt"], want["cpu_members"]
    accepted = 0
    for k in range(0, len(corrupt), CORRUPT_BLOCKS):
        part = corrupt[k:k + CORRUPT_BLOCKS]
        block_off = np.cumsum([0] + [len(m) for m in part]).tolist()
        out_off = np.cumsum([0] + [ic.range_of(m) for m in part]).tolist()
        err, status, out = inflate_dev(b"".join(part), block_off, out_off, k % 16, (k // 5) % 16)
        assert status == [s for s, _ in cpu[k:k + len(part)]], k
        bad = [b for b, s in enumerate(status) if s]
        assert (err.block if err else None) == (bad[0] if bad else None)
        for b, s in enumerate(status):
            if not s:
                assert out[out_off[b]:out_off[b + 1]] == cpu[k + b][1]
                accepted += 1
    print("%d of %d corrupted members accepted" % (accepted, len(corrupt)))


def test_files_the_block_table_refuses():
    for name, f, rc, first_bad in ic.bad_files():
        d_in = shifted_from(f or b"\0", 3)  # (an empty file still has an address)
        d_b, d_o = (torch.full((8,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
        for tables in ((0, 0, 0), (d_b.data_ptr(), d_o.data_ptr(), 7)):
            if rc:
                with pytest.raises(bam.BgzfError) as e:
                    bam.bgzf_blocks_dev(d_in.data_ptr(), len(f), *tables, stream=stream())
                assert (e.value.status, e.value.block) == (rc, first_bad), name
                assert bool((d_b == -1).all()) and bool((d_o == -1).all()), name  # the tables stay unwritten
            else:
                assert bam.bgzf_blocks_dev(d_in.data_ptr(), len(f), *tables, stream=stream()) == (1 if f else 0, 0), name
        if rc == 0:
            n = 1 if f else 0
            assert d_b[:n + 1].tolist() == [0, len(f)][:n + 1] and d_o[:n + 1].tolist() == [0] * (n + 1) and int(d_b[n + 1]) == -1, name
        with pytest.raises(bam.BgzfError) if rc else contextlib.nullcontext():
            assert bam.read_bgzf(f) == b""


def test_sizing_caps_and_refused_tables(want):
    f = want["files"][1]
    _, block_off, out_off, _ = ic.walk(f)
    n, total = len(block_off) - 1, out_off[-1]
    d_in = shifted_from(f, 2)
    d_b, d_o = (torch.full((n + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    nb, ob, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = _lib.lib().bg_bgzf_blocks_dev(_lib.default_context().h, d_in.data_ptr(), len(f), d_b.data_ptr(), d_o.data_ptr(), n - 1, C.byref(nb), C.byref(ob),
                                       C.byref(bad), stream())
    assert (rc, nb.value, ob.value) == (ic.OPS_CAP, n, total) and bool((d_b == -1).all()) and bool((d_o == -1).all())
    # inflate: one byte short of out_off[n_blocks]; tables that are not ascending, leave the input, or hold too large a range
    d_out = shifted(total, 5, fill=0x5A)
    d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")

    def call(bo, oo, cap, in_bytes=len(f)):
        d_b, d_o = table(bo), table(oo)
        bam.bgzf_inflate_dev(d_in.data_ptr(), in_bytes, n, d_b.data_ptr(), d_o.data_ptr(), d_out.data_ptr(), cap, d_status.data_ptr(), stream())
    with pytest.raises(_lib.BiogpuError) as e:
        call(block_off, out_off, total - 1)
    assert e.value.status == ic.OPS_CAP
    swapped = list(block_off)
    swapped[5], swapped[6] = swapped[6], swapped[5]
    wide = [0 if b < 9 else o + 65536 for b, o in enumerate(out_off)]  # block 8 gets more than 65 536 bytes
    back = list(out_off)
    back[4] = back[3] - 1
    short = [o if b < 3 else o - (block_off[3] - block_off[2] - 27) for b, o in enumerate(block_off)]  # member 2 is 27 bytes long
    for bo, oo, in_bytes, row in ((swapped, out_off, len(f), 5), (block_off, out_off, len(f) - 1, n - 1), (block_off, wide, len(f), 8),
                                  (block_off, back, len(f), 3), (short, out_off, len(f), 2)):
        with pytest.raises(bam.BgzfError) as e:
            call(bo, oo, total + 65536, in_bytes)
        assert (e.value.status, e.value.block) == (-1, row)
    torch.cuda.synchronize()
    assert bool((d_out == 0x5A).all()) and bool((d_status == 0xEE).all()) and guards_intact(d_out)  # nothing was written by any of them
    call(block_off, out_off, total)
    assert d_out.cpu().numpy().tobytes() == want["cpu_files"][1][8] and not bool(d_status.any())


def test_host_flavours_and_the_error_they_raise(want):
    f = want["files"][0]
    _, block_off, out_off, _ = ic.walk(f)
    got_b, got_o = bam.bgzf_blocks_arrays(f)
    assert got_b.tolist() == block_off and got_o.tolist() == out_off
    out, status = bam.bgzf_inflate_arrays(f, got_b, got_o)
    assert out == want["cpu_files"][0][8] == bam.read_bgzf(f) and not status.any()
    assert bam.read_bgzf(b"") == b"" and bam.read_bgzf(ic.EOF_BLOCK) == b""
    mixed = want["mixed"]
    with pytest.raises(bam.BgzfError) as e:
        bam.read_bgzf(mixed)
    first = want["hand"][0]
    assert (e.value.status, e.value.block, e.value.offset, e.value.inflate_status) == (-1, 1, len(want["good"][3][1]), first[2])
    assert first[2] == ic.BAD_DISTANCE and bam.INFLATE_STATUS[first[2]] == "bad distance"

"""The `__host__ __device__` bodies behind bg_bgzf_blocks and bg_bgzf_inflate (csrc/bgzf_inflate_rule.h: the verdict on a member,
the bit reader, the code sets and their legality, both table levels, the token queue and its copies, the stored copy, the
CRC-32 shares) run on the CPU by a stand-alone program (tests/bgzf_inflate_host_bodies.cpp: lanes 0 .. 63 in turn wherever the
kernel has a barrier; the working set, every member and every output range exact-size heap buffers) built with
AddressSanitizer and UBSan.  Nothing is loaded into Python.

Good members (tests/bgzf_inflate_cases.py): every payload of the deflate tests and the cut BAM-like body through zlib levels
0, 1, 6, 9; memLevel 1 and 8 under the default, Z_FIXED, Z_HUFFMAN_ONLY and Z_RLE strategies; Z_SYNC_FLUSH in the middle;
empty members (also one file with them in front, in the middle and at the end); 65 536 bytes in one member; fake member headers inside stored payloads.  Each must come out as the bytes that
went in, and the table of a file must be the Python walk over BSIZE.
Hand-made members stand between two good ones: the status is the one the rule names, accept / reject is zlib's at test time,
the neighbours' payloads are intact.  2 000 single-byte corruptions must get exactly zlib-plus-trailer's accept / reject."""
import pytest

import bgzf_inflate_cases as ic

FILE_BLOCKS = 60


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("inf")
    exe = ic.build_program(str(tmp / "bodies"), sanitize=True)
    good = ic.good_members()
    hand = ic.hand_made()
    bad = ic.bad_files()
    corrupt = ic.corruptions()
    a, b = good[3][1], good[40][1]
    files = [b"".join(m for _, m, _ in good[k:k + FILE_BLOCKS]) for k in range(0, len(good), FILE_BLOCKS)]
    files += [a + m + b for _, m, _ in hand] + [f for _, f, _, _ in bad] + [b"".join(m for _, m, _ in ic.empty_member_file())]
    got_files, got_members = ic.run_program(exe, tmp, files, [(m, ic.range_of(m)) for m in corrupt])
    n_good = (len(good) + FILE_BLOCKS - 1) // FILE_BLOCKS
    return dict(good=good, hand=hand, bad=bad, corrupt=corrupt, files=files, good_files=got_files[:n_good],
                hand_files=got_files[n_good:n_good + len(hand)], bad_files=got_files[n_good + len(hand):-1], empty_file=got_files[-1], members=got_members, a=good[3], b=good[40])


def test_good_members_give_their_payloads_and_the_walks_table(ran):
    good = ran["good"]
    for k, got in enumerate(ran["good_files"]):
        part = good[k * FILE_BLOCKS:(k + 1) * FILE_BLOCKS]
        rc, block_off, out_off, _ = ic.walk(ran["files"][k])
        assert rc == 0 and got[0] == 0 and got[1] == len(part) and got[3] == ic.NONE
        assert got[4] == block_off and got[5] == out_off and got[2] == out_off[-1]
        assert got[7] == ic.NONE and got[6] == [0] * len(part), [name for (name, _, _), s in zip(part, got[6]) if s]
        for (name, _, data), o0, o1 in zip(part, out_off, out_off[1:]):
            assert got[8][o0:o1] == data, name


def test_empty_members_in_front_in_the_middle_and_at_the_end(ran):
    part, got = ic.empty_member_file(), ran["empty_file"]
    rc, block_off, out_off, _ = ic.walk(ran["files"][-1])
    assert rc == 0 and out_off[0] == out_off[1] == out_off[2] == 0 and out_off[-1] == out_off[-2] == out_off[-3]  # empty at both ends
    assert got[:4] == (0, len(part), out_off[-1], ic.NONE) and got[4] == block_off and got[5] == out_off
    assert got[6] == [0] * len(part) and got[7] == ic.NONE and got[8] == b"".join(d for _, _, d in part)


def test_hand_made_members_between_two_good_ones(ran):
    (_, _, da), (_, _, db) = ran["a"], ran["b"]
    seen = set()
    for (name, m, status), got in zip(ran["hand"], ran["hand_files"]):
        want = ic.verdict(m)
        assert got[0] == 0 and got[1] == 3, name
        assert got[6] == [0, status, 0], (name, got[6])
        assert (status == ic.OK) == (want is not None), name  # zlib's accept / reject
        assert got[7] == (ic.NONE if status == ic.OK else 1), name
        o = got[5]
        assert got[8][:o[1]] == da and got[8][o[2]:] == db, name
        if want is not None:
            assert got[8][o[1]:o[2]] == want, name
        seen.add(status)
    assert seen == set(range(10))  # every status of the enum


def test_single_byte_corruptions_get_zlibs_verdict(ran):
    accepted = 0
    for m, (status, out) in zip(ran["corrupt"], ran["members"]):
        want = ic.verdict(m)
        assert (status == ic.OK) == (want is not None)
        if want is not None:
            assert out == want
            accepted += 1
    print("%d of %d corrupted members are accepted by zlib and the trailer" % (accepted, len(ran["corrupt"])))


def test_the_walk_names_the_first_offending_member(ran):
    for (name, f, rc, first_bad), got in zip(ran["bad"], ran["bad_files"]):
        assert (got[0], got[3]) == (rc, first_bad), name
        assert (got[0], got[3]) == (ic.walk(f)[0], ic.walk(f)[3]), name
        if rc == 0:
            assert got[1] == (1 if f else 0) and got[2] == 0, name

"""The `__host__ __device__` bodies behind bg_bgzf_deflate (csrc/bgzf_deflate_rule.h: matches, the parse, Huffman code lengths
under a limit, the three encodings and the choice between them, the bits) run on the CPU by a stand-alone program
(tests/bgzf_deflate_host_bodies.cpp: every phase of a block for lane 0 .. 255 in turn, every array an exact-size heap buffer)
built with AddressSanitizer and UBSan.  Nothing is loaded into Python.

Every block: the gzip header and BSIZE, zlib inflates the raw deflate stream to exactly the payload, reaches the end and leaves
the 8 trailer bytes, which are zlib's CRC-32 and the length; the block is at most len + 31 bytes.

Random payloads and the stored fallback.  The encoding is the smallest by exact bit count, stored winning a tie, and a stored
block is bam_oracle.block(data).  For the random payloads of 257 bytes and more stored must win: a byte costs at least
log2(256) - (a few hundredths) bits under any prefix code fitted to them while the dynamic header alone costs hundreds of
bits, and the fixed codes spend 9 bits on every byte above 143.  For the random payloads of 1 .. 4 bytes it cannot: the fixed
encoding is 3 + 7 + at most 9 bits a byte = at most 46 bits against the stored 8 * (len + 5) >= 48.  Those are asserted to be
the fixed encoding of exactly that many bits (and to pass every check above); the larger ones to equal bam_oracle.block.

Compression does both halves of its work: on ~700 BAM-like records (4 blocks) the total must be below zlib level 1 with
Z_FIXED (matches, no fitted codes) and below zlib level 1 with Z_HUFFMAN_ONLY (fitted codes, no matches), both computed at
test time.  The ratio to zlib level 1 itself is printed, not asserted."""
import zlib

import pytest

import bam_oracle as bo
import bgzf_deflate_cases as dc

STORED, FIXED, DYNAMIC = 0, 1, 2


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dfl")
    exe = dc.build_program(str(tmp / "bodies"), sanitize=True)
    named = dc.payloads()
    body = dc.bam_like()
    cut = [body[a:a + dc.P] for a in range(0, len(body), dc.P)]
    lens, blocks = dc.run_program(exe, tmp, dc.limiter_cases(), [d for _, d in named] + cut)
    return named, blocks[:len(named)], cut, blocks[len(named):], lens


def test_every_block_inflates_to_its_payload(ran):
    named, blocks, cut, cut_blocks, _ = ran
    for (name, data), (block, mode, cost) in zip(named, blocks):
        dc.check_block(block, data, name)
        assert cost[mode] == min(cost) and mode == cost.index(min(cost)), (name, mode, cost)  # stored wins a tie, then fixed
    for data, (block, _, _) in zip(cut, cut_blocks):
        dc.check_block(block, data, "BAM-like")


def test_stored_fallback_and_small_outputs(ran):
    named, blocks, _, _, _ = ran
    by_name = {name: (data, got) for (name, data), got in zip(named, blocks)}
    for n in dc.LENGTHS:
        data, (block, mode, cost) = by_name["random %d" % n]
        if n >= 257:
            assert mode == STORED and block == bo.block(data), n
        else:  # the fixed codes are strictly shorter (module docstring)
            assert mode == FIXED and cost[FIXED] == 3 + 7 + sum(8 if b < 144 else 9 for b in data) < cost[STORED] == 8 * (n + 5), n
    data, (block, mode, _) = by_name["zeros %d" % dc.P]
    assert len(block) <= 1024 and mode != STORED  # 253 matches of 258 under the fixed codes: 412 bytes and 26 of framing
    for period in dc.PERIODS[:5]:
        assert len(by_name["period %d" % period][1][0]) < dc.P // 3, period  # 2 bits a base even without a match
    # the limiter at work inside a block: 22 symbols whose unlimited tree is 21 deep
    data, (block, mode, _) = by_name["fibonacci counts"]
    assert mode == DYNAMIC


def test_length_limiter(ran):
    lens = ran[4]
    for (counts, limit), got in zip(dc.limiter_cases(), lens):
        used = [l for c, l in zip(counts, got) if c]
        assert all((c > 0) == (l > 0) for c, l in zip(counts, got)) and max(got) <= limit
        kraft = sum(2.0 ** -l for l in used)
        assert kraft <= 1 and (len(used) < 2 or kraft == 1), (counts, got)
        # rarer symbols never get shorter codes
        order = sorted((c, l) for c, l in zip(counts, got) if c)
        assert all(a[1] >= b[1] for a, b in zip(order, order[1:]) if a[0] < b[0]), (counts, got)
    assert max(lens[0]) == 15 and max(lens[1]) == 7 and sum(lens[2]) == 1


def test_matches_and_fitted_codes_both_work(ran):
    _, _, cut, cut_blocks, _ = ran
    assert len(cut) == 4 and 200_000 < sum(map(len, cut)) < 230_000

    def deflated(data, strategy):
        z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, strategy)
        return len(z.compress(data) + z.flush())
    total = sum(map(len, cut))
    ours = sum(len(b) - 26 for b, _, _ in cut_blocks)  # the deflate streams alone
    level1, fixed, huffman = (sum(deflated(d, s) for d in cut) for s in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY))
    print("BAM-like body, %d bytes: ours %.3f, zlib level 1 %.3f, Z_FIXED %.3f, Z_HUFFMAN_ONLY %.3f of the input; ours / level 1 = %.3f"
          % (total, ours / total, level1 / total, fixed / total, huffman / total, ours / level1))
    assert level1 < huffman and level1 < fixed  # the ordering the two bounds rest on
    assert ours < fixed and ours < huffman

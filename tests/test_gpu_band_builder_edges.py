"""The device band builder (rust-bio_amd/csrc/band_device.hip) on the pairs of tests/band_edge_cases.py: match counts on
its caps, 32 / 33 matches of one k-mer, no matches at every buffer alignment, reads around the raster tile, a long pair
on either side of each k-mer join's size limit, sub-batches of handed-over pairs only, 1023 / 1024 pairs.

Every run is compared with the host builder (band_on_host = 1) on the same pairs — Band::num_cells, every record field,
every operation — and the host builder with the oracle on the same pairs in tests/test_band_edge_cases.py.  Both builders
give the same band, so that comparison alone cannot tell a device builder that hands a pair back one match early or
late, or every pair: the number of pairs rebuilt on the host is read from the BG_TRACE lines of the call and must equal
the number the oracle's match counts give, exactly."""
import re

import numpy as np
import pytest

import band_edge_cases as ec
import oracle_py as orc
from rust_bio_amd import _lib
from rust_bio_amd.banded import Aligner
from rust_bio_amd.pairwise import Scoring

pytestmark = pytest.mark.gpu

MODE = 2  # semiglobal, the benchmark's
REBUILT = re.compile(r"^\[bg banded\] (\d+) of (\d+) pairs rebuilt on the host$", re.M)
DEFAULTS = {"band_on_host": 0, "band_chain_global": -1, "band_chain_rows": 1, "band_join_global": 0, "chunk_pairs": 0}
FIELDS = [f for f in _lib.ALN_DTYPE.names if not f.startswith("_")]
# the chain tree's placements the existing builder test runs: LDS, global with four pairs per wavefront, global with one
CHAINS = {"lds-tree": {"band_chain_global": 0}, "global-rows": {"band_chain_global": 1, "band_chain_rows": 1},
          "global-single": {"band_chain_global": 1, "band_chain_rows": 0}}


class Batch:
    def __init__(self, pairs, k=ec.K, w=ec.W):
        self.pairs, self.k, self.w = pairs, k, w
        self.x, self.xo = _lib.concat([p.x for p in pairs])
        self.y, self.yo = _lib.concat([p.y for p in pairs])
        self.al = Aligner.with_scoring(Scoring.from_scores(-5, -1, 1, -1), k, w)
        self.host = None

    def run(self, capfd, opts):
        """one call under `opts` -> (records, operations, cells, pairs rebuilt on the host, stderr of the call)"""
        ctx = self.al.ctx
        try:
            for key, value in opts.items():
                ctx.set_option(key, value)
            capfd.readouterr()
            out, ops = self.al.align_arrays(MODE, self.x, self.xo, self.y, self.yo)
            err = capfd.readouterr().err
        finally:
            for key in opts:  # (the default ctx is shared)
                ctx.set_option(key, DEFAULTS[key])
        return out.copy(), ops.copy(), self.al.last_cells.copy(), sum(int(a) for a, _ in REBUILT.findall(err)), err

    def host_run(self, capfd):
        if self.host is None:
            out, ops, cells, rebuilt, err = self.run(capfd, {"band_on_host": 1})
            assert rebuilt == 0 and (out["status"] == 0).all()
            self.host = (out, ops, cells)
        return self.host

    def device_run(self, capfd, opts, same_sub_batches=True):
        """the device builder under `opts` against the host builder -> pairs rebuilt on the host"""
        out_h, ops_h, cells_h = self.host_run(capfd)
        out_d, ops_d, cells_d, rebuilt, err = self.run(capfd, dict(opts, band_on_host=0))
        assert "band build (device)" in err, err  # the trace is on: no line about rebuilt pairs means none was
        assert_same_records((out_d, ops_d, cells_d), (out_h, ops_h, cells_h), opts, ops_off=same_sub_batches)
        return rebuilt


def assert_same_records(got, want, what, ops_off=True, n=None):
    """cells, every field of the records and every operation of the first n pairs (operations and clip lengths are what
    decode_ops reads).  ops_off: the operations lie in the order the sub-batches ran, compared only between equal splits."""
    (out_g, ops_g, cells_g), (out_w, ops_w, cells_w) = got, want
    n = len(out_w) if n is None else n
    assert (cells_g[:n] == cells_w[:n]).all(), what
    for f in FIELDS:
        if f != "ops_off" or ops_off:
            assert np.array_equal(out_g[f][:n], out_w[f][:n]), (what, f, np.flatnonzero(out_g[f][:n] != out_w[f][:n])[:8])
    for p in range(n):
        k_, a, b = int(out_w["n_ops"][p]), int(out_g["ops_off"][p]), int(out_w["ops_off"][p])
        assert np.array_equal(ops_g[a:a + k_], ops_w[b:b + k_]), (what, p)


def n_handed(pairs):
    """what tests/test_band_edge_cases.py proves the kinds to mean at k = 16"""
    return sum(p.kind == "handed" for p in pairs)


@pytest.fixture(scope="module")
def short():
    return Batch(ec.short_batch())


@pytest.fixture(autouse=True)
def _trace(monkeypatch):
    monkeypatch.setenv("BG_TRACE", "1")  # read inside every call


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("join", ["lds-join", "global-join"])
def test_short_batch_under_both_joins_and_three_chain_placements(short, capfd, join, chain):
    """4095 / 4096 matches, 2047 / 2048 (the LDS tree's size classes), 32 / 33 matches of one k-mer, no matches at every
    residue of x and y, reads of one, two and three raster tiles: one sub-batch of 129 pairs"""
    assert n_handed(short.pairs) == 35
    opts = dict(CHAINS[chain], band_join_global=1 if join == "global-join" else 0)
    assert short.device_run(capfd, opts) == n_handed(short.pairs)


@pytest.mark.parametrize("length", ec.LONG_L)
def test_short_batch_with_a_long_pair_on_each_join_limit(short, capfd, length):
    """The longest pair of a sub-batch selects its join: the LDS join at its largest size (20 128), the staged global
    join (20 129), the same at its largest size (20 464), the unstaged one (20 465).  The 129 pairs in front get the same
    records from each, and as many of them are rebuilt."""
    batch = Batch(short.pairs + [ec.long_pair(length)])
    assert ec.join_flavour(int(np.diff(batch.xo).max()), int(np.diff(batch.yo).max())) == ec.LONG_FLAVOUR[length]
    for chain, opts in CHAINS.items():
        assert batch.device_run(capfd, opts) == n_handed(short.pairs), (length, chain)
    assert_same_records(batch.host_run(capfd), short.host_run(capfd), length, n=len(short.pairs))


@pytest.mark.parametrize("chunk", [4, 5])
def test_sub_batches_pick_their_flavours_one_by_one(short, capfd, chunk):
    """Sub-batches of 4 and 5 pairs, the remainder first: one of handed-over pairs only, one without any, the long-list
    and the 4096-match pairs spread over the others"""
    subs = ec.sub_batches(len(short.pairs), chunk)
    handed = [n_handed(short.pairs[p0:p0 + want]) for p0, want in subs]
    assert subs[0][1] == len(short.pairs) % chunk != 0
    assert any(h == want for h, (_, want) in zip(handed, subs)) and 0 in handed
    assert short.device_run(capfd, {"chunk_pairs": chunk}, same_sub_batches=False) == n_handed(short.pairs)


def test_device_resident_entry(short, capfd):
    import torch
    out_h, ops_h, cells_h = short.host_run(capfd)
    dev = torch.device("cuda:0")
    dx, dy = torch.from_numpy(short.x.copy()).to(dev), torch.from_numpy(short.y.copy()).to(dev)
    dxo, dyo = torch.from_numpy(short.xo.astype(np.int64)).to(dev), torch.from_numpy(short.yo.astype(np.int64)).to(dev)
    n = len(short.pairs)
    stride = int(np.diff(short.xo).max() + np.diff(short.yo).max()) + 8
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_ops = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    capfd.readouterr()
    cells = short.al.align_dev(MODE, n, dx.data_ptr(), dxo.data_ptr(), dy.data_ptr(), dyo.data_ptr(), d_out.data_ptr(),
                               d_ops.data_ptr(), stride, want_cells=True)
    err = capfd.readouterr().err
    rec = d_out.cpu().numpy().view(_lib.ALN_DTYPE)
    assert (rec["ops_off"] == (np.arange(n, dtype=np.uint64) + 1) * stride - rec["n_ops"]).all()
    assert_same_records((rec, d_ops.cpu().numpy(), cells), (out_h, ops_h, cells_h), "align_dev", ops_off=False)
    assert "band build (device)" in err and sum(int(a) for a, _ in REBUILT.findall(err)) == n_handed(short.pairs)


@pytest.mark.parametrize("n_pairs", [ec.CHAIN_GLOBAL_MIN_PAIRS - 1, ec.CHAIN_GLOBAL_MIN_PAIRS])
def test_tree_placement_switches_at_1024_pairs(capfd, n_pairs):
    """default options: the LDS tree for 1023 pairs, the global one for 1024.  No pair is near a cap: none is rebuilt."""
    batch = Batch(ec.many_small_pairs(n_pairs))
    assert batch.device_run(capfd, {}) == 0


def test_short_batch_k8_w6(short, capfd):
    """k below 16: the LDS join compares a candidate's first 16 bytes under a mask that is not all ones.  Random 8-mers
    repeat: other pairs than at k = 16 exceed 4095 matches, counted with the oracle."""
    batch = Batch(short.pairs, 8, 6)
    want = sum(ec.handed_over(*ec.match_stats(orc.find_kmer_matches, p.x, p.y, 8)) for p in batch.pairs)
    assert 0 < want < len(batch.pairs)
    for join_global in (0, 1):
        assert batch.device_run(capfd, {"band_join_global": join_global}) == want, join_global

"""bench.py's one JSON line on a scaled-down workload: the driver's contract (metric / value / unit / n_gpus / steps /
warmup / ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config.workload); with --full also the
`roofline` and `cpu_baseline` objects of the tier brief, a leg for every BASELINE config (configs[1] headline, [2] fm, [3]
banded, [4] seed_extend — each with its strong variant where the config is multi-GPU), and every parity flag true."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_contract_fields(d, steps, warmup):
    for k, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                   ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str)):
        assert isinstance(d[k], typ), k
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup and d["vs_baseline"] is None
    assert d["scaling"] == "weak" and "workload" in d["config"] and "model" not in d["config"]


def test_plain_line_is_the_headline_alone():
    """Without --full the run times the headline and prints its line: no other leg, no roofline, no CPU leg."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--pairs", "20000"]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [ln for ln in out.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "rank 0 prints ONE JSON line"
    d = json.loads(lines[0])
    assert_contract_fields(d, steps=3, warmup=2)
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "GCUPS" and d["dtype"] == "int16"
    assert d["config"]["pairs_per_gpu"] == 20000
    assert set(d) == {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                      "vs_baseline", "dtype", "data", "config"}, sorted(d)


def test_bench_line_has_the_contract_fields_and_green_parity():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--pairs", "20000",
           "--k1-pairs", "4096", "--genome", "300000", "--fm-big-genome", "400000", "--queries", "20000", "--banded-pairs", "70",
           "--banded-parity-pairs", "70", "--pipeline-reads", "3000", "--pipeline-reads-total", "4001", "--ingest-reads", "3000",
           "--fmd-genome", "200000", "--fmd-reads", "2000"]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [ln for ln in out.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "rank 0 prints ONE JSON line"
    d = json.loads(lines[0])
    assert_contract_fields(d, steps=2, warmup=1)
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert "traffic" in r and r["peak"] == 8000.0
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
    # the other BASELINE configs, each with roofline + cpu_baseline + its strong variant
    for leg in ("fm", "fm_big", "seed_extend", "banded", "fmd_smems"):
        assert d[leg]["value"] > 0 and "roofline" in d[leg] and "cpu_baseline" in d[leg], leg
    assert d["fm"]["strong"]["queries_total"] == 20000 and d["banded"]["strong"]["pairs_total"] == 70
    assert d["seed_extend"]["strong"]["reads_total"] == 4001 and d["seed_extend"]["strong"]["gathered_records"] == 4001
    assert d["value_int32"] > 0 and d["int32"]["records_and_ops_equal_int16_run"] is True
    sg = d["semiglobal"]  # north_star: Aligner::local / semiglobal
    assert sg["value"] > 0 and sg["roofline"]["frac"] > 0 and sg["cpu_baseline"]["value"] > 0 and d["parity"]["semiglobal_bit_exact"] is True
    assert d["packed2"]["records_and_ops_equal_byte_run"] is True and d["fm"]["packed2"]["results_equal_byte_run"] is True
    assert d["fm"]["roofline"]["requested_lines_per_launch"] > 0
    flags = {k: v for k, v in d["parity"].items() if isinstance(v, bool)}
    assert len(flags) >= 10 and all(flags.values()), flags


def test_dump_outputs_hold_the_headline_results(tmp_path):
    """--dump-outputs DIR: after `--steps` timed steps, DIR holds the headline step's records and operations as float .npy
    files, and they are the oracle's for the bench's own pairs (below 65536 pairs synth_gpu.sw_pairs_big makes exactly
    synth.sw_pairs(n, L, seed=2); every pair is dumped below 131072)."""
    import numpy as np

    import oracle_py as orc
    from rust_bio_amd import synth

    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    n, L, dump = 3000, 150, tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pairs", str(n),
           "--read-len", str(L), "--skip-cpu", "--skip-packed", "--skip-k1", "--skip-semiglobal", "--skip-fm", "--fm-big-genome", "0",
           "--skip-fmd", "--skip-banded", "--skip-ingest", "--skip-pipeline", "--dump-outputs", str(dump)]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    d = json.loads([ln for ln in out.stdout.decode().splitlines() if ln.startswith("{")][0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    a = {nm: np.load(dump / (nm + ".npy")) for nm in ("sw_pairs", "sw_records", "sw_ops_pairs", "sw_ops")}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert (a["sw_pairs"] == np.arange(n)).all() and (a["sw_ops_pairs"] == np.arange(n)).all()
    rec, ops = a["sw_records"], a["sw_ops"]
    stride = 2 * L + 4
    assert rec.shape == (n, 16) and ops.shape == (n, stride)
    x, xo, y, yo = synth.sw_pairs(n, L, seed=2)
    oout, oops, ostride = orc.align_batch(orc.make_scoring(-5, -1, 1, -1), "local", x, xo, y, yo)
    # columns: score xstart xend ystart yend xlen ylen n_ops ops_off clip_len[4] n_clips mode status
    for col, f in ((0, "score"), (1, "xstart"), (2, "xend"), (3, "ystart"), (4, "yend"), (7, "n_ops")):
        assert (rec[:, col] == oout[f].astype(np.float64)).all(), f
    kq = rec[:, 7].astype(np.int64)
    assert (rec[:, 8] == (np.arange(n) + 1) * stride - kq).all()
    assert ((ops >= 0).sum(axis=1) == kq).all()
    kind = (oops.reshape(n, ostride) & np.uint64(0xFF)).astype(np.float32)
    for p in range(n):
        assert (ops[p, stride - kq[p]:] == kind[p, :kq[p]]).all(), p

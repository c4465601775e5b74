"""One SHA-256 per case over what the banded pipeline returns (records, operations, band_cells), for comparing two builds of
the library bit by bit: python tools/exp/banded_identity.py <lib.so>
Cases: the three entry points x device / host band builder x chunk_pairs 0 / 16 / 32 x band_budget_gb 0 / 1 x band_fill_v1
-1 / 0 / 1 over two small batches (ragged 150-700 bp with free y clips; 1.5 kb semiglobal, which takes the interior runs),
a tabulated match function, and a 2 048-pair and a 2 049-pair call either side of the small-batch rule."""
import hashlib, itertools, os, sys
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
import numpy as np
import torch
torch.cuda.init()
from rust_bio_amd import _lib
_lib.SO_PATH = os.path.abspath(sys.argv[1])
from rust_bio_amd import synth
from rust_bio_amd.banded import Aligner
from rust_bio_amd.pairwise import MIN_SCORE, Scoring

dev = torch.device("cuda:0")
ctx = _lib.Context(0)
OPTS = ("band_on_host", "chunk_pairs", "band_budget_gb", "band_fill_v1")


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run(al, mode, entry, x, xo, y, yo):
    if entry == "host":
        out, ops = al.align_arrays(mode, x, xo, y, yo)
        return digest(out, ops[:int((out["n_ops"]).sum())], al.last_cells)
    if entry == "bands":
        bo, bs, be, _ = al.band_create_arrays(mode, x, xo, y, yo)
        out, ops = al.align_bands_arrays(mode, x, xo, y, yo, bo, bs, be)
        return digest(out, ops[:int((out["n_ops"]).sum())], al.last_cells)
    P = len(xo) - 1
    stride = int(np.diff(xo).max() + np.diff(yo).max()) + 8
    dx, dy = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(y)).to(dev)
    dxo, dyo = torch.from_numpy(xo.astype(np.int64)).to(dev), torch.from_numpy(yo.astype(np.int64)).to(dev)
    d_out = torch.zeros(P * 64, dtype=torch.uint8, device=dev)
    d_ops = torch.zeros(P * stride, dtype=torch.uint8, device=dev)
    cells = al.align_dev(mode, P, dx.data_ptr(), dxo.data_ptr(), dy.data_ptr(), dyo.data_ptr(), d_out.data_ptr(), d_ops.data_ptr(),
                         stride, want_cells=True)
    return digest(d_out.cpu().numpy(), d_ops.cpu().numpy(), cells)


def case(name, al, mode, entry, data, **opts):
    for k in OPTS:
        ctx.set_option(k, opts.get(k, 0))
    print("%-64s %s" % (name, run(al, mode, entry, *data)), flush=True)


rag = Scoring.from_scores(-5, -1, 1, -1)
rag.xclip_prefix = rag.xclip_suffix = MIN_SCORE
rag.yclip_prefix = rag.yclip_suffix = 0
xs, ys = synth.ragged_pairs(70, 700, seed=4711, min_len=150)
sx, so, sy, _ = synth.sw_pairs(96, 1500, seed=21, sub=0.06, ins=0.02, dele=0.02)
BATCHES = {
    "ragged70": (Aligner.with_scoring(rag, 9, 11, ctx=ctx), 0, _lib.concat(xs) + _lib.concat(ys)),
    "semi96": (Aligner.with_scoring(Scoring.from_scores(-5, -1, 1, -1), 12, 16, ctx=ctx), 2, (sx, so, sy, so)),
}
for b, (al, mode, data) in BATCHES.items():
    for entry, on_host in (("host", 0), ("host", 1), ("dev", 0), ("dev", 1), ("bands", 1)):
        for chunk, budget, v1 in itertools.product((0, 16, 32), (0, 1), (-1, 0, 1)):
            case("%s %s %s-builder chunk=%d budget=%d fill_v1=%d" % (b, entry, "host" if on_host else "device", chunk, budget, v1),
                 al, mode, entry, data, band_on_host=on_host, chunk_pairs=chunk, band_budget_gb=budget, band_fill_v1=v1)

# a tabulated match function (transitions cost less than transversions)
m = np.full((256, 256), -3, dtype=np.int32)
for a_, b_ in ("AG", "GA", "CT", "TC"):
    m[ord(a_), ord(b_)] = -1
m[np.arange(256), np.arange(256)] = 2
mat = Scoring(-6, -1, m, None)
mat.xclip_prefix = mat.xclip_suffix = MIN_SCORE
mat.yclip_prefix = mat.yclip_suffix = 0
for entry, chunk in itertools.product(("host", "dev"), (0, 16)):
    case("matrix ragged70 %s chunk=%d" % (entry, chunk), Aligner.with_scoring(mat, 9, 11, ctx=ctx), 0, entry, BATCHES["ragged70"][2],
         chunk_pairs=chunk)

# either side of the small-batch rule (2 048 pairs: K3; 2 049: K3v2 / K3p)
bx, bo, by, _ = synth.sw_pairs(2049, 300, seed=5, sub=0.06, ins=0.02, dele=0.02)
al = Aligner.with_scoring(Scoring.from_scores(-5, -1, 1, -1), 10, 12, ctx=ctx)
for P, entry in itertools.product((2048, 2049), ("host", "dev")):
    case("%d pairs x 300 bp %s" % (P, entry), al, 2, entry, (bx[:int(bo[P])], bo[:P + 1], by[:int(bo[P])], bo[:P + 1]))
    print("%-64s %s" % ("  fill kernels", sorted(k for k, v in _lib.FILL.items() if ctx.last_fill_kernels() & v)), flush=True)

"""Wall time of the bg_fm_build call alone (host BWT -> finished index) and of bg_fm_build_dev on a device copy of the same
bytes, for one or several builds of the library loaded side by side and called in turn:
python tools/exp/time_fm_build.py <lib.so> [<other lib.so> ...] [--sizes 65536,16777216,1073741824] [--runs 6]
The input is random ACGT bytes with one '$' at the end and `less` from a bincount (the builder does not need a true BWT).
Prints every run, then per size, entry point and library the median and the spread (max - min); with two libraries, whether
the second one's median stays within the first one's median + spread."""
import ctypes as C, os, statistics, sys, time
import numpy as np
import torch

args = sys.argv[1:]
sizes, runs = [1 << 16, 1 << 24, 1 << 30], 6
if "--sizes" in args:
    sizes = [int(s) for s in args[args.index("--sizes") + 1].split(",")]
if "--runs" in args:
    runs = int(args[args.index("--runs") + 1])
paths = [os.path.abspath(a) for a in args if a.endswith(".so")]
ALPHA = np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)
vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32


def load(path):
    L = C.CDLL(path)
    L.bg_init.argtypes = [C.c_int, C.POINTER(vp)]
    L.bg_fm_build.argtypes = [vp, vp, u64, vp, u32, u32, vp, u32, C.POINTER(vp)]
    L.bg_fm_build_dev.argtypes = [vp, vp, u64, u32, vp, u32, vp, C.POINTER(vp), vp]
    L.bg_fm_free.argtypes = [vp]
    ctx = vp()
    assert L.bg_init(0, C.byref(ctx)) == 0
    return L, ctx


def build(L, ctx, b, ls):
    h = vp()
    t0 = time.perf_counter()
    rc = L.bg_fm_build(ctx, b.ctypes.data, len(b), ls.ctypes.data, len(ls), 128, ALPHA.ctypes.data, len(ALPHA), C.byref(h))
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    L.bg_fm_free(h)
    return dt * 1e3


def build_dev(L, ctx, d_b):
    h = vp()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = L.bg_fm_build_dev(ctx, d_b.data_ptr(), d_b.numel(), 128, ALPHA.ctypes.data, len(ALPHA), None, C.byref(h), None)
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    L.bg_fm_free(h)
    return dt * 1e3


torch.cuda.init()
libs = [load(p) for p in paths]
letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda:0")
stats = {}
for n in sizes:
    g = torch.Generator(device="cuda:0").manual_seed(n)
    d_b = letters[torch.randint(0, 4, (n,), device="cuda:0", generator=g)]
    d_b[n - 1] = ord("$")
    b = d_b.cpu().numpy()
    ls = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=int(ALPHA.max()) + 1))]).astype(np.uint64)
    for k, (L, ctx) in enumerate(libs):  # untimed: code objects, the pools of the host threads
        build(L, ctx, b[-4096:], np.concatenate([[0], np.cumsum(np.bincount(b[-4096:], minlength=int(ALPHA.max()) + 1))]).astype(np.uint64))
        build_dev(L, ctx, d_b[-4096:].clone())
    for r in range(runs):
        for k, (L, ctx) in enumerate(libs):
            for entry, ms in (("bg_fm_build", build(L, ctx, b, ls)), ("bg_fm_build_dev", build_dev(L, ctx, d_b))):
                stats.setdefault((n, entry, k), []).append(ms)
                print("n=%d %s lib%d run %d: %.3f ms" % (n, entry, k, r, ms), flush=True)
    del d_b, b
for k, p in enumerate(paths):
    print("lib%d = %s" % (k, p))
for (n, entry, k), v in sorted(stats.items()):
    print("n=%d %-16s lib%d median %.3f ms spread %.3f ms (min %.3f max %.3f)" % (n, entry, k, statistics.median(v), max(v) - min(v), min(v), max(v)))
if len(libs) == 2:
    for n in sizes:
        for entry in ("bg_fm_build", "bg_fm_build_dev"):
            a, c = stats[(n, entry, 0)], stats[(n, entry, 1)]
            bound = statistics.median(a) + max(a) - min(a)
            print("n=%d %-16s lib1 median %.3f ms against lib0 median + spread %.3f ms: %s" % (n, entry, statistics.median(c), bound,
                                                                                            "within" if statistics.median(c) <= bound else "EXCEEDS"))

"""Times ``SyllableIndex.align_sequences`` with one pair split across workgroups (csrc/dtw_strings_split.hip) against the same call
with ``split=False`` (csrc/dtw_strings.hip, one workgroup per pair: the code path from before the split) and writes
profiles/dtw_strings_split_bench.md.

The sequences are stored in an index and the pairs name them, so a call copies no rows: it is the host checks, the pairs' table and
the launches.  Old and new run on the same device-resident pairs in one process and alternate: one warm-up call each, then ``--iters``
rounds of (old, new ...), host clock around a call that ends in a device synchronise; the medians with their min .. max.

1. One pair of ``--long`` x ``--long`` rows, D = 768 and D = 32, without and with the path: ``split=False`` against ``--blocks``.  The
   ideal of a block shape is the one-workgroup time divided by the mean number of blocks per anti-diagonal, ``nbr nbc / (nbr + nbc -
   1)``: every launch as long as one block, no gap between launches, every workgroup on a CU of its own.
2. One pair of 65 536 x ``--long`` rows, split only; the one-workgroup time is extrapolated from (1) by ``m L``.
3. The automatic threshold: one pair of n x n at D = 768, split (default blocks) against not split.
4. ``--pairs`` pairs of 500 x 500 at D = 768 through the default call, where the automatic rule does not engage, against
   ``split=False``: the cost of the host's partitioning.

``box_speed``: the library's 4096^3 bf16 GEMM loop (``sylber_debug_gemm_bench``, tile 97), bench.py's yardstick for the box."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternating(fns, iters):
    """one warm-up call of each, then ``iters`` rounds of every fn in turn -> [(median, min, max) ms]"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(iters):
        for fn, o in zip(fns, out):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            o.append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(o), min(o), max(o)) for o in out]


def fmt(t):
    return "%.2f (%.2f .. %.2f)" % t


def one_pair(g, dev, m, L, D):
    from sylber_amd import SyllableIndex
    return SyllableIndex(torch.randn((m + L, D), generator=g, device=dev), device=dev), np.array([0, m, m + L], np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--long", type=int, default=8192)
    ap.add_argument("--blocks", default="128x128,128x1024,256x256,512x512,1024x1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_strings_split_bench.md"))
    args = ap.parse_args()
    from sylber_amd import SyllableIndex, _lib
    from sylber_amd import search as S
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    shapes = [tuple(int(v) for v in b.split("x")) for b in args.blocks.split(",")]
    n = args.long
    lines = ["# Embedding strings, one pair split across workgroups: one MI355X, one run", "",
             "`python tools/dtw_strings_split_bench.py --iters %d`.  Old = `SyllableIndex.align_sequences(split=False)` (one workgroup per pair), "
             "new = the same call split into blocks, on the same device-resident pair of one index (metric \"l2\", Gaussian rows) in one "
             "process; host clock around a call that ends in a device synchronise, one warm-up call each, then %d rounds of (old, new ...): "
             "the medians with their min .. max.  %d CUs; the defaults in `sylber_amd/search.py`: `SPLIT_BLOCK = %r`, `SPLIT_MIN_CELLS = %d`."
             % (args.iters, args.iters, torch.cuda.get_device_properties(dev).multi_processor_count, S.SPLIT_BLOCK, S.SPLIT_MIN_CELLS), "",
             "## 1. One pair of %d x %d" % (n, n), "",
             "ideal = old / (mean blocks per anti-diagonal = nbr nbc / (nbr + nbc - 1)).", "",
             "| D | path | blocks | launches | mean blocks per diagonal | old ms (min .. max) | new ms (min .. max) | old / new | ideal ms | new / ideal |",
             "|---:|---|---:|---:|---:|---:|---:|---:|---:|---:|"]

    def emit(r):
        print(r, file=sys.stderr, flush=True)
        lines.append(r)

    old768 = None
    for D in (768, 32):
        idx, off = one_pair(g, dev, n, n, D)
        for path in (False, True):
            fns = [lambda: idx.align_sequences([[0, 1]], sequences=off, path=path, split=False)]
            fns += [(lambda b: lambda: idx.align_sequences([[0, 1]], sequences=off, path=path, split=b))(b) for b in shapes]
            ts = alternating(fns, args.iters)
            if D == 768 and not path:
                old768 = ts[0]
            for b, t in zip(shapes, ts[1:]):
                nbr, nbc = -(-n // b[0]), -(-n // b[1])
                mean = nbr * nbc / (nbr + nbc - 1)
                emit("| %d | %s | %d x %d | %d | %.1f | %s | %s | %.1f | %.2f | %.2f |" % (
                    D, "yes" if path else "no", b[0], b[1], nbr + nbc - 1, mean, fmt(ts[0]), fmt(t), ts[0][0] / t[0], ts[0][0] / mean, t[0] / (ts[0][0] / mean)))
        del idx
    lines += ["", "## 2. One pair of 65536 x %d, no path, split only (default blocks)" % n, "",
              "| D | launches | new ms (min .. max) | one workgroup, EXTRAPOLATED from (1) by m L, ms | extrapolated old / new |", "|---:|---:|---:|---:|---:|"]
    idx, off = one_pair(g, dev, 65536, n, 768)
    (t,) = alternating([lambda: idx.align_sequences([[0, 1]], sequences=off, split=True)], args.iters)
    ext = old768[0] * 65536 / n
    emit("| 768 | %d | %s | %.0f | %.1f |" % (-(-65536 // S.SPLIT_BLOCK[0]) + -(-n // S.SPLIT_BLOCK[1]) - 1, fmt(t), ext, ext / t[0]))
    del idx
    lines += ["", "## 3. The automatic threshold: one pair of n x n, D = 768, no path", "",
              "Split wins where its max lies below the unsplit min.", "",
              "| n | old ms (min .. max) | new ms (min .. max) | old / new | split wins beyond the spread |", "|---:|---:|---:|---:|---|"]
    for k in (256, 512, 1024, 2048, 4096):
        idx, off = one_pair(g, dev, k, k, 768)
        told, tnew = alternating([lambda: idx.align_sequences([[0, 1]], sequences=off, split=False),
                                  lambda: idx.align_sequences([[0, 1]], sequences=off, split=True)], args.iters)
        emit("| %d | %s | %s | %.2f | %s |" % (k, fmt(told), fmt(tnew), told[0] / tnew[0], "yes" if tnew[2] < told[1] else "no"))
        del idx
    P = args.pairs
    lines += ["", "## 4. %d pairs of 500 x 500, D = 768, no path: the default call against `split=False`" % P, "",
              "The automatic rule does not engage (more pairs than CUs): the same kernel, plus the host's look at the lengths.", "",
              "| split=False ms (min .. max) | default ms (min .. max) | default / split=False |", "|---:|---:|---:|"]
    idx = SyllableIndex(torch.randn((P * 1000, 768), generator=g, device=dev), device=dev)
    off = np.arange(2 * P + 1, dtype=np.int64) * 500
    pairs = np.arange(2 * P, dtype=np.int64).reshape(P, 2)
    told, tnew = alternating([lambda: idx.align_sequences(pairs, sequences=off, split=False), lambda: idx.align_sequences(pairs, sequences=off)], args.iters)
    emit("| %s | %s | %.3f |" % (fmt(told), fmt(tnew), tnew[0] / told[0]))
    del idx
    ms = ctypes.c_float()
    try:
        torch.cuda.synchronize()
        _lib.check(lib.sylber_debug_gemm_bench(4096, 4096, 4096, 4096, 0, 0, 1000097, 30, ctypes.byref(ms)), "gemm_bench")
        lines += ["", "box_speed: %.1f TFLOP/s on the library's 4096^3 bf16 GEMM loop (tile 97, 30 launches), right after the measurements above."
                  % (2.0 * 4096 ** 3 / (ms.value * 1e-3) / 1e12)]
    except Exception as e:  # noqa: BLE001
        lines += ["", "box_speed: not available (%s: %s)" % (type(e).__name__, e)]
    lines.append("")
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()

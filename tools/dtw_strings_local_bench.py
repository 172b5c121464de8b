"""Times ``SyllableIndex.local_align_sequences`` (csrc/dtw_strings_local.hip) against ``SyllableIndex.align_sequences(path=False)``
(csrc/dtw_strings.hip, the kernel it shares its contraction and its walk with) and writes profiles/dtw_strings_local_bench.md.

The sequences are stored in an index and the pairs name them, so a call copies no rows: it is the host checks, the pairs' table and
one launch.  Old and new run on the same device-resident pairs in one process and alternate: one warm-up call each, then ``--iters``
rounds of (old, new), host clock around a call that ends in a device synchronise; the medians with their min .. max.

1. Round 0: ``--pairs`` pairs of 500 x 500 and of 64 x 512 (every pair its own two sequences of Gaussian rows), D = 768 and D = 32,
   ``n_best = 1``.  At D = 768 the contraction sets the time and the new kernel gets a margin of 1.10 over the old; at D = 32 the
   walk is the whole cost and the ratio is reported without a bar.
2. Cost of a round: the same shapes with 1, 2 and 4 noisy copies of rows of x written into y, ``n_best = 4``.  A pair runs one round
   per repeat it finds and one more that finds nothing, four at most; reported is the time per round run against round 0
   (``n_best = 1``) on the same pairs.
3. One sequence of ``--long`` rows against itself with ``min_sep = 1``, against the same kernel on two such sequences (no band) and
   against the yardstick's pair: the share that the skipped tiles save.

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
MARGIN = 1.10


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


def make_index(g, dev, n, m, L, D, copies):
    """``n`` pairs (2 p, 2 p + 1) of a sequence of m rows and one of L rows; ``copies`` runs of rows of x written into y with a little
    noise, one per slot on both sides and in opposite order, so no path joins two of them"""
    from sylber_amd import SyllableIndex
    rows = torch.randn((n * (m + L), D), generator=g, device=dev)
    if copies:
        sx, sy = m // copies, L // copies
        ln = min(24, sx - 4)
        base = torch.arange(n, device=dev)[:, None, None] * (m + L)
        q = torch.arange(copies, device=dev)[None, :, None]
        r = torch.arange(ln, device=dev)[None, None, :]
        src = (base + q * sx + 2 + r).reshape(-1)
        dst = (base + m + (copies - 1 - q) * sy + 3 + r).reshape(-1)
        rows[dst] = rows[src] + 0.05 * torch.randn((src.numel(), D), generator=g, device=dev)
    off = np.zeros(2 * n + 1, np.int64)
    off[1:] = np.cumsum(np.tile([m, L], n))
    pairs = np.arange(2 * n, dtype=np.int64).reshape(n, 2)
    return SyllableIndex(rows, device=dev), off, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--long", type=int, default=8192, help="rows of the sequence that is aligned against itself")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_strings_local_bench.md"))
    args = ap.parse_args()
    from sylber_amd import SyllableIndex, _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    n = args.pairs
    lines = ["# Embedding strings, local: one MI355X, one run", "",
             "`python tools/dtw_strings_local_bench.py --iters %d`.  Old = `SyllableIndex.align_sequences(path=False)`, new = "
             "`SyllableIndex.local_align_sequences` on the same device-resident pairs of one index (metric \"l2\", Gaussian rows, `radius = "
             "0.75 D`, `gap` and `min_score` at their defaults) in one process; host clock around a call that ends in a device synchronise, "
             "one warm-up call each, then %d rounds of (old, new): the medians with their min .. max." % (args.iters, args.iters), "",
             "Round 0 (`n_best = 1`):", "",
             "| D | pairs | m x L | Mcells | old ms (min .. max) | new ms (min .. max) | new / old | margin |",
             "|---:|---:|---:|---:|---:|---:|---:|---|"]
    rounds = ["", "Cost of a round: the same shapes with noisy copies of 24 rows of x (12 with four copies at m = 64) written into y, `n_best = 4`.  A pair runs one "
              "round per repeat it finds and one more that finds nothing, four at most; rounds run = the mean over the pairs, counted from the "
              "scores.  round 0 = `n_best = 1` on the same pairs.", "",
              "| D | m x L | copies per pair | repeats found per pair | rounds run per pair | n_best = 4 ms (min .. max) | round 0 ms (min .. max) | ms per round run / round 0 ms |",
              "|---:|---:|---:|---:|---:|---:|---:|---:|"]

    def emit(to, r):
        print(r, file=sys.stderr, flush=True)
        to.append(r)

    for D in (768, 32):
        radius = 0.75 * D
        for m, L in ((500, 500), (64, 512)):
            idx, off, pairs = make_index(g, dev, n, m, L, D, 0)
            told, tnew = alternating([lambda: idx.align_sequences(pairs, sequences=off),
                                      lambda: idx.local_align_sequences(pairs, radius, sequences=off)], args.iters)
            ratio = tnew[0] / told[0]
            emit(lines, "| %d | %d | %d x %d | %.1f | %s | %s | %.3f | %s |" % (
                D, n, m, L, n * m * L / 1e6, fmt(told), fmt(tnew), ratio, ("within %.2f" % MARGIN if ratio <= MARGIN else "ABOVE %.2f" % MARGIN) if D == 768 else "no bar"))
            del idx
            for copies in (1, 2, 4):
                idx, off, pairs = make_index(g, dev, n, m, L, D, copies)
                t4, t1 = alternating([lambda: idx.local_align_sequences(pairs, radius, n_best=4, sequences=off),
                                      lambda: idx.local_align_sequences(pairs, radius, sequences=off)], args.iters)
                found = (idx.local_align_sequences(pairs, radius, n_best=4, sequences=off)[0] > 0).sum(1).to(torch.float64)
                run = float(torch.clamp(found + 1, max=4).mean())
                emit(rounds, "| %d | %d x %d | %d | %.3f | %.3f | %s | %s | %.3f |" % (D, m, L, copies, float(found.mean()), run, fmt(t4), fmt(t1), t4[0] / run / t1[0]))
                del idx
    lines += rounds
    lines += ["", "One sequence of %d rows against itself (`min_sep = 1`: the tiles wholly below the diagonal skip their contraction and their walk), "
              "the same call on two such sequences (no band) and the yardstick on those two; one workgroup each." % args.long, "",
              "| D | old, two sequences ms (min .. max) | new, two sequences ms (min .. max) | new, one against itself ms (min .. max) | itself / two | saved by the skipped tiles |",
              "|---:|---:|---:|---:|---:|---:|"]
    for D in (768, 32):
        off = np.array([0, args.long, 2 * args.long], np.int64)
        idx = SyllableIndex(torch.randn((2 * args.long, D), generator=g, device=dev), device=dev)
        told, tnew, tself = alternating([lambda: idx.align_sequences([[0, 1]], sequences=off),
                                         lambda: idx.local_align_sequences([[0, 1]], 0.75 * D, sequences=off),
                                         lambda: idx.local_align_sequences([[0, 0]], 0.75 * D, sequences=off)], args.iters)
        emit(lines, "| %d | %s | %s | %s | %.3f | %.1f %% |" % (D, fmt(told), fmt(tnew), fmt(tself), tself[0] / tnew[0], 100 * (1 - tself[0] / tnew[0])))
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

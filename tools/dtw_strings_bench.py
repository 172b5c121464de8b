"""Times ``SyllableIndex.align_sequences`` (csrc/dtw_strings.hip) and writes profiles/dtw_strings_bench.md.

The sequences are stored in an index and the pairs name them, so a call copies no rows: it is the host checks, the pairs' table
and the launches.  Four sets, each at D = 768 and at D = 32 (where the DP dominates):

1. 4096 pairs of 64 x 512 (all pairs of 64 sequences of 64 rows and 64 of 512), with the path, and ``align_phrases`` on the same
   pairs -- the existing fmaf-chain kernel, the only comparable code before this one;
2. 4096 pairs of 500 x 500 (random pairs of 128 sequences), counts only and with the path;
3. one pair of 8192 x 8192, counts only: the latency of a single long pair, whose DP is serial along y inside one workgroup.

The timing rule is tools/unit_strings_bench.py's: one warm-up call, then the median of ``--iters`` whole calls (host clock around a
call that ends in a device synchronise) with their min .. max.  Reported: milliseconds, DP cells per second ``sum(m L) / t``,
multiply-adds per second ``sum(m L) D / t`` and that as a share of the fp32 matrix peak (157.3 TFLOP/s = 78.65 T multiply-adds/s)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FMA = 157.3e12 / 2


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def row(name, D, n, shape, cells, t):
    fma = cells * D / (t[0] * 1e-3)
    return "| %s | %d | %d | %s | %.1f | %.2f (%.2f .. %.2f) | %.2f | %.2f | %.1f %% |" % (
        name, D, n, shape, cells / 1e6, t[0], t[1], t[2], cells / t[0] / 1e6, fma / 1e12, 100 * fma / PEAK_FMA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--long", type=int, default=8192, help="rows on each side of the single long pair")
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_strings_bench.md"))
    args = ap.parse_args()
    from sylber_amd import SyllableIndex
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    side = int(round(args.pairs ** 0.5))
    lines = ["# Embedding strings: one MI355X, one run", "",
             "`python tools/dtw_strings_bench.py --iters %d`: Gaussian rows stored in a `SyllableIndex` (metric \"l2\"), pairs of its sequences, "
             "so a call (`SyllableIndex.align_sequences`, host clock around a call that ends in a device synchronise) is the host checks, "
             "the pairs' table and the launches, without a copy of rows; one warm-up call, then the median of %d timed calls with their "
             "min .. max.  Gcells/s = `sum(m L) / t`; TFMA/s = `sum(m L) D / t`, and its share of the fp32 matrix peak of 78.65 T "
             "multiply-adds/s.  `align_phrases` is the existing fmaf-chain kernel on the same pairs of set 1." % (args.iters, args.iters), "",
             "| call | D | pairs | m x L | Mcells | ms (min .. max) | Gcells/s | TFMA/s | of peak |",
             "|---|---:|---:|---:|---:|---:|---:|---:|---:|"]

    def emit(r):
        print(r, file=sys.stderr, flush=True)
        lines.append(r)

    for D in (768, 32):
        # set 1: `side` sequences of 64 rows, then `side` of 512
        lens = [64] * side + [512] * side
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        idx = SyllableIndex(torch.randn((int(off[-1]), D), generator=g, device=dev), device=dev)
        pairs = np.array([[a, side + b] for a in range(side) for b in range(side)], np.int64)
        n, cells = len(pairs), len(pairs) * 64 * 512
        emit(row("align_sequences, path", D, n, "64 x 512", cells, timed(lambda: idx.align_sequences(pairs, path=True, sequences=off), args.iters)))
        emit(row("align_sequences, counts", D, n, "64 x 512", cells, timed(lambda: idx.align_sequences(pairs, sequences=off), args.iters)))
        phrases, lengths = idx.features[:side * 64], [64] * side
        spans = torch.from_numpy(np.tile(np.stack([off[side:-1], off[side + 1:]], 1)[None], (side, 1, 1))).to(dev)
        emit(row("align_phrases", D, n, "64 x 512", cells, timed(lambda: idx.align_phrases(phrases, spans, lengths=lengths), args.iters)))
        del idx, phrases, spans
        # set 2: 128 sequences of 500 rows, random pairs
        off = np.arange(129, dtype=np.int64) * 500
        idx = SyllableIndex(torch.randn((int(off[-1]), D), generator=g, device=dev), device=dev)
        pairs = rng.integers(0, 128, (args.pairs, 2)).astype(np.int64)
        cells = args.pairs * 500 * 500
        emit(row("align_sequences, counts", D, args.pairs, "500 x 500", cells, timed(lambda: idx.align_sequences(pairs, sequences=off), args.iters)))
        emit(row("align_sequences, path", D, args.pairs, "500 x 500", cells, timed(lambda: idx.align_sequences(pairs, path=True, sequences=off), args.iters)))
        del idx
        # set 3: one long pair
        off = np.array([0, args.long, 2 * args.long], np.int64)
        idx = SyllableIndex(torch.randn((2 * args.long, D), generator=g, device=dev), device=dev)
        emit(row("align_sequences, counts", D, 1, "%d x %d" % (args.long, args.long), args.long * args.long,
                 timed(lambda: idx.align_sequences([[0, 1]], sequences=off), args.iters)))
        del idx
    lines.append("")
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()

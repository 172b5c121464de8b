"""Times ``align_unit_strings`` (csrc/unit_strings.hip) and writes profiles/unit_strings_bench.md.

Three sets, in both modes where both exist: 4096 pairs of 20 to 60 units (utterances), 512 pairs of 250 to 350 units (the
long-form configuration: 60 s clips) and one pair of 20 000 x 20 000 units, counts only (its pairing would keep 100 MB of
predecessor codes; the bound on one pair's workspace is 256 MiB).  A reference is uniform over ``--alphabet`` symbols per column; its
hypothesis is the reference with about every tenth unit substituted, every twentieth deleted and a new unit after every
twentieth, so the lengths of a pair differ.  Strings are host arrays, as ``tokenize`` returns them: a call includes their checks,
the copy to the device and the launches.  The timing rule is tools/unit_search_bench.py's: one warm-up call, then the median of
``--iters`` whole calls (host clock around a call that ends in a device synchronise) with their min .. max.  Reported: milliseconds
and DP cells per second, ``sum(m L) / t``.

Yardstick, in the same run on the first set only (it takes references of at most 64 units): ``UnitIndex.align_phrases(...,
free_start=False)`` over one index of all hypotheses, each reference against its own hypothesis' rows; the index is built outside
the timed call."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def fmt(t):
    return "%.2f (%.2f .. %.2f)" % t


def pairs(rng, n, lo, hi, W, A):
    """n references of lo .. hi units and their corrupted hypotheses"""
    refs, hyps = [], []
    for m in rng.integers(lo, hi + 1, n):
        r = rng.integers(0, A, (int(m), W))
        h = r.copy()
        swap = rng.random(len(h)) < 0.10
        h[swap] = rng.integers(0, A, (int(swap.sum()), W))
        h = h[rng.random(len(h)) >= 0.05]
        at = np.nonzero(rng.random(len(h) + 1) < 0.05)[0]
        h = np.insert(h, at, rng.integers(0, A, (len(at), W)), 0)
        refs.append(r)
        hyps.append(h)
    return refs, hyps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--alphabet", type=int, default=10000)
    ap.add_argument("--widths", default="1,2")
    ap.add_argument("--long", type=int, default=20000, help="units on each side of the single long pair")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unit_strings_bench.md"))
    args = ap.parse_args()
    from sylber_amd import UnitIndex, align_unit_strings
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    A = args.alphabet
    lines = ["# Unit strings: one MI355X, one run", "",
             "`python tools/unit_strings_bench.py --iters %d`: references uniform over %s symbols per column, a hypothesis is its reference "
             "with about 10 %% of the units substituted, 5 %% deleted and 5 %% inserted.  Strings are host arrays, so a call "
             "(`align_unit_strings`, host clock around a call that ends in a device synchronise) includes their checks, the copy to the device "
             "and the launches; one warm-up call, then the median of %d timed calls with their min .. max.  Cells/s = `sum(m L) / t`.  "
             "Yardstick, first set only: `UnitIndex.align_phrases(free_start=False)` over one index of all hypotheses (built outside the "
             "timed call), each reference against its own hypothesis' rows." % (args.iters, "{:,}".format(A).replace(",", " "), args.iters), "",
             "| W | pairs | units per string | Mcells | counts only ms (min .. max) | Gcells/s | with pairing ms (min .. max) | Gcells/s | "
             "align_phrases global ms (min .. max) |",
             "|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for W in [int(v) for v in args.widths.split(",")]:
        for n, lo, hi, both, yard in ((4096, 20, 60, True, True), (512, 250, 350, True, False), (1, args.long, args.long, False, False)):
            refs, hyps = pairs(rng, n, lo, hi, W, A)
            cells = sum(len(r) * len(h) for r, h in zip(refs, hyps))
            tc = timed(lambda: align_unit_strings(refs, hyps), args.iters)
            tp = timed(lambda: align_unit_strings(refs, hyps, pairing=True), args.iters) if both else None
            ty = None
            if yard:
                idx = UnitIndex(np.concatenate(hyps), device=dev)
                off = np.concatenate([[0], np.cumsum([len(h) for h in hyps])])
                spans = torch.from_numpy(np.stack([off[:-1], off[1:]], 1).reshape(n, 1, 2).astype(np.int64))
                ty = timed(lambda: idx.align_phrases(refs, spans, free_start=False), args.iters)
                del idx
            row = "| %d | %d | %s | %.1f | %s | %.2f | %s | %s | %s |" % (
                W, n, "%d .. %d" % (lo, hi) if lo != hi else "%d" % lo, cells / 1e6, fmt(tc), cells / tc[0] / 1e6,
                fmt(tp) if tp else "-", "%.2f" % (cells / tp[0] / 1e6) if tp else "-", fmt(ty) if ty else "-")
            print(row, file=sys.stderr, flush=True)
            lines.append(row)
    lines.append("")
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()

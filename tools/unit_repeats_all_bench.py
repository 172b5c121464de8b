"""Times ``sylber_unit_local_align_all`` (csrc/unit_repeats_all.hip) against ``sylber_unit_local_align`` (csrc/unit_repeats.hip), the
rounds after the first, and ``UnitIndex.find_repeats(per_pair=4, within=True)`` beside ``find_repeats``; writes
profiles/unit_repeats_all_bench.md.  The pairs, the corpus and the timing are tools/unit_repeats_bench.py's.

Round-0 tax: the two C entries on the same device-resident pairs in one process, workspaces allocated beforehand, the new one with
``n_best = 1``, ``sep = 0``, ``min_score = 1`` -- the same results, which the tool checks.  One warm-up call each, then ``--iters``
rounds of (old, new), each call between two events; the medians with min .. max and new / old.  ``--pairs`` pairs of 200 x 200
units and one pair of ``--long`` x ``--long``, W = 1 and 2.

Cost of a round: ``--pairs`` pairs of 200 x 200 random units with 1, 2 or 4 phrases of 12 units of x planted in y, ``n_best = 4``,
``min_score = 6``.  A pair runs one round per repeat it finds and one more that finds nothing, four at most; the rounds run are
counted from the scores.  Reported: the time over the mean rounds run per pair, against the ``n_best = 1`` time on the same pairs.

``find_repeats``: the corpus of tools/unit_repeats_bench.py; ``find_repeats(k)`` and ``find_repeats(k, per_pair=4, within=True)``
alternating, host clock around a call that ends in a device synchronise.

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from unit_repeats_bench import fmt, make_pairs  # noqa: E402

_i32p = ctypes.POINTER(ctypes.c_int32)


def alternating(fns, iters):
    """one warm-up call of each, then ``iters`` rounds of every fn in turn, each between two events -> [(median, min, max) ms]"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(iters):
        for fn, o in zip(fns, out):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            o.append(a.elapsed_time(b))
    return [(statistics.median(o), min(o), max(o)) for o in out]


class Pairs:
    """device-resident pairs with the outputs and workspaces of both entries"""

    def __init__(self, lib, dev, xs, ys, W, n_best):
        from sylber_amd.kmeans import _stream
        self.lib, self.W, self.n, self.R = lib, W, len(xs), n_best
        self.xd = torch.from_numpy(np.concatenate(xs).astype(np.int32)).to(dev)
        self.yd = torch.from_numpy(np.concatenate(ys).astype(np.int32)).to(dev)
        xo = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)
        yo = np.concatenate([[0], np.cumsum([len(y) for y in ys])]).astype(np.int32)
        self.xw = np.ascontiguousarray(np.stack([xo[:-1], np.diff(xo)], 1), np.int32)
        self.yw = np.ascontiguousarray(np.stack([yo[:-1], np.diff(yo)], 1), np.int32)
        xp, yp, n = self.xw.ctypes.data_as(_i32p), self.yw.ctypes.data_as(_i32p), self.n
        self.score1 = torch.empty(n, dtype=torch.int32, device=dev)
        self.span1 = torch.empty((n, 4), dtype=torch.int32, device=dev)
        self.score = torch.empty((n, n_best), dtype=torch.int32, device=dev)
        self.span = torch.empty((n, n_best, 4), dtype=torch.int32, device=dev)
        self.w1 = torch.empty(int(lib.sylber_unit_local_workspace_bytes(xp, yp, n)), dtype=torch.uint8, device=dev)
        self.wa = torch.empty(int(lib.sylber_unit_local_all_workspace_bytes(xp, yp, n)), dtype=torch.uint8, device=dev)
        self.st = _stream(dev)

    def one(self):
        from sylber_amd import _lib
        from sylber_amd.kmeans import _vp
        _lib.check(self.lib.sylber_unit_local_align(_vp(self.xd), self.xd.shape[0], _vp(self.yd), self.yd.shape[0], self.W,
                                                    self.xw.ctypes.data_as(_i32p), self.yw.ctypes.data_as(_i32p), self.n, 2, 3, 4,
                                                    _vp(self.score1), _vp(self.span1), _vp(self.w1), self.st), "sylber_unit_local_align")

    def every(self, n_best, floor):
        from sylber_amd import _lib
        from sylber_amd.kmeans import _vp
        assert n_best <= self.R
        score = self.score if n_best == self.R else self.score.view(-1)[:self.n * n_best]
        span = self.span if n_best == self.R else self.span.view(-1)[:self.n * n_best * 4]
        _lib.check(self.lib.sylber_unit_local_align_all(_vp(self.xd), self.xd.shape[0], _vp(self.yd), self.yd.shape[0], self.W,
                                                        self.xw.ctypes.data_as(_i32p), self.yw.ctypes.data_as(_i32p), None, self.n, 2, 3, 4,
                                                        n_best, floor, _vp(score), _vp(span), _vp(self.wa), self.st),
                   "sylber_unit_local_align_all")
        return score.view(self.n, n_best)


def planted_pairs(rng, n, units, A, phrases):
    """random x and y with ``phrases`` phrases of 12 units of x written into y, one per slot of ``units / phrases`` units on both
    sides, so no two of them touch"""
    xs, ys, slot = [], [], units // phrases
    for _ in range(n):
        x, y = rng.integers(0, A, (units, 1)), rng.integers(0, A, (units, 1))
        for q in rng.permutation(phrases).tolist():
            a, b = (int(rng.integers(0, slot - 13)) for _ in range(2))
            y[q * slot + b:q * slot + b + 12] = x[a + slot * ((q + 1) % phrases):a + slot * ((q + 1) % phrases) + 12]
        xs.append(x)
        ys.append(y)
    return xs, ys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--alphabet", type=int, default=1000)
    ap.add_argument("--widths", default="1,2")
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--long", type=int, default=20000, help="units on each side of the single long pair")
    ap.add_argument("--sequences", type=int, default=2000)
    ap.add_argument("--planted", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unit_repeats_all_bench.md"))
    args = ap.parse_args()
    from sylber_amd import UnitIndex, _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    A = args.alphabet
    lines = ["# Unit repeats, every one: one MI355X, one run", "",
             "`python tools/unit_repeats_all_bench.py --iters %d`.  Round-0 tax: `sylber_unit_local_align` (old) and `sylber_unit_local_align_all` "
             "with `n_best = 1`, `sep = 0`, `min_score = 1` (new) on the same device-resident pairs in one process, each C entry between two "
             "events on the stream, workspaces allocated beforehand; one warm-up call each, then %d rounds of (old, new): the medians with their "
             "min .. max.  The pairs are tools/unit_repeats_bench.py's: units uniform over %d symbols per column, y is x with about 10 %% "
             "substituted, 5 %% deleted, 5 %% inserted.  The two entries' scores and spans were equal on every set."
             % (args.iters, args.iters, A), "",
             "| W | pairs | units per string | Mcells | old ms (min .. max) | new ms (min .. max) | new / old |",
             "|---:|---:|---:|---:|---:|---:|---:|"]
    for W in [int(v) for v in args.widths.split(",")]:
        for n, units in ((args.pairs, 200), (1, args.long)):
            xs, ys = make_pairs(rng, n, units, W, A)
            cells = sum(len(x) * len(y) for x, y in zip(xs, ys))
            p = Pairs(lib, dev, xs, ys, W, 1)
            told, tnew = alternating([p.one, lambda: p.every(1, 1)], args.iters)
            assert torch.equal(p.score1, p.score[:, 0]) and torch.equal(p.span1, p.span[:, 0]), "round 0 is not the one-repeat entry"
            row = "| %d | %d | %d | %.1f | %s | %s | %.3f |" % (W, n, units, cells / 1e6, fmt(told), fmt(tnew), tnew[0] / told[0])
            print(row, file=sys.stderr, flush=True)
            lines.append(row)

    lines += ["", "Cost of a round: %d pairs of 200 x 200 random units over %d symbols, W = 1, with phrases of 12 units of x written into y; "
              "`n_best = 4`, `min_score = 6`, timed as above.  A pair runs one round per repeat it finds and one more that finds nothing, four at "
              "most; rounds run = the mean over the pairs, counted from the scores.  round 0 = `n_best = 1` on the same pairs." % (args.pairs, A), "",
              "| phrases per pair | repeats found per pair | rounds run per pair | n_best = 4 ms (min .. max) | round 0 ms (min .. max) | ms per round run / round 0 ms |",
              "|---:|---:|---:|---:|---:|---:|"]
    for phrases in (1, 2, 4):
        xs, ys = planted_pairs(rng, args.pairs, 200, A, phrases)
        p = Pairs(lib, dev, xs, ys, 1, 4)
        t4, t1 = alternating([lambda: p.every(4, 6), lambda: p.every(1, 6)], args.iters)
        found = (p.every(4, 6) > 0).sum(1).to(torch.float64)
        torch.cuda.synchronize()
        run = float(torch.clamp(found + 1, max=4).mean())
        row = "| %d | %.3f | %.3f | %s | %s | %.3f |" % (phrases, float(found.mean()), run, fmt(t4), fmt(t1), t4[0] / run / t1[0])
        print(row, file=sys.stderr, flush=True)
        lines.append(row)

    # find_repeats over the corpus of tools/unit_repeats_bench.py
    S, P = args.sequences, args.planted
    lens = rng.integers(80, 121, S)
    seqs = [rng.integers(0, A, int(n)) for n in lens]
    planted = set()
    free = rng.permutation(S)[:2 * P].reshape(P, 2)       # every sequence holds at most one planted phrase
    for s, t in free.tolist():
        s, t = min(s, t), max(s, t)
        phrase = rng.integers(0, A, 12)
        for q in (s, t):
            at = int(rng.integers(0, len(seqs[q]) - 12 + 1))
            seqs[q][at:at + 12] = phrase
        planted.add((s, t))
    ix = UnitIndex(np.concatenate(seqs), groups=np.repeat(np.arange(S, dtype=np.int32), lens), device=dev)
    calls = [lambda: ix.find_repeats(P), lambda: ix.find_repeats(P, per_pair=4, within=True)]
    wall, got = [[], []], [None, None]
    for it in range(4):                                    # the first round warms up
        for e, fn in enumerate(calls):
            t0 = time.perf_counter()
            scores, pairs, spans = fn()
            torch.cuda.synchronize()
            if it:
                wall[e].append((time.perf_counter() - t0) * 1e3)
            got[e] = {tuple(q) for q in pairs.cpu().numpy().tolist()}
    w = [(statistics.median(o), min(o), max(o)) for o in wall]
    lines += ["", "`UnitIndex.find_repeats(k = %d)` and `find_repeats(k = %d, per_pair = 4, within = True)` (defaults 2 / 3 / 4, `min_score = 6`) "
              "over %d sequences of 80 .. 120 units, W = 1, %d symbols, %d pairs of sequences with a planted common phrase of 12 units: %d pairs of "
              "sequences, and %d more of a sequence with itself.  Host clock around a call that ends in a device synchronise, one warm-up call each, "
              "then alternating, the median of 3 with min .. max." % (P, P, S, A, P, S * (S - 1) // 2, S), "",
              "| call | wall ms (min .. max) | planted pairs among the k returned |", "|---|---:|---:|",
              "| `find_repeats(%d)` | %s | %d of %d |" % (P, fmt(w[0]), len(got[0] & planted), P),
              "| `find_repeats(%d, per_pair=4, within=True)` | %s | %d of %d |" % (P, fmt(w[1]), len(got[1] & planted), P),
              "", "every-repeat / one-repeat wall time: %.3f" % (w[1][0] / w[0][0])]
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

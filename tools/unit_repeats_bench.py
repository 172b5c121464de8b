"""Times ``sylber_unit_local_align`` (csrc/unit_repeats.hip) beside its sibling ``sylber_unit_strings_align`` (csrc/unit_strings.hip,
counts only) and one ``UnitIndex.find_repeats``, and writes profiles/unit_repeats_bench.md.

Kernel rows: the C entries themselves on device-resident strings with a workspace allocated beforehand, the same pairs through
both -- both kernels carry three ints per cell, walk the same wavefront and hand the same 12 B per column between strips; the local
one adds the floor, the choice of a start and the running best, the global one its counters.  Two sets: ``--pairs`` pairs of
200 x 200 units and one pair of ``--long`` x ``--long``.  y is x with about 10 % of the units substituted, 5 % deleted and 5 %
inserted, cut or padded to x's length.  Timing: one warm-up call, then ``--iters`` calls each between two events on the stream; the
median with its min .. max.  Cells/s = ``sum(m L) / t``.

``find_repeats``: a corpus of ``--sequences`` sequences of 80 .. 120 units over ``--alphabet`` symbols; ``--planted`` pairs of
sequences get a common phrase of 12 units written into both.  One call with ``k = --planted`` (host clock around a call that ends in a
device synchronise: the enumeration of the pairs on the host, the tables' copies, the launches, the running top-k); reported: wall
time, cells per second over all pairs and the share of the planted pairs among the returned ones.

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
_i32p = ctypes.POINTER(ctypes.c_int32)


def fmt(t):
    return "%.2f (%.2f .. %.2f)" % t


def event_timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def make_pairs(rng, n, units, W, A):
    xs, ys = [], []
    for _ in range(n):
        x = rng.integers(0, A, (units, W))
        y = x.copy()
        swap = rng.random(len(y)) < 0.10
        y[swap] = rng.integers(0, A, (int(swap.sum()), W))
        y = y[rng.random(len(y)) >= 0.05]
        at = np.nonzero(rng.random(len(y) + 1) < 0.05)[0]
        y = np.insert(y, at, rng.integers(0, A, (len(at), W)), 0)[:units]
        y = np.concatenate([y, rng.integers(0, A, (units - len(y), W))])
        xs.append(x)
        ys.append(y)
    return xs, ys


def kernels(lib, dev, xs, ys, W, iters):
    """(local ms, global ms) of the two C entries on the same device-resident pairs"""
    from sylber_amd import _lib
    from sylber_amd.kmeans import _stream, _vp
    n = len(xs)
    xd = torch.from_numpy(np.concatenate(xs).astype(np.int32)).to(dev)
    yd = torch.from_numpy(np.concatenate(ys).astype(np.int32)).to(dev)
    xo = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)
    yo = np.concatenate([[0], np.cumsum([len(y) for y in ys])]).astype(np.int32)
    xw = np.ascontiguousarray(np.stack([xo[:-1], np.diff(xo)], 1), np.int32)
    yw = np.ascontiguousarray(np.stack([yo[:-1], np.diff(yo)], 1), np.int32)
    score = torch.empty(n, dtype=torch.int32, device=dev)
    span = torch.empty((n, 4), dtype=torch.int32, device=dev)
    ops = torch.empty((n, 4), dtype=torch.int32, device=dev)
    cost = torch.empty(n, dtype=torch.int32, device=dev)
    wl = torch.empty(int(lib.sylber_unit_local_workspace_bytes(xw.ctypes.data_as(_i32p), yw.ctypes.data_as(_i32p), n)), dtype=torch.uint8, device=dev)
    wg = torch.empty(int(lib.sylber_unit_strings_workspace_bytes(xo.ctypes.data_as(_i32p), yo.ctypes.data_as(_i32p), n, 0)), dtype=torch.uint8, device=dev)
    st = _stream(dev)

    def local():
        _lib.check(lib.sylber_unit_local_align(_vp(xd), xd.shape[0], _vp(yd), yd.shape[0], W, xw.ctypes.data_as(_i32p), yw.ctypes.data_as(_i32p),
                                               n, 2, 3, 4, _vp(score), _vp(span), _vp(wl), st), "sylber_unit_local_align")

    def glob():
        _lib.check(lib.sylber_unit_strings_align(_vp(xd), xo.ctypes.data_as(_i32p), _vp(yd), yo.ctypes.data_as(_i32p), W, n, 0, None, None,
                                                 _vp(ops), _vp(cost), None, _vp(wg), st), "sylber_unit_strings_align")
    return event_timed(local, iters), event_timed(glob, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--alphabet", type=int, default=1000)
    ap.add_argument("--widths", default="1,2")
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--long", type=int, default=20000, help="units on each side of the single long pair")
    ap.add_argument("--sequences", type=int, default=2000)
    ap.add_argument("--planted", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unit_repeats_bench.md"))
    args = ap.parse_args()
    from sylber_amd import UnitIndex, _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    A = args.alphabet
    lines = ["# Unit repeats: one MI355X, one run", "",
             "`python tools/unit_repeats_bench.py --iters %d`.  Kernel rows: `sylber_unit_local_align` and, on the same device-resident pairs, "
             "`sylber_unit_strings_align` (counts only), each C entry between two events on the stream, workspace allocated beforehand; one warm-up "
             "call, then the median of %d timed calls with their min .. max.  Units uniform over %d symbols per column; y is x with about 10 %% of "
             "the units substituted, 5 %% deleted and 5 %% inserted.  Cells/s = `sum(m L) / t`; ratio = local / global cells per second."
             % (args.iters, args.iters, A), "",
             "| W | pairs | units per string | Mcells | local ms (min .. max) | Gcells/s | global ms (min .. max) | Gcells/s | ratio |",
             "|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for W in [int(v) for v in args.widths.split(",")]:
        for n, units in ((args.pairs, 200), (1, args.long)):
            xs, ys = make_pairs(rng, n, units, W, A)
            cells = sum(len(x) * len(y) for x, y in zip(xs, ys))
            tl, tg = kernels(lib, dev, xs, ys, W, args.iters)
            row = "| %d | %d | %d | %.1f | %s | %.2f | %s | %.2f | %.2f |" % (
                W, n, units, cells / 1e6, fmt(tl), cells / tl[0] / 1e6, fmt(tg), cells / tg[0] / 1e6, tg[0] / tl[0])
            print(row, file=sys.stderr, flush=True)
            lines.append(row)

    # find_repeats over a corpus with planted phrases
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
    total = int((lens.sum() ** 2 - (lens.astype(np.int64) ** 2).sum()) // 2)
    ix.find_repeats(P)
    torch.cuda.synchronize()
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        scores, pairs, spans = ix.find_repeats(P)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    got = {tuple(p) for p in pairs.cpu().numpy().tolist()}
    w = (statistics.median(wall), min(wall), max(wall))
    lines += ["", "`UnitIndex.find_repeats(k = %d)` (defaults 2 / 3 / 4, `min_score = 6`) over %d sequences of 80 .. 120 units, W = 1, %d symbols, "
              "%d pairs of sequences with a planted common phrase of 12 units: %d pairs of sequences, %.1f Gcells.  Host clock around a call that "
              "ends in a device synchronise, one warm-up call, the median of 3 with min .. max." % (P, S, A, P, S * (S - 1) // 2, total / 1e9), "",
              "| wall ms (min .. max) | Gcells/s | planted pairs among the k returned |", "|---:|---:|---:|",
              "| %s | %.2f | %d of %d (%.0f %%) |" % (fmt(w), total / w[0] / 1e6, len(got & planted), P, 100.0 * len(got & planted) / P)]
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

"""Times ``SyllableIndex.search_repeats`` (csrc/dtw_local.hip) beside ``SyllableIndex.search_phrases`` (csrc/dtw.hip) and one
``SyllableIndex.find_repeats``, and writes profiles/repeats_bench.md.

``search_repeats`` rows: seeded random data on the device, D = 768, L2, N database rows in sequences of 20 to 60 rows; probes of m
rows, P of them so that the probe rows total ``rows``; k = 10.  The same probes, N, D and k go through ``search_phrases`` in the same
process: the same grid, staging, contraction and cost tile with the subsequence-DTW wavefront in place of the local one, the code
of the parent commit -- the yardstick.  ``radius`` = 1400 (two unrelated rows are about 1536 apart, so about one cell in twenty
earns), ``gap`` and ``min_score`` at their defaults.  Per (rows, m): the median milliseconds of the whole call (host clock around a
call that ends in a device synchronise, after a warm-up call) with min .. max, and the ratio local / phrase time.

``find_repeats``: ``--sequences`` sequences of 20 .. 60 rows, ``--planted`` pairs of which share a phrase of 12 rows (the second
copy with 0.3 x gaussian noise); one call with ``k = min(128, planted)``; reported: the wall time, the windows searched and the
share of the returned pairs that are planted.

``box_speed``: the library's 4096^3 bf16 GEMM loop (``sylber_debug_gemm_bench``, tile 97), bench.py's yardstick for the box.

    python tools/repeats_bench.py [--iters 5] [--N 1048576] [--rows 128,1024,8192] [--ms 8,32,64]"""
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


def fmt(t):
    return "%.2f (%.2f .. %.2f)" % t


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--N", type=int, default=1 << 20)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rows", default="128,1024,8192")
    ap.add_argument("--ms", default="8,32,64")
    ap.add_argument("--radius", type=float, default=1400.0)
    ap.add_argument("--sequences", type=int, default=4000)
    ap.add_argument("--planted", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repeats_bench.md"))
    args = ap.parse_args()
    from sylber_amd import SyllableIndex, _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    gen = torch.Generator(device=dev).manual_seed(0)
    D, k = args.D, args.k
    lens = []
    while sum(lens) < args.N:
        lens.append(int(rng.integers(20, 61)))
    lens[-1] -= sum(lens) - args.N
    if lens[-1] < 1:
        lens.pop()
    N = sum(lens)
    x = torch.randn((N, D), generator=gen, device=dev)
    idx = SyllableIndex(x, metric="l2", groups=np.repeat(np.arange(len(lens), dtype=np.int32), lens), device=dev)
    lines = ["# Repeated phrases on embeddings: one MI355X, one run", "",
             "`python tools/repeats_bench.py --iters %d --N %d`.  `search_repeats` beside `search_phrases` (the parent commit's code: the "
             "yardstick) on the same probes, index and k = %d in the same process; D = %d, L2, %d sequences of 20 .. 60 rows; radius = %g, gap and "
             "min_score at their defaults.  Whole calls, host clock around a call that ends in a device synchronise; one warm-up call, then the "
             "median of %d timed calls with min .. max.  ratio = local / phrase time: above 1 is slower."
             % (args.iters, N, k, D, len(lens), args.radius, args.iters), "",
             "| probe rows | m | probes | search_phrases ms (min .. max) | search_repeats ms (min .. max) | ratio | probes with a result |",
             "|---:|---:|---:|---:|---:|---:|---:|"]
    for rows in [int(v) for v in args.rows.split(",")]:
        for m in [int(v) for v in args.ms.split(",")]:
            P = max(1, rows // m)
            at = rng.integers(0, N - m, P)
            q = torch.cat([x[a:a + m] for a in at.tolist()]) + 0.3 * torch.randn((P * m, D), generator=gen, device=dev)
            ln = [m] * P
            tp = timed(lambda: idx.search_phrases(q, k, lengths=ln), args.iters)
            tl = timed(lambda: idx.search_repeats(q, k, args.radius, lengths=ln), args.iters)
            hit = int((idx.search_repeats(q, k, args.radius, lengths=ln)[1][:, 0] >= 0).sum())
            row = "| %d | %d | %d | %s | %s | %.2f | %d |" % (P * m, m, P, fmt(tp), fmt(tl), tl[0] / tp[0], hit)
            print(row, file=sys.stderr, flush=True)
            lines.append(row)
    del idx, x

    # find_repeats over a corpus with planted phrases
    S, Pl = args.sequences, args.planted
    lens = rng.integers(20, 61, S)
    off = np.concatenate([[0], np.cumsum(lens)])
    x = rng.standard_normal((int(off[-1]), D)).astype(np.float32)
    planted = set()
    free = rng.permutation(S)[:2 * Pl].reshape(Pl, 2)         # every sequence holds at most one planted phrase
    for s, t in free.tolist():
        s, t = min(s, t), max(s, t)
        a, b = (int(off[q] + rng.integers(0, lens[q] - 12 + 1)) for q in (s, t))
        x[b:b + 12] = x[a:a + 12] + 0.3 * rng.standard_normal((12, D)).astype(np.float32)
        planted.add((s, t))
    ix = SyllableIndex(x, metric="l2", groups=np.repeat(np.arange(S, dtype=np.int32), lens), device=dev)
    kk = min(128, Pl)
    ix.find_repeats(kk, args.radius)
    torch.cuda.synchronize()
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        scores, pairs, spans = ix.find_repeats(kk, args.radius)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    got = {tuple(p) for p in pairs.cpu().numpy().tolist() if p[0] >= 0}
    w = (statistics.median(wall), min(wall), max(wall))
    lines += ["", "`SyllableIndex.find_repeats(k = %d, radius = %g)` (window 64, hop 32, defaults) over %d sequences of 20 .. 60 rows (%d rows, one "
              "window each), D = %d, %d pairs of sequences with a planted phrase of 12 rows (the copy with 0.3 x gaussian noise).  Host clock "
              "around a call that ends in a device synchronise, one warm-up call, the median of 3 with min .. max."
              % (kk, args.radius, S, int(off[-1]), D, Pl), "",
              "| wall ms (min .. max) | pairs returned | of them planted |", "|---:|---:|---:|",
              "| %s | %d | %d (%.0f %%) |" % (fmt(w), len(got), len(got & planted), 100.0 * len(got & planted) / max(1, len(got)))]
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

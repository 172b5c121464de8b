"""Times ``UnitIndex.search_phrases`` / ``search_occurrences`` (csrc/unit_search.hip) and writes profiles/unit_search_bench.md.

Sized like profiles/phrase_bench.md: N = 4 194 304 units in sequences of 20 to 60, k = 10; W = 1 and 2; P x m = 64 x 2, 128 x 8,
32 x 32, 1024 x 8 and 256 x 32.  Unit ids are uniform over ``--alphabet`` symbols per column; a phrase is a corpus substring with
about every fourth unit replaced by a random one.  The timing rule is tools/phrase_bench.py's: one warm-up call, then the median of
``--iters`` whole calls (host clock around a call that ends in a device synchronise) with their min .. max.  Reported: milliseconds
and DP cells per second, ``P m N / t``.

Yardstick, in the same process on the same box: ``PQSyllableIndex.search_phrases`` after ``drop_rows()`` (M = 48 codes of D = 768
gaussian rows, ``rerank=False``, refine 4, fp16) at the same N, P and m -- the cheapest phrase search the embedding indexes offer.
The two answer different questions (edit distance over tokens against DTW over embeddings), so the ratio is context, not a gate.
``--no-yardstick`` leaves it out.

``--align`` measures something else and writes profiles/unit_align_bench.md instead: on the same corpus and shapes it times
``UnitIndex.search_phrases`` and, beside it in the same run, ``UnitIndex.align_phrases`` (csrc/unit_align.hip) on the spans that this
search returned -- P k pairs of a phrase and a window of at most 2 m rows -- under the same timing rule.  No yardstick is run."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64, 2), (128, 8), (32, 32), (1024, 8), (256, 32)]


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


def sequence_lengths(N, rng):
    lens = rng.integers(20, 61, N // 20 + 1)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), N)) + 1]
    lens[-1] -= int(lens.sum()) - N
    return lens[lens > 0]


def fmt(t):
    return "%.2f (%.2f .. %.2f)" % t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--N", type=int, default=4194304)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--alphabet", type=int, default=10000)
    ap.add_argument("--widths", default="1,2")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--align", action="store_true", help="time align_phrases on the spans of search_phrases; writes unit_align_bench.md")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "unit_align_bench.md" if args.align else "unit_search_bench.md")
    if args.align:
        return align_main(args)
    from sylber_amd import PQSyllableIndex, SyllableIndex, UnitIndex
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    N, k, A = args.N, args.k, args.alphabet
    lens = sequence_lengths(N, rng)
    groups = np.repeat(np.arange(lens.size), lens).astype(np.int32)

    yard = {}
    if not args.no_yardstick:
        g = torch.Generator(device=dev).manual_seed(0)
        D, M = 768, 48
        idx = SyllableIndex(torch.randn(N, D, device=dev, generator=g), metric="l2", groups=groups, device=dev)
        pick = torch.randperm(N, device=dev, generator=g)[:256]
        pq = PQSyllableIndex.build(idx, M, codebooks=idx.features[pick].reshape(256, M, D // M).permute(1, 0, 2).contiguous())
        rows = max(P * m for P, m in SHAPES)
        q = (idx.features[1000:1000 + rows] + 0.5 * torch.randn(rows, D, device=dev, generator=g)).contiguous()
        pq.drop_rows()
        del idx
        torch.cuda.empty_cache()
        for P, m in SHAPES:
            yard[(P, m)] = timed(lambda: pq.search_phrases(q[:P * m], k, 4, "fp16", lengths=[m] * P, rerank=False), args.iters)
            print("yardstick", P, m, fmt(yard[(P, m)]), file=sys.stderr, flush=True)
        yard_bytes = pq.nbytes
        del pq, q
        torch.cuda.empty_cache()

    lines = ["# Unit search: one MI355X, one run", "",
             "`python tools/unit_search_bench.py --iters %d`: N = %s units in %s sequences of 20 to 60, k = %d, ids uniform over %s symbols per "
             "column; a phrase is a corpus substring with about every fourth unit replaced.  Times are whole calls "
             "(`UnitIndex.search_phrases` / `search_occurrences`, host clock around a call that ends in a device synchronise), one warm-up "
             "call, then the median of %d timed calls with their min .. max.  Cells/s = `P m N / t` of `search_phrases`.%s" %
             (args.iters, "{:,}".format(N).replace(",", " "), "{:,}".format(lens.size).replace(",", " "), k, "{:,}".format(A).replace(",", " "),
              args.iters, "" if args.no_yardstick else "  Yardstick: `PQSyllableIndex.search_phrases` after `drop_rows()` (D = 768, M = 48, "
              "refine 4, fp16, `rerank=False`) at the same N, P and m in the same process; `ratio` = yardstick time / `search_phrases` time."),
             "",
             "| W | phrases P | units m | search_phrases ms (min .. max) | Gcells/s | search_occurrences ms (min .. max) |" +
             ("" if args.no_yardstick else " PQ dropped ms (min .. max) | ratio |"),
             "|---:|---:|---:|---:|---:|---:|" + ("" if args.no_yardstick else "---:|---:|")]
    nbytes = {}
    for W in [int(v) for v in args.widths.split(",")]:
        corpus = torch.from_numpy(rng.integers(0, A, (N, W)).astype(np.int32))
        idx = UnitIndex(corpus, groups=groups, device=dev)
        idx.sequence_offsets()
        nbytes[W] = idx.nbytes
        for P, m in SHAPES:
            at = rng.integers(0, N - m, P)
            ph = torch.stack([corpus[a:a + m] for a in at]).reshape(P * m, W).clone()
            swap = torch.from_numpy(rng.random(P * m) < 0.25)
            ph[swap] = torch.from_numpy(rng.integers(0, A, (int(swap.sum()), W)).astype(np.int32))
            ph, ln = ph.to(dev), [m] * P
            tp = timed(lambda: idx.search_phrases(ph, k, lengths=ln), args.iters)
            to = timed(lambda: idx.search_occurrences(ph, k, lengths=ln), args.iters)
            row = "| %d | %d | %d | %s | %.1f | %s |" % (W, P, m, fmt(tp), P * m * N / tp[0] / 1e6, fmt(to))
            if yard:
                row += " %s | %.1f |" % (fmt(yard[(P, m)]), yard[(P, m)][0] / tp[0])
            print(row, file=sys.stderr, flush=True)
            lines.append(row)
        del idx
    lines += ["", "Device bytes (`nbytes`, ids and groups): " + ", ".join("%.1f MB at W = %d" % (b / 1e6, W) for W, b in nbytes.items()) +
              ("; the yardstick's `PQSyllableIndex` after `drop_rows()`: %.1f MB." % (yard_bytes / 1e6) if yard else "."), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


def align_main(args):
    from sylber_amd import UnitIndex
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    N, k, A = args.N, args.k, args.alphabet
    lens = sequence_lengths(N, rng)
    groups = np.repeat(np.arange(lens.size), lens).astype(np.int32)
    lines = ["# Edit scripts beside the search that found them: one MI355X, one run", "",
             "`python tools/unit_search_bench.py --align --iters %d`: the corpus, phrases and timing rule of profiles/unit_search_bench.md "
             "(N = %s units in %s sequences of 20 to 60, k = %d, ids uniform over %s symbols per column; one warm-up call, then the median of "
             "%d whole calls with their min .. max).  `align_phrases` is given the spans that the `search_phrases` call timed beside it "
             "returned: `pairs` of them are not padding, and a window has at most 2 m rows.  `ratio` = `align_phrases` time / "
             "`search_phrases` time." %
             (args.iters, "{:,}".format(N).replace(",", " "), "{:,}".format(lens.size).replace(",", " "), k, "{:,}".format(A).replace(",", " "),
              args.iters), "",
             "| W | phrases P | units m | pairs | widest window | search_phrases ms (min .. max) | align_phrases ms (min .. max) | "
             "align_phrases global ms (min .. max) | ratio |",
             "|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for W in [int(v) for v in args.widths.split(",")]:
        corpus = torch.from_numpy(rng.integers(0, A, (N, W)).astype(np.int32))
        idx = UnitIndex(corpus, groups=groups, device=dev)
        idx.sequence_offsets()
        for P, m in SHAPES:
            at = rng.integers(0, N - m, P)
            ph = torch.stack([corpus[a:a + m] for a in at]).reshape(P * m, W).clone()
            swap = torch.from_numpy(rng.random(P * m) < 0.25)
            ph[swap] = torch.from_numpy(rng.integers(0, A, (int(swap.sum()), W)).astype(np.int32))
            ph, ln = ph.to(dev), [m] * P
            tp = timed(lambda: idx.search_phrases(ph, k, lengths=ln), args.iters)
            spans = idx.search_phrases(ph, k, lengths=ln)[2]
            ta = timed(lambda: idx.align_phrases(ph, spans, lengths=ln), args.iters)
            tg = timed(lambda: idx.align_phrases(ph, spans, lengths=ln, free_start=False), args.iters)
            pairs, widest = int((spans[..., 0] >= 0).sum()), int((spans[..., 1] - spans[..., 0]).max())
            row = "| %d | %d | %d | %d | %d | %s | %s | %s | %.3f |" % (W, P, m, pairs, widest, fmt(tp), fmt(ta), fmt(tg), ta[0] / tp[0])
            print(row, file=sys.stderr, flush=True)
            lines.append(row)
        del idx
    lines.append("")
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()

"""Compressed inverted-file search on one MI355X (csrc/pq.hip ``sylber_ivfpq_scan`` behind ``IVFPQSyllableIndex``) against its
yardsticks in the same process on the same box: ``PQSyllableIndex.search`` on the same codebooks (with and without re-ranking),
``IVFSyllableIndex.search`` on the same centroids and ``SyllableIndex.search``.  Seeded clustered rows on the device (the mixture of
tools/ivf_bench.py), D = 768, L2.

Prints: the builds (seconds), device bytes of each index, and for every (n, nprobe): median wall-clock milliseconds of the whole call
(coarse step, table, scan, re-rank) with re-ranking (refine 4) and without, recall@k of each against ``search``, the fraction of
(query, row) pairs scanned and the workspace; for every n the yardsticks' times and recalls.  One JSON line at the end (rows also go
to stderr as they finish); ``--md PATH`` writes the tables as markdown (profiles/ivfpq_bench.md).

``--residual`` adds a leg in the same process on the same rows, lists and queries: ``IVFPQSyllableIndex.build(..., residual=True)`` on
the first index's centroids (its own codebooks, trained on the residuals), its build time beside a non-residual build from the same
centroids, its bytes per row, and for every (n, nprobe) its times and recalls beside the non-residual figures of that run -- the only
valid comparison, boxes differ by some per cent.

    python tools/ivfpq_bench.py [--N 4194304] [--nlist 4096] [--M 48] [--ns 16,1024,8192] [--nprobes 1,8,32] [--k 10] [--iters 3]
                                [--max-iter 10] [--train-rows 262144] [--residual] [--md profiles/ivfpq_bench.md]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)          # wall clock of the whole call: IVFSyllableIndex.search has host steps
    return statistics.median(out)


def markdown(res):
    h = res
    out = ["# Compressed inverted-file search (`IVFPQSyllableIndex`) against `PQSyllableIndex`, `IVFSyllableIndex` and `search`", "",
           "`tools/ivfpq_bench.py`, one process on one MI355X: N = %d clustered synthetic rows (%s), D = %d, L2, nlist = %d, M = %d, "
           "k = %d, refine 4; median of %d whole calls (wall clock, one warm-up call)." % (h["N"], h["data"], h["D"], h["nlist"], h["M"],
                                                                                         h["k"], h["iters"]), "",
           "Builds: centroids + lists + codebooks + codes %.1f s (`IVFPQSyllableIndex.build`, k-means max_iter %d on %d training rows); "
           "`IVFSyllableIndex` from the same centroids %.1f s; `PQSyllableIndex` from the same codebooks %.1f s."
           % (h["build_s"], h["kmeans_max_iter"], h["train_rows"], h["ivf_build_s"], h["pq_build_s"]), "",
           "Device bytes: IVF-PQ without the fp32 rows %.1f MB (%.1f per row); PQ without the rows %.1f MB; the fp32 rows %.1f MB; "
           "`IVFSyllableIndex` holds the rows twice." % (h["bytes_ivfpq_codes_only"] / 1e6, h["bytes_ivfpq_codes_only"] / h["N"],
                                                          h["bytes_pq_codes_only"] / 1e6, 4.0 * h["N"] * h["D"] / 1e6), "",
           "| n | nprobe | pairs scanned | IVF-PQ re-ranked ms | recall@%d | IVF-PQ scan only ms | recall@%d | IVF (fp32 lists) ms | recall@%d |"
           % (h["k"], h["k"], h["k"]), "|---|---|---|---|---|---|---|---|---|"]
    for r in h["rows"]:
        out.append("| %d | %d | %.4f | %.2f | %.4f | %.2f | %.4f | %.2f | %.4f |" % (
            r["n"], r["nprobe"], r["fraction"], r["ivfpq_rerank_ms"], r["ivfpq_rerank_recall"], r["ivfpq_scan_only_ms"],
            r["ivfpq_scan_only_recall"], r["ivf_ms"], r["ivf_recall"]))
    out += ["", "| n | `search` ms | PQ re-ranked ms | recall@%d | PQ scan only ms | recall@%d |" % (h["k"], h["k"]), "|---|---|---|---|---|---|"]
    for r in h["yardsticks"]:
        out.append("| %d | %.2f | %.2f | %.4f | %.2f | %.4f |" % (r["n"], r["search_ms"], r["pq_rerank_ms"], r["pq_rerank_recall"],
                                                                  r["pq_scan_only_ms"], r["pq_scan_only_recall"]))
    if "residual" in h:
        r = h["residual"]
        out += ["", "Residual codes (`build(..., residual=True)`) on the same centroids, rows and queries, same run: codebooks + codes "
                "%.1f s against %.1f s for the codes of the rows themselves from the same centroids; %.1f device bytes per row without "
                "the fp32 rows against %.1f." % (r["build_s"], r["plain_build_s"], r["bytes_codes_only"] / h["N"],
                                                 h["bytes_ivfpq_codes_only"] / h["N"]), "",
                "| n | nprobe | residual re-ranked ms | today ms | residual recall@%d | today | residual scan only ms | today ms | "
                "residual recall@%d | today |" % (h["k"], h["k"]), "|---|---|---|---|---|---|---|---|---|---|"]
        for r in h["rows"]:
            out.append("| %d | %d | %.2f | %.2f | %.4f | %.4f | %.2f | %.2f | %.4f | %.4f |" % (
                r["n"], r["nprobe"], r["res_rerank_ms"], r["ivfpq_rerank_ms"], r["res_rerank_recall"], r["ivfpq_rerank_recall"],
                r["res_scan_only_ms"], r["ivfpq_scan_only_ms"], r["res_scan_only_recall"], r["ivfpq_scan_only_recall"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4194304)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--M", type=int, default=48)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ns", default="16,1024,8192")
    ap.add_argument("--nprobes", default="1,8,32")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=10)
    ap.add_argument("--train-rows", type=int, default=262144)
    ap.add_argument("--centres", type=int, default=20000)
    ap.add_argument("--residual", action="store_true")
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    from sylber_amd import IVFPQSyllableIndex, IVFSyllableIndex, PQSyllableIndex, SyllableIndex
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    N, D, M, k, refine = args.N, 768, args.M, args.k, 4
    # clustered rows: random centres with uneven weights, unit-variance noise around them
    cent = 2.0 * torch.randn(args.centres, D, device=dev, generator=g)
    w = torch.rand(args.centres, device=dev, generator=g) ** 3
    x = torch.empty(N, D, device=dev)
    for r0 in range(0, N, 1 << 19):
        m = min(1 << 19, N - r0)
        x[r0:r0 + m] = cent[torch.multinomial(w, m, replacement=True, generator=g)] + torch.randn(m, D, device=dev, generator=g)
    index = SyllableIndex(x, device=dev)
    del x

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    ix, build_s = timed(lambda: IVFPQSyllableIndex.build(index, args.nlist, M, seed=0, max_iter=args.max_iter, train_rows=args.train_rows))
    ivf, ivf_s = timed(lambda: IVFSyllableIndex.build(index, centroids=ix.centroids))
    pq, pq_s = timed(lambda: PQSyllableIndex.build(index, M, codebooks=ix.codebooks))
    sizes = ix.list_sizes.cpu().numpy()
    head = {"D": D, "metric": "l2", "N": N, "nlist": args.nlist, "M": M, "k": k, "refine": refine, "iters": args.iters,
            "build_s": round(build_s, 2), "ivf_build_s": round(ivf_s, 2), "pq_build_s": round(pq_s, 2), "kmeans_max_iter": args.max_iter,
            "train_rows": args.train_rows, "bytes_ivfpq_with_rows": ix.nbytes, "bytes_ivfpq_codes_only": ix.nbytes - 4 * N * D,
            "bytes_pq_codes_only": pq.nbytes - 4 * N * D, "list_rows_min_median_max": [int(sizes.min()), int(statistics.median(sizes)), int(sizes.max())],
            "data": "synthetic mixture of %d Gaussians" % args.centres}
    rx = None
    if args.residual:
        kw = dict(centroids=ix.centroids, seed=0, max_iter=args.max_iter, train_rows=args.train_rows)
        rx, res_s = timed(lambda: IVFPQSyllableIndex.build(index, None, M, residual=True, **kw))
        plain_s = timed(lambda: IVFPQSyllableIndex.build(index, None, M, **kw))[1]       # built for its time only
        head["residual"] = {"build_s": round(res_s, 2), "plain_build_s": round(plain_s, 2), "bytes_codes_only": rx.nbytes - 4 * N * D}
    print(json.dumps(head), file=sys.stderr, flush=True)
    rows, yard = [], []
    for n in [int(v) for v in args.ns.split(",")]:
        q = index.features[torch.randint(0, N, (n,), device=dev, generator=g)] + 0.5 * torch.randn(n, D, device=dev, generator=g)
        ei = index.search(q, k)[1]
        recall = lambda ids: round(float((ids[:, :, None] == ei[:, None, :]).any(1).float().mean()), 4)
        y = {"n": n, "search_ms": round(median_ms(lambda: index.search(q, k), args.iters), 3),
             "pq_rerank_ms": round(median_ms(lambda: pq.search(q, k, refine), args.iters), 3),
             "pq_rerank_recall": recall(pq.search(q, k, refine)[1]),
             "pq_scan_only_ms": round(median_ms(lambda: pq.search(q, k, rerank=False), args.iters), 3),
             "pq_scan_only_recall": recall(pq.search(q, k, rerank=False)[1])}
        print(json.dumps(y), file=sys.stderr, flush=True)
        yard.append(y)
        for nprobe in [int(v) for v in args.nprobes.split(",")]:
            row = {"n": n, "nprobe": nprobe,
                   "ivfpq_rerank_ms": round(median_ms(lambda: ix.search(q, k, nprobe, refine), args.iters), 3),
                   "ivfpq_rerank_recall": recall(ix.search(q, k, nprobe, refine)[1]),
                   "ivfpq_scan_only_ms": round(median_ms(lambda: ix.search(q, k, nprobe, rerank=False), args.iters), 3),
                   "ivfpq_scan_only_recall": recall(ix.search(q, k, nprobe, rerank=False)[1])}
            ls = ix.last_search
            row.update({"fraction": round(ls["fraction"], 5), "workspace_mb": round(ls["workspace_bytes"] / 2 ** 20, 2),
                        "ivf_ms": round(median_ms(lambda: ivf.search(q, k, nprobe), args.iters), 3),
                        "ivf_recall": recall(ivf.search(q, k, nprobe)[1])})
            if rx is not None:
                row.update({"res_rerank_ms": round(median_ms(lambda: rx.search(q, k, nprobe, refine), args.iters), 3),
                            "res_rerank_recall": recall(rx.search(q, k, nprobe, refine)[1]),
                            "res_scan_only_ms": round(median_ms(lambda: rx.search(q, k, nprobe, rerank=False), args.iters), 3),
                            "res_scan_only_recall": recall(rx.search(q, k, nprobe, rerank=False)[1])})
            print(json.dumps(row), file=sys.stderr, flush=True)
            rows.append(row)
        del q
    res = dict(head, rows=rows, yardsticks=yard)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as fh:
            fh.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

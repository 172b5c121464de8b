"""Inverted-file search on one MI355X (csrc/knn.hip ``sylber_ivf_search`` behind ``IVFSyllableIndex``) against the exact search
(``SyllableIndex.search``) on the same rows and queries in the same process.  Seeded clustered rows on the device, D = 768, L2.

Build time (k-means, assign, layout) is reported apart from search time.  Per (n, nprobe): median milliseconds of
``ivf.search`` (coarse step, pair grouping and work-item table included) and of ``index.search``, the fraction of (query, row) pairs
scanned, the rate on scanned pairs (2 x pairs x D / time) beside the exact search's rate (2 n N D / time), recall@k against the
exact ids and the workspace.  One self-search chunk (rows of the database as queries, ``exclude_same_group``) closes the table.
Prints one JSON line (rows also go to stderr as they finish).

    python tools/ivf_bench.py [--N 4194304] [--nlist 4096] [--k 10] [--ns 16,1024,8192] [--nprobes 1,8,32,128] [--self-n 65536]
                              [--iters 5] [--exact-iters 2] [--max-iter 10] [--train-rows 524288]"""
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
        out.append((time.perf_counter() - t0) * 1e3)          # wall clock: the search has host steps between its launches
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4194304)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ns", default="16,1024,8192")
    ap.add_argument("--nprobes", default="1,8,32,128")
    ap.add_argument("--self-n", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--exact-iters", type=int, default=2)
    ap.add_argument("--max-iter", type=int, default=10)
    ap.add_argument("--train-rows", type=int, default=524288)
    ap.add_argument("--centres", type=int, default=20000)
    args = ap.parse_args()
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    N, D, k = args.N, 768, args.k
    # clustered rows: random centres with uneven weights, unit-variance noise around them
    cent = 2.0 * torch.randn(args.centres, D, device=dev, generator=g)
    w = torch.rand(args.centres, device=dev, generator=g) ** 3
    x = torch.empty(N, D, device=dev)
    for r0 in range(0, N, 1 << 19):
        m = min(1 << 19, N - r0)
        x[r0:r0 + m] = cent[torch.multinomial(w, m, replacement=True, generator=g)] + torch.randn(m, D, device=dev, generator=g)
    groups = torch.arange(N, device=dev, dtype=torch.int32) // 32            # "clips" of 32 consecutive rows
    index = SyllableIndex(x, groups=groups, device=dev)
    del x
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ivf = IVFSyllableIndex.build(index, nlist=args.nlist, seed=0, max_iter=args.max_iter, train_rows=args.train_rows)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    sizes = ivf.list_sizes.cpu()
    head = {"D": D, "metric": "l2", "N": N, "nlist": args.nlist, "k": k, "build_s": round(build_s, 2), "kmeans_max_iter": args.max_iter,
            "train_rows": args.train_rows, "list_rows_min": int(sizes.min()), "list_rows_median": int(sizes.median()),
            "list_rows_max": int(sizes.max()), "data": "synthetic mixture of %d Gaussians" % args.centres}
    print(json.dumps(head), file=sys.stderr, flush=True)
    rows = []

    def measure(q, qg, label):
        n = q.shape[0]
        kw = {} if qg is None else {"groups": qg, "exclude_same_group": True}
        t_exact = median_ms(lambda: index.search(q, k, **kw), args.exact_iters)
        exact = index.search(q, k, **kw)[1]
        for nprobe in [int(v) for v in args.nprobes.split(",")]:
            if nprobe > min(args.nlist, 128):
                continue
            t = median_ms(lambda: ivf.search(q, k, nprobe=nprobe, **kw), args.iters)
            ids = ivf.search(q, k, nprobe=nprobe, **kw)[1]
            ls = ivf.last_search
            recall = float(((ids[:, :, None] == exact[:, None, :]) & (exact[:, None, :] >= 0)).any(1).sum()) / max(1, int((exact >= 0).sum()))
            row = {"queries": label, "n": n, "nprobe": nprobe, "ivf_ms": round(t, 3), "exact_ms": round(t_exact, 3),
                   "speedup": round(t_exact / t, 2), "fraction": round(ls["fraction"], 6), "items": ls["items"],
                   "ivf_tflops_scanned": round(2.0 * ls["pairs"] * D / t / 1e9, 2), "exact_tflops": round(2.0 * n * N * D / t_exact / 1e9, 1),
                   "recall_at_k": round(recall, 4), "workspace_mb": round(ls["workspace_bytes"] / 2 ** 20, 2)}
            print(json.dumps(row), file=sys.stderr, flush=True)
            rows.append(row)

    for n in [int(v) for v in args.ns.split(",")]:
        pick = torch.randint(0, N, (n,), device=dev, generator=g)
        q = index.features[pick] + 0.5 * torch.randn(n, D, device=dev, generator=g)
        measure(q, None, "near database rows")
    if args.self_n:
        m = min(args.self_n, N)
        measure(index.features[:m], groups[:m].cpu().numpy(), "self-search chunk")
    gate = [r for r in rows if r["n"] >= 1024 and r["nprobe"] * 128 <= args.nlist]
    head.update({"rows": rows, "gate_rows": len(gate), "gate_ivf_faster_than_exact": bool(gate) and all(r["ivf_ms"] < r["exact_ms"] for r in gate)})
    print(json.dumps(head))


if __name__ == "__main__":
    main()

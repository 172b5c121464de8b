"""Product-quantized search on one MI355X (csrc/pq.hip, ``PQSyllableIndex``) against ``SyllableIndex.search`` and ``search_refined`` in
the same process.  Seeded clustered rows on the device (the mixture of tools/ivf_bench.py), D = 768, L2.

Prints: the build (``M`` k-means fits and the encode, seconds), the encode alone (ms, rows / s), bytes held with and without the
fp32 rows, and for every n: median milliseconds (device events, one warm-up call) of ``search``, ``search_refined`` (fp16, refine 4),
``pq.search`` with re-ranking (refine 4 and 12) and without, the scan's two C entry points on their own (``sylber_pq_lut``,
``sylber_pq_scan`` with look-ups / s on ``n N M``), and recall@k against ``search`` of each.  One JSON line at the end (rows also go to
stderr as they finish).

    python tools/pq_bench.py [--N 4194304] [--M 48] [--ns 16,1024,8192] [--k 10] [--iters 3] [--max-iter 10] [--train-rows 262144]"""
import argparse
import ctypes
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
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4194304)
    ap.add_argument("--M", type=int, default=48)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ns", default="16,1024,8192")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=10)
    ap.add_argument("--train-rows", type=int, default=262144)
    ap.add_argument("--centres", type=int, default=20000)
    args = ap.parse_args()
    from sylber_amd import PQSyllableIndex, SyllableIndex, _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device=dev).manual_seed(0)
    N, D, M, k = args.N, 768, args.M, args.k
    # clustered rows: random centres with uneven weights, unit-variance noise around them
    cent = 2.0 * torch.randn(args.centres, D, device=dev, generator=g)
    w = torch.rand(args.centres, device=dev, generator=g) ** 3
    x = torch.empty(N, D, device=dev)
    for r0 in range(0, N, 1 << 19):
        m = min(1 << 19, N - r0)
        x[r0:r0 + m] = cent[torch.multinomial(w, m, replacement=True, generator=g)] + torch.randn(m, D, device=dev, generator=g)
    index = SyllableIndex(x, device=dev)
    del x
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pq = PQSyllableIndex.build(index, M, seed=0, max_iter=args.max_iter, train_rows=args.train_rows)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    t_enc = median_ms(lambda: pq.encode(index.features, _stored=True), args.iters)
    head = {"D": D, "metric": "l2", "N": N, "M": M, "k": k, "build_s": round(build_s, 2), "kmeans_max_iter": args.max_iter,
            "train_rows": args.train_rows, "encode_ms": round(t_enc, 2), "encode_rows_per_s": round(N / t_enc * 1e3),
            "bytes_with_rows": pq.nbytes, "bytes_codes_only": pq.nbytes - 4 * N * D, "bytes_per_row_codes": M,
            "bad_rows": int(pq._bad.sum()), "data": "synthetic mixture of %d Gaussians" % args.centres}
    print(json.dumps(head), file=sys.stderr, flush=True)
    index.half_rows("fp16")
    rows = []
    for n in [int(v) for v in args.ns.split(",")]:
        q = index.features[torch.randint(0, N, (n,), device=dev, generator=g)] + 0.5 * torch.randn(n, D, device=dev, generator=g)
        ei = index.search(q, k)[1]
        recall = lambda ids: round(float((ids[:, :, None] == ei[:, None, :]).any(1).float().mean()), 4)
        row = {"n": n, "search_ms": round(median_ms(lambda: index.search(q, k), args.iters), 3),
               "refined_fp16_r4_ms": round(median_ms(lambda: index.search_refined(q, k, 4), args.iters), 3),
               "refined_fp16_r4_recall": recall(index.search_refined(q, k, 4)[1])}
        for refine in (4, 12):
            row["pq_rerank_r%d_ms" % refine] = round(median_ms(lambda: pq.search(q, k, refine), args.iters), 3)
            row["pq_rerank_r%d_recall" % refine] = recall(pq.search(q, k, refine)[1])
        row["pq_scan_only_ms"] = round(median_ms(lambda: pq.search(q, k, rerank=False), args.iters), 3)
        row["pq_scan_only_recall"] = recall(pq.search(q, k, rerank=False)[1])
        mc = 4 * k
        lut = torch.empty((n, M, 256), dtype=torch.float32, device=dev)
        ws = torch.empty(int(lib.sylber_pq_workspace_bytes(n, N, M, mc, 0)), dtype=torch.uint8, device=dev)
        tt = torch.empty((n, mc), dtype=torch.float32, device=dev)
        cand = torch.empty((n, mc), dtype=torch.int32, device=dev)
        t_lut = median_ms(lambda: _lib.check(lib.sylber_pq_lut(vp(q), n, D, vp(pq.codebooks), vp(pq._cnorm), M, 0, vp(lut), stream()),
                                             "sylber_pq_lut"), args.iters)
        t_scan = median_ms(lambda: _lib.check(lib.sylber_pq_scan(vp(lut), n, vp(pq.codes), vp(pq._bad), N, M, mc, None, None, 0, vp(tt), vp(cand),
                                                                 vp(ws), stream()), "sylber_pq_scan"), args.iters)
        row.update({"lut_ms": round(t_lut, 3), "scan_m40_ms": round(t_scan, 3), "scan_glookups_per_s": round(n * N * M / t_scan / 1e6, 1),
                    "table_mb": round(lut.numel() * 4 / 2 ** 20, 1), "workspace_mb": round(ws.numel() / 2 ** 20, 2)})
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
        del lut, ws, q
    print(json.dumps(dict(head, rows=rows)))


if __name__ == "__main__":
    main()

"""Two-stage k-NN search on one MI355X (csrc/knn16.hip, ``SyllableIndex.search_refined``) against the exact ``search`` in the same
process, seeded random data on the device, D = 768, L2.

For every N (database rows) x n (queries) x k: median milliseconds (device events, one warm-up call) of
  * search: ``SyllableIndex.search`` (the exact fp32 MFMA scan), once per (n, N, k);
  * refined: the whole ``search_refined`` call for each storage (fp16, bf16) and refine, timed alternately with ``search`` (A B A B;
    medians and min / max of both, ``speedup_worst`` = fastest search / slowest refined), then its two stages through the C entry points: ``sylber_knn16_scan`` (with TFLOP/s on 2 n N D and its workspace) and ``sylber_knn_rerank``;
    ``speedup`` = search_ms / refined_ms, recall@k = the share of ``search``'s ids that ``search_refined`` returns;
  * torch: chunked bf16 ``matmul`` + ``topk`` (chunks of queries holding at most 2^30 scores), once per (n, N, k).
Prints one JSON line (rows also go to stderr as they finish).

    python tools/knn16_bench.py [--iters 5] [--ns 16,1024,8192] [--Ns 262144,4194304] [--shapes 1:1,1:2,1:4,1:8,10:1,...] [--no-torch]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_SHAPES = ",".join("%d:%d" % (k, r) for k in (1, 10) for r in (1, 2, 4, 8)) + ",32:4"


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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternating_ms(fa, fb, iters):
    """both warmed, then A B A B ...: (times of A, times of B), so that drift of the box hits both alike"""
    fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(iters):
        ta.append(timed(fa))
        tb.append(timed(fb))
    return ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--ns", default="16,1024,8192")
    ap.add_argument("--Ns", default="262144,4194304")
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="k:refine pairs")
    ap.add_argument("--storages", default="fp16,bf16")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from sylber_amd import SyllableIndex, _lib
    from sylber_amd._index import _pack16
    from sylber_amd.search import STORAGES
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device=dev).manual_seed(0)
    D = 768
    shapes = [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    rows = []
    for N in [int(v) for v in args.Ns.split(",")]:
        x = torch.randn(N, D, device=dev, generator=g)
        idx = SyllableIndex(x, device=dev)
        for st in args.storages.split(","):
            idx.half_rows(st)
        xb = None if args.no_torch else idx.half_rows("bf16") if "bf16" in args.storages else x.to(torch.bfloat16)
        for n in [int(v) for v in args.ns.split(",")]:
            q = x[torch.randint(0, N, (n,), device=dev, generator=g)] + 0.5 * torch.randn(n, D, device=dev, generator=g)
            fl = 2.0 * n * N * D
            exact = {}
            for k in sorted({k for k, _ in shapes}):
                t = median_ms(lambda: idx.search(q, k), args.iters)
                exact[k] = (t, idx.search(q, k)[1])
                row = {"n": n, "N": N, "k": k, "what": "search", "ms": round(t, 3), "tflops": round(fl / t / 1e9, 1)}
                if not args.no_torch:
                    chunk = max(1, min(n, (1 << 30) // N))
                    qb = q.to(torch.bfloat16)

                    def ref():
                        for r0 in range(0, n, chunk):
                            s = torch.matmul(qb[r0:r0 + chunk], xb.t())
                            torch.topk(s, k, dim=1)
                            del s
                    t_ref = median_ms(ref, args.iters)
                    row.update({"torch_bf16_ms": round(t_ref, 3), "torch_bf16_tflops": round(fl / t_ref / 1e9, 1)})
                print(json.dumps(row), file=sys.stderr, flush=True)
                rows.append(row)
            for st in args.storages.split(","):
                code = STORAGES[st][0]
                q16 = _pack16(q, st, refuse=False)
                for k, refine in shapes:
                    m = k * refine
                    ts, tr = alternating_ms(lambda: idx.search(q, k), lambda: idx.search_refined(q, k, refine, st), args.iters)
                    t, t_search = statistics.median(tr), statistics.median(ts)
                    ids = idx.search_refined(q, k, refine, st)[1]
                    ei = exact[k][1]
                    recall = float((ids[:, :, None] == ei[:, None, :]).any(1).float().mean())
                    ws_bytes = int(lib.sylber_knn16_workspace_bytes(n, N, D, m, 0))
                    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
                    cand = torch.empty((n, m), dtype=torch.int32, device=dev)
                    so = torch.empty((n, k), dtype=torch.float32, device=dev)
                    io = torch.empty((n, k), dtype=torch.int64, device=dev)
                    scan = lambda: _lib.check(lib.sylber_knn16_scan(vp(q16), n, vp(idx.half_rows(st)), N, D, vp(idx._c), code, m, None, None, 0,
                                                                    vp(cand), vp(ws), stream()), "sylber_knn16_scan")
                    rerank = lambda: _lib.check(lib.sylber_knn_rerank(vp(q), n, vp(idx._x), N, D, vp(idx._c), 0, vp(cand), m, k, vp(so), vp(io),
                                                                      stream()), "sylber_knn_rerank")
                    t_scan = median_ms(scan, args.iters)
                    t_rr = median_ms(rerank, args.iters)
                    row = {"n": n, "N": N, "k": k, "what": "refined", "storage": st, "refine": refine, "m": m, "ms": round(t, 3),
                           "scan_ms": round(t_scan, 3), "rerank_ms": round(t_rr, 3), "scan_tflops": round(fl / t_scan / 1e9, 1),
                           "workspace_mb": round(ws_bytes / 2 ** 20, 2), "splits": int(lib.sylber_knn_splits(n, N, 0)),
                           "ms_min_max": [round(min(tr), 3), round(max(tr), 3)], "search_ms": round(t_search, 3),
                           "search_ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "speedup": round(t_search / t, 2),
                           "speedup_worst": round(min(ts) / max(tr), 2), "recall": round(recall, 4),
                           "ids_equal_search": bool(torch.equal(ids, ei))}
                    print(json.dumps(row), file=sys.stderr, flush=True)
                    rows.append(row)
                    del ws
                del q16
            del q
        del x, idx, xb
        torch.cuda.empty_cache()
    print(json.dumps({"D": D, "metric": "l2", "rows": rows}))


if __name__ == "__main__":
    main()

"""Exact k-NN search on one MI355X (csrc/knn.hip, ``sylber_knn_search``), seeded random data on the device, D = 768.

For every n (queries) x N (database rows) x k: median milliseconds and TFLOP/s (2 n N D per call) of
  * knn: ``sylber_knn_search`` (L2, automatic splits), with its workspace and split count;
  * kmeans_assign: ``sylber_kmeans_assign`` of the same queries against the same rows as centroids (the k = 1 contraction, one
    workgroup per 128 queries, no splits), once per (n, N);
  * torch: chunked ``||x||^2 - 2 q x^T`` (fp32 ``torch.mm``) + ``torch.topk``, chunks of queries holding at most 2^30 scores, with
    its peak extra device memory.
knn's k = 1 ids are checked against kmeans_assign's labels.  Prints one JSON line (rows also go to stderr as they finish).

    python tools/knn_bench.py [--iters 5] [--ns 16,1024,8192] [--Ns 262144,4194304] [--ks 1,10,100] [--no-torch]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--base-iters", type=int, default=2)
    ap.add_argument("--ns", default="16,1024,8192")
    ap.add_argument("--Ns", default="262144,4194304")
    ap.add_argument("--ks", default="1,10,100")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from sylber_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device=dev).manual_seed(0)
    D = 768
    rows = []
    for N in [int(v) for v in args.Ns.split(",")]:
        x = torch.randn(N, D, device=dev, generator=g)
        cn = torch.empty(N, dtype=torch.float32, device=dev)
        _lib.check(lib.sylber_knn_row_norms(vp(x), N, D, vp(cn), stream()), "sylber_knn_row_norms")
        for n in [int(v) for v in args.ns.split(",")]:
            q = x[torch.randint(0, N, (n,), device=dev, generator=g)] + 0.5 * torch.randn(n, D, device=dev, generator=g)
            fl = 2.0 * n * N * D
            # the k = 1 contraction with its per-row arg-min, same queries and rows
            lab = torch.empty(n, dtype=torch.int32, device=dev)
            dmin = torch.empty(n, dtype=torch.float32, device=dev)
            kws = torch.empty(int(lib.sylber_kmeans_assign_workspace_floats(n, N, D)), dtype=torch.float32, device=dev)
            km = lambda: _lib.check(lib.sylber_kmeans_assign(vp(q), n, vp(x), N, D, vp(lab), vp(dmin), None, None, None, vp(kws), stream()),
                                    "sylber_kmeans_assign")
            t_km = median_ms(km, args.base_iters)
            del kws
            for k in [int(v) for v in args.ks.split(",")]:
                ws_bytes = int(lib.sylber_knn_workspace_bytes(n, N, D, k, 0))
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
                so = torch.empty((n, k), dtype=torch.float32, device=dev)
                io = torch.empty((n, k), dtype=torch.int64, device=dev)
                run = lambda: _lib.check(lib.sylber_knn_search(vp(q), n, vp(x), N, D, vp(cn), 0, k, None, None, 0, vp(so), vp(io), vp(ws),
                                                               stream()), "sylber_knn_search")
                t = median_ms(run, args.iters)
                row = {"n": n, "N": N, "k": k, "splits": int(lib.sylber_knn_splits(n, N, 0)),
                       "grid": int((n + 127) // 128 * lib.sylber_knn_splits(n, N, 0)), "knn_ms": round(t, 3),
                       "knn_tflops": round(fl / t / 1e9, 1), "knn_workspace_mb": round(ws_bytes / 2 ** 20, 2),
                       "kmeans_assign_ms": round(t_km, 3), "kmeans_assign_tflops": round(fl / t_km / 1e9, 1),
                       "knn_over_kmeans_assign": round(t_km / t, 3)}
                if k == 1:
                    row["k1_ids_equal_kmeans_assign"] = bool(torch.equal(io[:, 0], lab.to(torch.int64)))
                del ws
                if not args.no_torch:
                    chunk = max(1, min(n, (1 << 30) // N))

                    def ref():
                        for r0 in range(0, n, chunk):
                            s = torch.addmm(cn[None, :], q[r0:r0 + chunk], x.t(), alpha=-2.0)
                            torch.topk(s, k, dim=1, largest=False)
                            del s
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats(dev)
                    base = torch.cuda.memory_allocated(dev)
                    t_ref = median_ms(ref, args.base_iters)
                    row.update({"torch_ms": round(t_ref, 3), "torch_tflops": round(fl / t_ref / 1e9, 1),
                                "torch_peak_extra_mb": round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, 1),
                                "torch_query_chunk": chunk})
                print(json.dumps(row), file=sys.stderr, flush=True)
                rows.append(row)
            del q
        del x, cn
        torch.cuda.empty_cache()
    print(json.dumps({"D": D, "metric": "l2", "rows": rows}))


if __name__ == "__main__":
    main()

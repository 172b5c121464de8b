"""k-means fitting on one MI355X (csrc/kmeans.hip), seeded random data on the device.

  * assign: the fused assign (``sylber_kmeans_assign``: labels, d_min, inertia, no [n, K] matrix) against the ``sylber_km_assign``
    path (exact-fp32 GEMM into an [n, K] dot matrix, then the arg-min kernel) at n = 262 144, D = 768, K in {1 024, 10 000, 20 000}:
    median milliseconds and TFLOP/s (2 n K D per call);
  * iteration: one full Lloyd iteration (assign with the changed-row count, stable sort of the labels, centroid update) at
    n = 4 M, K = 10 000, D = 768, with the workspace it used; the sylber_km_assign path would need n K 4 bytes for the dots alone.

Prints one JSON line.   python tools/kmeans_bench.py [--iters 5] [--n 262144] [--big-n 4194304] [--big-k 10000]"""
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
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--ks", default="1024,10000,20000")
    ap.add_argument("--big-n", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--big-k", type=int, default=10000)
    args = ap.parse_args()
    from sylber_amd import _lib
    from sylber_amd import kmeans as KM
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device=dev).manual_seed(0)
    D, n = 768, args.n
    x = torch.randn(n, D, device=dev, generator=g)
    res = {"n": n, "D": D, "assign": []}
    for K in [int(k) for k in args.ks.split(",")]:
        c = torch.randn(K, D, device=dev, generator=g)
        idx_old = torch.empty(n, dtype=torch.int32, device=dev)
        ws_old = torch.empty(int(lib.sylber_km_workspace_floats(n, K, D)), dtype=torch.float32, device=dev)
        old = lambda: _lib.check(lib.sylber_km_assign(vp(x), n, vp(c), K, D, 0, vp(idx_old), vp(ws_old), stream()), "sylber_km_assign")
        t_old = median_ms(old, args.iters)
        del ws_old
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        dmin = torch.empty(n, dtype=torch.float32, device=dev)
        inertia = torch.empty(1, dtype=torch.float64, device=dev)
        ws = torch.empty(int(lib.sylber_kmeans_assign_workspace_floats(n, K, D)), dtype=torch.float32, device=dev)
        new = lambda: _lib.check(lib.sylber_kmeans_assign(vp(x), n, vp(c), K, D, vp(idx), vp(dmin), vp(inertia), None, None, vp(ws),
                                                          stream()), "sylber_kmeans_assign")
        t_new = median_ms(new, args.iters)
        same = bool(torch.equal(idx, idx_old))
        fl = 2.0 * n * K * D
        row = {"K": K, "fused_ms": round(t_new, 3), "fused_tflops": round(fl / t_new / 1e9, 1), "km_assign_ms": round(t_old, 3),
               "km_assign_tflops": round(fl / t_old / 1e9, 1), "labels_equal": same, "fused_workspace_mb": round(ws.numel() * 4 / 2 ** 20, 2),
               "km_assign_workspace_mb": round(int(lib.sylber_km_workspace_floats(n, K, D)) * 4 / 2 ** 20, 1)}
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["assign"].append(row)
        del c, ws
    del x
    torch.cuda.empty_cache()

    N, K = args.big_n, args.big_k
    x = torch.randn(N, D, device=dev, generator=g)
    c = x[torch.randperm(N, device=dev, generator=g)[:K]].contiguous()
    prev = KM.assign(x, c)[0]
    torch.cuda.synchronize()

    def iteration():
        labels, _, _, _ = KM.assign(x, c, prev)
        KM.update(x, labels, c)

    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t_it = median_ms(iteration, max(1, args.iters // 2))
    peak = torch.cuda.max_memory_allocated(dev) - base
    res["iteration"] = {"n": N, "K": K, "D": D, "ms": round(t_it, 1), "assign_tflops_equiv": round(2.0 * N * K * D / t_it / 1e9, 1),
                        "extra_device_mb": round(peak / 2 ** 20, 1),
                        "assign_workspace_mb": round(int(lib.sylber_kmeans_assign_workspace_floats(N, K, D)) * 4 / 2 ** 20, 1),
                        "update_workspace_mb": round(int(lib.sylber_kmeans_update_workspace_bytes(N, K, D)) / 2 ** 20, 1),
                        "km_assign_dots_gb": round(N * K * 4 / 1e9, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

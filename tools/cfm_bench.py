"""Resynthesis decoder throughput on one MI355X: ``sylber_cfm_sample`` (csrc/cfm.hip) on a 32 x 10 s batch (499 frames, rows of
16 register tokens + 499 frames) with steps = 5 (8 evaluations), against the same decoder in torch eager (tests/cfm_ref.py under
bf16 autocast: hipBLASLt GEMMs) on the same box.  Prints one JSON line.

    python tools/cfm_bench.py [--batch 32] [--frames 499] [--steps 5] [--iters 10] [--precision bf16]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_BF16_TF = 2500.0     # dense bf16 / fp16 MFMA peak of the MI355X, TFLOP/s


def flops_per_eval(B, T):
    """useful FLOPs of one decoder evaluation: the four GEMMs of 8 layers on B (16 + T) rows at their true widths, and the
    attention's two contractions over 8 heads x 64"""
    L = 16 + T
    M = B * L
    gemm = 2.0 * M * 512 * (1536 + 512 + 2730) * 8 + 2.0 * M * 1365 * 512 * 8
    attn = 4.0 * B * 8 * L * L * 64 * 8
    return gemm, attn


def time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=499)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--no-eager", action="store_true")
    args = ap.parse_args()
    from sylber_amd.synthesis import CfmDecoder
    from sylber_amd.weights import synthetic_regressor_state_dict
    sd = synthetic_regressor_state_dict(0)
    B, T, steps = args.batch, args.frames, args.steps
    g = torch.Generator().manual_seed(0)
    cond = torch.randn(B, T, 256, generator=g).cuda()
    dec = CfmDecoder(sd, device="cuda:0", precision=args.precision)
    run = lambda: dec.sample(cond, steps=steps)          # noqa: E731
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ms = time_ms(run, args.iters)
    evals = 2 * (steps - 1)
    gemm, attn = flops_per_eval(B, T)
    out = {"metric": "cfm_sample_ms", "batch": B, "frames": T, "steps": steps, "precision": args.precision, "ms": round(ms, 3),
           "audio_s_per_s": round(B * T / 50.0 / (ms / 1e3), 1), "tflop_per_call": round(evals * (gemm + attn) / 1e12, 3),
           "tflops": round(evals * (gemm + attn) / (ms / 1e3) / 1e12, 1),
           "frac_of_bf16_peak": round(evals * (gemm + attn) / (ms / 1e3) / 1e12 / PEAK_BF16_TF, 4)}
    if not args.no_eager:
        import cfm_ref as R
        sdg = {k: v.cuda() for k, v in sd.items()}
        with torch.autocast("cuda", dtype=torch.bfloat16):
            eager = lambda: R.sample(sdg, cond, steps)    # noqa: E731
            eager()
            torch.cuda.synchronize()
            ems = time_ms(eager, max(2, args.iters // 3))
        out["eager_bf16_ms"] = round(ems, 3)
        out["speedup_vs_eager"] = round(ems / ms, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

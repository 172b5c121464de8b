"""(B, clip seconds) sweep of the resident step: is the GEMM scheduling shape-robust, or does the 32 x 10 s headline sit on a sweet spot?

For every grid point the step is timed exactly like bench.py's `other_configs` (two batches in flight on independent handles, boundary
detection on side streams, inputs resident in HBM), followed by a sequential profiling pass for the per-launch TFLOP/s of the four
encoder GEMMs.  The table's last column is the rate per FRAME relative to the 32 x 10 s point of the same run (same box, same clocks):
VERDICT r5 item 1 asks that no point with B x T >= 8192 frames falls more than 8 % below it.

    python tools/shape_sweep.py [--precision bf16] [--batches 8,16,24,32,48,64] [--seconds 5,10,15,30,60] [--opt KEY=VALUE ...] > profiles/r06_shape_sweep.md
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batches", default="8,16,24,32,48,64")
    ap.add_argument("--seconds", default="5,10,15,30,60")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE")
    ap.add_argument("--json", default="", help="also write the raw records here")
    args = ap.parse_args()
    import torch
    import bench
    from sylber_amd import HubertEncoderHIP
    from sylber_amd.streams import concurrent_streams
    from sylber_amd.weights import synthetic_state_dict

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sd = synthetic_state_dict(0)
    streams4 = concurrent_streams(4, dev)
    opts = [tuple(int(x) for x in kv.split("=")) for kv in args.opt]
    if opts:                                                    # A/B switches reach every handle measure_other_config creates
        orig = HubertEncoderHIP.__init__

        def patched(self, *a, **k):
            orig(self, *a, **k)
            for key, val in opts:
                self.set_option(key, val)
        HubertEncoderHIP.__init__ = patched
    grid = [(b, s) for s in (float(x) for x in args.seconds.split(",")) for b in (int(x) for x in args.batches.split(","))]
    if (32, 10.0) not in grid:
        grid.insert(0, (32, 10.0))
    recs = {}
    for b, s in grid:
        r = bench.measure_other_config(torch, dev, sd, streams4, args.precision, b, s, steps=args.steps, warmup=3)
        recs[(b, s)] = r
        sys.stderr.write("%d x %g s: %.3f ms\n" % (b, s, r["ms_per_step"]))
    ref = recs[(32, 10.0)]
    ref_rate = 32 * ref["frames_per_clip"] / ref["ms_per_step"]          # frames per ms
    print("# (B, seconds) sweep, precision=%s%s" % (args.precision, (", options " + " ".join(args.opt)) if args.opt else ""))
    print()
    print("| B | s | frames | ms/step | audio-s/s | q,k,v TF | out TF | FFN1 TF | FFN2 TF | enc GEMM frac | attn TF | frames/ms vs 32x10s |")
    print("|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    worst = None
    for (b, s), r in recs.items():
        eg = r["roofline"].get("encoder_gemms", {})
        pl = eg.get("per_launch_tflops", {})
        at = r["roofline"].get("attention") or {}
        frames = b * r["frames_per_clip"]
        rel = frames / r["ms_per_step"] / ref_rate
        if frames >= 8192 and (worst is None or rel < worst[0]):
            worst = (rel, b, s)
        print("| %d | %g | %d | %.3f | %.0f | %.0f | %.0f | %.0f | %.0f | %.4f | %.0f | %.3f |" % (
            b, s, frames, r["ms_per_step"], r["value"], pl.get("gemm_qkv", 0), pl.get("gemm_out", 0), pl.get("gemm_ffn1", 0),
            pl.get("gemm_ffn2", 0), eg.get("frac", 0), at.get("achieved", 0), rel))
    print()
    if worst:
        print("worst point with >= 8192 frames: %d x %g s at %.3f of the 32 x 10 s rate per frame" % (worst[1], worst[2], worst[0]))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"%dx%g" % k: v for k, v in recs.items()}, fh)


if __name__ == "__main__":
    main()

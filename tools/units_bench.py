"""Syllable-unit path on one MI355X, 32 x 10 s clips (499 frames each), steps = 5, synthetic seeded weights and codebooks
[64, 768] + [32, 768] at the hidden states' scale (a ResidualKMQuantizer).  Median milliseconds per call of:

  * ``synthesize_units``  units -> art with the fused conditioning (MLP on B*S + 1 unit rows, csrc/downstream.hip);
  * ``features_path``     what a caller does without it: ``decode`` on the device, upstream's expand_feature layout built in torch
                          on the device (``repeat_interleave``), then ``resynthesize(features=...)`` (MLP on B*T frame rows);
  * ``features_path_dev`` the same with the device ``expand_feature`` (``sylber_expand_units``);
  * ``tokenize``          wav -> units, against ``encoder_segment``: the encoder forward + segmentation share of ``resynthesize``.

Prints one JSON line.   python tools/units_bench.py [--batch 32] [--seconds 10] [--iters 20] [--precision bf16]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, iters):
    for _ in range(2):
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


def torch_expand(avg, dur):
    """upstream's duration layout, built with torch ops on the device: unit row then zero row, repeated by their durations"""
    B, S, D = avg.shape
    pairs = torch.stack([avg, torch.zeros_like(avg)], 2).reshape(B, 2 * S, D)
    reps = dur.reshape(B, 2 * S)
    return torch.stack([torch.repeat_interleave(pairs[b], reps[b], dim=0) for b in range(B)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--precision", default="bf16")
    args = ap.parse_args()
    import units_ref as U
    from sylber_amd import ResidualKMQuantizer, SegmentSynthesis, expand_feature
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_mlp_state_dict, synthetic_regressor_state_dict, synthetic_state_dict
    sd = {"speech_model." + k: v for k, v in synthetic_state_dict(0, num_layers=9).items()}
    sd.update({"input_model." + k: v for k, v in synthetic_mlp_state_dict(1).items()})
    sd.update({"regressor." + k: v for k, v in synthetic_regressor_state_dict(0).items()})
    g = torch.Generator().manual_seed(11)
    c1, c2 = torch.randn(64, 768, generator=g) * 0.09, torch.randn(32, 768, generator=g) * 0.03   # the hidden states' scale
    syn = SegmentSynthesis(model_ckpt=sd, device="cuda:0", precision=args.precision, quantizer=ResidualKMQuantizer(c1, c2, device="cuda:0"))
    n = int(16000 * args.seconds)
    x = torch.stack([syllable_wave(n, 100 + b)[0] for b in range(args.batch)]).cuda().contiguous()
    # the synthetic encoder's hidden-state norms sit below the yaml thresholder's value: segment at their 40th percentile instead
    h = syn.speech_model.forward(x)
    thr = float(np.round(torch.quantile(torch.sqrt((h.double() ** 2).sum(-1) + 1e-8).flatten(), 0.4).item(), 2))
    toks = syn.tokenize(x, normthreshold=thr)
    T = syn.speech_model.num_frames(n)
    units = [t["units"] for t in toks]
    spans = [t["segments"] for t in toks]
    S = max(1, max(len(u) for u in units))
    nunits = np.asarray([len(u) for u in units])
    P = np.zeros((args.batch, S, 2), np.int64)
    Uu = np.zeros((args.batch, S, 2), np.int64)
    for b in range(args.batch):
        P[b, :len(spans[b])], Uu[b, :len(units[b])] = spans[b], units[b]
    frames = [T] * args.batch

    def features_path(dev_expand):
        feats = syn.quantizer.decode(torch.from_numpy(Uu).cuda())
        avg, dur = U.spans_to_durations(feats.cpu().numpy(), P, nunits, T)
        if dev_expand:
            e = expand_feature(torch.from_numpy(avg).cuda(), torch.from_numpy(dur))
        else:
            e = torch_expand(torch.from_numpy(avg).cuda(), torch.from_numpy(dur).cuda())
        return syn.resynthesize(features=e, steps=5, frames=frames)[0]

    a = syn.synthesize_units(toks, steps=5)
    assert torch.equal(a, features_path(True)) and torch.equal(a, features_path(False))

    def encoder_segment():
        h = syn.speech_model.forward(x)
        syn.speech_model.segment(h, thr, 0.8)

    res = {"batch": args.batch, "normthreshold": thr, "seconds": args.seconds, "frames": T, "units_per_clip": float(nunits.mean()), "precision": args.precision,
           "steps": 5, "iters": args.iters,
           "synthesize_units_ms": median_ms(lambda: syn.synthesize_units(toks, steps=5), args.iters),
           "features_path_ms": median_ms(lambda: features_path(False), args.iters),
           "features_path_dev_ms": median_ms(lambda: features_path(True), args.iters),
           "tokenize_ms": median_ms(lambda: syn.tokenize(x, normthreshold=thr), args.iters),
           "encoder_segment_ms": median_ms(encoder_segment, args.iters),
           "resynthesize_ms": median_ms(lambda: syn.resynthesize(input_values=x, steps=5, normthreshold=thr), args.iters)}
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()

"""A/B of packed resynthesis on one GPU, in one process: ``SegmentSynthesis`` three ways on the same clips --

  * ``packed=True``: encoder, conditioning and decoder on each clip's own frames (decoder slots of round_up(16 + T_b, 64) rows);
  * ``batch_invariant=True``: the batch padded to its longest clip, each clip's results its own;
  * default: the padded batch as upstream computes it.

Timed: ``resynthesize(input_values=...)`` and ``synthesize_units(tokenize(...))`` with steps=5, and the decoder alone
(``CfmDecoder.sample_packed`` against ``sample(frames=)``).  Batch sets: those of tools/packed_ab.py (32 seeded clips of 2-20 s,
32 x 10 s, 8 seeded clips of 5-60 s).  The configurations alternate repetition by repetition, so drift of the box hits all of them
alike.  Prints one JSON line per (batch set, workload) with the median and minimum ms per call, and writes them with a table to --out.

    python tools/cfm_packed_ab.py [--reps 7] [--precision bf16] [--out profiles/cfm_packed_ab.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from packed_ab import batch_sets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cfm_packed_ab.md"))
    a = ap.parse_args()
    from sylber_amd import KMQuantizer, SegmentSynthesis
    from sylber_amd.synth import syllable_wave
    from sylber_amd.synthesis import cfm_packed_layout
    from sylber_amd.weights import synthetic_mlp_state_dict, synthetic_regressor_state_dict, synthetic_state_dict

    sd = {"speech_model." + k: v for k, v in synthetic_state_dict(0, num_layers=9).items()}
    sd.update({"input_model." + k: v for k, v in synthetic_mlp_state_dict(1).items()})
    sd.update({"regressor." + k: v for k, v in synthetic_regressor_state_dict(0).items()})
    g = torch.Generator().manual_seed(23)
    km = KMQuantizer(torch.randn(64, 768, generator=g) * 0.09, device="cuda:0")
    syn = {"packed": SegmentSynthesis(model_ckpt=sd, precision=a.precision, quantizer=km, packed=True),
           "invariant": SegmentSynthesis(model_ckpt=sd, precision=a.precision, quantizer=km, batch_invariant=True),
           "default": SegmentSynthesis(model_ckpt=sd, precision=a.precision, quantizer=km)}
    dec = syn["invariant"].decoder

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    lines = []
    for name, lens in batch_sets().items():
        clips = [syllable_wave(n, 100 + i)[0] for i, n in enumerate(lens)]
        B, N = len(lens), max(lens)
        x = torch.zeros(B, N)
        mask = torch.zeros(B, N)
        for i, c in enumerate(clips):
            x[i, :len(c)] = c
            mask[i, :len(c)] = 1
        x, mask = x.cuda(), mask.cuda()
        sm = syn["invariant"].speech_model
        frames = sm.frame_counts(lens)
        hidden = sm.forward(x.contiguous(), lens)
        norms = torch.cat([torch.sqrt((hidden[b, :f].double() ** 2).sum(-1) + 1e-8) for b, f in enumerate(frames)])
        thr = float(np.round(torch.quantile(norms, 0.4).item(), 2))      # a threshold inside the synthetic encoder's norm range
        del hidden
        toks = {k: s.tokenize(x, attention_mask=mask, normthreshold=thr) for k, s in syn.items()}
        T = sm.num_frames(N)
        slots = cfm_packed_layout(frames)
        tp = (16 + T + 31) // 32 * 32
        cond = torch.randn(B, T, 256, generator=g).cuda() * 0.5
        conds = [cond[b, :f] for b, f in enumerate(frames)]
        work = {
            "resynthesize": {k: (lambda s=s: s.resynthesize(input_values=x, attention_mask=mask, steps=a.steps, normthreshold=thr))
                             for k, s in syn.items()},
            "synthesize_units": {k: (lambda s=s, k=k: s.synthesize_units(toks[k], steps=a.steps)) for k, s in syn.items()},
            "decoder": {"packed": lambda: dec.sample_packed(conds, steps=a.steps),
                        "invariant": lambda: dec.sample(cond, steps=a.steps, frames=frames)},
        }
        for wname, runs in work.items():
            for fn in runs.values():               # warm-up: workspaces, kernel attributes
                timed(fn)
                timed(fn)
            ms = {k: [] for k in runs}
            for _ in range(a.reps):
                for k, fn in runs.items():
                    ms[k].append(timed(fn))
            res = {"set": name, "workload": wname, "clips": B, "precision": a.precision, "steps": a.steps, "reps": a.reps,
                   "decoder_rows_packed": int(slots[-1]), "decoder_rows_padded": B * tp, "valid_frames": int(sum(frames))}
            for k, v in ms.items():
                res[k] = {"ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
            res["packed_vs_invariant"] = round(res["invariant"]["ms"] / res["packed"]["ms"], 3)
            print(json.dumps(res), flush=True)
            lines.append(res)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# Packed resynthesis: `tools/cfm_packed_ab.py` on one MI355X\n\n")
        f.write("`SegmentSynthesis`, %s, synthetic weights, steps=%d, a `KMQuantizer` for the units.  The configurations alternate "
                "repetition by repetition, %d repetitions; median (min-max) ms per call.  `decoder_rows` = the rows of every decoder "
                "GEMM: the sum of the packed slots, or B x round_up(16 + T, 32) padded.\n\n" % (a.precision, a.steps, a.reps))
        f.write("```\n" + "\n".join(json.dumps(r) for r in lines) + "\n```\n\n")
        f.write("| batch set | workload | decoder rows packed / padded | packed ms | batch-invariant ms | default ms | invariant / packed |\n")
        f.write("|---|---|---|---|---|---|---|\n")
        for r in lines:
            cell = lambda k: "%.2f (%.2f-%.2f)" % (r[k]["ms"], r[k]["min_ms"], r[k]["max_ms"]) if k in r else "-"  # noqa: E731
            f.write("| %s | %s | %d / %d | %s | %s | %s | %.3f |\n" % (r["set"], r["workload"], r["decoder_rows_packed"], r["decoder_rows_padded"],
                                                                   cell("packed"), cell("invariant"), cell("default"), r["packed_vs_invariant"]))


if __name__ == "__main__":
    main()

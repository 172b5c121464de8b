"""A/B of the batch-invariant mode on one GPU, in one process: 32 seeded clips of 2-10 s through

  * ``Segmenter.__call__``: the default mode on the batch, ``batch_invariant=True`` on the same batch, and the same clips called
    one at a time (what the mode replaces);
  * ``SegmentSynthesis.resynthesize(steps=5)``: the same three ways.

The configurations alternate repetition by repetition, so drift of the box hits all of them alike.  Prints one JSON line:
median ms per call (a call = the whole batch, or all 32 single-clip calls) and audio-seconds per second.

    python tools/batch_invariant_ab.py [--reps 7] [--clips 32]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    a = ap.parse_args()
    from sylber_amd import Segmenter, SegmentSynthesis
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_mlp_state_dict, synthetic_regressor_state_dict, synthetic_state_dict

    rng = np.random.default_rng(0)
    lens = [int(rng.integers(2 * 16000, 10 * 16000 + 1)) for _ in range(a.clips)]
    clips = [syllable_wave(n, 100 + i) for i, n in enumerate(lens)]
    audio_s = sum(lens) / 16000.0
    sd = synthetic_state_dict(0, num_layers=9)
    seg = {"default": Segmenter(model_ckpt=sd, precision=a.precision),
           "invariant": Segmenter(model_ckpt=sd, precision=a.precision, batch_invariant=True)}
    full = {"speech_model." + k: v for k, v in sd.items()}
    full.update({"input_model." + k: v for k, v in synthetic_mlp_state_dict(1).items()})
    full.update({"regressor." + k: v for k, v in synthetic_regressor_state_dict(0).items()})
    full.update({"cfm_wrapper.regressor." + k: v for k, v in synthetic_regressor_state_dict(0).items()})
    ckpt = {"state_dict": {"net." + k: v for k, v in full.items()}}
    syn = {"default": SegmentSynthesis(model_ckpt=ckpt, precision=a.precision),
           "invariant": SegmentSynthesis(model_ckpt=ckpt, precision=a.precision, batch_invariant=True)}
    x = torch.zeros(len(clips), max(lens))
    mask = torch.zeros(len(clips), max(lens))
    for i, c in enumerate(clips):
        x[i, :lens[i]] = c[0]
        mask[i, :lens[i]] = 1
    x, mask = x.cuda(), mask.cuda()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    runs = {
        "segment_default_batch": lambda: seg["default"](wav=clips),
        "segment_invariant_batch": lambda: seg["invariant"](wav=clips),
        "segment_one_at_a_time": lambda: [seg["default"](wav=c) for c in clips],
        "resynth_default_batch": lambda: syn["default"].resynthesize(input_values=x, attention_mask=mask, steps=5),
        "resynth_invariant_batch": lambda: syn["invariant"].resynthesize(input_values=x, attention_mask=mask, steps=5),
        "resynth_one_at_a_time": lambda: [syn["default"].resynthesize(input_values=c, steps=5) for c in clips],
    }
    for fn in runs.values():                       # warm-up: workspaces, pinned blocks, kernel attributes
        timed(fn)
        timed(fn)
    ms = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    res = {"clips": a.clips, "audio_s": round(audio_s, 2), "precision": a.precision, "reps": a.reps}
    for k, v in ms.items():
        med = statistics.median(v)
        res[k] = {"ms": round(med, 3), "audio_s_per_s": round(audio_s / (med / 1e3), 1), "min_ms": round(min(v), 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

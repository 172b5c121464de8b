"""A/B of packed batches on one GPU, in one process: ``Segmenter.__call__`` three ways on the same clips --

  * ``packed=True``: every clip in a slot of its own frames rounded up to 64 (sylber_forward_packed);
  * ``batch_invariant=True``: the batch padded to its longest clip, each clip's results its own;
  * default: the padded batch as upstream computes it.

Batch sets: 32 seeded clips of 2-20 s, 32 x 10 s, 8 seeded clips of 5-60 s.  The configurations alternate repetition by repetition,
so drift of the box hits all of them alike.  Prints one JSON line per batch set: median ms per call, audio-seconds per second, and the
fill of the packed layout sum(slot_b) / (B x Tp) (Tp = the padded layout's frame pitch per clip, sylber_padded_frames).

    python tools/packed_ab.py [--reps 9] [--precision bf16]
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


def batch_sets():
    rng = np.random.default_rng(0)
    return {
        "32_clips_2-20s": [int(rng.integers(2 * 16000, 20 * 16000 + 1)) for _ in range(32)],
        "32_x_10s": [160000] * 32,
        "8_clips_5-60s": [int(rng.integers(5 * 16000, 60 * 16000 + 1)) for _ in range(8)],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--precision", default="bf16")
    a = ap.parse_args()
    from sylber_amd import Segmenter, _lib
    from sylber_amd.segmenter import packed_layout
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_state_dict

    sd = synthetic_state_dict(0, num_layers=9)
    seg = {"packed": Segmenter(model_ckpt=sd, precision=a.precision, packed=True),
           "invariant": Segmenter(model_ckpt=sd, precision=a.precision, batch_invariant=True),
           "default": Segmenter(model_ckpt=sd, precision=a.precision)}
    lib = _lib.load()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, lens in batch_sets().items():
        clips = [syllable_wave(n, 100 + i) for i, n in enumerate(lens)]
        audio_s = sum(lens) / 16000.0
        off, frames = packed_layout(lens)
        tp = int(lib.sylber_padded_frames(max(lens)))
        runs = {k: (lambda s=s: s(wav=clips)) for k, s in seg.items()}
        for fn in runs.values():                   # warm-up: workspaces, pinned blocks, kernel attributes
            timed(fn)
            timed(fn)
        ms = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, fn in runs.items():
                ms[k].append(timed(fn))
        res = {"set": name, "clips": len(lens), "audio_s": round(audio_s, 2), "precision": a.precision, "reps": a.reps,
               "packed_frames": int(off[-1]), "padded_frames": len(lens) * tp, "fill": round(int(off[-1]) / (len(lens) * tp), 4),
               "valid_frames": int(frames.sum())}
        for k, v in ms.items():
            med = statistics.median(v)
            res[k] = {"ms": round(med, 3), "audio_s_per_s": round(audio_s / (med / 1e3), 1), "min_ms": round(min(v), 3)}
        res["packed_vs_invariant"] = round(res["invariant"]["ms"] / res["packed"]["ms"], 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

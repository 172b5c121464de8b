"""Same-process A/B of the host-side hand-over of Segmenter.__call__ (development aid, GPU box): padding threads"""
import os, sys, time, statistics, gc
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sylber_amd import Segmenter
from sylber_amd.synth import noise_batch
from sylber_amd.weights import synthetic_state_dict
sd = synthetic_state_dict(0)
wavs = [w[None, :].clone() for w in noise_batch(32, 160000, seed=1)]
variants = {t: Segmenter(model_ckpt=sd, host_pad_threads=t) for t in (1, 2)}
for S in variants.values():
    for _ in range(3): S(wav=wavs)
res = {k: [] for k in variants}
for rep in range(6):
    for k, S in variants.items():
        for _ in range(5):
            torch.cuda.synchronize(); t0 = time.perf_counter(); out = S(wav=wavs); res[k].append((time.perf_counter() - t0) * 1e3); del out
for k, v in res.items():
    print("pad threads %d: min %.2f  med %.2f  p90 %.2f ms" % (k, min(v), statistics.median(v), sorted(v)[int(len(v) * 0.9)]), flush=True)

"""Learned quantizer on one MI355X, config (a) of tests/golden/quantizer.npz (768 -> [512] -> 72, art 4 x 1024, pitch 2 x 64,
synthetic seeded weights).  Median milliseconds per ``get_indices`` call on

  * 1400 rows: about the segment means of a 32 x 10 s batch (~44 syllables per clip);
  * 16000 rows: frame level (32 x 499 frames).

Beside each, ``eager``: the same contract in torch eager fp32 on the same GPU (F.linear, cdist + argmin per stage, TF32 off), and the
fraction of rows whose ids agree with it.  Random tokens; the timings do not depend on their values.

Prints one JSON line.   python tools/quantizer_bench.py [--iters 50] [--rows 1400,16000]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = dict(encoder_configs=dict(input_dim=768, hidden_dims=[512], output_dim=72),
           art_vq_configs=dict(dim=64, codebook_size=1024, num_quantizers=4),
           pitch_vq_configs=dict(dim=8, codebook_size=64, num_quantizers=2), pitch_emb_dim=8)


def median_ms(fn, iters):
    for _ in range(3):
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


class Eager:
    """Quantizer.get_indices restated with torch ops (separate_norm, both unit norms, keep_blank_zero)"""

    def __init__(self, sd):
        dev = "cuda:0"
        self.lin = [(sd["encoder.mlp.%s.weight" % k].to(dev), sd["encoder.mlp.%s.bias" % k].to(dev)) for k in ("0", "1.0", "1.3", "2")]
        self.books = {st: [sd["%s.rvqs.0.layers.%d._codebook.embed" % (st, q)][0].to(dev) for q in range(Q)]
                      for st, Q in (("art_vq", 4), ("pitch_vq", 2))}

    @staticmethod
    def unit(x):
        return x / torch.sqrt((x ** 2).sum(-1, keepdim=True) + 1e-5)

    def __call__(self, x):
        blank = ~((x ** 2).sum(-1) > 0)
        t = self.unit(x)
        (w0, b0), (w1, b1), (w2, b2), (w3, b3) = self.lin
        t = F.linear(t, w0, b0)
        t = F.linear(torch.relu(F.linear(t, w1, b1)), w2, b2)
        t = F.linear(t, w3, b3)
        t = torch.cat([self.unit(t[:, :64]), self.unit(t[:, 64:])], -1)
        t[blank] = 0.0
        ids = []
        for st, r in (("art_vq", t[:, :64]), ("pitch_vq", t[:, 64:])):
            for E in self.books[st]:
                i = torch.cdist(r, E).argmin(-1)
                ids.append(i)
                r = r - E[i]
        return torch.stack(ids, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rows", default="1400,16000")
    args = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    from sylber_amd import Quantizer
    from sylber_amd.weights import synthetic_quantizer_state_dict
    sd = synthetic_quantizer_state_dict(CFG, 0)
    q = Quantizer(**CFG, state_dict=sd, device="cuda:0")
    eager = Eager(sd)
    res = {"config": "a", "iters": args.iters, "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(0)
    for n in [int(v) for v in args.rows.split(",")]:
        x = torch.from_numpy(rng.standard_normal((n, 768)).astype(np.float32)).cuda()
        with torch.no_grad():
            agree = float((q.get_indices(x) == eager(x)).all(-1).float().mean().item())
            res["rows%d_hip_ms" % n] = median_ms(lambda: q.get_indices(x), args.iters)
            res["rows%d_eager_ms" % n] = median_ms(lambda: eager(x), args.iters)
        res["rows%d_ids_agree_eager" % n] = agree
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()

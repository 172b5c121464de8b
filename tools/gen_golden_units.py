"""Golden vectors for the syllable-unit path (CPU only; survey container only, never on the GPU box): runs the REFERENCE's own
``expand_feature`` (sylber/model/flowmatching.py:873-882) and ``SegmentSynthesis.resynthesize(features=...)``
(sylber/model/segment_synthesis.py:135-146) on decoded units, with the stubs of tools/gen_golden_cfm.py, the MLP of
``synthetic_mlp_state_dict(1)`` and the decoder of ``synthetic_regressor_state_dict(0)``, and writes tests/golden/units.npz.

The codebook look-up itself cannot run here (upstream's quantizers sit on vector_quantize_pytorch, which is not installed), so the
units are decoded as upstream's ``decode`` defines it: ``c1[i1]`` for one codebook, ``c1[i1] + c2[i2]`` for two, in fp32.
Seeded codebooks [64, 768] and [32, 768]; c1[5] and c2[3] are near zero (decoded norm < 1e-4: the unit is silence-masked).

Two utterances of T = 64 frames:
  * row 0 opens with a 4-frame gap (upstream has no slot for one: the golden encodes it as a first pair with an all-zero feature;
    the span form starts the first span at 4), then units back to back (zero gap), a 3-frame gap, the near-zero unit, a trailing gap;
  * row 1 starts at frame 0, with adjacent units and a 1-frame unit.
Contains no reference code."""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import units_ref as U                                                           # noqa: E402
from sylber_amd.weights import synthetic_mlp_state_dict                         # noqa: E402
from tools.gen_golden_cfm import build_wrapper, load_reference                  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "units.npz")
T = 64


def codebooks():
    g = torch.Generator().manual_seed(11)
    c1 = torch.randn(64, 768, generator=g)
    c2 = torch.randn(32, 768, generator=g) * 0.3
    c1[5] = torch.randn(768, generator=g) * 1e-6
    c2[3] = torch.randn(768, generator=g) * 1e-6
    return c1.numpy(), c2.numpy()


def tables():
    spans = [[(4, 12), (12, 20), (23, 35), (35, 50)],
             [(0, 7), (7, 9), (15, 40), (40, 41), (41, 60)]]
    ids = [[(17, 9), (40, 0), (5, 3), (63, 31)],
           [(0, 12), (33, 7), (8, 30), (52, 1), (17, 9)]]
    S = max(len(s) for s in spans)
    sp = np.zeros((2, S, 2), np.int32)
    un = np.zeros((2, S, 2), np.int32)
    for b in range(2):
        sp[b, :len(spans[b])] = spans[b]
        un[b, :len(ids[b])] = ids[b]
    return un, sp, np.asarray([len(s) for s in spans], np.int32)


def main():
    fm = load_reference()
    seg_mod = importlib.import_module("sylber.model.segment_synthesis")
    c1, c2 = codebooks()
    units, spans, nunits = tables()
    out = dict(c1=c1, c2=c2, units=units, spans=spans, nunits=nunits, T=np.int32(T))
    syn = object.__new__(seg_mod.SegmentSynthesis)
    torch.nn.Module.__init__(syn)
    mlp = seg_mod.MLP(768, output_dim=256, hidden_dims=[512, 512]).eval()
    mlp.load_state_dict(synthetic_mlp_state_dict(1), strict=True)
    syn.input_model = mlp
    syn.cfm_wrapper = build_wrapper(fm)
    syn.pitch_amp = 5
    syn.quantizer = None
    with torch.inference_mode():
        for ncb, books in ((1, [c1]), (2, [c1, c2])):
            feats = U.decode(units[..., :ncb], books)                     # [B, S, 768]: the decoded units
            avg, dur = U.spans_to_durations(feats, spans, nunits, T)
            expanded = fm.expand_feature(torch.from_numpy(avg), torch.from_numpy(dur))
            assert tuple(expanded.shape) == (2, T, 768)
            art, segs = syn.resynthesize(features=expanded, steps=5, rand_scale=0.0)
            assert segs is None
            out["durations%d" % ncb] = dur.astype(np.int32)
            out["art%d" % ncb] = art.numpy()
            if ncb == 2:
                out["expanded2"] = expanded.numpy()
    # tokens with known residual ids: c1[i] + c2[j] + small noise (parity of the look-up itself is unpinned upstream)
    g = np.random.default_rng(5)
    tid = np.stack([g.integers(6, 64, 16), g.integers(4, 32, 16)], 1)
    out["tok_ids"] = tid.astype(np.int32)
    out["tokens"] = (c1[tid[:, 0]] + c2[tid[:, 1]] + 0.01 * g.standard_normal((16, 768))).astype(np.float32)
    meta = {"mlp": "synthetic_mlp_state_dict(1)", "regressor": "synthetic_regressor_state_dict(0)", "steps": 5, "pitch_amp": 5}
    out["meta_json"] = np.asarray(json.dumps(meta, sort_keys=True))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

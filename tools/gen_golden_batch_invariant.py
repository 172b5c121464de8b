"""Generate tests/golden/batch_invariant.npz: the reference's results for clips processed ONE AT A TIME, the way its
README usage processes a file -- the targets of the batch-invariant mode (``Segmenter(batch_invariant=True)``,
``CfmDecoder.sample(frames=...)``), which must give every clip of a padded batch exactly what it gets alone.

    python tools/gen_golden_batch_invariant.py

Runs the real reference on the CPU through tools/ref_shim.py (as tools/gen_golden.py and tools/gen_golden_cfm.py do).
Writes data only:
  * encoder: the reference ``Segmenter`` on each of the three ragged clips of e2e.npz (``syllable_wave(32000, 21)``,
    ``(20000, 22)``, ``(26000, 23)``) ALONE: ``alone{i}_segments`` (frames), ``alone{i}_features``, ``alone{i}_hidden``;
  * decoder: the reference ``sample(steps=5)`` on each of cfm_decoder.npz's ragged clips ``rag_cond[b, :rag_lens[b]]``
    ALONE: ``cfm_alone{b}`` [rag_lens[b], 14].
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_shim  # noqa: E402
from oracle import segment_oracle  # noqa: E402
from sylber_amd.synth import syllable_wave  # noqa: E402
from sylber_amd.weights import synthetic_state_dict  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "batch_invariant.npz")
CLIPS = [(32000, 21), (20000, 22), (26000, 23)]
warnings.simplefilter("ignore")


def main():
    ref, _seg_utils, cfg_dir = ref_shim.load()
    out = {}
    S = ref.Segmenter(model_ckpt=None, speech_upstream=cfg_dir, device="cpu")
    S.speech_model.load_state_dict(synthetic_state_dict(0), strict=True)
    with torch.inference_mode():
        for i, (n, seed) in enumerate(CLIPS):
            r = S(wav=syllable_wave(n, seed), in_second=False)
            out[f"alone{i}_segments"] = np.asarray(r["segments"], np.int64).reshape(-1, 2)
            out[f"alone{i}_features"] = np.asarray(r["segment_features"], np.float32)
            out[f"alone{i}_hidden"] = r["hidden_states"]
            # the reference's own tables, re-derived by the repository's oracle on the same hidden states
            assert np.array_equal(segment_oracle.get_segment(r["hidden_states"], 2.6, 0.8).reshape(-1, 2), out[f"alone{i}_segments"])
            print("clip %d: hidden %s, %d segments" % (i, r["hidden_states"].shape, len(out[f"alone{i}_segments"])))
    out["clip_lengths"] = np.array([n for n, _ in CLIPS])
    out["clip_seeds"] = np.array([s for _, s in CLIPS])

    from tools import gen_golden_cfm as G
    fm = G.load_reference()
    w = G.build_wrapper(fm)
    inp = G.golden_inputs()
    lens = [int(v) for v in inp["rag_lens"]]
    with torch.inference_mode():
        for b, n in enumerate(lens):
            out[f"cfm_alone{b}"] = G.sample_with(w, inp["rag_cond"][b:b + 1, :n], 5)[0].numpy()
    out["cfm_rag_lens"] = np.asarray(lens, np.int32)
    meta = {"generator": "tools/gen_golden_batch_invariant.py", "encoder_weights": "synthetic_state_dict(0)",
            "decoder_weights": "synthetic_regressor_state_dict(0)", "steps": 5, "torch": torch.__version__, "numpy": np.__version__}
    out["meta_json"] = np.asarray(json.dumps(meta, sort_keys=True))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

"""CPU tier, batch-invariant mode: the fixture of the reference's per-clip results (tests/golden/batch_invariant.npz, written by
tools/gen_golden_batch_invariant.py), the premise that per-row GroupNorm statistics are the ONLY batch dependence of the encoder,
and the C-ABI declarations of the mode (include/sylber_hip.h)."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cfm_ref as R
from oracle import hubert_ref, segment_oracle
from sylber_amd.synth import syllable_wave
from sylber_amd.weights import synthetic_regressor_state_dict, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "batch_invariant.npz"))


@pytest.fixture(scope="module")
def manifest(golden_dir):
    with open(os.path.join(golden_dir, "manifest.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def sd():
    return synthetic_state_dict(0)


def clips(gold):
    return [syllable_wave(int(n), int(s))[0] for n, s in zip(gold["clip_lengths"], gold["clip_seeds"])]


def padded(wavs):
    n = max(len(w) for w in wavs)
    x = torch.zeros(len(wavs), n)
    for i, w in enumerate(wavs):
        x[i, :len(w)] = w
    return x, [len(w) for w in wavs]


def per_row_groupnorm_forward(sd, wav, lengths):
    """oracle/hubert_ref.forward with conv0's GroupNorm statistics of row b taken over its own (n_b - 10) // 5 + 1 frames
    (what SYLBER_OPT_PER_UTTERANCE does); every other stage is the oracle's own"""
    l0 = [(int(n) - 10) // 5 + 1 for n in lengths]

    def group_norm(x, groups, weight, bias, eps):
        rows = []
        for b in range(x.shape[0]):
            own = x[b:b + 1, :, :l0[b]]
            mean = own.mean(-1, keepdim=True)
            var = own.var(-1, unbiased=False, keepdim=True)
            rows.append((x[b:b + 1] - mean) / torch.sqrt(var + eps) * weight[None, :, None] + bias[None, :, None])
        return torch.cat(rows)

    ns = types.SimpleNamespace(**{k: getattr(F, k) for k in dir(F) if not k.startswith("__")})
    ns.group_norm = group_norm
    saved = hubert_ref.F
    hubert_ref.F = ns
    try:
        return hubert_ref.forward(sd, wav, lengths)["hidden"]
    finally:
        hubert_ref.F = saved


def test_fixture_matches_oracle_alone(gold, sd, manifest):
    """the reference's alone results == the oracle on each clip alone (fp32 floor), and the oracle's tables are the stored ones"""
    floor = manifest["tolerances"]["fp32_floor_max_abs"]
    for i, w in enumerate(clips(gold)):
        h = hubert_ref.forward(sd, w[None], None)["hidden"][0].numpy()
        ref = gold[f"alone{i}_hidden"]
        assert h.shape == ref.shape == (hubert_ref.num_frames(len(w)), 768)
        err = float(np.abs(h - ref).max())
        print("clip %d: oracle vs reference alone max-abs %.2e" % (i, err))
        assert err <= floor, err
        exp = gold[f"alone{i}_segments"]
        assert np.array_equal(segment_oracle.get_segment(ref, 2.6, 0.8).reshape(-1, 2), exp)
        if len(exp):
            assert np.array_equal(segment_oracle.mean_pool(ref, exp), gold[f"alone{i}_features"])


def test_per_row_groupnorm_is_the_whole_batch_dependence(gold, sd, manifest):
    """per-row GroupNorm statistics on the padded batch == each clip alone (fp32 floor); the plain padded oracle is not"""
    floor = manifest["tolerances"]["fp32_floor_max_abs"]
    wavs = clips(gold)
    x, lengths = padded(wavs)
    inv = per_row_groupnorm_forward(sd, x, lengths)
    plain = hubert_ref.forward(sd, x, lengths)["hidden"]
    for i, w in enumerate(wavs):
        alone = hubert_ref.forward(sd, w[None], None)["hidden"][0]
        T = alone.shape[0]
        err = float((inv[i, :T] - alone).abs().max())
        err_plain = float((plain[i, :T] - alone).abs().max())
        print("clip %d: per-row %.2e, padded %.2e" % (i, err, err_plain))
        assert err <= floor, err
        if len(w) < x.shape[1]:
            assert err_plain > 1e-3, err_plain


def test_padded_batch_has_phantom_segments(gold):
    """the stored padded-batch tables (e2e.npz) differ from the alone tables for the shorter clips: the premise of the mode"""
    e2e = np.load(os.path.join(ROOT, "tests", "golden", "e2e.npz"))
    assert list(e2e["batch_lengths"]) == list(gold["clip_lengths"]) and list(e2e["batch_seeds"]) == list(gold["clip_seeds"])
    differs = [not np.array_equal(e2e[f"batch{i}_segments"], gold[f"alone{i}_segments"]) for i in range(3)]
    assert any(differs[1:]), differs


def test_decoder_fixture_matches_restatement_alone(gold):
    """tests/cfm_ref.sample on each ragged clip alone == the reference's alone golden (fp32 tolerance of test_cfm_ref)"""
    cfm = np.load(os.path.join(ROOT, "tests", "golden", "cfm_decoder.npz"))
    sdr = synthetic_regressor_state_dict(0)
    assert list(gold["cfm_rag_lens"]) == list(cfm["rag_lens"])
    for b, n in enumerate(cfm["rag_lens"]):
        with torch.inference_mode():
            y = R.sample(sdr, torch.from_numpy(cfm["rag_cond"][b:b + 1, :n]), steps=5)[0].numpy()
        ref = gold[f"cfm_alone{b}"]
        assert y.shape == ref.shape == (int(n), 14)
        r = float(np.sqrt(((y.astype(np.float64) - ref) ** 2).mean() / (ref.astype(np.float64) ** 2).mean()))
        print("clip %d: restatement vs reference alone rel-rms %.2e" % (b, r))
        assert r <= 1e-5, r


def test_header_declares_the_mode():
    with open(os.path.join(ROOT, "include", "sylber_hip.h")) as f:
        h = f.read()
    assert re.search(r"SYLBER_OPT_PER_UTTERANCE\s*=\s*14\b", h)
    assert re.search(r"int sylber_segment_frames\(sylber_t h, const float\* hidden_dev, const int32_t\* frames_host, int32_t B, int32_t T,",
                     h)
    assert re.search(r"int sylber_cfm_sample_frames\(sylber_cfm_t h, const float\* cond_emb_dev, const int32_t\* frames_host,", h)


def test_library_exports_the_mode():
    """the built library has both entry points and accepts the option key without a GPU-side call"""
    from sylber_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "sylber_segment_frames") and hasattr(lib, "sylber_cfm_sample_frames")
    assert _lib.OPT_PER_UTTERANCE == 14

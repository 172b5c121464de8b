"""GPU tier, batch-invariant mode: every clip of a ragged batch gets, bit for bit, the results it gets alone.

  * encoder: SYLBER_OPT_PER_UTTERANCE (conv0 GroupNorm statistics over each row's own frames), every precision, graph mode;
  * segmentation: sylber_segment_frames against the oracle on each row's own frames, with high-norm "speech" in the padding;
  * Segmenter(batch_invariant=True) / stream() against Segmenter()(wav=clip) and the reference's alone tables
    (tests/golden/batch_invariant.npz);
  * decoder: sylber_cfm_sample_frames against [1, T_b] calls and the reference's alone golden;
  * SegmentSynthesis(batch_invariant=True).resynthesize against each clip resynthesized alone."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import segment_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TOL = 1e-4                                   # tests/test_gpu_fp32_parity.py
CFM_TOL = {"fp32": 1e-4, "fp16": 4e-3, "bf16": 2e-2}   # tests/test_gpu_synthesis.py


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean() / (b ** 2).mean()))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "batch_invariant.npz"))


@pytest.fixture(scope="module")
def sd():
    from sylber_amd.weights import synthetic_state_dict
    return synthetic_state_dict(0, num_layers=9)


def _pad(wavs):
    n = max(len(w) for w in wavs)
    x = torch.zeros(len(wavs), n)
    for i, w in enumerate(wavs):
        x[i, :len(w)] = w
    return x.cuda(), [len(w) for w in wavs]


def _ragged_clips():
    from sylber_amd.synth import syllable_wave
    # a 400-sample clip (one frame), a 10 s clip and a 60 s clip, which sets Lmax
    return [syllable_wave(400, 31)[0], syllable_wave(160000, 32)[0], syllable_wave(960000, 33)[0]]


@pytest.mark.parametrize("prec", ["bf16", "fp16", "mixed16", "split16", "fp32", "fp8"])
def test_encoder_rows_equal_clips_alone(sd, prec):
    from sylber_amd import HubertEncoderHIP
    wavs = _ragged_clips()
    x, lengths = _pad(wavs)
    enc = HubertEncoderHIP(sd, device="cuda:0", precision=prec)
    if prec == "fp8":
        enc.set_option(7, -1)                     # fp8's attention core is chosen by batch shape: the guarantee holds with it off
    enc.set_per_utterance(True)
    on = enc.forward(x, lengths).cpu().numpy()
    for b, w in enumerate(wavs):
        alone = enc.forward(w[None].cuda().contiguous()).cpu().numpy()[0]
        T = enc.num_frames(len(w))
        assert alone.shape[0] == T
        assert np.array_equal(on[b, :T], alone), (prec, b, float(np.abs(on[b, :T] - alone).max()))
    # back to 0: the same batch gives exactly what a fresh handle gives without the option
    enc.set_per_utterance(False)
    off = enc.forward(x, lengths).cpu().numpy()
    del enc
    fresh = HubertEncoderHIP(sd, device="cuda:0", precision=prec)
    if prec == "fp8":
        fresh.set_option(7, -1)
    ref = fresh.forward(x, lengths).cpu().numpy()
    assert np.array_equal(off, ref)
    T1 = fresh.num_frames(len(wavs[1]))
    assert not np.array_equal(off[1, :T1], on[1, :T1])        # the option changes the padded rows' statistics


def test_encoder_graph_mode_replays_new_lengths(sd):
    from sylber_amd import HubertEncoderHIP
    from sylber_amd.synth import syllable_wave
    enc = HubertEncoderHIP(sd, device="cuda:0", precision="bf16")
    enc.set_per_utterance(True)
    enc.set_graph_mode(True)
    plain = HubertEncoderHIP(sd, device="cuda:0", precision="bf16")
    sets = [[syllable_wave(80000, 41)[0], syllable_wave(48000, 42)[0]],
            [syllable_wave(30000, 43)[0], syllable_wave(80000, 44)[0]]]
    Lmax = 80000
    buf = torch.zeros(2, Lmax, device="cuda:0")
    out = torch.empty(2, enc.num_frames(Lmax), 768, device="cuda:0")
    for k in [0, 1, 0, 1, 0]:                     # eager, capture, replays with alternating lengths
        buf.zero_()
        for b, w in enumerate(sets[k]):
            buf[b, :len(w)] = w.cuda()
        h = enc.forward(buf, [len(w) for w in sets[k]], out=out).cpu().numpy()
        for b, w in enumerate(sets[k]):
            alone = plain.forward(w[None].cuda().contiguous()).cpu().numpy()[0]
            assert np.array_equal(h[b, :alone.shape[0]], alone), (k, b)


def _padded_states(rows, T, seed):
    """rows of own lengths padded to T with high-norm, mutually similar 'speech' frames that would form segments if read"""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(768).astype(np.float32)
    base *= 10.0 / np.linalg.norm(base)
    x = np.empty((len(rows), T, 768), np.float32)
    for b, st in enumerate(rows):
        x[b, :len(st)] = st
        x[b, len(st):] = base + 0.01 * rng.standard_normal((T - len(st), 768)).astype(np.float32)
    return x


def test_segment_frames_vs_oracle():
    from sylber_amd import HubertEncoderHIP, _lib
    from sylber_amd.synth_states import syllable_states
    from sylber_amd.weights import synthetic_state_dict
    enc = HubertEncoderHIP(synthetic_state_dict(0, num_layers=1), num_layers=1, device="cuda:0")
    T = 900
    rows = [syllable_states(1, 5, mode="allspeech"),           # T_b = 1
            syllable_states(37, 6, mode="allspeech"),          # a run of speech that reaches T_b
            syllable_states(700, 7, mode="allspeech"),         # one run longer than 512 frames: the slab path
            syllable_states(420, 8, mode="normal"),
            syllable_states(T, 9, mode="edge"),                # a full row
            syllable_states(250, 10, mode="long")]
    x = _padded_states(rows, T, 1)
    frames = [len(r) for r in rows]
    seg, nseg, feats = enc.segment(torch.from_numpy(x).cuda(), 2.6, 0.8, frames=frames)
    torch.cuda.synchronize()
    seg, nseg, feats = seg.cpu().numpy(), nseg.cpu().numpy(), feats.cpu().numpy()
    for b, st in enumerate(rows):
        exp = segment_oracle.get_segment(st, 2.6, 0.8).reshape(-1, 2)
        assert nseg[b] == len(exp) and np.array_equal(seg[b, :nseg[b]], exp), b
        assert len(exp) == 0 or exp.max() <= len(st)
        if len(exp):
            assert np.array_equal(feats[b, :nseg[b]], segment_oracle.mean_pool(st, exp), equal_nan=True), b
    # without the bound the padding does create segments (the fixture exercises what it claims to)
    s0, n0, _ = enc.segment(torch.from_numpy(x).cuda(), 2.6, 0.8)
    s0, n0 = s0.cpu().numpy(), n0.cpu().numpy()
    assert any(n0[b] and s0[b, :n0[b]].max() > frames[b] for b in range(len(rows)) if frames[b] < T)
    with pytest.raises(ValueError):
        enc.segment(torch.from_numpy(x).cuda(), 2.6, 0.8, frames=[0] + frames[1:])
    with pytest.raises(ValueError):
        enc.segment(torch.from_numpy(x).cuda(), 2.6, 0.8, frames=[T + 1] + frames[1:])
    enc.set_option(9, -1)
    with pytest.raises(_lib.SylberHipError, match="SYLBER_OPT_SEGMENT"):
        enc.segment(torch.from_numpy(x).cuda(), 2.6, 0.8, frames=frames)


def _same_dict(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (k, x.shape, y.shape)
        assert np.array_equal(x, y), k


@pytest.mark.parametrize("prec", ["bf16", "split16", "fp32"])
def test_segmenter_batch_invariant(sd, gold, golden_dir, prec):
    from sylber_amd import Segmenter
    from sylber_amd.synth import syllable_wave
    clips = [syllable_wave(int(n), int(s)) for n, s in zip(gold["clip_lengths"], gold["clip_seeds"])] + [syllable_wave(400, 3)]
    inv = Segmenter(model_ckpt=sd, device="cuda:0", precision=prec, batch_invariant=True)
    alone = Segmenter(model_ckpt=sd, device="cuda:0", precision=prec)
    for in_second in (False, True):
        outs = inv(wav=clips, in_second=in_second)
        for c, o in zip(clips, outs):
            _same_dict(o, alone(wav=c, in_second=in_second))
    outs = inv(wav=clips, in_second=False)
    streamed = list(inv.stream([clips, clips[::-1]], in_second=False))
    for o, s in zip(outs, streamed[0]):
        _same_dict(o, s)
    for o, s in zip(outs[::-1], streamed[1]):
        _same_dict(o, s)
    with open(os.path.join(golden_dir, "manifest.json")) as f:
        budget = json.load(f)["tolerances"]["bf16_budget_rel_rms"]
    for i in range(3):
        h = outs[i]["hidden_states"]
        ref = gold[f"alone{i}_hidden"]
        assert h.shape == ref.shape
        if prec in ("split16", "fp32"):
            assert np.array_equal(np.asarray(outs[i]["segments"]).reshape(-1, 2), gold[f"alone{i}_segments"]), i
            assert np.abs(h - ref).max() < FP32_TOL, float(np.abs(h - ref).max())
            assert np.abs(outs[i]["segment_features"] - gold[f"alone{i}_features"]).max() < FP32_TOL
        else:
            r = rel_rms(h, ref)
            print("bf16 clip %d hidden rel %.3e" % (i, r))
            assert r <= budget, r


def test_segmenter_segment_method(sd):
    from sylber_amd import Segmenter
    from sylber_amd.synth import syllable_wave
    wavs = [syllable_wave(32000, 21)[0], syllable_wave(20000, 22)[0]]
    x, lengths = _pad(wavs)
    mask = torch.zeros_like(x)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    inv = Segmenter(model_ckpt=sd, device="cuda:0", batch_invariant=True)
    feats, segments, avg = inv.segment(x, attention_mask=mask)
    for b, w in enumerate(wavs):
        f1, s1, a1 = inv.segment(w[None].cuda())
        T = f1.shape[1]
        assert torch.equal(feats[b, :T], f1[0]) and bool((feats[b, T:] == 0).all())
        assert np.array_equal(np.asarray(segments[b]).reshape(-1, 2), np.asarray(s1[0]).reshape(-1, 2))
        n = len(s1[0])
        assert torch.equal(avg[b, :n], a1[0, :n])
    # the features= branch with frames= gives the same tables
    frames = [inv.speech_model.num_frames(n) for n in lengths]
    _, s2, _ = inv.segment(features=feats, frames=frames)
    for a, b_ in zip(segments, s2):
        assert np.array_equal(np.asarray(a).reshape(-1, 2), np.asarray(b_).reshape(-1, 2))


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_decoder_frames_equal_clips_alone(gold, golden_dir, prec):
    from sylber_amd.synthesis import CfmDecoder
    from sylber_amd.weights import synthetic_regressor_state_dict
    cfm = np.load(os.path.join(golden_dir, "cfm_decoder.npz"))
    d = CfmDecoder(synthetic_regressor_state_dict(0), device="cuda:0", precision=prec)
    cond = torch.from_numpy(cfm["rag_cond"]).cuda()
    lens = [int(n) for n in cfm["rag_lens"]]
    art = d.sample(cond, steps=5, frames=lens).cpu().numpy()
    for b, n in enumerate(lens):
        alone = d.sample(cond[b:b + 1, :n].contiguous(), steps=5).cpu().numpy()[0]
        assert np.array_equal(art[b, :n], alone), (prec, b)
        assert (art[b, n:] == 0).all()
        r = rel_rms(art[b, :n], gold[f"cfm_alone{b}"])
        print("%s clip %d vs reference alone rel %.3e" % (prec, b, r))
        assert r <= CFM_TOL[prec], r
    with pytest.raises(ValueError):
        d.sample(cond, steps=5, frames=[0, 1, 1])


def _synthesis(prec, batch_invariant):
    from sylber_amd import SegmentSynthesis
    from sylber_amd.weights import synthetic_mlp_state_dict, synthetic_regressor_state_dict, synthetic_state_dict
    sd = {"speech_model." + k: v for k, v in synthetic_state_dict(0, num_layers=9).items()}
    sd.update({"input_model." + k: v for k, v in synthetic_mlp_state_dict(1).items()})
    sd.update({"regressor." + k: v for k, v in synthetic_regressor_state_dict(0).items()})
    sd.update({"cfm_wrapper.regressor." + k: v for k, v in synthetic_regressor_state_dict(0).items()})
    return SegmentSynthesis(model_ckpt={"state_dict": {"net." + k: v for k, v in sd.items()}}, device="cuda:0", precision=prec,
                            batch_invariant=batch_invariant)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_resynthesize_rows_equal_clips_alone(prec):
    from sylber_amd.synth import syllable_wave
    wavs = [syllable_wave(32000, 21)[0], syllable_wave(20000, 22)[0], syllable_wave(26000, 23)[0]]
    x, lengths = _pad(wavs)
    mask = torch.zeros_like(x)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    inv = _synthesis(prec, True)
    art, segments = inv.resynthesize(input_values=x, attention_mask=mask, steps=5)
    art = art.cpu().numpy()
    alone_syn = _synthesis(prec, False)
    for b, w in enumerate(wavs):
        a1, s1 = alone_syn.resynthesize(input_values=w[None], steps=5)
        a1 = a1.cpu().numpy()[0]
        T = a1.shape[0]
        assert np.array_equal(art[b, :T], a1), (prec, b)
        assert (art[b, T:] == 0).all()
        assert np.array_equal(np.asarray(segments[b]).reshape(-1, 2), np.asarray(s1[0]).reshape(-1, 2))

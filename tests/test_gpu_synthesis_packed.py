"""GPU tier, packed resynthesis (CfmDecoder.sample_packed, SegmentSynthesis(packed=True)): every clip gets, bit for bit, what
batch-invariant mode gives it -- in the encoder, the conditioning and the decoder -- whatever its slot, its neighbours, stale workspace
contents or a non-finite neighbour."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRECS = ["bf16", "fp16"]
CFM_TOL = {"fp32": 1e-4, "fp16": 4e-3, "bf16": 2e-2}   # tests/test_gpu_synthesis.py


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean() / max((b ** 2).mean(), 1e-30)))


@pytest.fixture(scope="module")
def cfm(golden_dir):
    return np.load(os.path.join(golden_dir, "cfm_decoder.npz"))


@pytest.fixture(scope="module")
def gold_bi(golden_dir):
    return np.load(os.path.join(golden_dir, "batch_invariant.npz"))


_DEC = {}


def _decoder(prec):
    if prec not in _DEC:
        from sylber_amd.synthesis import CfmDecoder
        from sylber_amd.weights import synthetic_regressor_state_dict
        _DEC[prec] = CfmDecoder(synthetic_regressor_state_dict(0), device="cuda:0", precision=prec)
    return _DEC[prec]


def _checkpoint():
    from sylber_amd.weights import synthetic_mlp_state_dict, synthetic_regressor_state_dict, synthetic_state_dict
    sd = {"speech_model." + k: v for k, v in synthetic_state_dict(0, num_layers=9).items()}
    sd.update({"input_model." + k: v for k, v in synthetic_mlp_state_dict(1).items()})
    sd.update({"regressor." + k: v for k, v in synthetic_regressor_state_dict(0).items()})
    return sd


_SYN = {}


def _synthesis(prec, mode, quantizer=None):
    """mode: "packed" or "bi" (batch_invariant=True); one pair per (precision, quantizer kind), the quantizer set per call"""
    from sylber_amd import SegmentSynthesis
    k = (prec, mode)
    if k not in _SYN:
        _SYN[k] = SegmentSynthesis(model_ckpt=_checkpoint(), device="cuda:0", precision=prec, batch_invariant=mode == "bi",
                                   packed=mode == "packed")
    syn = _SYN[k]
    syn.quantizer = quantizer
    return syn


def _speech_codebooks(ncb):
    """seeded codebooks at the scale of the synthetic encoder's hidden states (tests/test_gpu_units.py)"""
    from sylber_amd import KMQuantizer, ResidualKMQuantizer
    g = torch.Generator().manual_seed(23)
    c1 = torch.randn(64, 768, generator=g) * 0.09
    c2 = torch.randn(32, 768, generator=g) * 0.03
    return KMQuantizer(c1, device="cuda:0") if ncb == 1 else ResidualKMQuantizer(c1, c2, device="cuda:0")


def _wavs():
    """ragged clips, two of them with 16 + T_b = 64 and 128 (T_b = 48 and 112: whole decoder slots)"""
    from sylber_amd.synth import syllable_wave
    t_of = lambda t: 400 + 320 * (t - 1)                                   # noqa: E731 (the shortest clip with t frames)
    lengths = [32000, t_of(48), 20000, t_of(112) + 100, 26000, 9000]
    return [syllable_wave(n, 40 + i)[0] for i, n in enumerate(lengths)]


def _pad(wavs):
    n = max(len(w) for w in wavs)
    x = torch.zeros(len(wavs), n)
    mask = torch.zeros(len(wavs), n)
    for i, w in enumerate(wavs):
        x[i, :len(w)] = w
        mask[i, :len(w)] = 1
    return x.cuda(), mask.cuda()


def _threshold(syn, x, mask):
    """the synthetic encoder's hidden-state norms sit below the yaml thresholder's value: a threshold inside their range, rounded
    (tests/test_gpu_units.py), so that the clips have segments"""
    lengths = [int(v) for v in mask.sum(-1).tolist()]
    hidden = syn.speech_model.forward(x.contiguous(), lengths)
    frames = syn.speech_model.frame_counts(lengths)
    norms = torch.cat([torch.sqrt((hidden[b, :f].double() ** 2).sum(-1) + 1e-8) for b, f in enumerate(frames)])
    return float(np.round(torch.quantile(norms, 0.4).item(), 2))


def _same_segments(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).reshape(-1, 2), np.asarray(y).reshape(-1, 2))


def _same_tokens(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        assert x["frames"] == y["frames"]
        assert np.array_equal(x["units"], y["units"]) and x["units"].dtype == y["units"].dtype
        assert np.array_equal(x["segments"], y["segments"])


# ---- 1. the decoder -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_sample_packed_equals_sample_frames(cfm, gold_bi, prec):
    d = _decoder(prec)
    cond = torch.from_numpy(cfm["rag_cond"]).cuda()
    lens = [int(n) for n in cfm["rag_lens"]]
    ref = d.sample(cond, steps=5, frames=lens).cpu().numpy()
    art, starts = d.sample_packed([cond[b, :n] for b, n in enumerate(lens)], steps=5)
    assert art.shape == (sum(lens), 14) and list(starts) == list(np.cumsum([0] + lens))
    art = art.cpu().numpy()
    for b, n in enumerate(lens):
        assert np.array_equal(art[starts[b]:starts[b + 1]], ref[b, :n]), (prec, b)
        r = rel_rms(art[starts[b]:starts[b + 1]], gold_bi[f"cfm_alone{b}"])
        print("%s clip %d vs reference alone rel %.3e" % (prec, b, r))
        assert r <= CFM_TOL[prec], r
    # the (packed, frames) form, a start state and the one-step grid
    packed = torch.cat([cond[b, :n] for b, n in enumerate(lens)])
    art2, _ = d.sample_packed((packed, lens), steps=5)
    assert torch.equal(art2.cpu(), torch.from_numpy(art))
    g = torch.Generator().manual_seed(3)
    y0 = torch.randn(len(lens), cond.shape[1], 14, generator=g).cuda()
    y0p = torch.cat([y0[b, :n] for b, n in enumerate(lens)])
    for steps in (1, 4):
        ref = d.sample(cond, steps=steps, y0=y0, pitch_amp=5.0, frames=lens)
        got, _ = d.sample_packed((packed, lens), steps=steps, y0=y0p, pitch_amp=5.0)
        assert torch.equal(got, torch.cat([ref[b, :n] for b, n in enumerate(lens)])), (prec, steps)


# ---- 2. SegmentSynthesis(packed=True) against batch-invariant mode -----------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_resynthesize_equals_batch_invariant(prec):
    wavs = _wavs()
    x, mask = _pad(wavs)
    bi, pk = _synthesis(prec, "bi"), _synthesis(prec, "packed")
    assert pk.packed and pk.batch_invariant
    thr = _threshold(bi, x, mask)
    art_b, seg_b = bi.resynthesize(input_values=x, attention_mask=mask, steps=5, normthreshold=thr)
    art_p, seg_p = pk.resynthesize(input_values=x, attention_mask=mask, steps=5, normthreshold=thr)
    assert art_p.shape == art_b.shape and art_p.dtype == art_b.dtype and art_p.is_cuda
    assert torch.equal(art_p, art_b), prec
    _same_segments(seg_p, seg_b)
    assert sum(len(s) for s in seg_p) > len(wavs)
    # a list of clips: T is the longest clip's frames, which is the padded batch's here
    art_l, seg_l = pk.resynthesize(input_values=[w for w in wavs], steps=5, normthreshold=thr)
    assert torch.equal(art_l, art_b)
    _same_segments(seg_l, seg_b)
    # a random start: the same seed draws the same padded [B, T, 14] state
    torch.manual_seed(1234)
    art_b, _ = bi.resynthesize(input_values=x, attention_mask=mask, steps=3, rand_scale=0.7)
    torch.manual_seed(1234)
    art_p, _ = pk.resynthesize(input_values=x, attention_mask=mask, steps=3, rand_scale=0.7)
    assert torch.equal(art_p, art_b), prec
    for b, w in enumerate(wavs):                                           # zeros past each clip's frames
        assert (art_p[b, bi.speech_model.num_frames(len(w)):] == 0).all()


@pytest.mark.parametrize("prec", PRECS)
def test_features_branch_equals_batch_invariant(prec):
    bi, pk = _synthesis(prec, "bi"), _synthesis(prec, "packed")
    g = torch.Generator().manual_seed(9)
    feats = (torch.randn(4, 150, 768, generator=g) * 0.1).cuda()
    feats[1, 30:40] = 0                                                    # silent frames
    frames = [150, 48, 112, 7]
    ref, none = bi.resynthesize(features=feats, frames=frames, steps=5)
    got, none2 = pk.resynthesize(features=feats, frames=frames, steps=5)
    assert none is None and none2 is None
    assert torch.equal(got, ref), prec
    ref, _ = bi.resynthesize(features=feats, steps=2)
    got, _ = pk.resynthesize(features=feats, steps=2)
    assert torch.equal(got, ref), prec


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ncb", [1, 2])
def test_tokenize_and_units_equal_batch_invariant(prec, ncb):
    q = _speech_codebooks(ncb)
    bi, pk = _synthesis(prec, "bi", q), _synthesis(prec, "packed", q)
    x, mask = _pad(_wavs())
    thr = _threshold(bi, x, mask)
    tok_b = bi.tokenize(x, attention_mask=mask, normthreshold=thr)
    tok_p = pk.tokenize(x, attention_mask=mask, normthreshold=thr)
    _same_tokens(tok_p, tok_b)
    assert sum(len(t["units"]) for t in tok_p) > 0
    art_b = bi.synthesize_units(tok_b, steps=5)
    art_p = pk.synthesize_units(tok_p, steps=5)
    assert art_p.shape == art_b.shape and torch.equal(art_p, art_b), (prec, ncb)
    # resynthesize with the quantizer substituting the segment means
    ra, rs = bi.resynthesize(input_values=x, attention_mask=mask, steps=5, normthreshold=thr)
    pa, ps = pk.resynthesize(input_values=x, attention_mask=mask, steps=5, normthreshold=thr)
    assert torch.equal(pa, ra), (prec, ncb)
    _same_segments(ps, rs)
    # the padded units form and a random start
    S = max(1, max(len(t["units"]) for t in tok_b))
    U = np.zeros((len(tok_b), S, ncb), np.int64)
    P = np.zeros((len(tok_b), S, 2), np.int64)
    for b, t in enumerate(tok_b):
        U[b, :len(t["units"])], P[b, :len(t["units"])] = t["units"], t["segments"]
    n = [len(t["units"]) for t in tok_b]
    fr = [t["frames"] for t in tok_b]
    torch.manual_seed(77)
    art_b = bi.synthesize_units(torch.from_numpy(U), segments=torch.from_numpy(P), nunits=n, frames=fr, steps=3, rand_scale=0.5)
    torch.manual_seed(77)
    art_p = pk.synthesize_units(torch.from_numpy(U), segments=torch.from_numpy(P), nunits=n, frames=fr, steps=3, rand_scale=0.5)
    assert torch.equal(art_p, art_b), (prec, ncb)


# ---- 3. slots and neighbours ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_clip_bits_do_not_depend_on_slot_or_neighbours(cfm, prec):
    d = _decoder(prec)
    cond = torch.from_numpy(cfm["rag_cond"]).cuda()
    # 16 + T = 64 and 128 (whole slots), one frame either side, and the golden clips
    clips = [cond[0, :48], cond[1, :112], cond[2, :47], cond[2, :113], cond[0, :100], cond[1, :230], cond[2, :300], cond[1, :1]]
    alone = [d.sample_packed([c], steps=5)[0] for c in clips]
    for c, a in zip(clips, alone):                                         # a clip alone is sample()'s [1, T] call
        assert torch.equal(a, d.sample(c[None].contiguous(), steps=5)[0])
    for order in (list(range(len(clips))), list(reversed(range(len(clips)))), [3, 0, 7, 5, 1, 6, 2, 4]):
        art, starts = d.sample_packed([clips[i] for i in order], steps=5)
        for j, i in enumerate(order):
            assert torch.equal(art[starts[j]:starts[j + 1]], alone[i]), (prec, order, i)
    # with a neighbour added in front and behind
    extra = cond[2, 5:205]
    art, starts = d.sample_packed([extra, clips[0], clips[1], extra], steps=5)
    assert torch.equal(art[starts[1]:starts[2]], alone[0]) and torch.equal(art[starts[2]:starts[3]], alone[1])


@pytest.mark.parametrize("prec", PRECS)
def test_resynthesize_permuted_clips(prec):
    pk = _synthesis(prec, "packed")
    wavs = _wavs()
    art, segs = pk.resynthesize(input_values=wavs, steps=5)
    order = [4, 2, 0, 5, 1, 3]
    art2, segs2 = pk.resynthesize(input_values=[wavs[i] for i in order], steps=5)
    for j, i in enumerate(order):
        assert torch.equal(art2[j], art[i]), (prec, i)
        assert np.array_equal(np.asarray(segs2[j]).reshape(-1, 2), np.asarray(segs[i]).reshape(-1, 2))
    one, s1 = pk.resynthesize(input_values=[wavs[1]], steps=5)
    T1 = one.shape[1]
    assert torch.equal(one[0], art[1, :T1]) and (art[1, T1:] == 0).all()


# ---- 4. stale workspace and non-finite neighbours ------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_nan_workspace_and_nan_neighbour(cfm, prec):
    d = _decoder(prec)
    cond = torch.from_numpy(cfm["rag_cond"]).cuda()
    lens = [112, 230, 48, 300]
    clips = [cond[0, :112], cond[1, :230], cond[2, :48], cond[2, :300]]
    clean, starts = d.sample_packed(clips, steps=5)
    # NaN-filled memory for the caching allocator to hand back as the next call's workspace
    from sylber_amd import _lib
    n = int(d.lib.sylber_cfm_workspace_bytes_packed(d.handle, (_lib.ctypes.c_int32 * 4)(*lens), 4))
    junk = torch.full(((n + 3) // 4 + 4096,), float("nan"), device=d.device)
    del junk
    again, _ = d.sample_packed(clips, steps=5)
    assert torch.equal(again, clean), prec
    # a clip of non-finite conditioning leaves its neighbours bit-identical
    for bad_at in (1, 2):
        bad = list(clips)
        bad[bad_at] = bad[bad_at].clone()
        bad[bad_at][3:9] = float("nan")
        bad[bad_at][0, 0] = float("inf")
        art, _ = d.sample_packed(bad, steps=5)
        mine = art[starts[bad_at]:starts[bad_at + 1]]
        assert not torch.equal(mine, clean[starts[bad_at]:starts[bad_at + 1]])
        if prec == "bf16":                        # (the fp16 modes saturate non-finite values on conversion to 16 bits)
            assert not torch.isfinite(mine).all()
        for b in range(len(clips)):
            if b != bad_at:
                assert torch.equal(art[starts[b]:starts[b + 1]], clean[starts[b]:starts[b + 1]]), (prec, bad_at, b)


@pytest.mark.parametrize("prec", PRECS)
def test_nan_features_clip_leaves_neighbours(prec):
    pk = _synthesis(prec, "packed")
    g = torch.Generator().manual_seed(4)
    feats = (torch.randn(3, 120, 768, generator=g) * 0.1).cuda()
    frames = [120, 48, 90]
    clean, _ = pk.resynthesize(features=feats, frames=frames, steps=3)
    bad = feats.clone()
    bad[1, :20] = float("nan")
    art, _ = pk.resynthesize(features=bad, frames=frames, steps=3)
    assert torch.equal(art[0], clean[0]) and torch.equal(art[2], clean[2])
    assert not torch.equal(art[1], clean[1])


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(golden_dir, cfm):
    from sylber_amd import HubertEncoderHIP, Quantizer, SegmentSynthesis, _lib
    from sylber_amd.weights import synthetic_quantizer_state_dict
    with pytest.raises(ValueError, match="packed"):
        SegmentSynthesis(model_ckpt=_checkpoint(), device="cuda:0", precision="fp32", packed=True)
    d32 = _decoder("fp32")
    cond = torch.from_numpy(cfm["rag_cond"]).cuda()
    with pytest.raises(ValueError, match="packed"):
        d32.sample_packed([cond[0, :10]])
    d = _decoder("bf16")
    with pytest.raises(ValueError):
        d.sample_packed([cond[0, :10]], steps=0)
    with pytest.raises(ValueError):
        d.sample_packed([cond[0, :10]], steps=66)
    with pytest.raises(ValueError):
        d.sample_packed((cond[0, :10], [4, 0, 6]))
    with pytest.raises(ValueError):
        d.sample_packed([])
    # the C entry point refuses an fp32 handle and bad counts with a message naming the call
    c = _lib.ctypes.c_int32
    assert d32.lib.sylber_cfm_sample_packed(d32.handle, None, (c * 1)(5), 1, 5, None, 1.0, None, None, None) == 1
    assert b"sylber_cfm_sample_packed" in d32.lib.sylber_last_error()
    assert d.lib.sylber_cfm_workspace_bytes_packed(d.handle, (c * 2)(5, 0), 2) == -1
    assert d.lib.sylber_cfm_workspace_bytes_packed(d32.handle, (c * 1)(5), 1) == -1
    # the learned quantizer, where resynthesize / synthesize_units refuse it today
    meta = json.loads(str(np.load(os.path.join(golden_dir, "quantizer.npz"))["meta_json"]))["a"]
    lq = Quantizer(**meta["cfg"], state_dict=synthetic_quantizer_state_dict(meta["cfg"], meta["seed"], bias_std=meta["bias_std"]),
                   device="cuda:0")
    pk = _synthesis("bf16", "packed", lq)
    x, mask = _pad(_wavs()[:2])
    with pytest.raises(ValueError):
        pk.resynthesize(input_values=x, attention_mask=mask)
    with pytest.raises(ValueError):
        pk.synthesize_units([{"units": np.zeros((1, 1), np.int64), "segments": np.array([[0, 5]]), "frames": 5}])
    # what Segmenter(packed=True) refuses on the encoder side
    pk.quantizer = None
    pk.speech_model.set_option(_lib.OPT_SEGMENT, -1)
    try:
        with pytest.raises(ValueError, match="packed"):
            pk.resynthesize(input_values=x, attention_mask=mask)
    finally:
        pk.speech_model.set_option(_lib.OPT_SEGMENT, 0)
    assert isinstance(pk.speech_model, HubertEncoderHIP)

"""GPU tier, packed batches (sylber_forward_packed / sylber_segment_packed, Segmenter(packed=True)): every clip gets, bit for bit, what
batch-invariant mode (SYLBER_OPT_PER_UTTERANCE on the padded batch) gives it -- whatever its slot, its neighbours, stale workspace
contents or a non-finite neighbour."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRECS = ["bf16", "fp16"]


@pytest.fixture(scope="module")
def sd():
    from sylber_amd.weights import synthetic_state_dict
    return synthetic_state_dict(0, num_layers=9)


@pytest.fixture(scope="module")
def encoders(sd):
    from sylber_amd import HubertEncoderHIP
    out = {}
    for p in PRECS:
        e = HubertEncoderHIP(sd, device="cuda:0", precision=p)
        e.set_per_utterance(True)
        out[p] = e
    return out


def _pad(wavs):
    n = max(len(w) for w in wavs)
    x = torch.zeros(len(wavs), n)
    for i, w in enumerate(wavs):
        x[i, :len(w)] = w
    return x.cuda(), [len(w) for w in wavs]


def _ragged_clips():
    from sylber_amd.synth import syllable_wave
    return [syllable_wave(400, 31)[0], syllable_wave(160000, 32)[0], syllable_wave(960000, 33)[0]]


def _seeded_clips(n=32, seed=5):
    """n clips of 1-20 s, some with T_b % 64 in {0, 1, 63} and some whose conv rows need one frame more than T_b"""
    from sylber_amd.synth import syllable_wave
    rng = np.random.default_rng(seed)
    lengths = [int(x) for x in rng.integers(16000, 20 * 16000, n)]
    t_of = lambda t: 400 + 320 * (t - 1)                                   # noqa: E731 (the shortest clip with t frames)
    lengths[:6] = [t_of(128), t_of(129), t_of(191), t_of(192), t_of(449) - 1, t_of(640) + 300]
    return [syllable_wave(n_, 100 + i)[0] for i, n_ in enumerate(lengths)]


def _packed_rows(enc, wavs):
    h, off, fr = enc.forward_packed(wavs)
    h = h.cpu().numpy()
    return [h[off[b]:off[b] + fr[b]] for b in range(len(wavs))]


def _batch_invariant_rows(enc, wavs):
    x, lengths = _pad(wavs)
    h = enc.forward(x, lengths).cpu().numpy()
    return [h[b, :enc.num_frames(n)] for b, n in enumerate(lengths)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("batch", ["ragged", "seeded32"])
def test_encoder_equals_batch_invariant(encoders, prec, batch):
    enc = encoders[prec]
    wavs = _ragged_clips() if batch == "ragged" else _seeded_clips()
    got = _packed_rows(enc, wavs)
    exp = _batch_invariant_rows(enc, wavs)
    for b in range(len(wavs)):
        assert got[b].shape == exp[b].shape
        assert np.array_equal(got[b], exp[b]), (prec, batch, b, float(np.nanmax(np.abs(got[b] - exp[b]))))


@pytest.mark.parametrize("prec", PRECS)
def test_clip_independent_of_position_and_neighbours(encoders, prec):
    from sylber_amd.synth import syllable_wave
    enc = encoders[prec]
    t = 400 + 320 * 191                                                     # T = 192 (a multiple of 64)
    clip = syllable_wave(t, 61)[0]
    others = [syllable_wave(n, 62 + i)[0] for i, n in enumerate([400, 48000, 33000, 90000, 1200])]
    alone = _packed_rows(enc, [clip])[0]
    assert alone.shape[0] == enc.num_frames(t)
    for batch, pos in (([clip] + others, 0), (others[:2] + [clip] + others[2:], 2), (others[::-1] + [clip], 5),
                       ([others[3], clip, others[1]], 1)):
        rows = _packed_rows(enc, batch)
        assert np.array_equal(rows[pos], alone), (prec, pos)


def _same_dict(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (k, x.shape, y.shape)
        assert np.array_equal(x, y), k


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("outputs", [None, ("segments", "segment_features")])
def test_segmenter_packed_equals_batch_invariant(sd, prec, outputs):
    from sylber_amd import Segmenter
    from sylber_amd.synth import syllable_wave
    kw = {} if outputs is None else {"outputs": outputs}
    clips = [syllable_wave(n, 70 + i) for i, n in enumerate([400, 52000, 16000, 130000, 401, 87000])]
    pk = Segmenter(model_ckpt=sd, device="cuda:0", precision=prec, packed=True, **kw)
    inv = Segmenter(model_ckpt=sd, device="cuda:0", precision=prec, batch_invariant=True, **kw)
    for in_second in (False, True):
        a, b = pk(wav=clips, in_second=in_second), inv(wav=clips, in_second=in_second)
        assert len(a) == len(b) == len(clips)
        for x, y in zip(a, b):
            _same_dict(x, y)
        if outputs is None:
            assert any(len(x["segments"]) for x in a)                      # the batch has segments to compare
    for in_second in (False, True):
        exp = inv(wav=clips, in_second=in_second)
        streamed = list(pk.stream([clips, clips[::-1], clips[1:3]], in_second=in_second))
        for o, s in zip(exp, streamed[0]):
            _same_dict(o, s)
        for o, s in zip(exp[::-1], streamed[1]):
            _same_dict(o, s)
        for o, s in zip(exp[1:3], streamed[2]):
            _same_dict(o, s)
    # a device-resident batch goes through the same packed forward
    exp = inv(wav=clips, in_second=False)
    dev = pk(wav=[c.cuda() for c in clips], in_second=False)
    for o, s in zip(exp, dev):
        _same_dict(o, s)


@pytest.mark.parametrize("prec", PRECS)
def test_segmenter_packed_wav_files(sd, prec, tmp_path):
    """a `wav_file=` list: decoded and normalised on the device (ingest_file), then staged at the slots from device rows"""
    import wave
    from sylber_amd import Segmenter
    from sylber_amd.synth import syllable_wave
    files = []
    for i, n in enumerate([400, 41000, 9000, 120000]):
        pcm = (syllable_wave(n, 80 + i)[0].numpy() * 3000).clip(-32768, 32767).astype(np.int16)
        p = str(tmp_path / ("clip%d.wav" % i))
        with wave.open(p, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
        files.append(p)
    pk = Segmenter(model_ckpt=sd, device="cuda:0", precision=prec, packed=True)
    inv = Segmenter(model_ckpt=sd, device="cuda:0", precision=prec, batch_invariant=True)
    for in_second in (False, True):
        a, b = pk(wav_file=files, in_second=in_second), inv(wav_file=files, in_second=in_second)
        assert len(a) == len(b) == len(files)
        for x, y in zip(a, b):
            _same_dict(x, y)


@pytest.mark.parametrize("prec", PRECS)
def test_poisoned_workspace(encoders, prec):
    from sylber_amd import _lib
    enc = encoders[prec]
    wavs = _seeded_clips(8, seed=9)
    lengths = [len(w) for w in wavs]
    ref = _packed_rows(enc, wavs)
    seg_ref = [t.cpu().numpy() for t in enc.segment_packed(enc.forward_packed(wavs)[0], lengths, 2.6, 0.8)]
    for byte in (0xFF, 0x7F):
        _lib.check(enc.lib.sylber_debug_poison_workspace(enc.handle, byte), "poison")
        got = _packed_rows(enc, wavs)
        for b in range(len(wavs)):
            assert np.array_equal(got[b], ref[b]), (prec, hex(byte), b)
        _lib.check(enc.lib.sylber_debug_poison_workspace(enc.handle, byte), "poison")
        seg = [t.cpu().numpy() for t in enc.segment_packed(enc.forward_packed(wavs)[0], lengths, 2.6, 0.8)]
        n = seg_ref[1]
        assert np.array_equal(seg[1], n)
        for b in range(len(wavs)):
            assert np.array_equal(seg[0][b, :n[b]], seg_ref[0][b, :n[b]])
            assert np.array_equal(seg[2][b, :n[b]], seg_ref[2][b, :n[b]])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("poison", ["head", "first5"])
def test_nan_clip_stays_in_its_slot(encoders, prec, poison):
    """Non-finite samples at the START of clip 3, where clip 2's slot reads into it: conv0's last rows of slot 2 read the first 5
    samples of slot 3, and the last row of slot 2 in conv layers 1-4 reads the first row of slot 3 (all of whose rows are non-finite:
    its GroupNorm statistics are).  So the last conv6 frame of slot 2 -- a padded frame -- is non-finite before the projection.  Clip 2
    has T = 191 in a 192-frame slot: that frame is key 191 of its last 64-key attention tile, masked, but 0 x NaN if its V were
    non-finite.  zero_slot_tails_kernel is what keeps it finite; without it clip 2's rows become NaN."""
    from sylber_amd.segmenter import packed_layout
    enc = encoders[prec]
    wavs = _seeded_clips(6, seed=11)
    off, fr = packed_layout([len(w) for w in wavs])
    assert fr[2] == 191 and off[3] - off[2] == 192                          # clip 2's padded frame lies in its last key tile
    clean = _packed_rows(enc, wavs)
    bad = [w.clone() for w in wavs]
    if poison == "head":
        bad[3][:5000] = float("nan")
        bad[3][6000] = float("inf")
    else:
        bad[3][:5] = float("nan")
    got = _packed_rows(enc, bad)
    assert not np.array_equal(got[3], clean[3])
    if prec == "bf16":                                                      # (the fp16 modes saturate non-finite values on conversion)
        assert np.isnan(got[3]).any()
    for b in range(len(wavs)):
        if b != 3:
            assert np.array_equal(got[b], clean[b]), (prec, poison, b)


def test_refusals(sd):
    from sylber_amd import HubertEncoderHIP, Segmenter
    from sylber_amd.synth import syllable_wave
    wavs = [syllable_wave(16000, 1)[0], syllable_wave(8000, 2)[0]]
    for prec in ("fp32", "fp8", "split16", "mixed16"):
        with pytest.raises(ValueError, match="bf16"):
            Segmenter(model_ckpt=sd, device="cuda:0", precision=prec, packed=True)
    e8 = HubertEncoderHIP(sd, device="cuda:0", precision="fp8")
    with pytest.raises(ValueError, match="bf16"):
        e8.forward_packed(wavs)
    del e8
    seg = Segmenter(model_ckpt=sd, device="cuda:0", packed=True)
    seg.speech_model.set_graph_mode(True)
    with pytest.raises(ValueError, match="graph mode"):
        seg(wav=[w[None] for w in wavs])
    with pytest.raises(ValueError, match="graph mode"):
        seg.speech_model.forward_packed(wavs)
    seg.speech_model.set_graph_mode(False)
    h, off, fr = seg.speech_model.forward_packed(wavs)
    seg.speech_model.set_option(9, -1)
    with pytest.raises(ValueError, match="SYLBER_OPT_SEGMENT"):
        seg.speech_model.segment_packed(h, [len(w) for w in wavs], 2.6, 0.8)
    with pytest.raises(ValueError, match="SYLBER_OPT_SEGMENT"):
        seg(wav=[w[None] for w in wavs])
    seg.speech_model.set_option(9, 0)
    with pytest.raises(ValueError):
        seg.speech_model.forward_packed([wavs[0], wavs[1][:399]])
    assert len(seg(wav=[w[None] for w in wavs])) == 2

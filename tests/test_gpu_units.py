"""GPU tier, syllable units end to end: ``ResidualKMQuantizer`` (csrc/downstream.hip ``sylber_km_assign_residual`` /
``sylber_km_decode_residual``), the fused unit conditioning ``sylber_condition_units`` behind ``SegmentSynthesis.synthesize_units``,
the device ``expand_feature`` (``sylber_expand_units``) and ``SegmentSynthesis.tokenize``.

* residual ids against the float64 restatement tests/units_ref.py (a different id only on a numerical tie); decode bitwise;
* ``synthesize_units`` bitwise ``resynthesize(features=expand_feature(decode(units)))`` in fp32 / bf16 / fp16 with one and two
  codebooks, and within the decoder's measured error of the reference's golden (tests/golden/units.npz, relative RMS:
  fp32 2e-6, fp16 1.2e-3, bf16 1e-2);
* ``synthesize_units(tokenize(wav))`` bitwise ``resynthesize(wav)`` in batch-invariant mode;
* each row of a ragged ``synthesize_units`` batch bitwise the clip alone; bad tables refused with messages."""
import os

import numpy as np
import pytest
import torch

import units_ref as U

pytestmark = pytest.mark.gpu

GOLD_TOL = {"fp32": 2e-6, "fp16": 1.2e-3, "bf16": 1e-2}


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean() / (b ** 2).mean()))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "units.npz"))


def _quantizer(gold, ncb):
    from sylber_amd import KMQuantizer, ResidualKMQuantizer
    return KMQuantizer(gold["c1"], device="cuda:0") if ncb == 1 else ResidualKMQuantizer(gold["c1"], gold["c2"], device="cuda:0")


_SYN = {}


def _checkpoint():
    from sylber_amd.weights import synthetic_mlp_state_dict, synthetic_regressor_state_dict, synthetic_state_dict
    sd = {"speech_model." + k: v for k, v in synthetic_state_dict(0, num_layers=9).items()}
    sd.update({"input_model." + k: v for k, v in synthetic_mlp_state_dict(1).items()})
    sd.update({"regressor." + k: v for k, v in synthetic_regressor_state_dict(0).items()})
    return sd


def _synthesis(prec, quantizer=None, batch_invariant=False, key=None):
    from sylber_amd import SegmentSynthesis
    k = (prec, batch_invariant, key)
    if key is None or k not in _SYN:
        syn = SegmentSynthesis(model_ckpt=_checkpoint(), device="cuda:0", precision=prec, quantizer=quantizer, batch_invariant=batch_invariant)
        if key is None:
            return syn
        _SYN[k] = syn
    return _SYN[k]


def test_residual_ids_match_restatement(gold):
    from sylber_amd import KMQuantizer
    c1, c2 = gold["c1"], gold["c2"]
    q = _quantizer(gold, 2)
    rng = np.random.default_rng(17)
    rand = (c1[rng.integers(0, 64, 300)] + 0.6 * rng.standard_normal((300, 768))).astype(np.float32)
    x = np.concatenate([gold["tokens"], rand])
    idx = q.get_indices(torch.from_numpy(x)[None]).cpu().numpy()
    assert idx.shape == (1, len(x), 2) and idx.dtype == np.int64
    got = idx[0]
    assert np.array_equal(got[:16], gold["tok_ids"])
    exp, d1, d2 = U.residual_assign(x, c1, c2)
    # stage 1 is KMQuantizer(c1) exactly
    k1 = KMQuantizer(c1, device="cuda:0").get_indices(torch.from_numpy(x)).cpu().numpy()[:, 0]
    assert np.array_equal(k1, got[:, 0])
    ties = 0
    for r in range(len(x)):
        if got[r, 0] != exp[r, 0]:                     # a numerical tie of stage 1: stage 2 then sees another residual
            assert abs(d1[r, got[r, 0]] - d1[r, exp[r, 0]]) <= 1e-4 * abs(d1[r, exp[r, 0]]) + 1e-4
            ties += 1
        elif got[r, 1] != exp[r, 1]:
            assert abs(d2[r, got[r, 1]] - d2[r, exp[r, 1]]) <= 1e-4 * abs(d2[r, exp[r, 1]]) + 1e-4
            ties += 1
    print("residual ids: %d of %d rows on a numerical tie" % (ties, len(x)))
    assert ties <= 3
    # and every row under the id rule of tests/tokenizer_ref.py, stage 2 on the residual of the device's own stage-1 id
    import tokenizer_ref as T
    s1, b1 = T.km_bounds(x, c1, False)
    s2, b2 = T.km_bounds((x - c1[got[:, 0]]).astype(np.float32), c2, False)
    assert T.judge_ids(s1, b1, got[:, 0]) == [] and T.judge_ids(s2, b2, got[:, 1]) == []
    dec =q.decode(torch.from_numpy(idx)).cpu().numpy()
    assert np.array_equal(dec[0], c1[got[:, 0]] + c2[got[:, 1]])
    out = q(torch.from_numpy(x[:4]).cuda())
    assert torch.equal(out["indices"].cpu(), torch.from_numpy(got[:4]))
    assert np.array_equal(q.decode(torch.tensor([[-1, -1]])).cpu().numpy()[0], c1[0] + c2[0])     # clip(0), quantizer.py:129


def test_quantizer_paths_and_loaders(gold, tmp_path):
    from sylber_amd import KMQuantizer, ResidualKMQuantizer, load_km_quantizer, load_residualkm_quantizer
    p1, p2 = str(tmp_path / "c1.npy"), str(tmp_path / "c2.npy")
    np.save(p1, gold["c1"]); np.save(p2, gold["c2"])
    q = load_residualkm_quantizer(p1, p2, normalize=True)
    assert isinstance(q, ResidualKMQuantizer)
    assert np.array_equal(q.km2.centroids.cpu().numpy(), gold["c2"])
    assert isinstance(load_km_quantizer(p1, normalize=True), KMQuantizer) and load_km_quantizer(p1, normalize=True).normalize
    # normalize is ignored, as upstream: ids are those of the un-normalised stages
    x = torch.from_numpy(gold["tokens"])
    assert torch.equal(q.get_indices(x), ResidualKMQuantizer(gold["c1"], gold["c2"]).get_indices(x))
    syn = _synthesis("bf16", quantizer=p1, key="paths1")
    assert isinstance(syn.quantizer, KMQuantizer) and not syn.quantizer.normalize
    from sylber_amd import SegmentSynthesis
    sd = _checkpoint()
    syn = SegmentSynthesis(model_ckpt=sd, device="cuda:0", quantizer=p1, residual_quantizer=p2)
    assert isinstance(syn.quantizer, ResidualKMQuantizer)
    assert np.array_equal(syn.quantizer.km.centroids.cpu().numpy(), gold["c1"])
    syn = SegmentSynthesis(model_ckpt=sd, device="cuda:0", quantizer=p1, normalize_embed=True)
    assert isinstance(syn.quantizer, KMQuantizer) and syn.quantizer.normalize
    with pytest.raises(ValueError, match="residual_quantizer"):
        SegmentSynthesis(model_ckpt=sd, device="cuda:0", quantizer=q, residual_quantizer=p2)


def test_device_expand_feature_matches_reference(gold):
    from sylber_amd import expand_feature
    feats = U.decode(gold["units"], [gold["c1"], gold["c2"]])
    avg, dur = U.spans_to_durations(feats, gold["spans"], gold["nunits"], int(gold["T"]))
    out = expand_feature(torch.from_numpy(avg).cuda(), torch.from_numpy(dur))
    assert np.array_equal(out.cpu().numpy(), gold["expanded2"])


@pytest.mark.parametrize("ncb", [1, 2])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_synthesize_units_bitwise_features_path(gold, prec, ncb):
    from sylber_amd import expand_feature
    syn = _synthesis(prec, quantizer=_quantizer(gold, ncb), key="q%d" % ncb)
    T = int(gold["T"])
    units = torch.from_numpy(gold["units"][..., :ncb].astype(np.int64))
    spans, nunits = gold["spans"], gold["nunits"]
    feats = syn.quantizer.decode(units.cuda()).cpu().numpy()                  # [B, S, 768]
    avg, dur = U.spans_to_durations(feats, spans, nunits, T)
    expanded = expand_feature(torch.from_numpy(avg).cuda(), torch.from_numpy(dur))
    # the conditioning input itself
    from sylber_amd.downstream import quantizer_codebooks
    cu = syn.input_model.from_units(quantizer_codebooks(syn.quantizer), units, torch.from_numpy(spans), torch.from_numpy(nunits), T)
    cf = syn.input_model.from_features(expanded)
    assert torch.equal(cu, cf)
    assert (cu[0, 23:35] == 0).all() and (cu[0, :4] == 0).all()                # near-zero unit and leading gap
    art_u = syn.synthesize_units(units, torch.from_numpy(spans), frames=[T, T], nunits=torch.from_numpy(nunits))
    art_f, _ = syn.resynthesize(features=expanded, steps=5, frames=[T, T])
    assert torch.equal(art_u, art_f), (prec, ncb)
    # the same as a list of per-clip tables
    art_l = syn.synthesize_units([units[b, :n] for b, n in enumerate(nunits)], [spans[b, :n] for b, n in enumerate(nunits)], frames=[T, T])
    assert torch.equal(art_u, art_l)
    r = rel_rms(art_u.cpu().numpy(), gold["art%d" % ncb])
    print("%s ncb=%d synthesize_units vs reference golden rel %.3e" % (prec, ncb, r))
    assert r <= GOLD_TOL[prec], r


def _wavs():
    from sylber_amd.synth import syllable_wave
    wavs = [syllable_wave(32000, 21)[0], syllable_wave(20000, 22)[0], syllable_wave(26000, 23)[0]]
    n = max(len(w) for w in wavs)
    x = torch.zeros(len(wavs), n)
    mask = torch.zeros(len(wavs), n)
    for i, w in enumerate(wavs):
        x[i, :len(w)] = w
        mask[i, :len(w)] = 1
    return x.cuda(), mask.cuda()


def _speech_codebooks(ncb):
    """seeded codebooks at the scale of the synthetic encoder's hidden states (norms ~2.5), none near zero: with the golden's
    codebooks every segment mean would pick the near-zero row, whose units synthesize_units silences by design while
    resynthesize masks by the frame's hidden-state norm"""
    from sylber_amd import KMQuantizer, ResidualKMQuantizer
    g = torch.Generator().manual_seed(23)
    c1 = torch.randn(64, 768, generator=g) * 0.09
    c2 = torch.randn(32, 768, generator=g) * 0.03
    return KMQuantizer(c1, device="cuda:0") if ncb == 1 else ResidualKMQuantizer(c1, c2, device="cuda:0")


@pytest.mark.parametrize("ncb,prec", [(1, "bf16"), (2, "bf16"), (2, "fp32")])
def test_round_trip_equals_resynthesize(ncb, prec):
    syn = _synthesis(prec, quantizer=_speech_codebooks(ncb), batch_invariant=True, key="rt%d" % ncb)
    x, mask = _wavs()
    lengths = [int(v) for v in mask.sum(-1).tolist()]
    # the synthetic encoder's hidden-state norms sit below the yaml thresholder's value: take a threshold inside their range,
    # rounded so that no frame sits on it, and report any frame close to it (the two silence masks could disagree there)
    hidden = syn.speech_model.forward(x.contiguous(), lengths)
    frames = syn.speech_model.frame_counts(lengths)
    norms = torch.cat([torch.sqrt((hidden[b, :f].double() ** 2).sum(-1) + 1e-8) for b, f in enumerate(frames)])
    thr = float(np.round(torch.quantile(norms, 0.4).item(), 2))
    near = int(((norms - thr).abs() <= 1e-6 * thr).sum().item())
    print("%s ncb=%d: threshold %.2f, %d frame(s) within 1e-6 of it" % (prec, ncb, thr, near))
    toks = syn.tokenize(x, attention_mask=mask, normthreshold=thr)
    assert len(toks) == 3
    art_r, segs = syn.resynthesize(input_values=x, attention_mask=mask, steps=5, normthreshold=thr)
    for b, t in enumerate(toks):
        assert t["units"].dtype == np.int64 and t["units"].shape == (len(t["segments"]), ncb) and len(t["segments"]) > 0
        assert np.array_equal(t["segments"], np.asarray(segs[b]).reshape(-1, 2))
        assert t["frames"] == frames[b]
    ids = np.concatenate([t["units"] for t in toks])
    print("%d units, %d distinct stage-1 ids" % (len(ids), len(np.unique(ids[:, 0]))))
    assert len(np.unique(ids[:, 0])) > 4
    from sylber_amd.downstream import quantizer_codebooks
    books = [c.cpu().numpy() for c in quantizer_codebooks(syn.quantizer)]
    assert (np.sqrt((U.decode(ids, books).astype(np.float64) ** 2).sum(-1)) > 1e-2).all()
    art_u = syn.synthesize_units(toks, steps=5)
    assert art_u.shape == art_r.shape
    assert torch.equal(art_u, art_r), (prec, ncb)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_ragged_rows_equal_clips_alone(gold, prec):
    syn = _synthesis(prec, quantizer=_quantizer(gold, 2), key="q2")
    units, spans, n = gold["units"].astype(np.int64), gold["spans"].astype(np.int64), gold["nunits"]
    clips = [(units[0, :n[0]], spans[0, :n[0]], 50), (units[1, :n[1]], spans[1, :n[1]], 64), (units[1, :2], spans[1, :2], 9)]
    art = syn.synthesize_units([c[0] for c in clips], [c[1] for c in clips], frames=[c[2] for c in clips]).cpu()
    assert art.shape == (3, 64, 14)
    for b, (u, s, f) in enumerate(clips):
        one = syn.synthesize_units([u], [s], frames=[f]).cpu()
        assert one.shape == (1, f, 14)
        assert torch.equal(art[b, :f], one[0]), (prec, b)
        assert (art[b, f:] == 0).all()
    # default frames: each clip's last segment end
    d = syn.synthesize_units([c[0] for c in clips[2:]], [c[1] for c in clips[2:]])
    assert d.shape == (1, 9, 14) and torch.equal(d.cpu()[0], art[2, :9])


def test_bad_input_is_refused(gold):
    from sylber_amd import _lib, expand_feature
    syn = _synthesis("bf16", quantizer=_quantizer(gold, 2), key="q2")
    u = gold["units"][0, :2].astype(np.int64)
    s = gold["spans"][0, :2].astype(np.int64)
    for bad_u in ([[64, 0], [1, 1]], [[0, 32], [1, 1]], [[-2, 0], [1, 1]]):
        with pytest.raises(_lib.SylberHipError, match="sylber_condition_units.*unit ids"):
            syn.synthesize_units([np.asarray(bad_u)], [s])
    assert syn.synthesize_units([np.asarray([[-1, -1], [1, 1]])], [s]).shape == (1, 20, 14)     # -1 reads as 0
    for bad_s in ([[4, 12], [11, 20]], [[4, 4], [12, 20]], [[-1, 12], [12, 20]], [[12, 20], [4, 12]]):
        with pytest.raises(_lib.SylberHipError, match="sylber_condition_units.*spans"):
            syn.synthesize_units([u], [np.asarray(bad_s)])
    with pytest.raises(_lib.SylberHipError, match="spans"):
        syn.synthesize_units([u], [s], frames=[15])                          # a span past T = max(frames)
    with pytest.raises(ValueError, match="id"):
        syn.synthesize_units([u[:, :1]], [s])                                # one id per unit for a two-codebook quantizer
    with pytest.raises(ValueError, match="segment"):
        syn.synthesize_units([u], [s[:1]])
    # durations: ragged sums, negative entries (Python) and the C-ABI's own check
    feats = torch.zeros(2, 3, 768, device="cuda:0")
    with pytest.raises(ValueError, match="sum"):
        expand_feature(feats, torch.tensor([[[2, 1], [1, 0], [0, 0]], [[2, 1], [1, 1], [0, 0]]]))
    with pytest.raises(ValueError, match=">= 0"):
        expand_feature(feats, torch.tensor([[[2, 1], [1, 0], [0, 0]], [[5, -1], [0, 0], [0, 0]]]))
    lib = _lib.load()
    dur = torch.tensor([[[2, 1], [1, 0], [0, 0]], [[2, 1], [1, 1], [0, 0]]], dtype=torch.int32, device="cuda:0")
    out = torch.empty(2, 5, 768, device="cuda:0")
    ws = torch.empty(7, dtype=torch.int32, device="cuda:0")
    st = lib.sylber_expand_units(feats.data_ptr(), dur.data_ptr(), 2, 3, 768, 4, out.data_ptr(), ws.data_ptr(), None)
    assert st != 0 and b"sylber_expand_units" in lib.sylber_last_error() and b"sum to T" in lib.sylber_last_error()
    assert lib.sylber_expand_units(None, dur.data_ptr(), 2, 3, 768, 4, out.data_ptr(), ws.data_ptr(), None) != 0
    # no quantizer
    plain = _synthesis("bf16", key="plain")
    x, mask = _wavs()
    with pytest.raises(ValueError, match="quantizer"):
        plain.tokenize(x, attention_mask=mask)
    with pytest.raises(ValueError, match="quantizer"):
        plain.synthesize_units([u], [s])

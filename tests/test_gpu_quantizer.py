"""GPU tier, learned quantizer (``sylber_amd.Quantizer`` / ``load_quantizer``; csrc/downstream.hip ``sylber_lq_norm``, ``sylber_ffenc``,
``sylber_rvq_*``):

* the reference's own run (tests/golden/quantizer.npz) for configs (a) and (b): ids bitwise, ``non_quantized`` / ``quantize`` /
  ``decode`` within 2e-6 relative RMS;
* 20 k random rows of (a) against the float64 restatement tests/quantizer_ref.py: exact ids wherever every stage's margin exceeds
  1e-5, and >= 99.9 % of all rows exact;
* ``forward(x)["quantize"]`` bitwise ``decode(get_indices(x))``; a row's ids independent of the batch around it;
* ``n = 0``, blank rows, host / numpy / device inputs, leading shapes; ``load_quantizer`` from a checkpoint file;
* ``SegmentSynthesis(quantizer=Quantizer).tokenize``; ``resynthesize`` / ``synthesize_units`` refuse a learned quantizer."""
import json
import os

import numpy as np
import pytest
import torch

import quantizer_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-6


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean() / (b ** 2).mean()))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "quantizer.npz"))


_Q = {}


def _case(gold, case):
    """(Quantizer, cfg, state dict) of a golden config, built once per module"""
    if case not in _Q:
        from sylber_amd import Quantizer
        from sylber_amd.weights import synthetic_quantizer_state_dict
        meta = json.loads(str(gold["meta_json"]))[case]
        sd = synthetic_quantizer_state_dict(meta["cfg"], meta["seed"], bias_std=meta["bias_std"])
        _Q[case] = (Quantizer(**meta["cfg"], state_dict=sd, device="cuda:0"), meta["cfg"], sd)
    return _Q[case]


@pytest.mark.parametrize("case", ["a", "b"])
def test_golden(gold, case):
    q, cfg, sd = _case(gold, case)
    x = gold[case + "_tokens"]
    o = q(x)
    assert o["indices"].dtype == torch.int64 and o["indices"].is_cuda
    assert np.array_equal(o["indices"].cpu().numpy(), gold[case + "_indices"])
    assert np.array_equal(q.get_indices(x).cpu().numpy(), gold[case + "_indices"])
    for key in ("non_quantized", "quantize"):
        r = rel_rms(o[key].cpu().numpy(), gold[case + "_" + key])
        print("%s %s rel-rms %.2e" % (case, key, r))
        assert r < TOL, (key, r)
    dec = q.decode(torch.from_numpy(gold[case + "_decode_ids"]).cuda())
    r = rel_rms(dec.cpu().numpy(), gold[case + "_decode"])
    print("%s decode rel-rms %.2e" % (case, r))
    assert r < TOL
    blank = (x.astype(np.float64) ** 2).sum(1) == 0
    assert (o["non_quantized"].cpu().numpy()[blank] == 0).all()
    assert float(o["commitment_loss"]) == 0.0


def _random_rows(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 768)) * rng.choice([0.1, 1.0, 10.0], (n, 1))
    x[rng.integers(0, n, n // 200)] = 0.0
    return x.astype(np.float32)


def test_random_rows_against_restatement(gold):
    q, cfg, sd = _case(gold, "a")
    x = _random_rows(20000, 5)
    got = q.get_indices(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = R.forward(x, sd, cfg)
    clear = (ref["gaps"] > 1e-5).all(1)
    exact = (got == ref["indices"]).all(1)
    print("20000 rows: %d with a margin > 1e-5 at every stage, %d exact" % (clear.sum(), exact.sum()))
    assert exact[clear].all(), np.flatnonzero(clear & ~exact)[:10]
    assert exact.mean() >= 0.999


def test_quantize_is_decode_of_ids(gold):
    for case in ("a", "b"):
        q, _, _ = _case(gold, case)
        x = torch.from_numpy(_random_rows(3000, 6)[:, :q.input_dim].copy()).cuda()
        o = q(x)
        assert torch.equal(o["indices"], q.get_indices(x))
        assert torch.equal(o["quantize"], q.decode(o["indices"])), case


def test_ids_independent_of_batch(gold):
    q, _, _ = _case(gold, "a")
    x = torch.from_numpy(_random_rows(20000, 7)).cuda()
    full = q.get_indices(x)
    pick = torch.tensor([0, 1, 63, 64, 65, 4095, 12345, 19999], device="cuda")
    alone = torch.cat([q.get_indices(x[i:i + 1]) for i in pick.tolist()])
    assert torch.equal(alone, full[pick])
    assert torch.equal(q.get_indices(x[pick]), full[pick])
    assert torch.equal(q.get_indices(x[5:300]), full[5:300])
    o_full, o_part = q(x[:700]), q(x[100:101])
    for k in ("non_quantized", "quantize"):
        assert torch.equal(o_part[k][0], o_full[k][100])


def test_shapes_and_inputs(gold):
    q, _, _ = _case(gold, "a")
    x = _random_rows(24, 8)
    x[3] = 0.0
    ref = q.get_indices(torch.from_numpy(x).cuda())
    assert tuple(ref.shape) == (24, 6)
    assert torch.equal(q.get_indices(x), ref)                                  # numpy
    assert torch.equal(q.get_indices(torch.from_numpy(x)), ref)                # host tensor
    assert torch.equal(q.get_indices(torch.from_numpy(x).double()), ref)       # other dtype
    b = q.get_indices(torch.from_numpy(x.reshape(2, 3, 4, 768)))
    assert tuple(b.shape) == (2, 3, 4, 6) and torch.equal(b.reshape(24, 6), ref)
    o = q(torch.from_numpy(x.reshape(4, 6, 768)).cuda())
    assert tuple(o["quantize"].shape) == (4, 6, 72) and tuple(o["non_quantized"].shape) == (4, 6, 72)
    assert (o["non_quantized"].reshape(24, 72)[3] == 0).all()
    d = q.decode(b)
    assert tuple(d.shape) == (2, 3, 4, 72) and torch.equal(d.reshape(24, 72), o["quantize"].reshape(24, 72))
    for lead in ((0,), (2, 0)):
        e = q.get_indices(torch.zeros(lead + (768,)))
        assert tuple(e.shape) == lead + (6,) and e.dtype == torch.int64
        oe = q(np.zeros(lead + (768,), np.float32))
        assert tuple(oe["quantize"].shape) == lead + (72,) and tuple(oe["indices"].shape) == lead + (6,)
        assert tuple(q.decode(e).shape) == lead + (72,)
    with pytest.raises(ValueError):
        q.get_indices(torch.zeros(3, 767))
    with pytest.raises(ValueError):
        q.decode(torch.zeros(3, 5, dtype=torch.int64))
    # ids past the codebook clamp to its last row, negative ones clip to 0
    big = torch.tensor([[5000, 0, 0, 0, 0, 0], [-1, -7, 0, 0, 70, -2]])
    want = torch.tensor([[1023, 0, 0, 0, 0, 0], [0, 0, 0, 0, 63, 0]])
    assert torch.equal(q.decode(big), q.decode(want))


def test_load_quantizer_from_checkpoint(gold, tmp_path):
    from sylber_amd import load_quantizer
    q, cfg, sd = _case(gold, "b")
    path = str(tmp_path / "q.ckpt")
    torch.save({"config": cfg, "state_dict": sd}, path)
    x = gold["b_tokens"]
    o = q(x)
    for loaded in (load_quantizer(path, device="cuda:0"), load_quantizer(ckpt=path, device="cuda:0"), load_quantizer(cfg, ckpt=path)):
        ol = loaded(x)
        for k in ("indices", "quantize", "non_quantized"):
            assert torch.equal(ol[k], o[k]), k
    with pytest.raises(ValueError, match="without weights"):
        load_quantizer(cfg)


def test_segment_synthesis_tokenize(gold):
    from sylber_amd import SegmentSynthesis
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_mlp_state_dict, synthetic_regressor_state_dict, synthetic_state_dict
    q, _, _ = _case(gold, "a")
    sd = {"speech_model." + k: v for k, v in synthetic_state_dict(0, num_layers=9).items()}
    sd.update({"input_model." + k: v for k, v in synthetic_mlp_state_dict(1).items()})
    sd.update({"regressor." + k: v for k, v in synthetic_regressor_state_dict(0).items()})
    syn = SegmentSynthesis(model_ckpt=sd, device="cuda:0", precision="fp32", quantizer=q)
    wavs = [syllable_wave(32000, 21)[0], syllable_wave(20000, 22)[0]]
    x = torch.zeros(2, 32000)
    mask = torch.zeros(2, 32000)
    for i, w in enumerate(wavs):
        x[i, :len(w)] = w
        mask[i, :len(w)] = 1
    x, mask = x.cuda(), mask.cuda()
    hidden = syn.speech_model.forward(x.contiguous(), [int(v) for v in mask.sum(-1).tolist()])
    thr = float(torch.quantile(torch.sqrt((hidden.double() ** 2).sum(-1) + 1e-8).flatten(), 0.4).item())
    toks = syn.tokenize(x, attention_mask=mask, normthreshold=thr)
    _, _, _, nseg, feats, nseg_h, _ = syn.speech_model.segment_batch(x, mask, thr, 0.8, False)
    assert len(toks) == 2 and sum(int(n) for n in nseg_h) > 2
    for b, t in enumerate(toks):
        n = int(nseg_h[b])
        assert t["units"].dtype == np.int64 and t["units"].shape == (n, 6) and t["segments"].shape == (n, 2)
        means = feats[b, :n].contiguous()
        assert np.array_equal(t["units"], q.get_indices(means).cpu().numpy())
    with pytest.raises(ValueError, match="Quantizer"):
        syn.resynthesize(input_values=x, attention_mask=mask, steps=2, normthreshold=thr)
    with pytest.raises(ValueError, match="Quantizer"):
        syn.synthesize_units(toks, steps=2)
    from sylber_amd.downstream import quantizer_codebooks
    with pytest.raises(ValueError, match="Quantizer"):
        quantizer_codebooks(q)

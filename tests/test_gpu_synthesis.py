"""GPU tier, resynthesis decoder through the C-ABI (``sylber_cfm_*``, csrc/cfm.hip) and ``SegmentSynthesis.resynthesize`` end to
end, against the golden of the reference's own ``Regressor`` / ``sample`` (tests/golden/cfm_decoder.npz, tools/gen_golden_cfm.py)
and the test-only restatement tests/cfm_ref.py.

Tolerances (relative RMS against the fp32 golden): fp32 1e-4, bf16 2e-2, fp16 4e-3.  Measured on an MI355X, largest over these
cases: fp32 2.0e-6, bf16 9.9e-3, fp16 1.2e-3, so the 16-bit bounds sit 2-3x above what the kernels do."""
import os

import numpy as np
import pytest
import torch

import cfm_ref as R

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-4, "bf16": 2e-2, "fp16": 4e-3}
PRECS = ["fp32", "bf16", "fp16"]


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean() / (b ** 2).mean()))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cfm_decoder.npz"))


@pytest.fixture(scope="module")
def sd():
    from sylber_amd.weights import synthetic_regressor_state_dict
    return synthetic_regressor_state_dict(0)


_DEC = {}


def decoder(sd, prec):
    from sylber_amd.synthesis import CfmDecoder
    if prec not in _DEC:
        _DEC[prec] = CfmDecoder(sd, device="cuda:0", precision=prec)
    return _DEC[prec]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("prec", PRECS)
def test_eval_matches_golden(golden, sd, prec):
    d = decoder(sd, prec)
    for i in range(2):
        v = d.eval(dev(golden["x"]), float(golden["eval_t%d_time" % i]), dev(golden["cond"])).cpu().numpy()
        r = rel_rms(v, golden["eval_t%d" % i])
        print("%s eval t%d rel %.3e" % (prec, i, r))
        assert np.isfinite(v).all() and r <= TOL[prec], r


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("steps", [2, 5])
def test_sample_matches_golden(golden, sd, prec, steps):
    d = decoder(sd, prec)
    for kind in ("zero", "y0"):
        y0 = dev(golden["y0"]) if kind == "y0" else None
        art = d.sample(dev(golden["cond"]), steps=steps, y0=y0).cpu().numpy()
        r = rel_rms(art, golden["s%d_%s" % (steps, kind)])
        print("%s sample steps=%d %s rel %.3e" % (prec, steps, kind, r))
        assert r <= TOL[prec], r


@pytest.mark.parametrize("prec", PRECS)
def test_one_step_returns_y0_with_pitch_scaling(golden, sd, prec):
    d = decoder(sd, prec)
    y0 = torch.from_numpy(golden["y0"])
    exp = y0.clone()
    exp[..., 12] = exp[..., 12] / 5
    art = d.sample(dev(golden["cond"]), steps=1, y0=y0.cuda(), pitch_amp=5).cpu()
    assert torch.equal(art, exp)
    assert np.array_equal(d.sample(dev(golden["cond"]), steps=1).cpu().numpy(), golden["s1_zero"])


@pytest.mark.parametrize("prec", PRECS)
def test_ragged_batch_golden_and_batch_shape_invariance(golden, sd, prec):
    """clip b of a ragged batch is bit-identical to that clip alone, zero-padded to the same Tmax"""
    d = decoder(sd, prec)
    cond = dev(golden["rag_cond"])
    art = d.sample(cond, steps=5).cpu().numpy()
    r = rel_rms(art, golden["ragged"])
    print("%s ragged rel %.3e" % (prec, r))
    assert r <= TOL[prec], r
    for b in range(cond.shape[0]):
        one = d.sample(cond[b:b + 1].contiguous(), steps=5).cpu().numpy()
        assert np.array_equal(one[0], art[b]), b


def _synthesis(prec):
    from sylber_amd import SegmentSynthesis
    from sylber_amd.weights import synthetic_mlp_state_dict, synthetic_regressor_state_dict, synthetic_state_dict
    sd = {"speech_model." + k: v for k, v in synthetic_state_dict(0, num_layers=9).items()}
    sd.update({"input_model." + k: v for k, v in synthetic_mlp_state_dict(1).items()})
    reg = synthetic_regressor_state_dict(0)
    sd.update({"regressor." + k: v for k, v in reg.items()})
    sd.update({"cfm_wrapper.regressor." + k: v for k, v in reg.items()})
    return SegmentSynthesis(model_ckpt={"state_dict": {"net." + k: v for k, v in sd.items()}}, device="cuda:0", precision=prec), sd


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_resynthesize_end_to_end(sd, prec):
    from sylber_amd import Segmenter
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_state_dict
    syn, _ = _synthesis(prec)
    wavs = [syllable_wave(24000, 1), syllable_wave(24000, 2)]
    x = torch.cat(wavs, dim=0)
    art, segments = syn.resynthesize(input_values=x, steps=5)
    assert art.shape == (2, syn.speech_model.num_frames(24000), 14) and art.dtype == torch.float32 and art.is_cuda
    # segments equal the Segmenter's on the same audio at the thresholder's value
    thr = syn.get_threshold()
    seg = Segmenter(model_ckpt=synthetic_state_dict(0, num_layers=9), device="cuda:0", norm_threshold=thr, merge_threshold=0.8,
                    precision=prec)
    outs = seg(wav=[w for w in wavs], in_second=False)
    assert len(segments) == 2
    for o, s in zip(outs, segments):
        assert np.array_equal(np.asarray(o["segments"]).reshape(-1, 2), np.asarray(s).reshape(-1, 2))
    # art against the restatement run on the engine's own conditioning input
    hidden = syn.speech_model.forward(x.cuda().contiguous())
    sg, ns, ft = syn.speech_model.segment(hidden, thr, 0.8)
    cond, _ = syn.input_model(hidden, sg, ns, ft, thr)
    exp = R.sample(sd, cond.cpu(), 5, pitch_amp=5).numpy()
    r = rel_rms(art.cpu().numpy(), exp)
    print("%s resynthesize rel %.3e" % (prec, r))
    assert r <= TOL[prec], r


def test_resynthesize_features_branch_matches_golden(golden):
    syn, _ = _synthesis("fp32")
    art, segments = syn.resynthesize(features=dev(golden["feat"]), steps=5)
    assert segments is None
    r = rel_rms(art.cpu().numpy(), golden["feat_art"])
    assert r <= TOL["fp32"], r
    # rand_scale with an explicit start: y0 = the noise
    y0 = torch.zeros(2, 37, 14, device="cuda:0")
    art2, _ = syn.resynthesize(features=dev(golden["feat"]), steps=5, rand_scale=1.0, y0=y0)
    assert torch.equal(art, art2)


def test_errors_are_clean(golden, sd):
    from sylber_amd.synthesis import CfmDecoder
    d = decoder(sd, "bf16")
    cond = dev(golden["cond"])
    for steps in (0, -1, 66, 2.5):
        with pytest.raises(ValueError, match="steps"):
            d.sample(cond, steps=steps)
    with pytest.raises(ValueError, match="cond_emb"):
        d.sample(cond[..., :128])
    with pytest.raises(ValueError, match="y0"):
        d.sample(cond, y0=torch.zeros(2, 41, 14, device="cuda:0"))
    with pytest.raises(ValueError, match="precision"):
        CfmDecoder(sd, precision="fp8")
    bad = dict(sd)
    bad["transformer.register_tokens"] = torch.zeros(4, 512)
    with pytest.raises(ValueError, match="register_tokens"):
        CfmDecoder(bad)
    # the C-ABI's own checks
    lib = d.lib
    ws = torch.empty(16, dtype=torch.uint8, device="cuda:0")
    st = lib.sylber_cfm_sample(d.handle, cond.data_ptr(), 2, 40, 0, None, 5.0, cond.data_ptr(), ws.data_ptr(), None)
    assert st != 0 and b"steps" in lib.sylber_last_error()
    st = lib.sylber_cfm_sample(d.handle, cond.data_ptr(), 0, 40, 5, None, 5.0, cond.data_ptr(), ws.data_ptr(), None)
    assert st != 0
    assert lib.sylber_cfm_workspace_bytes(d.handle, 0, 40) == -1

"""CPU tier, resynthesis decoder: the test-only restatement (tests/cfm_ref.py) against the golden the reference's own
``Regressor`` / ``ConditionalFlowMatcherWrapperRegressor.sample`` produced (tools/gen_golden_cfm.py), the thresholder's closed
form, and the checkpoint mapping of ``sylber_amd.synthesis`` (no GPU needed for any of it)."""
import json
import os
import re

import numpy as np
import pytest
import torch

import cfm_ref as R
from sylber_amd import synthesis as S
from sylber_amd.weights import synthetic_mlp_state_dict, synthetic_regressor_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean() / (b ** 2).mean()))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cfm_decoder.npz"))


@pytest.fixture(scope="module")
def sd():
    return synthetic_regressor_state_dict(0)


def test_restatement_eval_matches_reference_golden(golden, sd):
    for i in range(2):
        v = R.evaluate(sd, torch.from_numpy(golden["x"]), float(golden["eval_t%d_time" % i]), torch.from_numpy(golden["cond"]))
        assert rel_rms(v.numpy(), golden["eval_t%d" % i]) <= 1e-5


@pytest.mark.parametrize("steps", [1, 2, 5])
def test_restatement_sample_matches_reference_golden(golden, sd, steps):
    cond, y0 = torch.from_numpy(golden["cond"]), torch.from_numpy(golden["y0"])
    out = R.sample(sd, cond, steps, y0)
    if steps == 1:
        assert np.array_equal(out.numpy(), golden["s1_y0"])
        assert not golden["s1_zero"].any()
    else:
        assert rel_rms(out.numpy(), golden["s%d_y0" % steps]) <= 1e-5
        assert rel_rms(R.sample(sd, cond, steps).numpy(), golden["s%d_zero" % steps]) <= 1e-5


def test_restatement_ragged_batch_matches_reference_golden(golden, sd):
    out = R.sample(sd, torch.from_numpy(golden["rag_cond"]), 5)
    assert rel_rms(out.numpy(), golden["ragged"]) <= 1e-5


def test_restatement_features_branch_matches_reference_golden(golden, sd):
    from oracle import downstream_ref
    f = torch.from_numpy(golden["feat"])
    cond = downstream_ref.resynth_front_features(synthetic_mlp_state_dict(1), f)
    art = R.sample(sd, cond, 5, pitch_amp=5)
    assert rel_rms(art.numpy(), golden["feat_art"]) <= 1e-5


def test_thresholder_closed_form_matches_golden(golden):
    c = S.DEFAULT_THRESHOLDER_CONFIGS
    thr = S.threshold_from_stats(c["signal_mean"], c["signal_var"], c["noise_mean"], c["noise_var"])
    # the same fp32 operations as the reference, in its order; torch's vectorised log / sqrt on the CPU may differ by one ulp
    # between CPU generations (the golden was written on one, the suite also runs on others), so: within two ulp
    assert abs(np.float32(thr) - golden["thr"]) <= 2 * np.spacing(golden["thr"]), (thr, golden["thr"])
    meta = json.loads(str(golden["meta_json"]))
    assert meta["thr_stats"] == c


def test_golden_is_small_and_holds_every_case(golden):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "cfm_decoder.npz")) < 3_000_000
    for k in ("eval_t0", "eval_t1", "s1_zero", "s1_y0", "s2_zero", "s2_y0", "s5_zero", "s5_y0", "ragged", "feat_art", "thr"):
        assert k in golden.files, k


def _synthesis_state_dict():
    """a SegmentSynthesis.state_dict()-shaped dict (encoder: one synthetic layer) with the regressor twice, as upstream saves it"""
    from sylber_amd.weights import synthetic_state_dict
    sd = {"speech_model." + k: v for k, v in synthetic_state_dict(0, num_layers=1).items()}
    sd.update({"input_model." + k: v for k, v in synthetic_mlp_state_dict(1).items()})
    reg = synthetic_regressor_state_dict(0)
    sd.update({"regressor." + k: v for k, v in reg.items()})
    sd.update({"cfm_wrapper.regressor." + k: v for k, v in reg.items()})
    for k, v in S.DEFAULT_THRESHOLDER_CONFIGS.items():
        sd["thresholder." + k] = torch.tensor([v])
    return sd, reg


def test_checkpoint_layouts_map_to_the_regressor(tmp_path):
    sd, reg = _synthesis_state_dict()
    path = tmp_path / "syn.pt"
    torch.save(sd, path)
    for ckpt in (str(path), sd, {"state_dict": {"net." + k: v for k, v in sd.items()}}):
        got = S.regressor_state_dict(S.unwrap_checkpoint(ckpt))
        assert set(got) == set(reg)
        assert all(torch.equal(got[k], reg[k]) for k in reg)
    only_dup = {k: v for k, v in sd.items() if not k.startswith("regressor.")}          # the cfm_wrapper. duplicate alone
    assert set(S.regressor_state_dict(only_dup)) == set(reg)
    # unused keys are ignored
    assert "to_cond_emb.weight" in reg and "null_cond" in reg


def test_checkpoint_missing_key_raises_keyerror():
    reg = synthetic_regressor_state_dict(0)
    del reg["transformer.layers.3.5.0.bias"]
    with pytest.raises(KeyError, match=re.escape("transformer.layers.3.5.0.bias")):
        S.regressor_state_dict(reg)


def test_foreign_geometry_raises_valueerror():
    reg = synthetic_regressor_state_dict(0)
    reg["transformer.layers.0.3.to_qkv.weight"] = torch.zeros(3 * 1024, 512)
    with pytest.raises(ValueError, match="to_qkv"):
        S.regressor_state_dict(reg)
    with pytest.raises(ValueError, match="dim"):
        S.check_regressor_configs(dict(S.DEFAULT_REGRESSOR_CONFIGS, dim=1024))
    with pytest.raises(ValueError, match="depth"):
        S.check_regressor_configs(dict(S.DEFAULT_REGRESSOR_CONFIGS, depth=24))
    S.check_regressor_configs(S.DEFAULT_REGRESSOR_CONFIGS)


def test_thresholder_falls_back_to_checkpoint_stats():
    stats = dict(signal_mean=5.0, signal_var=1.1, noise_mean=0.5, noise_var=0.4)
    a = S.threshold_from_stats(**stats)
    b = S.threshold_from_stats(**{k: torch.tensor([v]) for k, v in stats.items()})
    assert a == b and 0.5 < a < 5.0


def test_product_does_not_import_the_restatement():
    """tests/cfm_ref.py is test infrastructure: nothing under sylber_amd/ may import it"""
    pkg = os.path.join(ROOT, "sylber_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+(tests\.)?cfm_ref\b", src, re.M), f
                assert "cfm_ref" not in src, f


@pytest.mark.reference
def test_golden_regenerates_from_the_reference(golden, sd):
    """one golden case regenerated live from the reference's own code (needs the upstream checkout)"""
    from tools import ref_shim
    if not ref_shim.available():
        pytest.skip("reference checkout not present")
    from tools import gen_golden_cfm as G
    fm = G.load_reference()
    w = G.build_wrapper(fm)
    inp = G.golden_inputs()
    assert np.array_equal(inp["cond"].numpy(), golden["cond"]) and np.array_equal(inp["y0"].numpy(), golden["y0"])
    out = G.sample_with(w, inp["cond"], 2, inp["y0"]).numpy()
    assert rel_rms(out, golden["s2_y0"]) <= 1e-6           # (bit-identical on the machine that wrote it; CPU kernels may differ elsewhere)


# ---- the float64 path (tests/test_gpu_decoder_ref.py's reference) ---------------------------------------------------------------
def test_float64_path_matches_reference_golden(golden, sd):
    """the restatement in float64 (``to_f64``; the time grid and the rotary angles stay fp32, as upstream computes them) against the
    fp32 golden: within fp32 noise.  Measured 1.2e-6 (eval), 1.0e-6 / 5.2e-7 (steps 2 / 5), 6.0e-7 (ragged)."""
    sd64 = R.to_f64(sd)
    cond, y0 = torch.from_numpy(golden["cond"]).double(), torch.from_numpy(golden["y0"]).double()
    v = R.evaluate(sd64, torch.from_numpy(golden["x"]).double(), float(golden["eval_t0_time"]), cond)
    assert v.dtype == torch.float64 and rel_rms(v.numpy(), golden["eval_t0"]) <= 1e-5
    for steps in (2, 5):
        out = R.sample(sd64, cond, steps, y0)
        assert out.dtype == torch.float64 and rel_rms(out.numpy(), golden["s%d_y0" % steps]) <= 1e-5, steps
    out = R.sample(sd64, cond, 5)                                           # y0 = None: the zero start is float64 too
    assert out.dtype == torch.float64 and rel_rms(out.numpy(), golden["s5_zero"]) <= 1e-5
    out = R.sample(sd64, torch.from_numpy(golden["rag_cond"]).double(), 5)
    assert rel_rms(out.numpy(), golden["ragged"]) <= 1e-5


def test_float64_path_is_more_than_fp32_noise_away_from_fp32(golden, sd):
    """the float64 path really runs in float64: not bit-equal to the fp32 path, but within fp32 noise of it"""
    cond = torch.from_numpy(golden["cond"])
    a = R.sample(sd, cond, 2).numpy()
    b = R.sample(R.to_f64(sd), cond.double(), 2).numpy()
    assert not np.array_equal(a.astype(np.float64), b)
    assert rel_rms(a, b) <= 1e-5


@pytest.mark.parametrize("T", [1, 15])
def test_float64_path_short_clips_are_sane(sd, T):
    """below 31 frames the conv's 31-tap window pads both ends at once: finite, the right shape, O(1) velocities, and frame t of a
    padded batch row is not the lone clip's (padded frames are ordinary frames)"""
    g = torch.Generator().manual_seed(T)
    cond = torch.randn(1, T, 256, generator=g, dtype=torch.float64)
    y0 = torch.randn(1, T, 14, generator=g, dtype=torch.float64)
    sd64 = R.to_f64(sd)
    v = R.evaluate(sd64, y0, 0.25, cond)
    out = R.sample(sd64, cond, 3, y0, pitch_amp=5)
    for a in (v, out):
        assert a.shape == (1, T, 14) and a.dtype == torch.float64 and torch.isfinite(a).all()
        assert 1e-2 < a.pow(2).mean().sqrt().item() < 1e2
    # fp32 agrees within fp32 noise
    assert rel_rms(R.evaluate(sd, y0.float(), 0.25, cond.float()).numpy(), v.numpy()) <= 1e-5


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_round16_reference_rounds_where_the_kernels_round(sd, prec):
    """round16= changes the result by about the format's rounding (bf16 ~1e-2, fp16 ~1e-3 relative RMS at the synthetic weights'
    logit scale) and leaves the default path alone"""
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(1, 40, 256, generator=g, dtype=torch.float64)
    x = torch.randn(1, 40, 14, generator=g, dtype=torch.float64)
    sd64 = R.to_f64(sd)
    exact = R.evaluate(sd64, x, 0.25, cond).numpy()
    r = rel_rms(R.evaluate(sd64, x, 0.25, cond, round16=prec).numpy(), exact)
    lo, hi = {"bf16": (2e-3, 3e-2), "fp16": (2e-4, 4e-3)}[prec]
    assert lo < r < hi, r
    assert np.array_equal(R.evaluate(sd64, x, 0.25, cond, round16=None).numpy(), exact)

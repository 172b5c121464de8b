"""CPU tier, learned quantizer: the reference's own ``Quantizer`` / ``load_quantizer`` run (tests/golden/quantizer.npz, written by
tools/gen_golden_quantizer.py) against the float64 restatement tests/quantizer_ref.py, the host-side config validation (every
refused key), the strict state-dict rules and the argument forms of ``load_quantizer``."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import quantizer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "quantizer.npz"))


def _meta(gold):
    return json.loads(str(gold["meta_json"]))


def _sd(meta):
    from sylber_amd.weights import synthetic_quantizer_state_dict
    return synthetic_quantizer_state_dict(meta["cfg"], meta["seed"], bias_std=meta["bias_std"])


def _sha(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k].numpy()).tobytes())
    return h.hexdigest()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("case", ["a", "b"])
def test_synthetic_weights_reproduce_the_fixture(gold, case):
    """the fixture stores a checksum of its weights, not the weights: the seeded generator must give them bit for bit"""
    meta = _meta(gold)[case]
    assert _sha(_sd(meta)) == meta["sd_sha256"]


@pytest.mark.parametrize("case", ["a", "b"])
def test_reference_run_matches_restatement(gold, case):
    """upstream's forward / decode (run by the generator) == the float64 restatement: ids exactly, the rest to fp32 accuracy"""
    meta = _meta(gold)[case]
    sd, cfg = _sd(meta), meta["cfg"]
    x = gold[case + "_tokens"]
    ref = R.forward(x, sd, cfg)
    assert np.array_equal(ref["indices"], gold[case + "_indices"])
    assert (ref["gaps"] > 1e-4).all()
    assert _rel(gold[case + "_non_quantized"], ref["non_quantized"]) < 1e-5
    assert _rel(gold[case + "_quantize"], ref["quantize"]) < 1e-5
    assert _rel(gold[case + "_decode"], R.decode(gold[case + "_decode_ids"], sd, cfg)) < 1e-5


def test_fixture_cases(gold):
    """blank rows, clipped ids and rows far from unit norm are in the fixture; its size stays small"""
    for case in ("a", "b"):
        x = gold[case + "_tokens"]
        blank = (x.astype(np.float64) ** 2).sum(1) == 0
        assert blank.sum() == 3 and (gold[case + "_non_quantized"][blank] == 0).all()
        assert (gold[case + "_decode_ids"] < 0).any()
    nq = gold["b_non_quantized"].astype(np.float64)
    norms = np.sqrt((nq ** 2).sum(1))
    assert (norms[norms > 0] < 0.9).sum() >= 5                         # (b): encoder outputs where the 1e-5 epsilon matters
    a = gold["a_tokens"].astype(np.float64)
    assert (((a ** 2).sum(1) > 0) & ((a ** 2).sum(1) < 1e-4)).sum() >= 5   # (a): inputs where it matters
    assert gold["a_indices"].shape[1] == 6 and gold["b_indices"].shape[1] == 2
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "quantizer.npz")) < 1 << 20


# ---- config validation --------------------------------------------------------------------------------------------------------
def _cfg(**over):
    cfg = dict(encoder_configs=dict(input_dim=768, hidden_dims=[512], output_dim=72),
               art_vq_configs=dict(dim=64, codebook_size=16, num_quantizers=2),
               pitch_vq_configs=dict(dim=8, codebook_size=8, num_quantizers=1), pitch_emb_dim=8)
    for k, v in over.items():
        if k in ("art", "pitch", "enc"):
            key = {"art": "art_vq_configs", "pitch": "pitch_vq_configs", "enc": "encoder_configs"}[k]
            cfg[key] = dict(cfg[key], **v)
        else:
            cfg[k] = v
    return cfg


def _check(cfg):
    from sylber_amd.quantizer import check_quantizer_config
    return check_quantizer_config(cfg["encoder_configs"], cfg["art_vq_configs"], cfg["pitch_vq_configs"], cfg.get("pitch_emb_dim", 8))


def test_config_geometry():
    g = _check(_cfg())
    assert (g["A"], g["p"], g["art"]["num_quantizers"], g["pitch"]["codebook_size"]) == (64, 8, 2, 8)


@pytest.mark.parametrize("key,value", [
    ("groups", 2), ("heads", 2), ("codebook_dim", 32), ("use_cosine_sim", True), ("shared_codebook", True),
    ("stochastic_sample_codes", True), ("accept_image_fmap", True), ("rotation_trick", True), ("implicit_neural_codebook", True)])
def test_refused_vq_keys_are_named(key, value):
    for stack in ("art", "pitch"):
        with pytest.raises(ValueError, match=key):
            _check(_cfg(**{stack: {key: value}}))


def test_accepted_vq_keys():
    training = dict(decay=0.8, commitment_weight=0.25, kmeans_init=True, kmeans_iters=10, threshold_ema_dead_code=2, quantize_dropout=True,
                    quantize_dropout_cutoff_index=1, orthogonal_reg_weight=0.1, orthogonal_reg_max_codes=128, sample_codebook_temp=0.0,
                    learnable_codebook=False, ema_update=True)
    fixed = dict(groups=1, heads=1, codebook_dim=64, use_cosine_sim=False, shared_codebook=False, stochastic_sample_codes=False,
                 accept_image_fmap=False)
    _check(_cfg(art=dict(training, **fixed)))
    _check(_cfg(pitch=dict(training, codebook_dim=8)))


def test_refused_geometry():
    with pytest.raises(ValueError, match="dim"):
        _check(_cfg(art={"dim": 63}))
    with pytest.raises(ValueError, match="dim"):
        _check(_cfg(pitch={"dim": 16}))
    with pytest.raises(ValueError, match="pitch_emb_dim"):
        _check(_cfg(pitch_emb_dim=0, pitch={"dim": 0}))
    with pytest.raises(ValueError, match="pitch_emb_dim"):
        _check(_cfg(pitch_emb_dim=72, art={"dim": 0}, pitch={"dim": 72}))
    with pytest.raises(ValueError, match="activation"):
        _check(_cfg(enc={"activation": "gelu"}))
    with pytest.raises(ValueError, match="codebook_size"):
        _check(_cfg(art={"codebook_size": 0}))
    cfg = _cfg()
    del cfg["art_vq_configs"]["num_quantizers"]
    with pytest.raises(ValueError, match="num_quantizers"):
        _check(cfg)
    g = _check(_cfg(enc={"hidden_dims": []}))                          # FFEncoder with no hidden block: one Linear
    assert g["hidden_dims"] == []


# ---- state dict ---------------------------------------------------------------------------------------------------------------
def _small():
    cfg = dict(encoder_configs=dict(input_dim=20, hidden_dims=[24, 40], output_dim=13),
               art_vq_configs=dict(dim=5, codebook_size=7, num_quantizers=3),
               pitch_vq_configs=dict(dim=8, codebook_size=5, num_quantizers=2), pitch_emb_dim=8)
    from sylber_amd.weights import synthetic_quantizer_state_dict
    return cfg, synthetic_quantizer_state_dict(cfg, 3)


def test_state_dict_rules():
    from sylber_amd.quantizer import padded_host_weights
    cfg, sd = _small()
    g = _check(cfg)
    enc, books = padded_host_weights(g, sd)
    # encoder.mlp.{0, 1.0, 1.3, 2, 3.0, 3.3, 4}: 7 Linears, (W, b) each, zero-padded to multiples of 16
    assert len(enc) == 14 and tuple(enc[0].shape) == (32, 32) and tuple(enc[-2].shape) == (16, 48)
    assert torch.equal(enc[0][:24, :20], sd["encoder.mlp.0.weight"]) and not enc[0][24:].any() and not enc[0][:, 20:].any()
    assert torch.equal(enc[4][:24, :24], sd["encoder.mlp.1.3.weight"])
    cb, K, d = books["art_vq"]
    assert (K, d) == (7, 5) and tuple(cb.shape) == (3, 8, 16) and not cb[:, 7:].any() and not cb[:, :, 5:].any()
    assert torch.equal(cb[2, :7, :5], sd["art_vq.rvqs.0.layers.2._codebook.embed"][0])
    # [K, d] codebooks are accepted as well as [1, K, d]
    sd2 = dict(sd)
    sd2["pitch_vq.rvqs.0.layers.1._codebook.embed"] = sd["pitch_vq.rvqs.0.layers.1._codebook.embed"][0]
    assert torch.equal(padded_host_weights(g, sd2)[1]["pitch_vq"][0], books["pitch_vq"][0])
    # the training buffers may be absent
    sd3 = {k: v for k, v in sd.items() if not k.endswith(("initted", "cluster_size", "embed_avg"))}
    padded_host_weights(g, sd3)
    for missing in ("encoder.mlp.3.0.bias", "encoder.mlp.4.weight", "art_vq.rvqs.0.layers.2._codebook.embed",
                    "pitch_vq.rvqs.0.layers.0._codebook.embed"):
        bad = {k: v for k, v in sd.items() if k != missing}
        with pytest.raises(KeyError, match=missing.replace(".", r"\.")):
            padded_host_weights(g, bad)
    for extra in ("encoder.mlp.5.weight", "encoder.mlp.1.1.weight", "art_vq.rvqs.0.layers.3._codebook.embed", "other.weight"):
        with pytest.raises(KeyError, match=extra.replace(".", r"\.")):
            padded_host_weights(g, dict(sd, **{extra: torch.zeros(1)}))
    with pytest.raises(ValueError, match="encoder.mlp.2"):
        padded_host_weights(g, dict(sd, **{"encoder.mlp.2.weight": torch.zeros(13, 41)}))
    with pytest.raises(ValueError, match="art_vq.rvqs.0.layers.0"):
        padded_host_weights(g, dict(sd, **{"art_vq.rvqs.0.layers.0._codebook.embed": torch.zeros(1, 6, 5)}))


# ---- load_quantizer argument forms ----------------------------------------------------------------------------------------------
def test_load_quantizer_argument_forms(tmp_path):
    import yaml
    from sylber_amd.quantizer import resolve_quantizer_args
    cfg, sd = _small()
    ck = str(tmp_path / "q.ckpt")
    torch.save({"config": cfg, "state_dict": sd}, ck)
    bare = str(tmp_path / "weights.pt")
    torch.save(sd, bare)
    wrapped = str(tmp_path / "wrapped.pt")
    torch.save({"state_dict": sd}, wrapped)
    ym = str(tmp_path / "q.yaml")
    with open(ym, "w") as f:
        yaml.safe_dump({"model": cfg}, f)
    yf = str(tmp_path / "flat.yaml")
    with open(yf, "w") as f:
        yaml.safe_dump(cfg, f)

    def same(got):
        c, s = got
        assert c == cfg and sorted(s) == sorted(sd) and all(torch.equal(s[k], sd[k]) for k in sd)

    same(resolve_quantizer_args(ckpt=ck))                      # a checkpoint alone
    same(resolve_quantizer_args(config=ck))                    # a .ckpt path as the config
    same(resolve_quantizer_args(config=cfg, ckpt=ck))          # a dict and a checkpoint
    same(resolve_quantizer_args(config={"model": cfg}, ckpt=bare))
    same(resolve_quantizer_args(config=ym, ckpt=wrapped))      # YAML nested under `model`
    same(resolve_quantizer_args(config=yf, ckpt=bare))         # flat YAML
    for c in (cfg, ym, yf):
        with pytest.raises(ValueError, match="without weights"):
            resolve_quantizer_args(config=c)
    with pytest.raises(ValueError):
        resolve_quantizer_args()
    with pytest.raises(KeyError):
        resolve_quantizer_args(ckpt=bare)                      # no config anywhere


def test_construction_off_the_gpu_refused():
    from sylber_amd import Quantizer, _lib, load_quantizer
    cfg, sd = _small()
    with pytest.raises(_lib.SylberHipError):
        Quantizer(**cfg, state_dict=sd, device="cpu")
    with pytest.raises(_lib.SylberHipError):
        load_quantizer(cfg, ckpt={"state_dict": sd}, device="cpu")
    with pytest.raises(ValueError, match="pitch_vq_configs"):      # the config is checked before the device
        Quantizer(**_cfg(pitch={"groups": 2}), device="cpu")

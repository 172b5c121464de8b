"""GPU tier: conv layer 0 (+ GroupNorm + GELU), the feature projection and the positional convolution, each ALONE, against the
float64 references of tests/frontend_ref.py -- every element inside a bound derived from the kernel's arithmetic (no element is
left out, nothing is averaged).  The kernels are reached through the taps of sylber_set_stop_stage (negative stages), i.e.
through the launches every forward runs.  tests/test_frontend_ref.py shows on the CPU that these bounds reject an off-by-one
window, a swapped 4-channel run, a row from the next 256-row block, statistics over one frame too few, a late zero tail and a
nonzero halo row at every shape used here."""
import numpy as np
import pytest
import torch

import frontend_ref as fr
from oracle import hubert_ref
from sylber_amd import _lib
from sylber_amd.weights import POS_G_KEYS, synthetic_state_dict
from frontend_ref import CONV0_COMBOS, CONV0_LMAX, FMTS, POSCONV_SHAPES, PROJ_SHAPES, RAGGED_LENS, RAGGED_LMAX, conv0_weights, noise

pytestmark = pytest.mark.gpu

PRECISION = {"bf16": "bf16", "fp16": "fp16", "split16": "split16", "fp32": "fp32", "fp8": "fp8", "mixed16": "mixed16"}


@pytest.fixture(scope="module")
def sds():
    """one encoder layer (the taps stop in front of it); the projection bias is LARGE (+8 on every channel), so a frame that should
    have been zeroed, or a halo row that should be zero, is an O(8) error and not noise.  "x8": the pos-conv gain times 8 as well"""
    sd = synthetic_state_dict(0, num_layers=1)
    sd["feature_projection.projection.bias"] = sd["feature_projection.projection.bias"] + 8.0
    x8 = dict(sd)
    x8[POS_G_KEYS[0]] = sd[POS_G_KEYS[0]] * 8.0
    return {"base": sd, "x8": x8}


@pytest.fixture(scope="module")
def encoders(sds):
    from sylber_amd import HubertEncoderHIP
    cache = {}

    def get(fmt, which="base"):
        if (fmt, which) not in cache:
            cache[(fmt, which)] = HubertEncoderHIP(sds[which], num_layers=1, precision=PRECISION[fmt])
        return cache[(fmt, which)]
    return get


# ---- conv0 -----------------------------------------------------------------------------------------------------------------------
def check_conv0(enc, sd, wav, lens, fmt, kernel, per_utt, label):
    """one forward to the conv0 tap: every live element inside conv0_bound, rows [L0, R0) bitwise +0, the scale / shift table inside
    conv0_stats_bound.  -> (max err / bound of the output, of the scales, of the shifts)"""
    w0, gw, gb = conv0_weights(sd)
    B, Lmax = wav.shape
    L0 = (Lmax - 10) // 5 + 1
    got = enc.forward(torch.from_numpy(wav).cuda(), lens, stop_stage=_lib.TAP_CONV0).cpu().numpy()
    ss = enc.conv0_scale_shift(B).astype(np.float64)
    assert got.shape == (B, 64 * enc.padded_frames(Lmax), 512) and got.shape[1] >= L0
    rows = [(n - 10) // 5 + 1 for n in lens] if per_utt else None
    ref = fr.conv0_ref(wav, w0, gw, gb, rows)
    r, at = fr.worst_ratio(got[:, :L0], ref["y"], fr.conv0_bound(ref, fmt, kernel))
    da, db = fr.conv0_stats_bound(ref)
    ra = float((np.abs(ss[..., 0] - ref["scale"]) / da).max())
    rb = float((np.abs(ss[..., 1] - ref["shift"]) / db).max())
    print("float64 check conv0 %s %s %s L0 %d B %d max err / bound %.3f at %s scale %.3f shift %.3f" % (fmt, kernel, label, L0, B, r, at, ra, rb))
    assert not got[:, L0:].view(np.uint32).any(), (label, "rows [L0, R0) must be +0")
    return r, ra, rb


def conv0_scale_cases():
    """input scales at L0 = 257 (two 256-row blocks): unit variance is every shape case; here a DC offset of 50, the quiet
    un-normalised clips (the lo halves of the matrix-pipe kernel's operands, then the hi halves too, are subnormal halves), silence and a
    constant (variance 0 in the reference: the output is gelu(beta))"""
    n = 5 * 256 + 10
    base = noise(1, n, 11)
    yield "dc50", base + np.float32(50.0)
    yield "amp1e-3", base * np.float32(1e-3)
    yield "amp1e-5", base * np.float32(1e-5)
    yield "zeros", np.zeros_like(base)
    yield "const", np.full_like(base, 0.5)


@pytest.mark.parametrize("fmt,kernel", CONV0_COMBOS)
def test_conv0_vs_float64(encoders, sds, fmt, kernel):
    """conv0 alone (tap -1) and its scale / shift table, per (format, kernel): the frame counts of CONV0_LMAX, a ragged batch of 3 with
    padded and with per-utterance statistics, and the input scales of conv0_scale_cases.
    Measured max err / bound on MI355X (output; scale; shift):
      kernel            shapes  ragged  per-utt  dc50   1e-3   1e-5   zeros  const   scale  shift
      bf16 matrix pipe  0.994   0.996   0.992    0.933  0.971  0.837  0.765  0.170   0.493  0.472
      fp16 matrix pipe  0.967   0.956   0.956    0.656  0.836  0.450  0.363  0.028   0.493  0.472
      bf16 VALU         0.996   0.997   0.993    0.979  0.982  0.884  0.813  0.465   0.493  0.472
      fp16 VALU         0.974   0.977   0.969    0.859  0.895  0.488  0.464  0.114   0.493  0.472
      split16           0.233   0.803   0.791    0.126  0.176  0.902  0.817  0.056   0.493  0.472
      fp32              0.291   0.229   0.227    0.127  0.191  0.077  0.029  0.056   0.493  0.472
    ("shapes": the worst of the seven lone-clip lengths; bf16 / fp16 sit just below 1 because the store's half-ulp is the bound's
    largest term and some element always rounds by nearly half an ulp; the scale / shift table is the same in every mode.)"""
    enc, sd = encoders(fmt), sds["base"]
    enc.set_option(_lib.OPT_CONV0_VALU, 1 if kernel == "valu" else 0)
    worst = []
    try:
        for lmax in CONV0_LMAX:
            worst.append(check_conv0(enc, sd, noise(1, lmax, lmax), None, fmt, kernel, False, "Lmax%d" % lmax))
        ragged = noise(3, RAGGED_LMAX, 7, RAGGED_LENS)
        worst.append(check_conv0(enc, sd, ragged, list(RAGGED_LENS), fmt, kernel, False, "ragged"))
        enc.set_option(_lib.OPT_PER_UTTERANCE, 1)
        worst.append(check_conv0(enc, sd, ragged, list(RAGGED_LENS), fmt, kernel, True, "ragged_per_utterance"))
        enc.set_option(_lib.OPT_PER_UTTERANCE, 0)
        for label, wav in conv0_scale_cases():
            worst.append(check_conv0(enc, sd, wav, None, fmt, kernel, False, label))
    finally:
        enc.set_option(_lib.OPT_PER_UTTERANCE, 0)
        enc.set_option(_lib.OPT_CONV0_VALU, 0)
    w = np.array(worst).max(0)
    assert (w <= 1.0).all(), w


def test_conv0_constant_clip_is_gelu_of_beta(encoders, sds):
    """a constant clip has variance 0: every live output is gelu(beta_c), whatever the kernel (checked above inside the bound; here
    the reference side of that statement)"""
    w0, gw, gb = conv0_weights(sds["base"])
    ref = fr.conv0_ref(np.full((1, 1290), 0.5, np.float32), w0, gw, gb)
    assert np.abs(ref["var"]).max() < 1e-28 and np.abs(ref["y"] - fr.gelu64(gb.astype(np.float64))[None, None]).max() < 1e-9


# ---- projection ------------------------------------------------------------------------------------------------------------------
def frames_to_samples(t):
    return 320 * t + 80


def check_projection(enc, sd, fmt, T, valid, label):
    lens = [frames_to_samples(t) for t in valid]
    wav = torch.from_numpy(noise(len(valid), frames_to_samples(T), 21 + T, lens)).cuda()
    feats = enc.forward(wav, lens, stop_stage=1).cpu().numpy()
    x = enc.forward(wav, lens, stop_stage=_lib.TAP_PROJ).cpu().numpy()
    assert x.shape == (len(valid), T, 768)
    ref = fr.proj_ref(feats, valid, sd["feature_projection.layer_norm.weight"].numpy(), sd["feature_projection.layer_norm.bias"].numpy(),
                      sd["feature_projection.projection.weight"].numpy(), sd["feature_projection.projection.bias"].numpy(), fmt)
    bound = fr.proj_bound(ref, fmt)
    r, at = fr.worst_ratio(x, ref["x"], bound)
    print("float64 check projection %s %s T %d valid %s max err / bound %.3f at %s (largest bound %.2e, |x| ~ %.1f)"
          % (fmt, label, T, list(valid), r, at, bound.max(), np.abs(ref["x"]).max()))
    for b, nv in enumerate(valid):
        assert not x[b, nv:].view(np.uint32).any(), b
        assert np.abs(x[b, :nv]).min() > 1.0               # (the large bias: no valid frame looks like a zeroed one)
    return r


@pytest.mark.parametrize("fmt", FMTS)
def test_projection_vs_float64(encoders, sds, fmt):
    """tap -2 from the stage-1 tap: LayerNorm(512) -> Linear(512 -> 768) inside proj_bound, frames at or past valid_b bitwise +0; the
    shapes of PROJ_SHAPES, the larger one once more with per-utterance statistics (SYLBER_OPT_PER_UTTERANCE).
    Measured max err / bound on MI355X: bf16 0.117 / 0.145 / 0.145 (T = 9 / T = 257 / T = 257 per-utterance), fp16 0.103 / 0.126 / 0.126,
    split16 0.003 / 0.004 / 0.004, fp32 0.004 / 0.006 / 0.006 (the bound is loose by construction, see proj_bound)."""
    enc, sd = encoders(fmt), sds["base"]
    worst = [check_projection(enc, sd, fmt, T, valid, "padded") for T, valid in PROJ_SHAPES]
    enc.set_option(_lib.OPT_PER_UTTERANCE, 1)
    try:
        worst.append(check_projection(enc, sd, fmt, *PROJ_SHAPES[-1], "per_utterance"))
    finally:
        enc.set_option(_lib.OPT_PER_UTTERANCE, 0)
    assert max(worst) <= 1.0, worst


# ---- pos-conv --------------------------------------------------------------------------------------------------------------------
def check_posconv(enc, sd, fmt, T, valid, label, wr):
    lens = [frames_to_samples(t) for t in valid]
    wav = torch.from_numpy(noise(len(valid), frames_to_samples(T), 100 + T, lens)).cuda()
    x = enc.forward(wav, lens, stop_stage=_lib.TAP_PROJ).cpu().numpy()
    out = enc.forward(wav, lens, stop_stage=_lib.TAP_POSCONV).cpu().numpy()
    assert x.shape == out.shape == (len(valid), T, 768)
    ref = fr.posconv_ref(x, valid, None, sd["encoder.pos_conv_embed.conv.bias"].numpy(), fmt, wr=wr)
    r, at = fr.worst_ratio(out, ref["out"], fr.posconv_bound(ref, fmt))
    zmax = float(np.abs(ref["z"]).max())
    print("float64 check posconv %s %s T %d valid %s max err / bound %.3f at %s max |gelu arg| %.1f" % (fmt, label, T, list(valid), r, at, zmax))
    return r, zmax


@pytest.mark.parametrize("fmt", FMTS)
def test_posconv_vs_float64(encoders, sds, fmt):
    """tap -3 from tap -2, every frame of every utterance (the padded ones too): lone clips of 1 / 64 / 65 frames, a batch of T = 257
    whose zero tails begin inside valid frames' 128-tap windows, a batch of T = 385 whose windows cross the 256-frame workgroup edge;
    the T = 257 batch once more with per-utterance statistics.
    Measured max err / bound on MI355X: bf16 and fp16 0.005 / 0.001 / 0.001 / 0.011 / 0.007 (T = 1 / 64 / 65 / 257 / 385) and 0.011
    per-utterance; split16 0.000 / 0.000 / 0.000 / 0.300 / 0.000 and 0.300; fp32 0.001 / 0.000 / 0.000 / 0.088 / 0.001 and 0.088 (K u sum |x| |w|
    assumes every one of 6144 roundings at its worst; the T = 257 figure of split16 / fp32 is a zero-tail frame, where the residual is 0)."""
    enc, sd = encoders(fmt), sds["base"]
    wr = fr.posconv_weights(hubert_ref.pos_conv_weight(sd).numpy(), fmt)
    worst = [check_posconv(enc, sd, fmt, T, valid, "padded", wr)[0] for T, valid in POSCONV_SHAPES]
    enc.set_option(_lib.OPT_PER_UTTERANCE, 1)
    try:
        worst.append(check_posconv(enc, sd, fmt, *POSCONV_SHAPES[3], "per_utterance", wr)[0])
    finally:
        enc.set_option(_lib.OPT_PER_UTTERANCE, 0)
    assert max(worst) <= 1.0, worst


def test_posconv_outside_the_gelu_core(encoders, sds):
    """the pos-conv gain times 8: the GELU's argument leaves gelu_fast's polynomial core |x| <= 4.2 (asserted on the reference), where
    the kernel freezes Phi.  Measured max err / bound on MI355X: 0.012 (max |GELU argument| 104.7)."""
    enc, sd = encoders("bf16", "x8"), sds["x8"]
    r, zmax = check_posconv(enc, sd, "bf16", 257, POSCONV_SHAPES[3][1], "x8", fr.posconv_weights(hubert_ref.pos_conv_weight(sd).numpy(), "bf16"))
    assert zmax > 4.2
    assert r <= 1.0, r


# ---- stage 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_stage2_is_the_layernorm_of_the_posconv_tap(encoders, sds, fmt):
    """stop_stage = 2 (what the older tests see) equals LayerNorm(768) of tap -3 to the noise of an fp32 LayerNorm: ties the taps to
    the stages.  Measured max err / bound on MI355X: bf16 0.074, fp16 0.073, split16 0.097, fp32 0.076."""
    enc, sd = encoders(fmt), sds["base"]
    valid = (65, 64, 1)
    lens = [frames_to_samples(t) for t in valid]
    wav = torch.from_numpy(noise(3, lens[0], 31, lens)).cuda()
    pre = enc.forward(wav, lens, stop_stage=_lib.TAP_POSCONV).cpu().numpy()
    s2 = enc.forward(wav, lens, stop_stage=2).cpu().numpy()
    ln, bound = fr.layernorm_ref(pre, sd["encoder.layer_norm.weight"].numpy(), sd["encoder.layer_norm.bias"].numpy())
    r, at = fr.worst_ratio(s2, ln, bound)
    print("float64 check stage2 %s max err / bound %.3f at %s" % (fmt, r, at))
    assert r <= 1.0, r


def test_taps_are_refused_where_they_do_not_apply(encoders):
    enc = encoders("bf16")
    wav = torch.from_numpy(noise(1, 400, 1)).cuda()
    with pytest.raises(_lib.SylberHipError):
        enc.forward(wav, None, stop_stage=-4)
    assert enc.forward(wav, None).shape == (1, 1, 768)          # (the refused stage left the handle at stage 0)
    with pytest.raises(_lib.SylberHipError):
        enc.conv0_scale_shift(2)                                 # the last forward had one utterance


def test_taps_in_the_fp8_and_mixed16_precisions(encoders, sds):
    """the front half of fp8 is the bf16 one and mixed16 is the fp16 conv stack in front of the bf16 encoder: their taps return the same
    bits as those handles' (conv0, and for fp8 the projection and the pos-conv too), and mixed16's projection -- fp16 features into
    a bf16 LayerNorm output -- sits inside proj_bound"""
    sd = sds["base"]
    valid = (9, 6, 1)
    lens = [frames_to_samples(t) for t in valid]
    wav = torch.from_numpy(noise(3, lens[0], 41, lens)).cuda()
    for tap in (_lib.TAP_CONV0, _lib.TAP_PROJ, _lib.TAP_POSCONV):
        assert torch.equal(encoders("fp8").forward(wav, lens, stop_stage=tap), encoders("bf16").forward(wav, lens, stop_stage=tap)), tap
    assert torch.equal(encoders("mixed16").forward(wav, lens, stop_stage=_lib.TAP_CONV0), encoders("fp16").forward(wav, lens, stop_stage=_lib.TAP_CONV0))
    r = check_projection(encoders("mixed16"), sd, "bf16", *PROJ_SHAPES[0], "mixed16")
    assert r <= 1.0, r

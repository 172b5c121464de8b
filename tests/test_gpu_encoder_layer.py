"""GPU tier: ONE encoder layer, launch by launch, against the float64 references of tests/encoder_layer_ref.py -- every element of every
tap inside a bound derived from the arithmetic of the kernel behind that launch (no element is left out, the padded frames
t >= valid_b included: they are still queries and still flow through the layer; nothing is averaged).  The kernels are reached through
the layer taps of sylber_set_stop_stage (SYLBER_TAP_LAYER(l, k)), i.e. through the launches every forward runs, and every stage is
referenced from the tap in front of it, so a failure names the launch, the element and the shape.
tests/test_encoder_layer_ref.py shows on the CPU that these bounds reject, at every shape and format used here, a softmax over one key
too many or too few, a masked key contributing, V^T's key permutation left in or applied twice, exchanged heads, q without log2(e), a
residual re-derived from the wrong row's statistics or the wrong affine, LayerNorm statistics over 767 elements, a row from the next
256-row tile, the GELU polynomial outside its core, FFN2 with a 64-chunk of K missing and a repeated last frame."""
import numpy as np
import pytest
import torch

import encoder_layer_ref as el
from sylber_amd import _lib
from sylber_amd.weights import synthetic_state_dict
from encoder_layer_ref import LAYER1_SHAPE, SHAPES, STAGES, TAPS
from frontend_ref import FMTS, noise, worst_ratio

pytestmark = pytest.mark.gpu


def frames_to_samples(t):
    return 320 * t + 80


@pytest.fixture(scope="module")
def sds():
    """two layers; FFN1's weights times FFN1_GAIN, so that its GELU argument leaves gelu_fast's core |z| <= 4.2 at every shape; "qk": layer
    0's q / k weights times QK_GAIN as well (scores of a trained checkpoint's size)"""
    sd = synthetic_state_dict(0, num_layers=2)
    return {"base": el.scaled_state_dict(sd, 2), "qk": el.scaled_state_dict(sd, 2, qk_gain=el.QK_GAIN)}


@pytest.fixture(scope="module")
def encoders(sds):
    from sylber_amd import HubertEncoderHIP
    cache = {}

    def get(fmt, which="base"):
        if (fmt, which) not in cache:
            cache[(fmt, which)] = HubertEncoderHIP(sds[which], num_layers=2, precision=fmt)
        return cache[(fmt, which)]
    return get


@pytest.fixture(scope="module")
def weights(sds):
    cache = {}

    def get(fmt, l, which="base"):
        if (fmt, l, which) not in cache:
            cache[(fmt, l, which)] = el.layer_weights(sds[which], l, fmt)
        return cache[(fmt, l, which)]
    return get


def batch(T, valid, seed=0):
    lens = [frames_to_samples(t) for t in valid]
    return torch.from_numpy(noise(len(valid), frames_to_samples(T), 300 + T + seed, lens)).cuda(), lens


def read_taps(enc, wav, lens, l, stages=STAGES):
    """the actual values around layer l needed to reference ``stages``: one stopped forward each"""
    def fwd(stage):
        return enc.forward(wav, lens, stop_stage=stage).cpu().numpy()
    need = set(stages)
    t = {}
    if need & {"attn_sum"}:
        t["pre_prev"] = fwd(_lib.TAP_POSCONV if l == 0 else _lib.TAP_LAYER(l - 1, _lib.LTAP_FFN2_SUM))
    if "qkv" in need:
        t["hin"] = fwd(2 + l)
    before = {"ctx": "qkv", "attn_sum": "ctx", "ln1": "attn_sum", "ffn1": "ln1", "ffn2_sum": "ffn1", "out": "ffn2_sum"}
    want = need | {before[s] for s in need if s in before} | ({"attn_sum"} if "ffn2_sum" in need else set())
    for k, name in enumerate(TAPS):
        if name in want:
            t[name] = fwd(_lib.TAP_LAYER(l, k))
            assert t[name].shape == (wav.shape[0], enc.num_frames(wav.shape[1]), _lib.LTAP_WIDTH[k]), name
    if "out" in need:
        t["out"] = fwd(3 + l)
    return t


def check_layer(enc, lw, fmt, T, valid, l, label, stages=STAGES, seed=0):
    """-> {stage: max err / bound}, one line per stage: the ratio, where, the largest bound and the reference's typical magnitude"""
    wav, lens = batch(T, valid, seed)
    t = read_taps(enc, wav, lens, l, stages)
    refs = el.stage_refs(t, lw, list(valid), fmt, stages)
    out = {}
    for st in stages:
        ref, bound = refs[st]
        r, at = worst_ratio(t[st], ref, bound)
        print("float64 check layer %d %-8s %s %s T %d valid %s max err / bound %.3f at %s (largest bound %.2e, rms |ref| %.2e)"
              % (l, st, fmt, label, T, list(valid), r, at, bound.max(), np.sqrt((ref ** 2).mean())))
        out[st] = r
    return out, t


SHAPE_IDS = ["T%d" % s[0] for s in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_layer0_taps_vs_float64(encoders, weights, fmt, shape):
    """every tap of layer 0 and its output, each from the tap in front of it, at the lone clips of 1 / 17 / 33 / 64 / 65 frames and the
    batches of T = 257 and T = 385 (encoder_layer_ref.SHAPES).
    Measured max err / bound on MI355X, the worst shape per (format, stage):
               qkv    ctx    attn_sum  ln1    ffn1   ffn2_sum  out
      bf16     0.942  0.610  0.006     0.999  0.919  0.001     0.111
      fp16     0.692  0.539  0.005     0.995  0.590  0.001     0.108
      split16  0.002  0.002  0.002     0.134  0.002  0.001     0.120
      fp32     0.008  0.011  0.008     0.109  0.007  0.003     0.129
    (bf16 / fp16: the store's half-ulp is the largest term of the 16-bit taps' bounds and some element always rounds by nearly half an
    ulp; the K u sum |x| |w| accumulation term assumes every rounding at its worst, hence the small figures of the fp32 sums.)"""
    T, valid = shape
    r, _ = check_layer(encoders(fmt), weights(fmt, 0), fmt, T, valid, 0, "padded")
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("fmt", FMTS)
def test_layer1_taps_vs_float64(encoders, weights, fmt):
    """every tap of layer 1 at the T = 257 batch: its operand is layer 0's output, its first residual is re-derived from layer 0's
    FFN2_SUM with layer 0's final LayerNorm affine (the res_g / res_b hand-off between layers).
    Measured max err / bound on MI355X:
               qkv    ctx    attn_sum  ln1    ffn1   ffn2_sum  out
      bf16     0.937  0.567  0.005     0.999  0.916  0.001     0.104
      fp16     0.716  0.530  0.005     0.995  0.594  0.001     0.115
      split16  0.003  0.002  0.002     0.120  0.002  0.001     0.120
      fp32     0.008  0.012  0.007     0.104  0.007  0.002     0.112"""
    T, valid = LAYER1_SHAPE
    r, _ = check_layer(encoders(fmt), weights(fmt, 1), fmt, T, valid, 1, "padded")
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("qw", (0, 32, 64))
@pytest.mark.parametrize("fmt", ("bf16", "fp16"))
def test_context_of_every_attention_kernel(encoders, weights, fmt, qw):
    """CTX from QKV with SYLBER_OPT_ATTN_QUERIES_PER_WAVE 0 (the hand-scheduled key loop, the default) / 32 / 64 (the compiled kernels), at
    T = 65 and both batches.
    Measured max err / bound on MI355X:
      bf16 0.548 / 0.573 / 0.509 (T = 65 / 257 / 385), fp16 0.491 / 0.523 / 0.459 -- the same figures, at the same elements, for all three
      kernels."""
    enc = encoders(fmt)
    enc.set_option(_lib.OPT_ATTN_QUERIES_PER_WAVE, qw)
    try:
        worst = [check_layer(enc, weights(fmt, 0), fmt, T, valid, 0, "qw%d" % qw, ("ctx",))[0]["ctx"] for T, valid in SHAPES[4:]]
    finally:
        enc.set_option(_lib.OPT_ATTN_QUERIES_PER_WAVE, 0)
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("fmt", ("bf16", "fp16"))
def test_fused_outproj_layernorm_is_bitwise_the_pair(encoders, weights, fmt):
    """ATTN_SUM and LN1 with SYLBER_OPT_FUSE_OUTPROJ_LN forced on, bitwise equal to off, and ATTN_SUM inside its float64 bound.
    gemm_rowln_applicable is FALSE at every shape of encoder_layer_ref.SHAPES (it wants 75 % of 256 workgroup slots filled by 64-row
    tiles: at least 192 x 64 rows), where forcing the option on changes nothing; so this runs the smallest batch of 33-frame clips
    (pitch 64 rows) at which it is true, 192 clips with ragged valid counts.
    Measured max err / bound of the fused ATTN_SUM on MI355X: bf16 0.006, fp16 0.006."""
    enc = encoders(fmt)
    T = 33
    B = -(-192 * 64 // enc.padded_frames(frames_to_samples(T)))
    valid = tuple(T - (b % 5) * 8 for b in range(B))                  # 33, 25, 17, 9, 1, ...
    wav, lens = batch(T, valid)
    taps = (_lib.TAP_LAYER(0, _lib.LTAP_ATTN_SUM), _lib.TAP_LAYER(0, _lib.LTAP_LN1), _lib.TAP_LAYER(0, _lib.LTAP_FFN2_SUM))
    off = [enc.forward(wav, lens, stop_stage=s).clone() for s in taps]
    enc.set_option(_lib.OPT_FUSE_OUTPROJ_LN, 1)
    try:
        r, t = check_layer(enc, weights(fmt, 0), fmt, T, valid, 0, "fused", ("attn_sum",))
        on = [enc.forward(wav, lens, stop_stage=s) for s in taps]
        enc.set_profiling(True)                                       # the fused launch really ran (and not at the small shapes)
        enc.forward(wav, lens, stop_stage=taps[1])
        names = set(enc.get_profile())
        enc.forward(*batch(*SHAPES[5]), stop_stage=taps[1])
        small = set(enc.get_profile())
    finally:
        enc.set_profiling(False)
        enc.set_option(_lib.OPT_FUSE_OUTPROJ_LN, 0)
    assert "gemm_out_ln" in names and "gemm_out" not in names, names
    assert "gemm_out" in small and "gemm_out_ln" not in small, small
    for a, b, s in zip(off, on, taps):
        assert torch.equal(a, b), s
    assert np.array_equal(t["attn_sum"], off[0].cpu().numpy())
    assert r["attn_sum"] <= 1.0, r


def test_scores_of_a_trained_checkpoints_size(encoders, weights):
    """layer 0's q / k weights times QK_GAIN: max |score| exceeds 100 in log2 units (asserted on the float64 reference), the softmax is
    nearly one-hot and the running maximum moves by more than its lazy slack; bf16, the T = 257 batch, QKV and CTX.
    Measured max err / bound on MI355X: qkv 0.940, ctx 0.790 (max |score| 182.3)."""
    T, valid = LAYER1_SHAPE
    r, t = check_layer(encoders("bf16", "qk"), weights("bf16", 0, "qk"), "bf16", T, valid, 0, "qk_gain", ("qkv", "ctx"))
    s = el.ctx_ref(t["qkv"], valid, "bf16")[2]["s"]
    smax = float(np.abs(s[np.isfinite(s)]).max())
    print("float64 check trained scale: max |score| %.1f log2 units" % smax)
    assert smax > 100.0
    assert max(r.values()) <= 1.0, r


def test_layer_taps_are_refused_where_they_do_not_apply(encoders, sds):
    from sylber_amd import HubertEncoderHIP
    enc = encoders("bf16")
    wav, lens = batch(1, (1,))
    for stage in (-4, -5, -6, -7, _lib.TAP_LAYER(0, 6), _lib.TAP_LAYER(0, 7), _lib.TAP_LAYER(2, 0), _lib.TAP_LAYER(15, 5)):
        with pytest.raises(_lib.SylberHipError):
            enc.forward(wav, lens, stop_stage=stage)
    assert enc.forward(wav, lens).shape == (1, 1, 768)                # (a refused stage left the handle at stage 0)
    # (the fp8 precision has layer taps of its own, values + block exponents: tests/test_gpu_fp8_layer.py; the same refusals apply)
    e8 = HubertEncoderHIP(sds["base"], num_layers=2, precision="fp8")
    assert e8.forward(wav, lens, stop_stage=_lib.TAP_LAYER(0, _lib.LTAP_CTX)).shape == (1, 1, 2 * 768)
    for stage in (-4, _lib.TAP_LAYER(0, 6), _lib.TAP_LAYER(2, 0)):
        with pytest.raises(_lib.SylberHipError):
            e8.forward(wav, lens, stop_stage=stage)
    # the packed forward refuses every stop stage
    _lib.check(enc.lib.sylber_set_stop_stage(enc.handle, _lib.TAP_LAYER(0, _lib.LTAP_CTX)), "sylber_set_stop_stage")
    try:
        with pytest.raises(_lib.SylberHipError):
            enc.forward_packed([wav[0]])
    finally:
        enc.lib.sylber_set_stop_stage(enc.handle, 0)


@pytest.mark.parametrize("fmt", FMTS)
def test_taps_leave_the_full_forward_unchanged(encoders, fmt):
    """a forward after a round of taps returns the bits of a forward before it (a tap stops a forward early and copies; it leaves nothing
    behind), and stage 3 + l of the last layer is the full forward"""
    enc = encoders(fmt)
    wav, lens = batch(65, (65, 64, 1))
    before = enc.forward(wav, lens).clone()
    for k in range(6):
        enc.forward(wav, lens, stop_stage=_lib.TAP_LAYER(1, k))
    assert torch.equal(enc.forward(wav, lens), before)
    assert torch.equal(enc.forward(wav, lens, stop_stage=4), before)

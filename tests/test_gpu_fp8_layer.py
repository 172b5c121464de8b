"""GPU tier: ONE encoder layer of the fp8 precision, launch by launch, against the float64 references of tests/fp8_layer_ref.py -- every
element of every tap inside a bound derived from the arithmetic of the kernel behind that launch, and every stored E8M0 scale byte
inside the set its block maximum admits (no element and no block is left out, the padded frames t >= valid_b included).  The kernels
are reached through the layer taps of sylber_set_stop_stage on a SYLBER_FP8 handle, i.e. through the launches every fp8 forward runs;
an MXFP8 buffer comes back dequantised exactly, with each element's block exponent next to it, and every stage is referenced from the
tap in front of it, so a failure names the launch, the element (or the block) and the shape.
tests/test_fp8_layer_ref.py shows on the CPU that these bounds reject, at the shapes used here, a scale from half a block, a scale byte
off by one, truncation in e4m3, a block maximum taken before the bias or the GELU, V scaled per 32 features or key-permuted, q without
0.125, log2(e) missing, a masked key, a missing key, exchanged heads, the wrong residual affine, a missing K chunk and a row from the
next 256-row tile -- and that P without its 2^7 bias is only seen on the designed op-level inputs, which run here too."""
import ctypes

import numpy as np
import pytest
import torch

import encoder_layer_ref as el
import fp8_layer_ref as f8
from sylber_amd import _lib
from sylber_amd.weights import synthetic_state_dict
from encoder_layer_ref import LAYER1_SHAPE, SHAPES, STAGES, TAPS
from fp8_layer_ref import OP_SHAPES, QUANT_STAGES
from frontend_ref import noise, worst_ratio

pytestmark = pytest.mark.gpu


def frames_to_samples(t):
    return 320 * t + 80


@pytest.fixture(scope="module")
def sds():
    sd = synthetic_state_dict(0, num_layers=2)
    return {"base": el.scaled_state_dict(sd, 2), "qk": el.scaled_state_dict(sd, 2, qk_gain=el.QK_GAIN)}


@pytest.fixture(scope="module")
def encoders(sds):
    from sylber_amd import HubertEncoderHIP
    cache = {}

    def get(which="base"):
        if which not in cache:
            cache[which] = HubertEncoderHIP(sds[which], num_layers=2, precision="fp8")
        return cache[which]
    return get


@pytest.fixture(scope="module")
def weights(sds):
    cache = {}

    def get(l, which="base"):
        if (l, which) not in cache:
            cache[(l, which)] = f8.layer_weights(sds[which], l)
        return cache[(l, which)]
    return get


def batch(T, valid, seed=0):
    lens = [frames_to_samples(t) for t in valid]
    return torch.from_numpy(noise(len(valid), frames_to_samples(T), 300 + T + seed, lens)).cuda(), lens


def quantised(st, attn8):
    return st in QUANT_STAGES and (attn8 or st != "qkv")


def read_taps(enc, wav, lens, l, stages=STAGES, attn8=True):
    """the actual values (t) and block exponents (x) around layer l needed to reference ``stages``: one stopped forward each"""
    def fwd(stage):
        return enc.forward(wav, lens, stop_stage=stage).cpu().numpy()
    need = set(stages)
    t, x = {}, {}
    if need & {"attn_sum"}:
        t["pre_prev"] = fwd(_lib.TAP_POSCONV if l == 0 else _lib.TAP_LAYER(l - 1, _lib.LTAP_FFN2_SUM))
    if "qkv" in need:
        t["hin"] = fwd(2 + l)
    before = {"ctx": "qkv", "attn_sum": "ctx", "ln1": "attn_sum", "ffn1": "ln1", "ffn2_sum": "ffn1", "out": "ffn2_sum"}
    want = need | {before[s] for s in need if s in before} | ({"attn_sum"} if "ffn2_sum" in need else set())
    for k, name in enumerate(TAPS):
        if name in want:
            y = fwd(_lib.TAP_LAYER(l, k))
            W = _lib.LTAP_WIDTH[k]
            assert y.shape == (wav.shape[0], enc.num_frames(wav.shape[1]), 2 * W if quantised(name, attn8) else W), name
            t[name], x[name] = f8.split_tap(y) if quantised(name, attn8) else (y, None)
    if "out" in need:
        t["out"] = fwd(3 + l)
    return t, x


def check_layer(enc, lw, T, valid, l, label, stages=STAGES, attn8=True, seed=0):
    """-> ({stage: max err / bound}, {stage: scale report}, t), one line per stage: the ratio, where, and for a quantised stage the
    blocks whose scale byte is outside its admissible set / not constant / the blocks that admit two bytes / all blocks"""
    wav, lens = batch(T, valid, seed)
    t, x = read_taps(enc, wav, lens, l, stages, attn8)
    refs = f8.stage_refs(t, lw, list(valid), stages, attn8)
    out, reps = {}, {}
    for st in stages:
        r, at, rep = f8.check_stage(st, t[st], x.get(st), *refs[st], attn8=attn8)
        print("float64 check layer %d %-8s fp8 %s T %d valid %s max err / bound %.3f at %s%s"
              % (l, st, label, T, list(valid), r, at, "" if rep is None else
                 "; scale bytes: %d outside their set, %d ragged, %d ambiguous of %d blocks%s"
                 % (rep["bad_scale"], rep["ragged"], rep["ambiguous"], rep["blocks"],
                    "" if rep["first_bad"] is None else " (first at %s)" % (rep["first_bad"],))))
        out[st], reps[st] = r, rep
    return out, reps, t


def assert_inside(r, reps):
    assert max(r.values()) <= 1.0, r
    for st, rep in reps.items():
        assert rep is None or (rep["bad_scale"] == 0 and rep["ragged"] == 0), (st, rep)


SHAPE_IDS = ["T%d" % s[0] for s in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fp8_layer0_taps_vs_float64(encoders, weights, shape):
    """every tap of layer 0 and its output, each from the tap in front of it, at the lone clips of 1 / 17 / 33 / 64 / 65 frames and the
    batches of T = 257 and T = 385 (encoder_layer_ref.SHAPES); every scale byte of q, k, v, the context, LayerNorm 1's output and
    FFN1's output inside its admissible set.
    Measured max err / bound on MI355X; no scale byte outside its set and no ragged block at any shape:
               qkv    ctx    attn_sum  ln1    ffn1   ffn2_sum  out
      T 1      0.947  0.000  0.008     0.999  0.941  0.010     0.039
      T 17     0.953  0.565  0.013     1.000  0.955  0.013     0.077
      T 33     0.954  0.565  0.011     1.000  0.956  0.013     0.086
      T 64     0.955  0.520  0.017     1.000  0.955  0.014     0.096
      T 65     0.955  0.527  0.019     1.000  0.960  0.013     0.073
      T 257    0.957  0.572  0.022     1.000  0.962  0.018     0.111
      T 385    0.969  0.482  0.019     1.000  0.961  0.018     0.112
    (qkv / ln1 / ffn1: the e4m3 half-ulp is the largest term of the bound and some element always rounds by nearly half an ulp -- ln1,
    whose fp32 bound is a few u, sits at exactly that; ctx over one key is v itself, requantised on the grid it came from: 0.000; the
    MX_MFMA x sum |x| |w| term assumes every 64-term sum at its worst, hence the small figures of the fp32 sums.)
    Blocks admitting two scale bytes: qkv 0.0 - 1.1 %, ln1 0.0 %, ffn1 0.9 - 4.2 %, ctx 12.5 - 22.5 % (tests/test_fp8_layer_ref.py
    ::test_ambiguous_scale_share_is_under_its_cap on why the context's share is what it is)."""
    T, valid = shape
    r, reps, _ = check_layer(encoders(), weights(0), T, valid, 0, "padded")
    assert_inside(r, reps)


def test_fp8_layer1_taps_vs_float64(encoders, weights):
    """every tap of layer 1 at the T = 257 batch: its operand is layer 0's output requantised, its first residual is re-derived from layer
    0's FFN2_SUM with layer 0's final LayerNorm affine (the res_g / res_b hand-off between layers).
    Measured max err / bound on MI355X (no scale byte outside its set):
               qkv    ctx    attn_sum  ln1    ffn1   ffn2_sum  out
      T 257    0.975  0.569  0.015     1.000  0.962  0.016     0.106"""
    T, valid = LAYER1_SHAPE
    r, reps, _ = check_layer(encoders(), weights(1), T, valid, 1, "padded")
    assert_inside(r, reps)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fp8_layer_with_the_bf16_attention_core(encoders, weights, shape):
    """QKV and CTX with SYLBER_OPT_FP8_ATTENTION = -1: the MXFP8 GEMM with the 16-bit EPI_QK epilogue (a plain bf16 tap of width 2304) and
    the bf16 core behind launch_attention_f8out, whose context leaves through the same quantising attn_finalize.
    Measured max err / bound on MI355X (qkv / ctx; no scale byte of the context outside its set, 0 - 2.7 % of its blocks admit two):
      T 1 0.551 / 0.885, T 17 0.632 / 0.889, T 33 0.632 / 0.884, T 64 0.661 / 0.888, T 65 0.686 / 0.888, T 257 0.716 / 0.891,
      T 385 0.712 / 0.886"""
    T, valid = shape
    enc = encoders()
    enc.set_option(_lib.OPT_FP8_ATTENTION, -1)
    try:
        r, reps, _ = check_layer(enc, weights(0), T, valid, 0, "attn16", ("qkv", "ctx"), attn8=False)
    finally:
        enc.set_option(_lib.OPT_FP8_ATTENTION, 0)
    assert_inside(r, reps)


def test_fp8_scores_of_a_trained_checkpoints_size(encoders, weights):
    """layer 0's q / k weights times QK_GAIN: max |score| exceeds 100 in log2 units (asserted on the float64 reference), the softmax is
    nearly one-hot and the running maximum moves by far more than its 2^1 slack; the T = 257 batch, QKV and CTX.
    Measured max err / bound on MI355X: qkv 0.969, ctx 0.489 (max |score| 186.0; no scale byte outside its set)."""
    T, valid = LAYER1_SHAPE
    r, reps, t = check_layer(encoders("qk"), weights(0, "qk"), T, valid, 0, "qk_gain", ("qkv", "ctx"))
    s = f8.ctx8_ref(t["qkv"], valid)[2]["s"]
    smax = float(np.abs(s[np.isfinite(s)]).max())
    print("float64 check trained scale: max |score| %.1f log2 units" % smax)
    assert smax > 100.0
    assert_inside(r, reps)


@pytest.mark.parametrize("shape", (SHAPES[1], SHAPES[0]), ids=("T17", "T1"))
def test_fp8_taps_do_not_read_stale_workspace(encoders, shape):
    """T = 17 (Tp = 32, Tpv = 64: V^T's key tail [Tp, Tpv) exists) and T = 1: every tap of layer 1 -- behind a whole layer 0 -- after the
    workspace was filled with 0xFF and with 0x7F (NaN patterns in e4m3, fp16 and fp32; 0xFF is also the E8M0 NaN) returns the bits of
    the unpoisoned run"""
    T, valid = shape
    enc = encoders()
    wav, lens = batch(T, valid)
    stages = [_lib.TAP_LAYER(1, k) for k in range(6)] + [4]
    clean = [enc.forward(wav, lens, stop_stage=s).clone() for s in stages]
    for byte in (0xFF, 0x7F):
        for s, want in zip(stages, clean):
            _lib.check(enc.lib.sylber_debug_poison_workspace(enc.handle, byte), "poison")
            got = enc.forward(wav, lens, stop_stage=s)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (hex(byte), s)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("shape", OP_SHAPES, ids=["T%d" % s[0] for s in OP_SHAPES])
def test_fp8_attention_op_vs_float64_on_designed_inputs(shape):
    """sylber_op_attention, precision fp8 (attention_f8_kernel with the bf16 store), per element against the float64 reference on the SAME
    quantised operands, on fp8_layer_ref.op_inputs: every masked key is aligned with its queries and carries |v| = 1e3 (the bound is
    built from the valid keys only), the last valid key carries a large weight and a distinctive v, and the last utterance's other
    keys carry equal weights near 2^-12 of the largest that only survive with P's 2^7 bias.  tests/test_fp8_layer_ref.py shows that a
    leak, a dropped key, log2(e) missing and P without its bias all leave this bound on these inputs.  Adds to
    tests/test_gpu_fp8.py::test_fp8_attention_core_op, replaces nothing.
    Measured max err / bound on MI355X: T = 33 0.683, T = 65 0.765 (the CPU emulation of a correct core: 0.683 / 0.760)."""
    T, valid = shape
    lib = _lib.load()
    q, k, v = f8.op_inputs(T, valid)
    B = len(valid)
    qd, kd, vd = (torch.from_numpy(a).cuda() for a in (q, k, v))
    nv = torch.tensor(valid, dtype=torch.int32).cuda()
    o = torch.full((B, T, 768), float("nan"), device="cuda")
    _lib.check(lib.sylber_op_attention(_p(qd), _p(kd), _p(vd), _p(nv), _p(o), B, T, 2, 0, None), "op_attention fp8")
    ref, bound, _ = f8.op_ctx_ref(f8.op_operands(q, k, v, valid), valid)
    r, at = worst_ratio(o.cpu().numpy(), ref, bound)
    print("float64 check op attention fp8 T %d valid %s max err / bound %.3f at %s (largest bound %.2e)" % (T, list(valid), r, at, bound.max()))
    assert r <= 1.0, (r, at)


def test_fp8_taps_leave_the_full_forward_unchanged(encoders):
    """a forward after a round of taps returns the bits of a forward before it, with either attention core, and stage 3 + l of the last
    layer is the full forward"""
    enc = encoders()
    wav, lens = batch(65, (65, 64, 1))
    before = enc.forward(wav, lens).clone()
    for opt in (0, -1):
        enc.set_option(_lib.OPT_FP8_ATTENTION, opt)
        try:
            for k in range(6):
                enc.forward(wav, lens, stop_stage=_lib.TAP_LAYER(1, k))
        finally:
            enc.set_option(_lib.OPT_FP8_ATTENTION, 0)
        assert torch.equal(enc.forward(wav, lens), before)
    assert torch.equal(enc.forward(wav, lens, stop_stage=4), before)

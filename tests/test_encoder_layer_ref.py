"""CPU tier: the float64 references of tests/encoder_layer_ref.py, chained over the taps of one encoder layer, are pinned to the oracle,
and their per-element bounds are shown to be SHARP at every (shape, format) pair tests/test_gpu_encoder_layer.py runs on the GPU: the
chain a correct kernel sequence would leave in the taps (the references with the format's operand, store and P roundings emulated in
numpy) stays inside every bound with no element excluded, and every planted defect -- a softmax over one key too many or too few, a
masked key contributing, V^T's key permutation left in (seen at the q / k / v tap) or applied twice (seen at the context), two heads
exchanged in a third of q | k | v, q scaled by 1/8 without log2(e), the residual re-derived with the neighbouring row's (mean, rstd)
or with the wrong LayerNorm's affine, LayerNorm statistics over 767 elements, a row from the next 256-row tile, the GELU of the wrong
kind outside |z| <= 4.2, FFN2 with its last 64-chunk of K missing, the last frame repeated from the one before -- leaves at least one
bound.  Nothing here needs a GPU, and nothing on the GPU has to misbehave for the bounds to be trusted."""
import numpy as np
import pytest
import torch

import encoder_layer_ref as el
import frontend_ref as fr
from oracle import hubert_ref
from sylber_amd.weights import synthetic_state_dict

from encoder_layer_ref import HIDDEN, LAYER1_SHAPE, SHAPES, STAGES
from frontend_ref import FMTS, noise, round_fmt, worst_ratio


@pytest.fixture(scope="module")
def sd():
    return el.scaled_state_dict(synthetic_state_dict(0, num_layers=2), 2)


def test_references_chained_agree_with_the_oracle(sd):
    """two layers of references, each stage fed the float64 reference of the stage before it (fp32 mode: no operand rounding), against
    oracle/hubert_ref.forward(collect=True) (fp32 torch) on a ragged batch, to the oracle's own fp32 noise"""
    lens = (4000, 3370, 1000)
    wav = noise(3, 4000, 5, lens)
    o = hubert_ref.forward(sd, torch.from_numpy(wav), lens, num_layers=2, collect=True)
    valid = [hubert_ref.num_frames(n) for n in lens]
    pr = fr.proj_ref(o["conv6"].numpy().transpose(0, 2, 1), valid, sd["feature_projection.layer_norm.weight"].numpy(),
                     sd["feature_projection.layer_norm.bias"].numpy(), sd["feature_projection.projection.weight"].numpy(),
                     sd["feature_projection.projection.bias"].numpy(), "fp32")
    pre = fr.posconv_ref(pr["x"], valid, hubert_ref.pos_conv_weight(sd).numpy(), sd["encoder.pos_conv_embed.conv.bias"].numpy(), "fp32")["out"]
    for l in range(2):
        lw = el.layer_weights(sd, l, "fp32")
        t = {"pre_prev": pre, "hin": fr.layernorm_ref(pre, lw["prev_g"], lw["prev_b"])[0]}
        for st in STAGES:                       # (float64 throughout: each stage from the reference of the one before)
            t[st] = el.stage_refs(t, lw, valid, "fp32", (st,))[st][0]
        got = o["layer%d" % l].numpy()
        assert np.abs(t["out"] - got).max() < 2e-4 * max(1.0, np.abs(got).max()), l
        pre = t["ffn2_sum"]


def attention_defects(t, refs, valid, fmt):
    """-> [(name, stage, slice of utterances, mutated output)]: the defects of the q / k / v projection and the attention that exist at
    this shape (key range, mask, V^T permutation, heads, score scale)"""
    T = t["qkv"].shape[1]
    bad = []
    q = t["qkv"]
    for b, nv in enumerate(valid):
        sl = slice(b, b + 1)
        if nv < T:
            bad.append(("softmax over one key too many (b %d)" % b, "ctx", sl, el.ctx_ref(q[sl], [nv + 1], fmt)[0]))
        if nv >= 2:
            bad.append(("softmax over one key too few (b %d)" % b, "ctx", sl, el.ctx_ref(q[sl], [nv - 1], fmt)[0]))
        if nv < T - 1:
            m = el.key_mask([nv], T)
            m[0, T - 1] = True
            bad.append(("a masked key contributing (b %d)" % b, "ctx", sl, el.ctx_ref(q[sl], [nv], fmt, mask=m)[0]))
    perm = el.vt_key_permutation(T)
    if T > 4:                                    # (the swap of key bits 2 and 3 moves nothing among fewer than 5 keys)
        assert (perm < T).all()
        sl = slice(0, 1)
        bad.append(("V^T key permutation applied twice", "ctx", sl, el.ctx_ref(q[sl], valid[:1], fmt, v_perm=perm)[0]))
        y = refs["qkv"][0].copy()
        y[:, :, 2 * HIDDEN:] = y[:, perm, 2 * HIDDEN:]
        bad.append(("V^T key permutation left in", "qkv", slice(None), y))
    for third in range(3):
        y = refs["qkv"][0].copy()
        c = third * HIDDEN
        y[..., c:c + 64], y[..., c + 64:c + 128] = refs["qkv"][0][..., c + 64:c + 128], refs["qkv"][0][..., c:c + 64]
        bad.append(("heads 0 and 1 exchanged in third %d" % third, "qkv", slice(None), y))
    if fmt == "fp32":                            # (the fp32 mode scales inside its attention kernel; over one key the softmax is 1 at any scale)
        if T > 1:
                bad.append(("q scaled by 1/8 without log2(e)", "ctx", slice(0, 1), el.ctx_ref(q[:1], valid[:1], fmt, score_gain=1 / el.LOG2E)[0]))
    else:
        y = refs["qkv"][0].copy()
        y[..., :HIDDEN] *= 0.125 / el.Q_SCALE
        bad.append(("q scaled by 1/8 without log2(e)", "qkv", slice(None), y))
    return bad


def planted_defects(t, refs, lw, valid, fmt):
    """-> attention_defects and those of the residual GEMMs, the LayerNorms, the FFN and the row order"""
    T = t["qkv"].shape[1]
    bad = attention_defects(t, refs, valid, fmt)
    # ---- the residual re-derived in the GEMM epilogue
    ln_prev = fr.layernorm_ref(t["pre_prev"], lw["prev_g"], lw["prev_b"])[0]
    if T > 1:                                    # (a lone frame has no neighbouring row in the tap)
        bad.append(("residual with the neighbouring row's (mean, rstd)", "attn_sum", slice(None),
                    refs["attn_sum"][0] - ln_prev + el.layernorm_rows(t["pre_prev"], lw["prev_g"], lw["prev_b"], shift=1)))
        ln1 = fr.layernorm_ref(t["attn_sum"], lw["ln1_g"], lw["ln1_b"])[0]
        bad.append(("FFN2's residual with the neighbouring row's (mean, rstd)", "ffn2_sum", slice(None),
                    refs["ffn2_sum"][0] - ln1 + el.layernorm_rows(t["attn_sum"], lw["ln1_g"], lw["ln1_b"], shift=1)))
    bad.append(("residual with this layer's final LayerNorm affine", "attn_sum", slice(None),
                refs["attn_sum"][0] - ln_prev + el.layernorm_rows(t["pre_prev"], lw["ln2_g"], lw["ln2_b"])))
    # ---- LayerNorm statistics over 767 elements
    bad.append(("LayerNorm 1 over 767 elements", "ln1", slice(None), round_fmt(el.layernorm_rows(t["attn_sum"], lw["ln1_g"], lw["ln1_b"], n=767), fmt)))
    bad.append(("LayerNorm 2 over 767 elements", "out", slice(None), el.layernorm_rows(t["ffn2_sum"], lw["ln2_g"], lw["ln2_b"], n=767)))
    # ---- FFN
    z = el.ffn1_ref(t["ln1"], lw, fmt)[2]
    assert np.abs(z).max() > 4.2, "FFN1's argument must leave gelu_fast's core at this shape"
    # the wrong kind: gelu_fast's polynomial continued past its core without the clamp (in the erf modes too: the CLAMPED gelu_fast in
    # place of erf is off by at most 2.7e-5 |z|, which is below the K u sum |h| |w| accumulation term of the split16 / fp32 bounds -- a
    # term no order-free argument can shrink -- so that swap cannot be told from a correct kernel by any per-element bound of this kind)
    wrong = el.gelu_fast64(z, clamp=False)
    bad.append(("FFN1's GELU of the wrong kind beyond |z| = 4.2", "ffn1", slice(None), round_fmt(np.where(np.abs(z) > 4.2, wrong, el.gelu64(z)), fmt)))
    bad.append(("FFN2 without its last 64-chunk of K", "ffn2_sum", slice(None),
                refs["ffn2_sum"][0] - t["ffn1"][..., -64:] @ lw["W2"][:, -64:].T))
    # ---- rows
    for st in STAGES:
        if T > 256:
            y = t[st].copy()
            y[0, 255] = t[st][0, 256]
            bad.append(("row 255 from the next 256-row tile", st, slice(None), y))
        if T > 1:
            y = t[st].copy()
            y[:, T - 1] = t[st][:, T - 2]
            bad.append(("frame T - 1 repeated from T - 2", st, slice(None), y))
    return bad


def check_shape(sd, fmt, T, valid, l, pre, defects=True):
    lw = el.layer_weights(sd, l, fmt)
    valid = list(valid)
    t = el.emulate_layer(pre, lw, valid, fmt)
    refs = el.stage_refs(t, lw, valid, fmt)
    for st in STAGES:
        r, at = worst_ratio(t[st], *refs[st])
        assert r <= 1.0, (fmt, T, l, st, "the emulated kernel", r, at)
    if defects:
        for name, st, sl, y in planted_defects(t, refs, lw, valid, fmt):
            r, _ = worst_ratio(y, refs[st][0][sl], refs[st][1][sl])
            assert r > 1.0, (fmt, T, l, st, name, r)
    return t


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d" % s[0])
@pytest.mark.parametrize("fmt", FMTS)
def test_layer_bounds_reject_planted_defects(sd, fmt, shape):
    T, valid = shape
    t = check_shape(sd, fmt, T, valid, 0, el.pre_input(T, valid, T))
    if shape == LAYER1_SHAPE:                  # the hand-off between layers: layer 1 from layer 0's FFN2_SUM, its residual from layer 0's ln2
        check_shape(sd, fmt, T, valid, 1, t["ffn2_sum"])


def test_trained_scale_scores(sd):
    """the case at a trained checkpoint's scale: with layer 0's q / k weights times QK_GAIN the reference's scores exceed 100 in log2
    units, and the bf16 bounds still hold for the emulated kernel and still reject the attention defects"""
    T, valid = LAYER1_SHAPE
    big = el.scaled_state_dict(synthetic_state_dict(0, num_layers=2), 2, qk_gain=el.QK_GAIN)
    lw = el.layer_weights(big, 0, "bf16")
    t = el.emulate_layer(el.pre_input(T, valid, T), lw, list(valid), "bf16")
    s = el.ctx_ref(t["qkv"], valid, "bf16")[2]["s"]
    assert np.abs(s[np.isfinite(s)]).max() > 100.0
    refs = el.stage_refs(t, lw, list(valid), "bf16", ("qkv", "ctx"))
    for st in ("qkv", "ctx"):
        assert worst_ratio(t[st], *refs[st])[0] <= 1.0, st
    for name, st, sl, y in attention_defects(t, refs, list(valid), "bf16"):
        assert worst_ratio(y, refs[st][0][sl], refs[st][1][sl])[0] > 1.0, name

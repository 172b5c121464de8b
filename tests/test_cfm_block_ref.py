"""CPU tier: the float64 stage references of tests/cfm_block_ref.py, chained, are pinned to the decoder's restatement (tests/cfm_ref.py in
float64), and their per-element bounds are shown to be SHARP at every (shape, format) pair tests/test_gpu_cfm_block.py runs on the GPU:
the chain a correct kernel sequence would leave in the taps (the references with each buffer's store emulated in numpy, the P rounding
inside the attention included) stays inside every bound with no element excluded, and every planted defect leaves at least one bound:
the conv window shifted by one, its zero padding taken at T instead of Tb, registers exchanged; the gamma / beta of the block's other
norm or of another time, the RMS over 511 elements; the rotary position off by one, the registers at position 0, pairs (i, i + 1), the
sign of sin flipped, q without its 10 or without log2(e), the next head's q-norm gamma; V^T's key-bit swap left out or applied twice, one
key too many or too few, a masked key contributing, heads exchanged; the residual added twice or not at all; value and gate halves
swapped, GELU on the value, a nonzero column >= 1365, a 64-chunk of FF2's K missing, b1 / b2 of the next block; the final norm's gamma
missing, two to_pred rows exchanged.  Nothing here needs a GPU, and nothing on the GPU has to misbehave for the bounds to be trusted.

Defects that exist only at some shapes are asserted at those: the padding at T needs a frames= row shorter than T.  One key too many and a
masked key contributing need a LIVE row behind the clip's keys: a frames= row shorter than T, or a packed slot that 16 + Tb does not fill
(cfm_qkprep writes every row of a slot).  In a plain padded call the rows behind the keys are never written: such a key has k = v = 0 and
only adds 2^-m (m the row's largest score, tens of log2 units) to the row sum, which no format's bound can see at every row -- measured
here: bf16 0.17 .. 0.55 of the bound, fp16 up to 0.81 -- so the two defects are asserted on the frames= and packed geometries alone.
With every q / k gamma equal (the trained-scale case) the next head's gamma is the same gamma: not planted there."""
import numpy as np
import pytest
import torch

import cfm_block_ref as cb
import cfm_ref
import encoder_layer_ref as el
from cfm_block_ref import D, FIP, Geom, LONE_T, RAGGED, block_stages
from frontend_ref import round_fmt, worst_ratio
from sylber_amd.weights import synthetic_regressor_state_dict

FMTS = ("fp32", "bf16", "fp16")
T_EVAL = 0.37


@pytest.fixture(scope="module")
def sd():
    return synthetic_regressor_state_dict(0)


_W = {}


def weights(sd, fmt, gamma=None):
    if (fmt, gamma) not in _W:
        _W[(fmt, gamma)] = cb.pack_weights(sd if gamma is None else cb.with_qk_gamma(sd, gamma), fmt)
    return _W[(fmt, gamma)]


def test_references_chained_agree_with_the_restatement(sd):
    """all eight blocks of references in float64 (fp32 mode: no operand rounding), each stage fed the reference of the stage before it,
    against cfm_ref.evaluate in float64 on a 49-frame clip: the packing (the fold, W1's halves, the 12-head layout, V^T's permutation
    and back) and every stage agree with the published forward to float64 noise"""
    T = 49
    cond, y = cb.clip(T)
    W = weights(sd, "fp32")
    g = Geom([T])
    c = g.clips[0]
    gb = cb.gb_ref(W, T_EVAL, fp32_arg=False)[0]
    t = {"cond": cond.double().numpy(), "y": y.double().numpy(), "gb": gb}
    for st in cb.FRONT:
        t[st] = cb.stage_refs(t, W, c, 0, "fp32", (st,))[st][0]
    t["x_in"] = t["x0"]
    for li in range(cb.DEPTH):
        for st in block_stages("fp32"):
            t[st] = cb.stage_refs(t, W, c, li, "fp32", (st,))[st][0]
        t["x_in"] = t["x_ff"]
    out = cb.final_ref(t["x_ff"], W, c)[0]
    with torch.no_grad():
        ref = cfm_ref.evaluate(cfm_ref.to_f64(sd), y[None].double(), T_EVAL, cond[None].double())[0].numpy()
    # (the restatement keeps the rotary angles in fp32, as the references do; the time embedding's argument is float64 on both sides here)
    assert np.abs(out - ref).max() < 1e-9 * np.abs(ref).max()


# ---- planted defects -----------------------------------------------------------------------------------------------------------------------
def attention_defects(t, W, c, li, fmt):
    R, nv = c["R"], c["nv"]
    bad = []
    if nv < c["Lq"]:                             # (module docstring: a live row behind the keys)
        bad.append(("one key too many", "ctx", cb.ctx_ref(t, fmt, c, nv=nv + 1)[0]))
    bad.append(("one key too few", "ctx", cb.ctx_ref(t, fmt, c, nv=nv - 1)[0]))
    if nv < c["Lq"] - 1:
        m = el.key_mask([nv], R)
        m[0, c["Lq"] - 1] = True
        bad.append(("a masked key contributing", "ctx", cb.ctx_ref(t, fmt, c, mask=m)[0]))
    bad.append(("heads 0 and 1 exchanged", "ctx", cb.ctx_ref(t, fmt, c, swap_heads=True)[0]))
    if fmt != "fp32":
        bad.append(("V^T key-bit swap applied twice", "ctx", cb.ctx_ref(t, fmt, c, v_perm=el.vt_key_permutation(R))[0]))
        bad.append(("V^T key-bit swap left out", "vt", round_fmt(cb.qk_ref(t["qkv"], W, li, fmt, c, vt_perm="none")["vt"][0], fmt)))
    return bad


def rotary_defects(t, W, c, li, fmt, heads=True):
    names = ("qkvf",) if fmt == "fp32" else ("q", "k")
    full = 80.0 if fmt == "fp32" else cb.C10
    muts = [("rotary position off by one", dict(pos_shift=1)), ("registers at position 0", dict(reg_pos=0.0)),
            ("pairs (i, i + 1)", dict(adjacent=True)), ("sign of sin flipped", dict(sin_sign=-1.0))]
    if heads:
        muts.append(("q-norm gamma of the next head", dict(head_shift=1)))
    bad = []
    for name, kw in muts:
        r = cb.qk_ref(t["qkv"], W, li, fmt, c, **kw)
        for st in names:
            bad.append(("%s (%s)" % (name, st), st, round_fmt(r[st][0], fmt)))
    for name, qs in (("q without its 10", full / 10.0), ("q without log2(e)", full / el.LOG2E)):
        if fmt == "fp32" and "log2" in name:
            continue                              # (the fp32 attention applies log2(e) itself: its q carries 80 alone)
        st = names[0]
        bad.append((name, st, round_fmt(cb.qk_ref(t["qkv"], W, li, fmt, c, qscale=qs)[st][0], fmt)))
    return bad


def planted_defects(t, refs, W, c, li, fmt, gb_other, front=True, final=False, upto_qk=False):
    """upto_qk: the defects of the front, the first norm, the rotary and V^T's layout alone (the long clip stops behind cfm_qkprep)"""
    gb = t["gb"]
    nx = (li + 1) % cb.DEPTH
    bad = []
    if front:
        bad.append(("conv window shifted by one", "x0", cb.x0_ref(t["xe"], W, c, shift=1)[0]))
        if c["Tb"] < c["Trow"]:
            bad.append(("conv zero padding at T instead of Tb", "x0", cb.x0_ref(t["xe"], W, c, pad_at=c["Trow"])[0]))
        bad.append(("registers 0 and 1 exchanged", "x0", cb.x0_ref(t["xe"], W, c, swap_reg=True)[0]))
    for st, src, n in (("h_attn", "x_in", 2 * li), ("h_ff", "x_attn", 2 * li + 1))[:1 if upto_qk else 2]:
        bad.append(("gamma / beta of the block's other norm", st, round_fmt(cb.norm_ref(t[src], gb[n ^ 1, 0], gb[n ^ 1, 1], fmt)[0], fmt)))
        bad.append(("gamma / beta of another time", st, round_fmt(cb.norm_ref(t[src], gb_other[n, 0], gb_other[n, 1], fmt)[0], fmt)))
        bad.append(("RMS over 511 elements", st, round_fmt(cb.norm_ref(t[src], gb[n, 0], gb[n, 1], fmt, count=511)[0], fmt)))
    bad += rotary_defects(t, W, c, li, fmt)
    if upto_qk:
        if fmt != "fp32":
            bad.append(("V^T key-bit swap left out", "vt", round_fmt(cb.qk_ref(t["qkv"], W, li, fmt, c, vt_perm="none")["vt"][0], fmt)))
        return bad
    bad += attention_defects(t, W, c, li, fmt)
    bad.append(("attention residual added twice", "x_attn", cb.res_ref(t["ctx"], W["wo"][li], None, t["x_in"], fmt, gain=2.0)[0]))
    bad.append(("attention residual not added", "x_attn", cb.res_ref(t["ctx"], W["wo"][li], None, t["x_in"], fmt, gain=0.0)[0]))
    bad.append(("FF residual added twice", "x_ff", cb.res_ref(t["g"], W["w2"][li], W["b2"][li], t["x_attn"], fmt, gain=2.0)[0]))
    bad.append(("FF residual not added", "x_ff", cb.res_ref(t["g"], W["w2"][li], W["b2"][li], t["x_attn"], fmt, gain=0.0)[0]))
    ff = refs["ff"][0]
    bad.append(("value and gate halves swapped", "ff", np.concatenate([ff[:, FIP:], ff[:, :FIP]], -1)))
    bad.append(("GELU on the value", "g", round_fmt(cb.geglu_ref(t["ff"], fmt, on_value=True)[0], fmt)))
    y = t["g"].copy()
    y[:, cb.FI] = 2.0 ** -24
    bad.append(("a nonzero column >= 1365", "g", y))
    bad.append(("FF2 without the second 64-chunk of K", "x_ff", refs["x_ff"][0] - t["g"][:, 64:128] @ W["w2"][li][:, 64:128].T))
    bad.append(("b1 of the next block", "ff", ff - W["b1"][li] + W["b1"][nx]))
    bad.append(("b2 of the next block", "x_ff", refs["x_ff"][0] - W["b2"][li] + W["b2"][nx]))
    if final:
        bad.append(("the final norm's gamma missing", "final", cb.final_ref(t["x_ff"], W, c, no_gamma=True)[0]))
        bad.append(("to_pred rows 0 and 1 exchanged", "final", cb.final_ref(t["x_ff"], W, c, swap_rows=True)[0]))
    return bad


def check_clip(W, c, fmt, cond, y, li=0, x_in=None, final=False, t_eval=T_EVAL, upto_qk=False):
    gb, gb_other = cb.gb_ref(W, t_eval)[0], cb.gb_ref(W, 0.5)[0]
    t = cb.emulate_clip(cond, y, W, c, li, fmt, gb, x_in=x_in, upto_qk=upto_qk)
    block = block_stages(fmt)
    block = block[:block.index("ctx")] if upto_qk else block
    stages = (cb.FRONT if x_in is None else ()) + block + (("final",) if final else ())
    refs = cb.stage_refs(t, W, c, li, fmt, stages)
    for st in stages:
        r, at = worst_ratio(t[st], *refs[st])
        assert r <= 1.0, (fmt, c, li, st, "the emulated kernel", r, at)
    for name, st, bad in planted_defects(t, refs, W, c, li, fmt, cb.f32(gb_other), front=x_in is None, final=final, upto_qk=upto_qk):
        r, _ = worst_ratio(bad, *refs[st])
        assert r > 1.0, (fmt, c, li, st, name, r)
    return t


@pytest.mark.parametrize("T", LONE_T)
@pytest.mark.parametrize("fmt", FMTS)
def test_block0_bounds_reject_planted_defects(sd, fmt, T):
    cond, y = cb.clip(T)
    check_clip(weights(sd, fmt), Geom([T]).clips[0], fmt, cond.numpy(), y.numpy())


@pytest.mark.parametrize("fmt", FMTS)
def test_blocks_0_1_7_and_final(sd, fmt):
    """row 0 of the padded B = 3, T = 113 batch through all eight blocks: blocks 0, 1 and 7 with their defects (the per-block offsets of
    the weights, biases, q / k gammas and norm index), the final launch behind block 7"""
    W = weights(sd, fmt)
    c = Geom(list(RAGGED)).clips[0]
    cond, y = cb.padded(RAGGED)
    t = check_clip(W, c, fmt, cond[0].numpy(), y[0].numpy())
    for li in range(1, cb.DEPTH):
        if li in (1, 7):
            t = check_clip(W, c, fmt, None, None, li=li, x_in=t["x_ff"], final=li == 7)
        else:
            t = cb.emulate_clip(None, None, W, c, li, fmt, cb.gb_ref(W, T_EVAL)[0], x_in=t["x_ff"])


@pytest.mark.parametrize("fmt", ["fp32", "bf16"])
def test_long_clip_front_of_block0(sd, fmt):
    """T = 2999 as the GPU tier runs it, the front and block 0 up to Q / K / V^T (QKVF): rotary angles near 3000 rad beside the registers'
    -10000, where the bounds of q and k rest on SINCOS_ERR; the defects of the front, the norm, the rotary and V^T's layout"""
    T = 2999
    cond, y = cb.clip(T)
    check_clip(weights(sd, fmt), Geom([T]).clips[0], fmt, cond.numpy(), y.numpy(), upto_qk=True)


# (fp32 has no packed form: sample_packed runs in bf16 / fp16 only)
@pytest.mark.parametrize("fmt,mode", [("fp32", "frames"), ("bf16", "frames"), ("fp16", "frames"), ("bf16", "packed"), ("fp16", "packed")])
def test_frames_and_packed_geometry(sd, fmt, mode):
    """the clips (113, 48, 1) as a frames= call and as a packed call, first evaluation of a sample (t = 0): block 0 of every clip"""
    g = Geom(list(RAGGED), mode)
    cond, y = cb.padded(RAGGED)
    for b, c in enumerate(g.clips):
        n = c["Trow"]
        check_clip(weights(sd, fmt), c, fmt, cond[b, :n].numpy(), y[b, :n].numpy(), t_eval=0.0)


def test_trained_scale_scores(sd, monkeypatch):
    """q / k gammas 1.0 (upstream's initial value), bf16, the T = 113 batch: the scores exceed 100 in log2 units (the condition of the
    encoder's trained-scale test) -- in every row, by tests/cfm_ref.py's own float64 forward (block 0's q.k product, taken as evaluate
    forms it), and by this module's reference on row 0's emulated taps; the emulated kernel stays inside the bounds of Q, K, V^T and CTX,
    and the rotary and attention defects are still rejected"""
    W = weights(sd, "bf16", 1.0)
    c = Geom(list(RAGGED)).clips[0]
    cond, y = cb.padded(RAGGED)
    sims, einsum = [], torch.einsum

    def spy(eq, *ops):
        out = einsum(eq, *ops)
        if eq == "b h i d, b h j d -> b h i j":
            sims.append(out)
        return out
    monkeypatch.setattr(torch, "einsum", spy)
    with torch.no_grad():
        cfm_ref.evaluate(cfm_ref.to_f64(cb.with_qk_gamma(sd, 1.0)), y.double(), T_EVAL, cond.double())
    monkeypatch.undo()
    assert len(sims) == cb.DEPTH and tuple(sims[0].shape) == (3, 8, 129, 129)
    s_ref = sims[0].numpy() * 10 * el.LOG2E                   # evaluate multiplies q.k by 10; log2 units as the kernels take them
    assert (np.abs(s_ref).reshape(3, -1).max(1) > 100.0).all()
    t = cb.emulate_clip(cond[0].numpy(), y[0].numpy(), W, c, 0, "bf16", cb.gb_ref(W, T_EVAL)[0])
    s = cb.ctx_ref(t, "bf16", c)[2]["s"]
    assert np.abs(s[np.isfinite(s)]).max() > 100.0
    # (the two agree to what bf16 operands lose: the emulated q, k carry 2^-8 relative each, the scores are sums of 64 such products)
    assert np.abs(s[0, :8, :129, :129] - s_ref[0]).max() < 2.0 ** -6 * np.abs(s_ref[0]).max()
    refs = cb.stage_refs(t, W, c, 0, "bf16", ("q", "k", "vt", "ctx"))
    for st in ("q", "k", "vt", "ctx"):
        assert worst_ratio(t[st], *refs[st])[0] <= 1.0, st
    for name, st, bad in rotary_defects(t, W, c, 0, "bf16", heads=False) + attention_defects(t, W, c, 0, "bf16"):
        assert worst_ratio(bad, *refs[st])[0] > 1.0, name

"""Test-only float64 references of ONE post-LN encoder layer, launch by launch, and per-element error bounds derived from the arithmetic
of the kernels behind each launch (the EPI_QK / EPI_BF16 / EPI_F32_RESLN GEMMs, csrc/attention.hip, layernorm_kernel, and their fp32
parity counterparts in csrc/fp32_path.hip).  In the style of tests/frontend_ref.py, whose formats, notation (u, h(fmt), q(fmt)) and
helpers are reused; plain numpy, written from the published algorithm (transformers' HubertEncoderLayer, restated in
oracle/hubert_ref.py); never imported by ``sylber_amd``.

Every stage is computed FROM THE PREVIOUS TAP'S ACTUAL VALUES (the layer taps of sylber_set_stop_stage, SYLBER_TAP_LAYER(l, k)): a tap
returns a 16-bit buffer widened exactly, so its values are exact operands of the next launch, and a comparison tests one kernel with a
bound that holds that kernel's arithmetic only.

The operand of the q / k / v projection (the LayerNorm output in front of the layer) has no tap of its own; it is round_fmt of stage
2 + l (the encoder LayerNorm for l = 0, the previous layer's output otherwise).  That is EXACT, not a modelled rounding: layernorm_kernel
computes one fp32 value y per element and stores it as fp32 (the last launch of a stopped forward) or rounds that same y into the 16-bit
buffer (every other forward) -- one kernel instantiation, one expression, the destination chosen by a run-time pointer -- and the
rounding of an fp32 value into a format is deterministic.  So nothing is added for it, unlike proj_bound.

Constants that can only be measured: the error of the hardware exp2 (v_exp_f32).  The ISA manual states 1 ulp, i.e. 2 u relative; EXP2_ERR
is twice that, a stated conservative value, not taken from any kernel output."""
import math

import numpy as np

from frontend_ref import EPS, GELU_LIP, HALF_ULP, SUB_Q, U, gelu64, gelu_error, layernorm_ref, round_fmt, store_error, worst_ratio  # noqa: F401

HEADS, HDIM, HIDDEN, FFN = 12, 64, 768, 3072
LOG2E = math.log2(math.e)
Q_SCALE = float(np.float32(0.18033688011112042))          # SYL_Q_SCALE (csrc/common.h): fl32(log2(e) / 8)
EXP2_ERR = 4 * U
LAZY = 8.0                                                # the lazy running maximum may lag the true one by 2^8 (attention.hip)
TAPS = ("qkv", "ctx", "attn_sum", "ln1", "ffn1", "ffn2_sum")      # tap k of a layer, in launch order
STAGES = TAPS + ("out",)                                         # + the layer's output (stop stage 3 + l)

# (T, valid frames per utterance): lone clips at the 32-key half-tile, the 64-key tile and one frame around them; a batch whose valid
# counts sit at and one past the 64-key tiles, the 128-query block and the 256-row GEMM tile; a batch past 384 = 3 x 128 queries
SHAPES = ((1, (1,)), (17, (17,)), (33, (33,)), (64, (64,)), (65, (65,)), (257, (257, 256, 193, 192, 65, 64, 1)), (385, (385, 384, 321)))
LAYER1_SHAPE = SHAPES[5]
FFN1_GAIN = 3.0           # both tiers scale FFN1's weights by this: its GELU argument then leaves gelu_fast's core |z| <= 4.2 at every shape
QK_GAIN = 5.0             # the "trained scale" case: q and k weight rows of layer 0 times this -> max |score| > 100 in log2 units


def q_scale(fmt):
    """what the q third of the projection is multiplied by before it is stored (the fp32 mode scales inside its attention kernel)"""
    return 1.0 if fmt == "fp32" else Q_SCALE


def scaled_state_dict(sd, num_layers, qk_gain=1.0):
    """the checkpoint both tiers use: FFN1's weights times FFN1_GAIN; optionally layer 0's q / k weights times qk_gain"""
    out = dict(sd)
    for l in range(num_layers):
        k = "encoder.layers.%d.feed_forward.intermediate_dense.weight" % l
        out[k] = sd[k] * FFN1_GAIN
    if qk_gain != 1.0:
        for n in ("q_proj", "k_proj"):
            k = "encoder.layers.0.attention.%s.weight" % n
            out[k] = sd[k] * qk_gain
    return out


def layer_weights(sd, l, fmt):
    """layer l's tensors as the kernels hold them: GEMM weights round_fmt'ed (once, at load time), everything else float64.
    "prev_g" / "prev_b": the affine of the LayerNorm in FRONT of the layer (the encoder LayerNorm, or layer l - 1's final one)"""
    def f(name):
        return sd[name].detach().numpy().astype(np.float64)
    p = "encoder.layers.%d." % l
    w = {"Wqkv": round_fmt(np.concatenate([f(p + "attention.%s_proj.weight" % n) for n in "qkv"]), fmt),
         "bqkv": np.concatenate([f(p + "attention.%s_proj.bias" % n) for n in "qkv"]),
         "Wo": round_fmt(f(p + "attention.out_proj.weight"), fmt), "bo": f(p + "attention.out_proj.bias"),
         "W1": round_fmt(f(p + "feed_forward.intermediate_dense.weight"), fmt), "b1": f(p + "feed_forward.intermediate_dense.bias"),
         "W2": round_fmt(f(p + "feed_forward.output_dense.weight"), fmt), "b2": f(p + "feed_forward.output_dense.bias"),
         "ln1_g": f(p + "layer_norm.weight"), "ln1_b": f(p + "layer_norm.bias"),
         "ln2_g": f(p + "final_layer_norm.weight"), "ln2_b": f(p + "final_layer_norm.bias")}
    q = "encoder.layer_norm." if l == 0 else "encoder.layers.%d.final_layer_norm." % (l - 1)
    w["prev_g"], w["prev_b"] = f(q + "weight"), f(q + "bias")
    return w


# ---- a Linear on exact operands ------------------------------------------------------------------------------------------------------
def linear_ref(x, W, b, fmt):
    """y = x W^T + b in float64 and the bound on what the kernel's accumulator + bias holds instead.  x and W are the kernel's operands
    exactly (tap values, rounded weights), and a product of two 16-bit operands is exact in fp32, so only the fp32 accumulation of
    K products and the bias add remain: (K + 2) u S with S = sum_k |x_k| |w_nk| + |b_n|, for any summation order.  split16 runs three
    passes hi.hi + lo.hi + hi.lo (3 K accumulated products) and drops lo.lo: 2^-22 S + 2^-36 (sum |w| + sum |x|) + K 2^-50, as in
    proj_bound.  The fp32 mode multiplies fp32 operands: one rounding more per product, (K + 3) u S."""
    x = np.asarray(x, np.float64)
    K = x.shape[-1]
    y = x @ W.T + b
    # S in fp32 (a K-term fp32 sum of non-negative terms is within K u of the truth: inflate by that)
    S = (np.abs(x).astype(np.float32) @ np.abs(W).T.astype(np.float32)).astype(np.float64) * (1 + 2 * K * U) + np.abs(b)
    if fmt == "split16":
        e = ((3 * K + 2) * U + 2.0 ** -22) * S + 2.0 ** -36 * (np.abs(W).sum(1) + np.abs(x).sum(-1, keepdims=True)) + K * 2.0 ** -50
    elif fmt == "fp32":
        e = (K + 3) * U * S
    else:
        e = (K + 2) * U * S
    return y, e


def qkv_ref(h, lw, fmt):
    """tap QKV from the layer's operand h [B, T, 768] (module docstring): q | k | v = h Wqkv^T + b, the q third times q_scale(fmt).
    Bound: linear_ref's, times the scale on the q third plus the rounding of that product (u |q|), plus the store's half-ulp."""
    y, e = linear_ref(h, lw["Wqkv"], lw["bqkv"], fmt)
    qs = q_scale(fmt)
    if qs != 1.0:
        y[..., :HIDDEN] *= qs
        e[..., :HIDDEN] = e[..., :HIDDEN] * qs + U * np.abs(y[..., :HIDDEN])
    return y, e + store_error(np.abs(y) + e, fmt)


# ---- attention -------------------------------------------------------------------------------------------------------------------------
def key_mask(valid, T):
    return np.arange(T)[None, :] < np.minimum(np.asarray(valid), T)[:, None]


def vt_key_permutation(T):
    """the key order of the V^T buffer: bits 2 and 3 of the key index swapped (an involution inside every group of 16 keys)"""
    t = np.arange(T)
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


def _heads(x):
    B, T, _ = x.shape
    return x.reshape(B, T, HEADS, HDIM).transpose(0, 2, 1, 3)                      # [B, H, T, 64]


def attention_parts(qkv, valid, fmt, mask=None, score_gain=1.0):
    """scores in log2 units s [B, H, T, T] (masked keys -inf), A = sum_d |q_d| |k_jd| in the same units, and the masked v"""
    qkv = np.asarray(qkv, np.float64)
    B, T, _ = qkv.shape
    q, k, v = (_heads(qkv[..., i * HIDDEN:(i + 1) * HIDDEN]) for i in range(3))
    c = (1.0 if fmt != "fp32" else 0.125 * LOG2E) * score_gain                         # the 16-bit modes' q arrives in log2 units
    kt = k.transpose(0, 1, 3, 2)
    s = (q @ kt) * c
    A = (np.abs(q) @ np.abs(kt)) * abs(c)
    mask = key_mask(valid, T) if mask is None else mask
    s = np.where(mask[:, None, None, :], s, -np.inf)
    return s, A, v, mask


def ctx_ref(qkv, valid, fmt, mask=None, score_gain=1.0, v_perm=None):
    """tap CTX from tap QKV [B, T, 2304]: base-2 softmax over the keys < min(valid_b, T) in float64 (q carries log2(e) / 8 in the 16-bit
    modes; the fp32 mode's q is unscaled and its kernel multiplies by 1/8 and log2(e) itself), times v.  Every query row is computed,
    the padded ones too.  ``mask`` [B, T] / ``score_gain`` / ``v_perm`` (a key permutation of v) exist for the planted defects.

    Bound, as c_i V_id + q(fmt) sum_j |v_jd| + the store, with w_j = p_j / sum p the float64 probabilities, V_id = sum_j w_j |v_jd|:
      * the score the kernel exponentiates, in log2 units, is off by ds_j: fp32 accumulation of 64 exact products, the subtraction of the
        running reference m (the hand-scheduled kernel seeds the accumulator with -m, the compiled one subtracts afterwards: either way
        each rounding is u relative to a partial sum <= A_j + |m|, A_j = sum_d |q_d| |k_jd|), one more for a rebase: (64 + 2) u (A_j + |m|)
        with |m| <= max_j |s_j| + 8 (the lazy reference lags by at most 2^8).  split16: three passes and the dropped lo.lo,
        (3 x 64 + 2) u (A_j + |m|) + 2^-22 A_j.  fp32 mode: rounded products (64 + 1) u A_j, then fma(s, log2 e, -fl(m log2 e)):
        4 u (|s_j| + |m|) covers the constant, the product and the fma;
      * p_j = exp2(.): relative error ln 2 ds_j (the exponent's sensitivity) + EXP2_ERR (the instruction), and every later rescale by
        alpha = exp2(m_old - m_new) multiplies O and l by a factor that is EXP2_ERR + 2 u off: R <= (keys / 32) rescales, one per half-tile;
        delta_i = max_j over the valid keys of that sum;
      * P enters the P.V MFMA rounded to the 16-bit format: h(fmt) relative (bf16 2^-8, fp16 2^-11), below 2^-14 the fp16 grid: an
        ABSOLUTE 2^-25 per key relative to a row sum >= 1 (the reference key has p >= 1), hence q(fmt) sum_j |v_jd|; split16 keeps a hi / lo
        pair (2^-22) and drops lo.lo (2^-22); fp32 keeps p and rounds the product (u).  The row sum l adds the UNROUNDED p (psum in
        attention_bf16_kernel, the v_add_f32 chain in front of the pack in tools/gen_attn_asm.py), so numerator and denominator do not
        share the rounding and the full h(fmt) V stays in the bound (a kernel summing rounded p would sit inside it as well);
      * fp32 accumulation over the keys, numerator and denominator: passes x keys x u each (keys rounded up to whole 32-key half-tiles);
      * 1 / l, the product with it: 2 u each.
      numerator errors are relative to sum_j p_j |v_jd|, denominator errors to |ctx_id| <= V_id: c_i = 2 x 1.01 delta_i + h_P +
      (2 passes keys + 6) u (1.01: the second-order terms of exp(delta)).
      * the final store: store_error at |ctx| + the error so far."""
    s, A, v, mask = attention_parts(qkv, valid, fmt, mask, score_gain)
    B, H, T, _ = s.shape
    if v_perm is not None:
        v = v[:, :, v_perm]
    m = s.max(-1, keepdims=True)
    p = np.exp2(s - m)
    w = p / p.sum(-1, keepdims=True)
    ctx = w @ v
    V = w @ np.abs(v)
    nk = mask.sum(1)                                                              # keys per utterance
    nk32 = ((nk + 31) // 32 * 32).astype(np.float64)[:, None, None]
    sabs = np.where(mask[:, None, None, :], np.abs(s), 0.0)
    mabs = sabs.max(-1, keepdims=True) + LAZY
    if fmt == "fp32":
        ds = (HDIM + 1) * U * A + 4 * U * (sabs + mabs)
        passes, hP = 1, U
    elif fmt == "split16":
        ds = (3 * HDIM + 2) * U * (A + mabs) + 2.0 ** -22 * A
        passes, hP = 3, 2 * 2.0 ** -22
    else:
        ds = (HDIM + 2) * U * (A + mabs)
        passes, hP = 1, HALF_ULP[fmt]
    ds = np.where(mask[:, None, None, :], ds, 0.0).max(-1)                          # [B, H, T]
    R = nk32 / 32
    delta = math.log(2.0) * ds + EXP2_ERR * (1 + R) + 2 * U * R
    c = 2 * 1.01 * delta + hP + (2 * passes * nk32 + 6) * U
    vsum = (np.abs(v) * mask[:, None, :, None]).sum(2, keepdims=True)              # [B, H, 1, 64]
    e = c[..., None] * V + (2 if fmt == "split16" else 1) * SUB_Q[fmt] * vsum

    def merge(x):
        return x.transpose(0, 2, 1, 3).reshape(B, T, HIDDEN)
    ctx, e = merge(ctx), merge(e)
    return ctx, e + store_error(np.abs(ctx) + e, fmt), {"s": s, "w": w}


# ---- the residual GEMMs, the LayerNorms, FFN1 ---------------------------------------------------------------------------------------------
def layernorm_rows(f, g, be, shift=0, n=None):
    """LayerNorm in float64 with the statistics of row t + shift (planted defect) or over the first n elements only (planted defect)"""
    f = np.asarray(f, np.float64)
    fs = f if n is None else f[..., :n]
    mean = fs.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((fs - mean) ** 2).mean(-1, keepdims=True) + EPS)
    if shift:
        mean, rstd = np.roll(mean, -shift, axis=1), np.roll(rstd, -shift, axis=1)
    return (f - mean) * rstd * g + be


def residual_sum_ref(x, W, b, pre, g, be, fmt):
    """taps ATTN_SUM / FFN2_SUM: x W^T + b + LayerNorm(pre; g, be).  The residual is not read from a buffer: EPI_F32_RESLN re-derives it
    from the pre-LayerNorm sum still sitting in ``pre`` and the (mean, rstd) table the LayerNorm kernel left behind, with that
    LayerNorm's affine -- the expression of layernorm_kernel, so layernorm_ref's bound is the bound of the re-derived value (the fp32
    mode reads the stored fp32 LayerNorm output: the same bound).  Plus linear_ref's, plus the two fp32 adds: u (|y| + |out|)."""
    y, e = linear_ref(x, W, b, fmt)
    ln, eln = layernorm_ref(pre, g, be)
    out = y + ln
    return out, e + eln + U * (np.abs(y) + e + np.abs(out) + e + eln)


def ln_store_ref(pre, g, be, fmt):
    """tap LN1: LayerNorm(768) of tap ATTN_SUM in fp32 (layernorm_ref's bound), stored in the 16-bit format (store_error)"""
    y, e = layernorm_ref(pre, g, be)
    return y, e + store_error(np.abs(y) + e, fmt)


def gelu_kind(fmt):
    return {"bf16": "fast", "fp16": "fast", "split16": "erf7", "fp32": "erf"}[fmt]


def ffn1_ref(h, lw, fmt):
    """tap FFN1 from tap LN1: gelu(h W1^T + b1), the GELU of the mode (gelu_fast for bf16 / fp16, gelu_erf7 for split16, gelu_erf for
    fp32).  linear_ref's bound through the GELU's Lipschitz constant, gelu_error of the variant at an argument known to that bound,
    and the store."""
    z, ez = linear_ref(h, lw["W1"], lw["b1"], fmt)
    y = gelu64(z)
    e = GELU_LIP * ez + gelu_error(z, gelu_kind(fmt), ez)
    return y, e + store_error(np.abs(y) + e, fmt), z


def gelu_fast64(x, clamp=True):
    """csrc/common.h's gelu_fast restated (float64 evaluation of its fp32 polynomial); clamp False: the polynomial continued past its
    core |x| <= 4.2 (planted defect)"""
    x = np.asarray(x, np.float64)
    xc = np.clip(x, -4.2, 4.2) if clamp else x
    u = xc * xc
    q = 6.949803233e-11 * u - 6.356798643e-09
    for c in (2.570604920e-07, -6.139445304e-06, 9.818511899e-05, -1.133762766e-03, 9.886963293e-03, -6.643489748e-02, 3.989362717e-01):
        q = q * u + c
    return x * (xc * q + 0.5)


# ---- one layer, stage by stage --------------------------------------------------------------------------------------------------------
def stage_refs(t, lw, valid, fmt, stages=STAGES):
    """t: the actual values around one layer -- "pre_prev" (the pre-LayerNorm sum in front of the layer: TAP_POSCONV or the previous
    layer's FFN2_SUM), "hin" (stage 2 + l, fp32) and the six taps by name -> {stage: (float64 reference, per-element bound)}, every
    stage from the tap in front of it"""
    out = {}
    for st in stages:
        if st == "qkv":
            out[st] = qkv_ref(round_fmt(t["hin"], fmt), lw, fmt)
        elif st == "ctx":
            out[st] = ctx_ref(t["qkv"], valid, fmt)[:2]
        elif st == "attn_sum":
            out[st] = residual_sum_ref(t["ctx"], lw["Wo"], lw["bo"], t["pre_prev"], lw["prev_g"], lw["prev_b"], fmt)
        elif st == "ln1":
            out[st] = ln_store_ref(t["attn_sum"], lw["ln1_g"], lw["ln1_b"], fmt)
        elif st == "ffn1":
            out[st] = ffn1_ref(t["ln1"], lw, fmt)[:2]
        elif st == "ffn2_sum":
            out[st] = residual_sum_ref(t["ffn1"], lw["W2"], lw["b2"], t["attn_sum"], lw["ln1_g"], lw["ln1_b"], fmt)
        else:
            out[st] = layernorm_ref(t["ffn2_sum"], lw["ln2_g"], lw["ln2_b"])
    return out


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def ctx_emulated(qkv, valid, fmt):
    """what a correct kernel stores: fp32 probabilities against the row maximum, ROUNDED to the format for the P.V product and
    unrounded in the row sum, the quotient rounded into the context buffer"""
    s, _, v, _ = attention_parts(qkv, valid, fmt)
    p = f32(np.exp2(s - s.max(-1, keepdims=True)))
    num = round_fmt(p, fmt) @ v
    ctx = num / f32(p.sum(-1, keepdims=True))
    B, H, T, _ = ctx.shape
    return round_fmt(ctx.transpose(0, 2, 1, 3).reshape(B, T, HIDDEN), fmt)


def emulate_layer(pre_prev, lw, valid, fmt):
    """the chain a correct kernel sequence leaves in the taps, emulated in numpy: every stage is the float64 reference of the stage
    before it with the operand / store roundings of the format applied (fp32 for the pre-LayerNorm sums and the LayerNorm outputs,
    round_fmt for the 16-bit buffers, the P rounding inside the attention)"""
    t = {"pre_prev": f32(pre_prev)}
    t["hin"] = f32(layernorm_ref(t["pre_prev"], lw["prev_g"], lw["prev_b"])[0])
    t["qkv"] = round_fmt(qkv_ref(round_fmt(t["hin"], fmt), lw, fmt)[0], fmt)
    t["ctx"] = ctx_emulated(t["qkv"], valid, fmt)
    t["attn_sum"] = f32(residual_sum_ref(t["ctx"], lw["Wo"], lw["bo"], t["pre_prev"], lw["prev_g"], lw["prev_b"], fmt)[0])
    t["ln1"] = round_fmt(f32(layernorm_ref(t["attn_sum"], lw["ln1_g"], lw["ln1_b"])[0]), fmt)
    z = linear_ref(t["ln1"], lw["W1"], lw["b1"], fmt)[0]
    t["ffn1"] = round_fmt(gelu64(z) if gelu_kind(fmt) != "fast" else gelu_fast64(z), fmt)
    t["ffn2_sum"] = f32(residual_sum_ref(t["ffn1"], lw["W2"], lw["b2"], t["attn_sum"], lw["ln1_g"], lw["ln1_b"], fmt)[0])
    t["out"] = f32(layernorm_ref(t["ffn2_sum"], lw["ln2_g"], lw["ln2_b"])[0])
    return t


def pre_input(T, valid, seed):
    """a stand-in for the pos-conv tap on the CPU tier: rows of unit-scale noise around a common offset, like the residual stream"""
    g = np.random.default_rng(seed)
    return (g.standard_normal((len(valid), T, HIDDEN)) + 0.5 * g.standard_normal((1, 1, HIDDEN))).astype(np.float32)

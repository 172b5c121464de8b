"""Test-only float64 references of ONE post-LN encoder layer of the fp8 precision (SYLBER_FP8: every GEMM and the attention core on
MXFP8 operands), launch by launch, and per-element bounds derived from the arithmetic of the kernels behind each launch: the
quantising LayerNorm store (the out_fp8 branch of layernorm_kernel), EPI_QK8 / EPI_MXFP8 / EPI_F32_RESLN of the MXFP8 GEMMs
(csrc/gemm_epilogue_f8.h), attention_f8_kernel and the MXFP8 branch of attn_finalize (csrc/attention.hip).  In the style of
tests/encoder_layer_ref.py, whose helpers are reused together with tests/frontend_ref.py and the bit-exact quantiser of
oracle/mxfp8_ref.py; plain numpy; never imported by ``sylber_amd``.

Every stage is computed FROM THE PREVIOUS TAP'S ACTUAL VALUES.  An fp8 layer tap (SYLBER_TAP_LAYER(l, k) on a SYLBER_FP8 handle) returns
an MXFP8 buffer as [B, T, 2 W]: W values dequantised exactly (e4m3 x 2^(s - 127) is an fp32 value) and W floats holding each
element's block exponent s - 127; ``split_tap`` takes the two apart.  So a tap's values are exact operands of the next launch.

OPERANDS ARE EXACT.
  * Weights are dequantize(quantize(W_fp32)): the device quantises the fp32 originals with the quantiser that
    tests/test_gpu_fp8.py::test_quantiser_bit_exact pins bit for bit to oracle/mxfp8_ref.py.
  * The layer's operand (the LayerNorm output in front of it) has no tap of its own; it is dequantize(quantize(stage 2 + l)).  That is
    exact: layernorm_kernel computes one fp32 value y per element (fmaf((x - mean) rstd, gamma, beta)) and either stores that y as fp32
    (the last launch of a stopped forward) or takes the block maximum of the same y over 8 lanes x 4 values = 32 features, mx_e8m0 of
    it, and pack_fp8x4(y 2^-e) -- one kernel instantiation, one expression, the destination chosen by run-time pointers; the
    scale rule and the e4m3 rounding are the oracle quantiser's.

A LINEAR ON MXFP8 OPERANDS.  The products of two dequantised operands are exact in fp32 (4 + 4 significand bits and a power of two),
so the bound is the fp32 accumulation of K products and the bias, (K + 2) u S with S = sum_k |x_k| |w_nk| + |b_n|, plus the block-scaled
MFMA's inexact 64-term sum (the products look aligned to the largest one and truncated): MX_MFMA x S with MX_MFMA = 3e-4, the
constant of tests/test_gpu_fp8.py::test_mxfp8_linear_matches_oracle.  It was measured there through sylber_op_linear against the
float64 contraction of the same operands (oracle.mxfp8_ref.linear): 2e-5 x S on Gaussian data, about 1e-4 x S with spread exponents;
3e-4 keeps a 3x margin over the larger figure.  It is NOT fitted to the kernels under test here.

A QUANTISING STORE (``quant_store_check``).  A pre-quantisation reference y with bound e (the kernel's fp32 value v has |v - y| <= e):
  * the block maximum the kernel sees lies in [max_i (|y_i| - e_i)+, max_i (|y_i| + e_i)], and block_scale is monotone, so the
    stored scale byte must lie in {block_scale(lower) ... block_scale(upper)} -- usually one value;
  * the stored element is v rounded to nearest onto the e4m3 grid of the stored scale: within e plus half an e4m3 ulp of |y| + e,
    2^-4 relative in the normal range (half an ulp of 2^(k - 3) in [2^k, 2^(k + 1))) and 2^(E - 10) absolute below 2^(E - 6) for the
    LARGEST admissible exponent E (the subnormal spacing 2^(E - 9));
  * no block and no element is skipped; the exponent plane must be constant inside every block along the block's axis.
  V^T is blocked over 32 KEYS per feature.  The keys [T, Tp) of an utterance's last block exist on the device (they are padded
  frames that flow through the layer) but are not visible through a T-frame tap, so the upper end of that one block's scale is not
  known: where T % 32 != 0 the last key block is held to the lower end only and its elements to the half-ulp of the STORED scale
  (``open_tail``).  Every other block of every buffer is held to both ends.

ATTENTION ON MXFP8 OPERANDS (``ctx8_ref``), following encoder_layer_ref.ctx_ref's derivation; see its docstring for the notation.

Constants that can only be measured: EXP2_ERR as in encoder_layer_ref (twice the ISA manual's 1 ulp) and MX_MFMA above."""
import math

import numpy as np

import encoder_layer_ref as el
from encoder_layer_ref import EXP2_ERR, HDIM, HEADS, HIDDEN, LOG2E, Q_SCALE, key_mask  # noqa: F401
from frontend_ref import GELU_LIP, U, gelu64, gelu_error, layernorm_ref, round_fmt, store_error, worst_ratio  # noqa: F401
from oracle import mxfp8_ref as Q

MX_MFMA = 3e-4            # the block-scaled MFMA's inexact 64-term sum, relative to sum |a_k| |b_k| (module docstring)
P_BIAS = 7                # P is carried as p 2^7 (attention_f8_kernel)
P_LAG = 1.0               # the running maximum may lag the true one by 2^1 (log2 units)
TAPS, STAGES = el.TAPS, el.STAGES
QUANT_STAGES = ("qkv", "ctx", "ln1", "ffn1")          # the taps that are MXFP8 buffers (qkv: with the fp8 attention core)
AMBIGUOUS_CAP = 0.15      # at most this share of a stage's blocks may admit more than one scale byte (asserted on the CPU tier)


# ---- MXFP8 along any axis ------------------------------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _blocks(x, axis):
    """x with ``axis`` moved last, zero-padded to whole 32-blocks and split: [..., nblocks, 32]; and the axis' length"""
    x = np.moveaxis(np.asarray(x, np.float64), axis, -1)
    n = x.shape[-1]
    pad = -n % 32
    if pad:
        x = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,))], -1)
    return x.reshape(x.shape[:-1] + (-1, 32)), n


def _unblocks(xb, n, axis):
    return np.moveaxis(xb.reshape(xb.shape[:-2] + (-1,))[..., :n], -1, axis)


def e4m3_round(x, truncate=False):
    """|x| <= 448 onto the e4m3 grid: to nearest even (the oracle's encoder), or towards zero (planted defect)"""
    x = np.asarray(x, np.float64)
    if not truncate:
        return Q.e4m3_decode(Q.e4m3_encode(x))
    a = np.abs(x)
    idx = np.clip(np.searchsorted(Q._VALS, a, side="right") - 1, 0, 126)
    return np.copysign(Q._VALS[idx], x)


def mx_quant(x, axis=-1, scale_of=None, scale_shift=0, truncate=False):
    """the oracle quantiser along ``axis`` in blocks of 32 (a partial last block is padded with zeros) -> (dequantised values, block
    exponents s - 127 per element), both of x's shape.  ``scale_of`` (the values the block maximum is taken over instead of x),
    ``scale_shift`` and ``truncate`` exist for the planted defects; a value past 448 x 2^e saturates like the oracle's encoder."""
    xb, n = _blocks(f32(x), axis)
    sb = xb if scale_of is None else _blocks(f32(scale_of), axis)[0]
    s = Q.block_scale(np.abs(sb).max(-1)).astype(np.int64) + scale_shift
    ex = (s - 127).astype(np.float64)[..., None]
    val = e4m3_round(np.clip(xb * 2.0 ** -ex, -448.0, 448.0), truncate) * 2.0 ** ex
    return _unblocks(val, n, axis), _unblocks(np.broadcast_to(ex, xb.shape).copy(), n, axis)


def mx_dequant_operand(x, axis=-1):
    return mx_quant(x, axis)[0]


def split_tap(y):
    """an fp8 layer tap [B, T, 2 W] -> (values [B, T, W], block exponents [B, T, W])"""
    y = np.asarray(y, np.float64)
    W = y.shape[-1] // 2
    return y[..., :W], y[..., W:]


def e4m3_half_ulp(a, E):
    """half an e4m3 ulp of a magnitude <= a on the grid of block exponent E: 2^(k - 4) for 2^k <= a < 2^(k + 1), at least 2^(E - 10)"""
    _, ex = np.frexp(a)                                           # a = m 2^ex, 0.5 <= m < 1: k = ex - 1
    return np.maximum(np.ldexp(1.0, ex - 5), np.ldexp(1.0, np.asarray(E, np.int64) - 10))


def quant_store_check(val, ex, y, e, axis=-1, open_tail=False):
    """the quantising store of the module docstring -> dict: "ratio" max |val - y| / (e + half ulp) and "at"; "bad_scale" the number of
    blocks whose stored exponent is outside the admissible set and "first_bad" one of them; "ragged" the number of blocks whose
    exponent plane is not constant; "blocks" / "ambiguous" the number of blocks and of those admitting more than one byte.
    open_tail: the last block along ``axis`` is partial and its hidden members may raise the maximum (V^T's keys [T, Tp))."""
    vb, n = _blocks(val, axis)
    xb = _blocks(ex, axis)[0]
    yb, eb = _blocks(y, axis)[0], _blocks(np.broadcast_to(e, np.shape(y)), axis)[0]
    live = _blocks(np.ones(np.shape(y)), axis)[0] > 0             # (the zero padding of a partial block is no element)
    lo = np.where(live, np.maximum(np.abs(yb) - eb, 0.0), 0.0).max(-1)
    hi = np.where(live, np.abs(yb) + eb, 0.0).max(-1)
    # block_scale works on fp32 bits: round the ends outwards on their way there
    s_lo = Q.block_scale((lo * (1 - 2.0 ** -23)).astype(np.float32)).astype(np.int64) - 127
    s_hi = Q.block_scale(np.nextafter((hi * (1 + 2.0 ** -23)).astype(np.float32), np.float32(np.inf))).astype(np.int64) - 127
    s_lo = np.where(lo == 0, -127, s_lo)                          # (the maximum may be anything from 0 up: no lower end ...)
    x0 = np.where(live, xb, -np.inf).max(-1)
    ragged = (np.where(live, xb, x0[..., None]) != x0[..., None]).any(-1) | ~np.isfinite(x0)
    stored = np.where(np.isfinite(x0), x0, 999).astype(np.int64)
    zero_ok = (lo == 0) & (stored == 0)                           # (... and an all-zero block stores 2^0)
    tail = np.zeros(stored.shape, bool)
    if open_tail and n % 32:
        tail[..., -1] = True
    bad = ~zero_ok & ((stored < s_lo) | ((stored > s_hi) & ~tail))
    E = np.where(tail | zero_ok, np.maximum(stored, s_hi), s_hi)
    tot = eb + e4m3_half_ulp(np.abs(yb) + eb, E[..., None])
    err = np.abs(vb - yb)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tot)
    r = np.where(live, np.where(np.isnan(r) | ~np.isfinite(vb), np.inf, r), 0.0)
    r = _unblocks(r, n, axis)
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    fb = np.argwhere(bad | ragged)
    return {"ratio": float(r[at]), "at": at, "bad_scale": int(bad.sum()), "ragged": int(ragged.sum()), "blocks": int(bad.size),
            "ambiguous": int(((s_hi > s_lo) & ~tail).sum()), "first_bad": tuple(fb[0]) if len(fb) else None, "tot": _unblocks(tot, n, axis)}


# ---- weights and Linears ----------------------------------------------------------------------------------------------------------------
def layer_weights(sd, l):
    """layer l's tensors as the fp8 kernels hold them: GEMM weights dequantize(quantize(W_fp32)) along K, everything else float64"""
    w = el.layer_weights(sd, l, "fp32")
    for k in ("Wqkv", "Wo", "W1", "W2"):
        w[k] = mx_dequant_operand(w[k])
    return w


def linear8_ref(x, W, b):
    """y = x W^T + b in float64 on exact (dequantised) operands, and the bound of the module docstring: ((K + 2) u + MX_MFMA) S"""
    x = np.asarray(x, np.float64)
    K = x.shape[-1]
    y = x @ W.T + b
    S = (np.abs(x).astype(np.float32) @ np.abs(W).T.astype(np.float32)).astype(np.float64) * (1 + 2 * K * U) + np.abs(b)
    return y, ((K + 2) * U + MX_MFMA) * S


def qkv8_ref(h, lw):
    """tap QKV with the fp8 attention core, BEFORE its quantising stores: q / 8 | k | v = h Wqkv^T + b from the layer's exact operand h
    (EPI_QK8: (acc + bias) x 0.125 for the q third -- exact -- then the stores: q, k one scale per (token, 32 features), v one per
    (feature, 32 keys))"""
    y, e = linear8_ref(h, lw["Wqkv"], lw["bqkv"])
    y[..., :HIDDEN] *= 0.125
    e[..., :HIDDEN] *= 0.125
    return y, e


def qkv16_ref(h, lw):
    """tap QKV with SYLBER_OPT_FP8_ATTENTION = -1: the MXFP8 GEMM with the 16-bit EPI_QK epilogue (bf16 q x log2(e) / 8, k, v):
    encoder_layer_ref.qkv_ref's bound with the MXFP8 Linear in place of the 16-bit one"""
    y, e = linear8_ref(h, lw["Wqkv"], lw["bqkv"])
    y[..., :HIDDEN] *= Q_SCALE
    e[..., :HIDDEN] = e[..., :HIDDEN] * Q_SCALE + U * np.abs(y[..., :HIDDEN])
    return y, e + store_error(np.abs(y) + e, "bf16")


# ---- attention --------------------------------------------------------------------------------------------------------------------------
def _merge(x):
    B, H, T, D = x.shape
    return x.transpose(0, 2, 1, 3).reshape(B, T, H * D)


def attention8_parts(qkv, valid, mask=None, score_gain=LOG2E):
    """scores in log2 units s2 [B, H, T, T] (masked keys -inf), A2 = sum_d |q_d| |k_jd| in the same units, v, the key mask.  q carries
    1 / 8; the kernel multiplies by log2(e) inside fma(s, log2 e, -mb).  score_gain 1.0: log2(e) missing (planted defect)"""
    qkv = np.asarray(qkv, np.float64)
    B, T, _ = qkv.shape
    q, k, v = (el._heads(qkv[..., i * HIDDEN:(i + 1) * HIDDEN]) for i in range(3))
    kt = k.transpose(0, 1, 3, 2)
    s = (q @ kt) * score_gain
    A = (np.abs(q) @ np.abs(kt)) * abs(score_gain)
    mask = key_mask(valid, T) if mask is None else mask
    return np.where(mask[:, None, None, :], s, -np.inf), A, v, mask


def ctx8_ref(qkv, valid, mask=None, score_gain=LOG2E, v_perm=None):
    """the attention core on MXFP8 operands, BEFORE its store: base-2 softmax of (q / 8) . k x log2(e) over the keys < min(valid_b, T),
    times v, in float64, from exact operands (tap QKV's values, or the quantised op-level inputs).  Every query row is computed.

    Bound c_i V_id + 2^-16 sum_j |v_jd| with w_j the float64 probabilities, V_id = sum_j w_j |v_jd|, in ctx_ref's shape:
      * the score: 64 exact products accumulated in fp32 by ONE block-scaled MFMA, (64 + 2) u A_j + MX_MFMA A_j in natural units
        (A_j = sum_d |q_d| |k_jd|), times log2(e); then fma(s, log2 e, -mb) with mb = fl(m log2 e) - 7: the constant, the product
        inside mb and the fma, 4 u (|s_j| + |m| + 7) in log2 units with |m| <= max_j |s_j| + P_LAG;
      * p_j = exp2(.): relative ln 2 ds_j + EXP2_ERR; each rescale by alpha = exp2((m_old - m_new) log2 e) is EXP2_ERR + 2 u off plus
        the rounding of its argument, ln 2 x 2 u (2 |m|): R <= keys / 64 rescales, one per 64-key tile; delta_i = the largest sum over
        the valid keys;
      * P to e4m3: the running maximum lags the row's true maximum by at most 2^1, so the row's largest biased p is >= 2^6 (in fact
        2^7 for the key that set the reference; 2^6 is the stated, conservative figure) and <= 2^8 < 448: nothing saturates.  Rounding
        costs 2^-4 relative in e4m3's normal range and, below the biased 2^-6, an ABSOLUTE 2^-10 per key against a row sum >= 2^6:
        2^-16 sum_j |v_jd|.  The row sum l adds the UNROUNDED p (psum in attention_f8_kernel), so numerator and denominator do not
        share the rounding and the full 2^-4 V stays in the bound;
      * the P.V MFMA: exact products (3 + 3 bits), fp32 accumulation over the keys, numerator and denominator, keys rounded up to
        whole 64-key tiles, (2 keys + 6) u with 1 / l and the product; plus MX_MFMA for the block-scaled MFMA's inexact sum.
      c_i = 2 x 1.01 delta_i + 2^-4 + MX_MFMA + (2 keys + 6) u."""
    s, A, v, mask = attention8_parts(qkv, valid, mask, score_gain)
    if v_perm is not None:
        v = v[:, :, v_perm]
    m = s.max(-1, keepdims=True)
    p = np.exp2(s - m)
    w = p / p.sum(-1, keepdims=True)
    ctx = w @ v
    V = w @ np.abs(v)
    nk = mask.sum(1)
    nk64 = ((nk + 63) // 64 * 64).astype(np.float64)[:, None, None]
    sabs = np.where(mask[:, None, None, :], np.abs(s), 0.0)
    mabs = sabs.max(-1, keepdims=True) + P_LAG
    ds = ((HDIM + 2) * U + MX_MFMA) * A + 4 * U * (sabs + mabs + P_BIAS)
    ds = np.where(mask[:, None, None, :], ds, 0.0).max(-1)
    R = nk64 / 64
    delta = math.log(2.0) * ds + EXP2_ERR * (1 + R) + R * (2 * U + math.log(2.0) * 4 * U * mabs[..., 0])
    c = 2 * 1.01 * delta + 2.0 ** -4 + MX_MFMA + (2 * nk64 + 6) * U
    vsum = (np.abs(v) * mask[:, None, :, None]).sum(2, keepdims=True)
    e = c[..., None] * V + 2.0 ** -16 * vsum
    return _merge(ctx), _merge(e), {"s": s, "w": w}


def ctx8_emulated(qkv, valid, mask=None, score_gain=LOG2E, bias=P_BIAS, v_perm=None):
    """what a correct attention_f8_kernel leaves before its store: fp32 probabilities against the row maximum carried as p 2^7, ROUNDED
    to e4m3 for the P.V product and unrounded in the row sum.  ``bias`` 0: P without its bias (planted defect: it flushes)"""
    s, _, v, _ = attention8_parts(qkv, valid, mask, score_gain)
    if v_perm is not None:
        v = v[:, :, v_perm]
    p = f32(np.exp2(s - s.max(-1, keepdims=True) + bias))
    num = e4m3_round(p) @ v
    return f32(_merge(num / f32(p.sum(-1, keepdims=True))))


# ---- the residual GEMMs, the LayerNorms, FFN1 ------------------------------------------------------------------------------------------
def residual_sum8_ref(x, W, b, pre, g, be):
    """taps ATTN_SUM / FFN2_SUM: encoder_layer_ref.residual_sum_ref with the MXFP8 Linear (EPI_F32_RESLN re-derives the residual from
    ``pre`` and the LayerNorm kernel's (mean, rstd) table with that LayerNorm's affine, as in the 16-bit modes)"""
    y, e = linear8_ref(x, W, b)
    ln, eln = layernorm_ref(pre, g, be)
    out = y + ln
    return out, e + eln + U * (np.abs(y) + e + np.abs(out) + e + eln)


def ffn1_8_ref(h, lw):
    """tap FFN1 before its quantising store: gelu_fast(h W1^T + b1) (EPI_MXFP8 with act = 1), as encoder_layer_ref.ffn1_ref"""
    z, ez = linear8_ref(h, lw["W1"], lw["b1"])
    y = gelu64(z)
    return y, GELU_LIP * ez + gelu_error(z, "fast", ez), z


# ---- one layer, stage by stage ------------------------------------------------------------------------------------------------------------
def layer_operand(hin):
    """the q / k / v projection's operand from stage 2 + l (module docstring): exact"""
    return mx_dequant_operand(f32(hin))


def stage_refs(t, lw, valid, stages=STAGES, attn8=True):
    """t: the actual VALUES around one layer -- "pre_prev", "hin" (stage 2 + l, fp32) and the six taps' values by name ->
    {stage: (float64 reference, per-element bound)}; for the QUANT_STAGES the pair is the PRE-quantisation one that
    quant_store_check takes (qkv with attn8 False: a plain bf16 tap, bound complete)"""
    out = {}
    for st in stages:
        if st == "qkv":
            out[st] = qkv8_ref(layer_operand(t["hin"]), lw) if attn8 else qkv16_ref(layer_operand(t["hin"]), lw)
        elif st == "ctx":
            out[st] = ctx8_ref(t["qkv"], valid)[:2] if attn8 else el.ctx_ref(t["qkv"], valid, "bf16")[:2]
        elif st == "attn_sum":
            out[st] = residual_sum8_ref(t["ctx"], lw["Wo"], lw["bo"], t["pre_prev"], lw["prev_g"], lw["prev_b"])
        elif st == "ln1":
            out[st] = layernorm_ref(t["attn_sum"], lw["ln1_g"], lw["ln1_b"])
        elif st == "ffn1":
            out[st] = ffn1_8_ref(t["ln1"], lw)[:2]
        elif st == "ffn2_sum":
            out[st] = residual_sum8_ref(t["ffn1"], lw["W2"], lw["b2"], t["attn_sum"], lw["ln1_g"], lw["ln1_b"])
        else:
            out[st] = layernorm_ref(t["ffn2_sum"], lw["ln2_g"], lw["ln2_b"])
    return out


def quant_axes(st):
    """the block axes of a quantised stage over its [B, T, W] values: [(column slice, axis, open_tail)]"""
    if st == "qkv":
        return [(slice(0, 2 * HIDDEN), -1, False), (slice(2 * HIDDEN, 3 * HIDDEN), 1, True)]
    return [(slice(None), -1, False)]


def check_stage(st, val, ex, ref, bound, attn8=True):
    """one stage of one layer -> (max err / bound, index, scale report): a quantised stage through quant_store_check on each of its
    block axes (report: bad / ragged / ambiguous / all blocks, the first bad one), any other through worst_ratio"""
    if st not in QUANT_STAGES or (st == "qkv" and not attn8):
        r, at = worst_ratio(val, ref, bound)
        return r, at, None
    worst, where = 0.0, None
    rep = {"bad_scale": 0, "ragged": 0, "blocks": 0, "ambiguous": 0, "first_bad": None}
    for cols, axis, tail in quant_axes(st):
        c = quant_store_check(val[..., cols], ex[..., cols], ref[..., cols], bound[..., cols], axis, tail)
        for k in ("bad_scale", "ragged", "blocks", "ambiguous"):
            rep[k] += c[k]
        if rep["first_bad"] is None and c["first_bad"] is not None:
            rep["first_bad"] = (cols.start or 0, axis) + c["first_bad"]
        if c["ratio"] >= worst:
            worst, where = c["ratio"], c["at"][:-1] + (c["at"][-1] + (cols.start or 0),)
    return worst, where, rep


def quant_store(st, y, scale_of=None, **kw):
    """what a correct quantising store of stage st leaves from the fp32 values y: (values, exponents); scale_of / kw: mx_quant's"""
    val, ex = np.empty(y.shape), np.empty(y.shape)
    for cols, axis, _ in quant_axes(st):
        val[..., cols], ex[..., cols] = mx_quant(y[..., cols], axis, None if scale_of is None else scale_of[..., cols], **kw)
    return val, ex


def half_blocks(st, y):
    """y with the second 16 members of every 32-block of stage st zeroed: what a block maximum without the lane ^ 32 exchange sees"""
    out = np.array(y, np.float64)
    for cols, axis, _ in quant_axes(st):
        part = np.moveaxis(out[..., cols], axis, -1)              # (a view: the assignment below lands in ``out``)
        part[..., np.arange(part.shape[-1]) % 32 >= 16] = 0.0
    return out


def emulate_layer(pre_prev, lw, valid):
    """the chain a correct fp8 kernel sequence leaves in the taps, emulated in numpy -> (t values, x exponents, y the fp32 values in
    front of every quantising store): every stage is the float64 reference of the stage before it, rounded to fp32, with the MXFP8
    operand / store quantisation and the e4m3 P applied"""
    t, x, y = {"pre_prev": f32(pre_prev)}, {}, {}
    t["hin"] = f32(layernorm_ref(t["pre_prev"], lw["prev_g"], lw["prev_b"])[0])
    y["qkv"] = f32(qkv8_ref(layer_operand(t["hin"]), lw)[0])
    t["qkv"], x["qkv"] = quant_store("qkv", y["qkv"])
    y["ctx"] = ctx8_emulated(t["qkv"], valid)
    t["ctx"], x["ctx"] = quant_store("ctx", y["ctx"])
    t["attn_sum"] = f32(residual_sum8_ref(t["ctx"], lw["Wo"], lw["bo"], t["pre_prev"], lw["prev_g"], lw["prev_b"])[0])
    y["ln1"] = f32(layernorm_ref(t["attn_sum"], lw["ln1_g"], lw["ln1_b"])[0])
    t["ln1"], x["ln1"] = quant_store("ln1", y["ln1"])
    y["z1"] = f32(linear8_ref(t["ln1"], lw["W1"], lw["b1"])[0])
    y["ffn1"] = f32(el.gelu_fast64(y["z1"]))
    t["ffn1"], x["ffn1"] = quant_store("ffn1", y["ffn1"])
    t["ffn2_sum"] = f32(residual_sum8_ref(t["ffn1"], lw["W2"], lw["b2"], t["attn_sum"], lw["ln1_g"], lw["ln1_b"])[0])
    t["out"] = f32(layernorm_ref(t["ffn2_sum"], lw["ln2_g"], lw["ln2_b"])[0])
    return t, x, y


# ---- designed op-level inputs (sylber_op_attention, precision fp8) -------------------------------------------------------------------------
# (T, valid): ragged, the last valid key inside / at the edge of a 32-key block; the LAST utterance of each is the "flat" one (op_inputs)
OP_SHAPES = ((33, (33, 20, 1, 28)), (65, (65, 40, 33, 50)))
OP_LEAK_V = 1e3                                            # |v| of every masked key
OP_LAST_V = 8.0                                            # the last valid key's distinctive v, against |v| ~ 1 elsewhere
OP_FLAT_GAP = 0.85                                         # the flat utterance's last key: k = kappa + this x the query direction


def op_inputs(T, valid, seed=0):
    """q, k, v [B, T, 768] fp32 for the op-level check, designed so that the defects the layer-level bound is too wide for dwarf it:
      * every masked key j >= valid_b carries k_j = 4 x (the mean query direction of its head) -- aligned with every query, so its
        weight would be among the largest -- and v_j = +-OP_LEAK_V, so ANY leak moves the context by hundreds of bounds (the bound is
        built from the valid keys only);
      * the last valid key carries k = 1 x that direction, i.e. usually the largest weight of its row without silencing the others,
        and v = OP_LAST_V in every feature against unit noise elsewhere, so dropping it (one key too few) moves every element by units;
      * the LAST utterance is flat: all its other valid keys share ONE k (kappa), hence one weight per query, around 2^-12 of the
        last key's (k = kappa + OP_FLAT_GAP x the query direction; 2^-6 to 2^-17 over the queries and heads), and carry positive v
        around 1, while the last key's v is 0 in the upper 32 features of every head.  There the context is the sum of those small
        equal weights: carried as p 2^7 most of them are e4m3 normals (rounded with relative error <= 2^-4 -- equal weights round the
        SAME way, which the bound's worst case covers; the smallest fall under the 2^-16 sum |v| term); without the bias those below
        2^-10 are under half of e4m3's smallest subnormal and flush, all of them at once, and the context there becomes 0 instead of
        sum_j w_j v_j = V: 16 x 2^-4 V, measured 11 bounds."""
    g = np.random.default_rng(1000 * T + seed)
    B = len(valid)
    q = g.standard_normal((B, T, HIDDEN)) + 3.0 * g.standard_normal((B, 1, HIDDEN))      # a strong common direction per head
    k = g.standard_normal((B, T, HIDDEN))
    v = g.standard_normal((B, T, HIDDEN))
    for b, nv in enumerate(valid):
        d = q[b].mean(0)
        d = (d.reshape(HEADS, HDIM) / np.abs(d.reshape(HEADS, HDIM)).max(-1, keepdims=True)).reshape(HIDDEN)
        k[b, nv - 1] = 1.0 * d
        v[b, nv - 1] = OP_LAST_V
        if b == B - 1:
            k[b, :nv - 1] = k[b, 0]
            k[b, nv - 1] = k[b, 0] + OP_FLAT_GAP * d
            v[b, :nv - 1] = 1.0 + 0.25 * g.random((nv - 1, HIDDEN))
            v[b, nv - 1, np.arange(HIDDEN) % HDIM >= 32] = 0.0
        k[b, nv:] = 4.0 * d
        v[b, nv:] = OP_LEAK_V * np.where(g.random((T - nv, HIDDEN)) < 0.5, -1.0, 1.0)
    return q.astype(np.float32), k.astype(np.float32), v.astype(np.float32)


def op_operands(q, k, v, valid):
    """what sylber_op_attention(precision fp8) quantises its inputs to (pack_qk_f8_kernel / pack_vt_f8_kernel): q / 8 and k per
    (token, 32 features), v per (feature, 32 keys) over ALL T keys, the masked ones included -> q | k | v [B, T, 2304], exact"""
    q8 = mx_dequant_operand(f32(q) * 0.125)
    return np.concatenate([q8, mx_dequant_operand(k), mx_dequant_operand(v, axis=1)], -1)


def op_ctx_ref(qkv, valid, **kw):
    """the op-level context (stored as bf16, not quantised): ctx8_ref's bound and the bf16 store"""
    ctx, e, aux = ctx8_ref(qkv, valid, **kw)
    return ctx, e + store_error(np.abs(ctx) + e, "bf16"), aux


# The CPU tier's inputs, one seed per shape of encoder_layer_ref.SHAPES.  The seeds are CHOSEN, not arbitrary: the context's bound carries
# the full 2^-4 of the e4m3 P relative to sum_j w_j |v_j| >= |ctx|, so its block maximum is known to a (1 -+ 2^-4) at best -- 0.18
# octaves against one scale threshold per octave.  The synthetic checkpoint's softmax is nearly flat, so an utterance's context rows
# are all close to the mean of v and the block maxima of one (utterance, head, half) column sit together: whether a column straddles a
# threshold is decided once per column, and the share of blocks that admit two scale bytes swings with the seed (measured over seeds
# 0 .. 5 at these shapes: 0 - 38 %, 20 - 35 % at T = 385; 18 % or more is what evenly spread maxima would give).  The cap of
# AMBIGUOUS_CAP is a condition on the REFERENCE's inputs -- with more blocks ambiguous the exact-byte check means little -- and is met
# by taking, per shape, a seed under which the context stays below it (the other stages are at 0 - 2.1 % under any seed tried).
PRE_SEEDS = {1: 0, 17: 2, 33: 0, 64: 5, 65: 2, 257: 2, 385: 24}


def pre_input(T, valid):
    return el.pre_input(T, valid, PRE_SEEDS[T])

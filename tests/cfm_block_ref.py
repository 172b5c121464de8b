"""Test-only float64 references of the resynthesis decoder (csrc/cfm.hip), launch by launch, and per-element error bounds derived from
the arithmetic of the kernel behind each launch.  In the style of tests/encoder_layer_ref.py, whose attention reference (the decoder
runs the encoder's attention kernels) and notation (u, h(fmt), q(fmt), tests/frontend_ref.py) are reused; plain numpy, written from the
published algorithm (the flow-matching Regressor restated in tests/cfm_ref.py); never imported by ``sylber_amd``.

Every stage is computed FROM THE ACTUAL VALUES OF THE TAP IN FRONT OF IT (sylber_cfm_set_tap, include/sylber_hip_dev.h): a tap returns a
buffer in storage order, 16-bit words widened exactly, so its values are exact operands of the next launch and a comparison tests one
kernel with a bound that holds that kernel's arithmetic only -- which stays well conditioned at a trained checkpoint's logit scale,
where the decoder's output as a whole is not.  The references apply the documented layouts themselves (the 12-head layout with heads
8..11 zero, V^T with key bits 2 and 3 swapped, W1 packed [value 1408 | gate 1408], the packed slots), so a layout bug cannot hide.

Weights are taken from the state dict the way sylber_cfm_create packs them (``pack_weights``).  The fold of proj_in into to_embed is
computed by the library in double and rounded to fp32 once: the reference keeps the float64 fold and the bounds charge that rounding
(u per folded weight).

Device math functions.  No maximum-ulp table for the device library is installed with the toolchain, so the constants are MEASURED, by
tools/ubench/devmath_err.hip: every fp32 argument of the stated range against the float64 function of the same argument; each
constant is twice the largest error seen (in units of u = 2^-24):
    ERFF_ERR    erff, |x| < 16             measured 1.4587 u absolute (at x = -0.96661)     cfm_gelu: the conv and the GEGLU
    SINCOS_ERR  sinf / cosf, |x| < 16384   measured 1.2008 u / 1.1963 u absolute (x = -25.927 / -2.3597)   rotary angles down to -10000 rad, the time embedding
    EXPF_ERR    expf, |x| < 64             measured 1.4108 u relative (at x = -42.932)      the SiLU of the time conditioning
Division and square root are correctly rounded (hipcc's default); the bounds allow 2 u for each anyway."""
import math

import numpy as np

import encoder_layer_ref as el
from frontend_ref import GELU_LIP, U, gelu64, round_fmt, store_error, worst_ratio  # noqa: F401

D, HEADS, REG, OUT, COND, FI, FIP, KW, DEPTH, TH = 512, 8, 16, 14, 256, 1365, 1408, 31, 8, 2048
SC = math.sqrt(512.0)
C10 = float(np.float32(10.0) * np.float32(1.4426950408889634))      # cfm_qkprep's 10.0f * CFM_LOG2E, an fp32 product
# MEAS_*: the largest error itself, as measured on an MI355X by tools/ubench/devmath_err.hip over every fp32 argument of the range
# (module docstring), in units of u.  *_ERR: what the bounds use, twice that.
MEAS_ERFF, MEAS_SIN, MEAS_COS, MEAS_EXP = 1.4587, 1.2008, 1.1963, 1.4108
ERFF_ERR = 2 * MEAS_ERFF * U
SINCOS_ERR = 2 * max(MEAS_SIN, MEAS_COS) * U
EXPF_ERR = 2 * MEAS_EXP * U

FRONT = ("condx", "xe", "x0")
BLOCK16 = ("h_attn", "qkv", "q", "k", "vt", "ctx", "x_attn", "h_ff", "ff", "g", "x_ff")
BLOCK32 = ("h_attn", "qkv", "qkvf", "ctx", "x_attn", "h_ff", "ff", "g", "x_ff")
LONE_T = (1, 15, 16, 17, 47, 48, 49, 111, 112, 113)
RAGGED = (113, 48, 1)


def block_stages(fmt):
    return BLOCK32 if fmt == "fp32" else BLOCK16


# ---- weights as sylber_cfm_create packs them ----------------------------------------------------------------------------------------
def pack_weights(sd, fmt):
    """GEMM operands round_fmt'ed (once, at load time: H16<FMT>::cvt, fp16 saturating), everything else float64"""
    def f(name):
        return sd[name].detach().double().numpy()
    E, Pw, Pb = f("to_embed.weight"), f("proj_in.weight"), f("proj_in.bias")
    W = {"wy": E[:, :64] @ Pw, "by": f("to_embed.bias") + E[:, :64] @ Pb, "wc": round_fmt(E[:, 64:64 + COND], fmt),
         "t_w": sd["sinu_pos_emb.0.weights"].detach().float().numpy(), "t1_w": f("sinu_pos_emb.1.weight"), "t1_b": f("sinu_pos_emb.1.bias"),
         "conv_w": f("conv_embed.dw_conv1d.0.weight").reshape(D, KW), "conv_b": f("conv_embed.dw_conv1d.0.bias"),
         "reg": f("transformer.register_tokens"), "inv_freq": sd["transformer.rotary_emb.inv_freq"].detach().float().numpy(),
         "fin_g": f("transformer.final_norm.gamma"), "pred_w": f("to_pred.weight")}
    gbw, gbb = np.zeros((2 * DEPTH, 2, D, TH)), np.zeros((2 * DEPTH, 2, D))
    for k in ("qg", "kg", "wqkv", "wo", "w1", "b1", "w2", "b2"):
        W[k] = []
    for i in range(DEPTH):
        p = "transformer.layers.%d." % i
        for j, m in enumerate(("2", "4")):
            gbw[2 * i + j, 0], gbb[2 * i + j, 0] = f(p + m + ".to_gamma.weight"), f(p + m + ".to_gamma.bias")
            gbw[2 * i + j, 1], gbb[2 * i + j, 1] = f(p + m + ".to_beta.weight"), f(p + m + ".to_beta.bias")
        W["qg"].append(f(p + "3.q_norm.gamma").reshape(HEADS, 64))
        W["kg"].append(f(p + "3.k_norm.gamma").reshape(HEADS, 64))
        W["wqkv"].append(round_fmt(f(p + "3.to_qkv.weight"), fmt))
        W["wo"].append(round_fmt(f(p + "3.to_out.weight"), fmt))
        w1, b1 = f(p + "5.0.weight"), f(p + "5.0.bias")
        w1p, b1p = np.zeros((2 * FIP, D)), np.zeros(2 * FIP)
        w1p[:FI], w1p[FIP:FIP + FI], b1p[:FI], b1p[FIP:FIP + FI] = w1[:FI], w1[FI:], b1[:FI], b1[FI:]       # [value | gate], zero rows pad
        W["w1"].append(round_fmt(w1p, fmt))
        W["b1"].append(b1p)
        w2p = np.zeros((D, FIP))
        w2p[:, :FI] = f(p + "5.3.weight")
        W["w2"].append(round_fmt(w2p, fmt))
        W["b2"].append(f(p + "5.3.bias"))
    W["gbw"], W["gbb"] = gbw, gbb
    return W


# ---- geometry: where a clip's rows sit in a tap -------------------------------------------------------------------------------------
class Geom:
    """frames: each clip's own frame count.  mode "padded": one [B, T] call, every row T = max frames ordinary frames; "frames": the
    same call with frames= (row b ends at frames[b]); "packed": slots of round_up(16 + Tb, 64) rows in one pseudo-utterance.
    Per clip b: R rows of the x-side buffers (Rv keys of V^T), Tb frames the conv treats as the clip, nv keys, Lq rows cfm_qkprep
    writes, Lw rows the attention writes, Trow frame rows of cond / xe / the state."""

    def __init__(self, frames, mode="padded"):
        self.mode, self.B = mode, len(frames)
        T = max(frames)
        self.T, self.L = T, REG + T
        self.clips = []
        if mode == "packed":
            off = foff = 0
            for Tb in frames:
                R = (REG + Tb + 63) // 64 * 64
                self.clips.append(dict(R=R, Rv=R, Tb=Tb, nv=REG + Tb, Lq=R, Lw=REG + Tb, Trow=Tb, x0=off, f0=foff))
                off, foff = off + R, foff + Tb
            self.M, self.NF, self.Tp, self.Tpv = off, foff, off, off
        else:
            self.Tp = (self.L + 31) // 32 * 32
            self.Tpv = (self.Tp + 63) // 64 * 64
            for b, Tb in enumerate(frames):
                own = Tb if mode == "frames" else T
                self.clips.append(dict(R=self.Tp, Rv=self.Tpv, Tb=own, nv=REG + own, Lq=self.L, Lw=self.L, Trow=T, x0=b * self.Tp, f0=b * T))
            self.M, self.NF = self.B * self.Tp, self.B * T

    def split(self, stage, tap):
        """a tap (flat, storage order) -> one array per clip: [R, W] rows, [Trow, W] frame rows, [12, R, 64] (q, k), [12, 64, Rv] (vt)"""
        tap = np.asarray(tap)
        pk = self.mode == "packed"
        if stage in ("condx", "xe", "cond", "y", "final"):
            a = tap.reshape(self.NF, -1)
            return [a[c["f0"]:c["f0"] + c["Trow"]] for c in self.clips]
        if stage in ("q", "k"):
            a = tap.reshape(1 if pk else self.B, 12, self.Tp, 64)
            return [a[0, :, c["x0"]:c["x0"] + c["R"]] if pk else a[b] for b, c in enumerate(self.clips)]
        if stage == "vt":
            a = tap.reshape(1 if pk else self.B, 12, 64, self.Tpv)
            return [a[0, :, :, c["x0"]:c["x0"] + c["R"]] if pk else a[b] for b, c in enumerate(self.clips)]
        a = tap.reshape(self.M, -1)
        return [a[c["x0"]:c["x0"] + c["R"]] for c in self.clips]


# ---- time conditioning -----------------------------------------------------------------------------------------------------------------
def gb_ref(W, t, fp32_arg=True):
    """the 16 x (gamma, beta) vectors of time t [16, 2, 512] and their bound.  cfm_time_hidden: the embedding's argument
    fl(fl(fl(t w) 2) pi) restated in fp32, sinf / cosf of it (SINCOS_ERR absolute), a 512-term fmaf chain + bias (513 u S, plus the
    embedding's error through |w|), SiLU a / (1 + expf(-a)): |silu'| <= 1.1 on the argument's error, the denominator's exponential
    EXPF_ERR relative, the add and the division 3 u.  cfm_time_gb: 32 fmaf per lane, six levels of the wave sum, the bias: 40 u S,
    plus the hidden vector's error through |w|.  fp32_arg False: the argument in float64 (tests/cfm_ref.py in float64 forms it so)."""
    f = ((np.float32(t) * W["t_w"]) * np.float32(2.0)) * np.float32(math.pi)
    f = f.astype(np.float64) if fp32_arg else float(t) * W["t_w"].astype(np.float64) * 2 * math.pi
    emb = np.concatenate([np.sin(f), np.cos(f)])
    a = W["t1_w"] @ emb + W["t1_b"]
    ea = 513 * U * (np.abs(W["t1_w"]) @ np.abs(emb) + np.abs(W["t1_b"])) + SINCOS_ERR * np.abs(W["t1_w"]).sum(1)
    h = a / (1 + np.exp(-a))
    eh = 1.1 * ea + np.abs(h) * (EXPF_ERR + 3 * U)
    gb = W["gbw"] @ h + W["gbb"]
    e = 40 * U * (np.abs(W["gbw"]) @ np.abs(h) + np.abs(W["gbb"])) + np.abs(W["gbw"]) @ eh
    return gb, e


# ---- the front: cond GEMM, embed, conv ------------------------------------------------------------------------------------------------
def condx_ref(cond, W, fmt):
    """CONDX = round_fmt(cond) Wc^T + by (the folded bias): el.linear_ref's bound, plus the fold's own rounding of by (u)"""
    y, e = el.linear_ref(round_fmt(cond, fmt), W["wc"], W["by"], fmt)
    return y, e + U * np.abs(W["by"])


def xe_ref(condx, y, W):
    """XE = CONDX + Wy y: a 14-term fmaf chain from 0 (14 u A, A = sum |wy| |y|), the fold's rounding of Wy (u A), the add (u)"""
    y = np.asarray(y, np.float64)
    acc, A = y @ W["wy"].T, np.abs(y) @ np.abs(W["wy"]).T
    out = np.asarray(condx, np.float64) + acc
    e = 15 * U * A
    return out, e + U * (np.abs(out) + e)


def gelu_erff_error(z):
    """cfm_gelu = 0.5 x (1 + erff(x c)), c = fl(1 / sqrt 2): the argument is 2 u relative off, |z erf'(z)| <= 0.484, so erf moves by
    less than u; erff itself ERFF_ERR; 1 + erf rounds by at most 2 u; the products u each: 0.5 |x| (ERFF_ERR + 3 u) + u |gelu|"""
    return 0.5 * np.abs(z) * (ERFF_ERR + 3 * U) + U * np.abs(gelu64(z))


def x0_ref(xe, W, c, shift=0, pad_at=None, swap_reg=False):
    """X0 of one clip [R, 512]: the 16 register rows (bit for bit), gelu(depthwise conv31(xe) + bias) + xe on its Tb frames (zero
    padding at both ends of the CLIP, not of the row), +0 rows behind.  Bound: the fmaf chain from the bias, one rounding per tap that
    lies inside the clip (<= 31 u S, S = |b| + sum |w| |x|), through the GELU (Lipschitz < 1.13) plus gelu_erff_error, the add (u).
    ``shift`` / ``pad_at`` / ``swap_reg``: planted defects (the window moved, the padding taken at pad_at frames, two registers exchanged)."""
    xe = np.asarray(xe, np.float64)
    Tb = c["Tb"]
    n = Tb if pad_at is None else pad_at
    xp = np.zeros((Tb + 2 * KW, D))
    m = min(n, Tb + KW)
    xp[KW:KW + m] = xe[:m]
    acc, S = np.tile(W["conv_b"], (Tb, 1)), np.tile(np.abs(W["conv_b"]), (Tb, 1))
    for k in range(KW):
        win = xp[KW - KW // 2 + k + shift:KW - KW // 2 + k + shift + Tb]
        acc += win * W["conv_w"][:, k]
        S += np.abs(win) * np.abs(W["conv_w"][:, k])
    ez = KW * U * S
    y = gelu64(acc) + xe[:Tb]
    e = GELU_LIP * ez + gelu_erff_error(acc)
    e = e + U * (np.abs(y) + e)
    out, eo = np.zeros((c["R"], D)), np.zeros((c["R"], D))
    out[:REG] = W["reg"] if not swap_reg else W["reg"][[1, 0] + list(range(2, REG))]
    out[REG:REG + Tb], eo[REG:REG + Tb] = y, e
    return out, eo


# ---- AdaRMSNorm ------------------------------------------------------------------------------------------------------------------------
def norm_ref(x, gamma, beta, fmt, count=D):
    """cfm_adanorm: F.normalize(x) sqrt(512) gamma + beta, stored in the format.  ss = sum x^2: 8 fmaf per lane and six levels of the wave
    sum (15 u relative, all terms positive); sqrt halves it and rounds (<= 9 u), the reciprocal 2 u: the scale is 11 u off; x inv, times
    fl(sqrt 512) (the constant's own rounding u), times gamma: 4 u more -> 15 u on the gamma term; the add of beta u of the result; the
    store.  A zero row gives beta exactly (1 / max(0, 1e-12) times 0).  ``count``: RMS over the first count elements (planted defect)."""
    x = np.asarray(x, np.float64)
    nrm = np.maximum(np.sqrt((x[..., :count] ** 2).sum(-1, keepdims=True)), 1e-12)
    g = x / nrm * SC * gamma
    y = g if beta is None else g + beta
    e = 16 * U * np.abs(g) + U * np.abs(y)
    return y, e + store_error(np.abs(y) + e, fmt)


# ---- q / k norm, rotary, the attention operands --------------------------------------------------------------------------------------
def rotary_angles(c, W, pos_shift=0, reg_pos=-10000.0):
    """fp32 angles pos inv_freq [R, 32] as the kernel forms them (one fp32 product), then float64"""
    r = np.arange(c["R"])
    pos = np.where(r < REG, np.float32(reg_pos), (r - REG).astype(np.float32)) + np.float32(pos_shift)
    return (pos.astype(np.float32)[:, None] * W["inv_freq"][None, :]).astype(np.float64)


def qk_ref(qkv, W, li, fmt, c, pos_shift=0, reg_pos=-10000.0, adjacent=False, sin_sign=1.0, qscale=None, head_shift=0, vt_perm="once"):
    """tap QKV [R, 1536] -> {"q", "k": [12, R, 64], "vt": [12, 64, Rv]} (16-bit modes) or {"qkvf": [R, 2304]} (fp32), each (ref, bound).
    Rows at or past Lq are not written (+0, bound 0), heads 8..11 are +0.
    Per (row, head): the sum of 64 squares over the wave (7 u), sqrt (<= 5 u), reciprocal (2 u), times the value, gamma and 8: the
    normalised value a is 12 u off; cos / sin of the fp32 angle SINCOS_ERR absolute; two products and one add: 2 u of |a cos| + |a' sin|:
        e_r = 14 u (|a cos| + |a' sin|) + SINCOS_ERR (|a| + |a'|)
    q times fl(10 log2 e) (16-bit) or 80 (fp32): u more; the store.  V^T is the store of v alone, at key p(r) (bits 2 and 3 swapped)."""
    qkv = np.asarray(qkv, np.float64)
    R, Lq = c["R"], c["Lq"]
    ang = rotary_angles(c, W, pos_shift, reg_pos)
    cs, sn = np.cos(ang), sin_sign * np.sin(ang)

    def rot(x, gam):
        x = x.reshape(R, HEADS, 64)
        nrm = np.maximum(np.sqrt((x ** 2).sum(-1, keepdims=True)), 1e-12)
        a = x / nrm * np.roll(gam, -head_shift, axis=0)[None] * 8.0
        if adjacent:       # pairs (2 i, 2 i + 1) with angle i
            ev, od = a[..., 0::2], a[..., 1::2]
            out = np.empty_like(a)
            out[..., 0::2], out[..., 1::2] = ev * cs[:, None] - od * sn[:, None], od * cs[:, None] + ev * sn[:, None]
            return out, np.zeros_like(a)
        lo, hi = a[..., :32], a[..., 32:]
        out = np.concatenate([lo * cs[:, None] - hi * sn[:, None], hi * cs[:, None] + lo * sn[:, None]], -1)
        mag = np.abs(lo * cs[:, None]) + np.abs(hi * sn[:, None])
        mag2 = np.abs(hi * cs[:, None]) + np.abs(lo * sn[:, None])
        tot = np.abs(lo) + np.abs(hi)
        e = 14 * U * np.concatenate([mag, mag2], -1) + SINCOS_ERR * np.concatenate([tot, tot], -1)
        return out, e
    q, eq = rot(qkv[:, :D], W["qg"][li])
    k, ek = rot(qkv[:, D:2 * D], W["kg"][li])
    v = qkv[:, 2 * D:].reshape(R, HEADS, 64)
    live = (np.arange(R) < Lq)[:, None, None]
    qs = (80.0 if fmt == "fp32" else C10) if qscale is None else qscale
    q, eq = q * qs, eq * abs(qs) + U * np.abs(q * qs)
    q, eq, k, ek, v = q * live, eq * live, k * live, ek * live, v * live
    if fmt == "fp32":
        y, e = np.zeros((R, 3, 12, 64)), np.zeros((R, 3, 12, 64))
        y[:, 0, :HEADS], y[:, 1, :HEADS], y[:, 2, :HEADS] = q, k, v
        e[:, 0, :HEADS], e[:, 1, :HEADS] = eq, ek
        return {"qkvf": (y.reshape(R, 2304), e.reshape(R, 2304))}
    out = {}
    for name, y, e in (("q", q, eq), ("k", k, ek)):
        y12, e12 = np.zeros((12, R, 64)), np.zeros((12, R, 64))
        y12[:HEADS], e12[:HEADS] = y.transpose(1, 0, 2), e.transpose(1, 0, 2)
        out[name] = (y12, e12 + store_error(np.abs(y12) + e12, fmt))
    perm = el.vt_key_permutation(R)
    dst = {"once": perm, "none": np.arange(R), "twice": perm[perm]}[vt_perm]
    vt = np.zeros((12, 64, c["Rv"]))
    vt[:HEADS, :, dst] = v.transpose(1, 2, 0)
    out["vt"] = (vt, store_error(np.abs(vt), fmt))
    return out


def qkv_of_taps(t, fmt, c):
    """the attention's operands as el.ctx_ref takes them, [1, R, 2304], from the taps in storage order: the reference undoes V^T's
    documented key permutation itself"""
    if fmt == "fp32":
        return np.asarray(t["qkvf"], np.float64)[None]
    R = c["R"]
    perm = el.vt_key_permutation(R)
    q = np.asarray(t["q"], np.float64).transpose(1, 0, 2).reshape(R, 768)
    k = np.asarray(t["k"], np.float64).transpose(1, 0, 2).reshape(R, 768)
    v = np.asarray(t["vt"], np.float64)[:, :, perm].transpose(2, 0, 1).reshape(R, 768)
    return np.concatenate([q, k, v], -1)[None]


def ctx_ref(t, fmt, c, nv=None, mask=None, swap_heads=False, v_perm=None):
    """tap CTX [R, 768] of one clip from its Q / K / V^T (or QKVF) taps: el.ctx_ref over the keys < nv, every row below Lw; the rows at
    or past Lw are +0 (padded: never written; packed: zeroed by the kernel) with bound 0, and so are heads 8..11 (zero operands)"""
    y, e, aux = el.ctx_ref(qkv_of_taps(t, fmt, c), [c["nv"] if nv is None else nv], fmt, mask=mask, v_perm=v_perm)
    y, e = y[0].copy(), e[0].copy()
    y[c["Lw"]:], e[c["Lw"]:] = 0.0, 0.0
    if swap_heads:
        y[:, :128] = np.concatenate([y[:, 64:128], y[:, :64]], -1)
    return y, e, aux


# ---- the GEMMs, GEGLU, the final launch -------------------------------------------------------------------------------------------------
def res_ref(a, Wm, bias, x, fmt, gain=1.0):
    """taps X_ATTN / X_FF: x + a W^T (+ bias), EPI_F32_RES in place: el.linear_ref's bound and the fp32 add (u of both sides).
    ``gain``: the residual added twice (2) or not at all (0), planted defects"""
    K = Wm.shape[1]
    y, e = el.linear_ref(np.asarray(a, np.float64)[:, :K], Wm, np.zeros(Wm.shape[0]) if bias is None else bias, fmt)
    out = y + gain * np.asarray(x, np.float64)
    return out, e + U * (np.abs(y) + np.abs(out) + 2 * e)


def geglu_ref(ff, fmt, on_value=False):
    """tap G [R, 1408] = gelu(gate) value from tap FF [value 1408 | gate 1408]: gelu_erff_error times |value|, the product (u), the
    store; the packed zero columns 1365.. give +0 with bound 0"""
    ff = np.asarray(ff, np.float64)
    val, gate = ff[:, :FIP], ff[:, FIP:]
    if on_value:
        val, gate = gate, val
    y = gelu64(gate) * val
    e = np.abs(val) * gelu_erff_error(gate) + U * np.abs(y)
    return y, e + store_error(np.abs(y) + e, fmt)


def final_ref(x, W, c, no_gamma=False, swap_rows=False):
    """the call's output [Tb, 14] from X_FF of block 7: RMSNorm of the frame rows (norm_ref's 16 u on each v_j), to_pred by 8 fmaf per
    lane and the wave sum (15 u): 31 u sum |w| |v|"""
    x = np.asarray(x, np.float64)[REG:REG + c["Tb"]]
    v = x / np.maximum(np.sqrt((x ** 2).sum(-1, keepdims=True)), 1e-12) * SC * (1.0 if no_gamma else W["fin_g"])
    wp = W["pred_w"] if not swap_rows else W["pred_w"][[1, 0] + list(range(2, OUT))]
    return v @ wp.T, 31 * U * (np.abs(v) @ np.abs(wp).T)


# ---- one clip, stage by stage ------------------------------------------------------------------------------------------------------------
def stage_refs(t, W, c, li, fmt, stages, gb=None):
    """t: one clip's actual values by name -- "cond", "y" (inputs), the taps, "x_in" (X0, or X_FF of block li - 1) and "gb" (the GB tap)
    -> {stage: (float64 reference, bound)}, every stage from the tap in front of it"""
    gb = t["gb"] if gb is None else gb
    out = {}
    for st in stages:
        if st == "condx":
            out[st] = condx_ref(t["cond"], W, fmt)
        elif st == "xe":
            out[st] = xe_ref(t["condx"], t["y"], W)
        elif st == "x0":
            out[st] = x0_ref(t["xe"], W, c)
        elif st == "h_attn":
            out[st] = norm_ref(t["x_in"], gb[2 * li, 0], gb[2 * li, 1], fmt)
        elif st == "qkv":
            out[st] = el.linear_ref(t["h_attn"], W["wqkv"][li], np.zeros(3 * D), fmt)
        elif st in ("q", "k", "vt", "qkvf"):
            if st not in out:
                out.update(qk_ref(t["qkv"], W, li, fmt, c))
        elif st == "ctx":
            out[st] = ctx_ref(t, fmt, c)[:2]
        elif st == "x_attn":
            out[st] = res_ref(t["ctx"], W["wo"][li], None, t["x_in"], fmt)
        elif st == "h_ff":
            out[st] = norm_ref(t["x_attn"], gb[2 * li + 1, 0], gb[2 * li + 1, 1], fmt)
        elif st == "ff":
            out[st] = el.linear_ref(t["h_ff"], W["w1"][li], W["b1"][li], fmt)
        elif st == "g":
            out[st] = geglu_ref(t["ff"], fmt)
        elif st == "x_ff":
            out[st] = res_ref(t["g"], W["w2"][li], W["b2"][li], t["x_attn"], fmt)
        elif st == "final":
            out[st] = final_ref(t["x_ff"], W, c)
        else:
            raise KeyError(st)
    return out


f32 = el.f32


def clip(T):
    """seeded (cond [T, 256], y [T, 14]) of a T-frame clip, fp32 (tests/test_gpu_decoder_ref.py's _clip)"""
    import torch
    g = torch.Generator().manual_seed(1000 + T)
    return torch.randn(T, 256, generator=g), 0.7 * torch.randn(T, 14, generator=g)


def padded(Ts):
    """the clips zero-padded to the longest: (cond [B, T, 256], y [B, T, 14])"""
    import torch
    Tm = max(Ts)
    cond, y = torch.zeros(len(Ts), Tm, 256), torch.zeros(len(Ts), Tm, 14)
    for b, T in enumerate(Ts):
        cond[b, :T], y[b, :T] = clip(T)
    return cond, y


def with_qk_gamma(sd, gamma):
    """the state dict with every q_norm / k_norm gamma set to ``gamma`` (upstream initialises them to ones: the trained scale)"""
    out = dict(sd)
    for k in sd:
        if k.endswith(("3.q_norm.gamma", "3.k_norm.gamma")):
            out[k] = sd[k] * 0 + gamma
    return out


def emulate_clip(cond, y, W, c, li, fmt, gb, x_in=None, upto_qk=False):
    """the chain a correct kernel sequence leaves in one clip's taps: every stage is the float64 reference of the stage before it with the
    store of its buffer applied (fp32, or round_fmt for the 16-bit buffers; inside the attention, el.ctx_emulated's P rounding).  x_in:
    start at block li from this residual stream instead of the front; upto_qk: stop behind cfm_qkprep (the long clip)"""
    t = {"cond": np.asarray(cond, np.float64), "y": np.asarray(y, np.float64), "gb": f32(gb)}
    if x_in is None:
        t["condx"] = f32(condx_ref(t["cond"], W, fmt)[0])
        t["xe"] = f32(xe_ref(t["condx"], t["y"], W)[0])
        t["x0"] = f32(x0_ref(t["xe"], W, c)[0])
        t["x_in"] = t["x0"]
    else:
        t["x_in"] = f32(x_in)
    g = t["gb"]
    t["h_attn"] = round_fmt(norm_ref(t["x_in"], g[2 * li, 0], g[2 * li, 1], fmt)[0], fmt)
    t["qkv"] = f32(el.linear_ref(t["h_attn"], W["wqkv"][li], np.zeros(3 * D), fmt)[0])
    for k, (v, _) in qk_ref(t["qkv"], W, li, fmt, c).items():
        t[k] = round_fmt(v, fmt)
    if upto_qk:
        return t
    ctx = el.ctx_emulated(qkv_of_taps(t, fmt, c), [c["nv"]], fmt)[0]
    ctx[c["Lw"]:] = 0.0
    t["ctx"] = ctx
    t["x_attn"] = f32(res_ref(t["ctx"], W["wo"][li], None, t["x_in"], fmt)[0])
    t["h_ff"] = round_fmt(norm_ref(t["x_attn"], g[2 * li + 1, 0], g[2 * li + 1, 1], fmt)[0], fmt)
    t["ff"] = f32(el.linear_ref(t["h_ff"], W["w1"][li], W["b1"][li], fmt)[0])
    t["g"] = round_fmt(geglu_ref(t["ff"], fmt)[0], fmt)
    t["x_ff"] = f32(res_ref(t["g"], W["w2"][li], W["b2"][li], t["x_attn"], fmt)[0])
    t["final"] = f32(final_ref(t["x_ff"], W, c)[0])
    return t

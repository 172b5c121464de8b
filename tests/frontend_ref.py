"""Test-only float64 references of the encoder's front half, and per-element error bounds DERIVED from the arithmetic of the
kernels that compute it (csrc/frontend.hip, the EPI_PROJ GEMM, csrc/posconv.hip).  Plain numpy / torch-double, written from the
published algorithm (transformers' HubertModel, restated in oracle/hubert_ref.py); never imported by ``sylber_amd``.

Formats (``fmt``): "bf16", "fp16", "split16" (a pair of IEEE halves hi = half(x), lo = half(x - hi)) and "fp32".  ``round_fmt``
is what a kernel's store of an fp32 value leaves in a buffer of that format, widened back.

Notation in the bounds: u = 2^-24 (fp32 unit roundoff); h(fmt) = the largest RELATIVE rounding error of a stored value, half an ulp
at the bottom of a binade: 2^-8 (bf16, 8 significand bits), 2^-11 (fp16, 11 bits), 2^-22 (split16: 11 + 11 bits), 0 (fp32); q(fmt)
= 2^-25, half the subnormal quantum of IEEE half, for fp16 and split16 (a value below 2^-14 is stored on a 2^-24 grid), else 0.
(Relative to the value the half-ulp of bf16 runs from 2^-9 at the top of a binade to 2^-8 at its bottom; where a bound is taken at
one result, store_error uses the exact half-ulp of that result's binade, not the relative form.)  Every bound is an upper bound
on |kernel - reference| that no correct implementation of the documented arithmetic can exceed; none is fitted to a measurement."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS = 1e-5
GELU_LIP = 1.13                      # max |gelu'| = 1.1289 (at x = sqrt 2)
HALF_ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "split16": 2.0 ** -22, "fp32": 0.0}
SIG_BITS = {"bf16": 8, "fp16": 11}
SUB_Q = {"bf16": 0.0, "fp16": 2.0 ** -25, "split16": 2.0 ** -25, "fp32": 0.0}
POS_K, POS_G, POS_C = 128, 16, 48


# ---- formats ------------------------------------------------------------------------------------------------------------------
def _bf16(x32):
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def _half(x32):
    return np.clip(np.asarray(x32, np.float32), -65504.0, 65504.0).astype(np.float16).astype(np.float32)


def round_fmt(x, fmt):
    """float64 array -> the value a store of fp32(x) in ``fmt`` holds, as float64"""
    x32 = np.asarray(x, dtype=np.float64).astype(np.float32)
    if fmt == "fp32":
        return x32.astype(np.float64)
    if fmt == "bf16":
        return _bf16(x32).astype(np.float64)
    hi = _half(x32)
    if fmt == "fp16":
        return hi.astype(np.float64)
    assert fmt == "split16", fmt
    lo = _half(x32 - hi)
    return hi.astype(np.float64) + lo.astype(np.float64)


def gelu64(z):
    """exact erf GELU in float64"""
    t = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64))
    return (0.5 * t * (1.0 + torch.erf(t * (1.0 / math.sqrt(2.0))))).numpy()


def gelu_error(z, kind, dz=0.0):
    """|kernel GELU(t) - gelu(t)| for any fp32 argument t with |t - z| <= dz, from the errors csrc/common.h states:
    "fast"  gelu_fast: 6.4e-5 on the polynomial's core |t| <= 4.2; beyond, Phi is frozen at Phi(+-4.2) = 1 - 2.7e-5 / 2.7e-5, so the
            error is at most 2.7e-5 |t|.  Where [|z| - dz, |z| + dz] straddles 4.2, the larger of the two;
    "erf7"  gelu_erf7: erf by A&S 7.1.26, |error| <= 1.5e-7, evaluated with a hardware reciprocal and exp2 (1 ulp each) and 8 fp32
            operations: 16 u on erf; gelu = t/2 (1 + erf), so t/2 times that, plus 2 u |t| for the last fma and the halving;
    "erf"   gelu_erf: erff to 4 ulp of 1 (4 u), t/2 times that, plus 2 u |t|."""
    az = np.abs(z)
    lo, hi = az - dz, az + dz
    if kind == "fast":
        e = np.where(hi <= 4.2, 6.4e-5, np.where(lo > 4.2, 2.7e-5 * hi, np.maximum(6.4e-5, 2.7e-5 * hi)))
        return e + 2 * U * hi
    e = {"erf7": 1.5e-7 + 16 * U, "erf": 4 * U}[kind]
    return 0.5 * hi * e + 2 * U * hi


def store_error(y_abs, fmt):
    """rounding of an fp32 value of magnitude <= y_abs on its way into a buffer of ``fmt``: half an ulp of the format in y_abs's
    binade (2^(e - p - 1) for 2^(e - 1) <= y_abs < 2^e and p significand bits), at least half the subnormal quantum for fp16; the
    two-plane split16 has no single ulp: 2^-22 relative plus the quantum"""
    if fmt == "fp32":
        return np.zeros_like(y_abs)
    if fmt == "split16":
        return HALF_ULP[fmt] * y_abs + SUB_Q[fmt]
    _, e = np.frexp(y_abs)
    return np.maximum(np.ldexp(1.0, e - SIG_BITS[fmt] - 1), SUB_Q[fmt]) * (y_abs > 0)


# ---- conv layer 0 + GroupNorm + GELU ------------------------------------------------------------------------------------------
def conv0_windows(wav):
    """wav [B, Lmax] -> the conv's input windows [B, L0, 10] (k = 10, stride 5; trailing samples that fill no window are unused)"""
    wav = np.asarray(wav, dtype=np.float64)
    B, Lmax = wav.shape
    L0 = (Lmax - 10) // 5 + 1
    idx = 5 * np.arange(L0)[:, None] + np.arange(10)[None, :]
    return wav[:, idx]


def conv0_ref(wav, w0, gn_w, gn_b, rows=None):
    """Conv1d(1 -> 512, k = 10, stride 5, no bias) -> GroupNorm(512 groups: per (utterance, channel) over time) -> GELU, in float64.

    wav [B, Lmax] (zero padded), w0 [512, 10] (or [512, 1, 10]), gn_w / gn_b [512].  The statistics are two-pass mean / variance over
    all L0 = (Lmax - 10) / 5 + 1 frames, padding included (rows None), or over row b's own first rows[b] frames
    (SYLBER_OPT_PER_UTTERANCE); eps = 1e-5.  Every one of the L0 frames is normalised with them and returned.

    Returns a dict: "v" the raw conv [B, L0, 512], "z" = scale v + shift (the GELU's argument), "y" = gelu(z), "scale" / "shift"
    [B, 512] (a = gamma / sqrt(var + eps), b = beta - mean a), "mean" / "var", "S" = sum_j |a w_j x_j| + |b| per element, "A" = sum_j
    |w_j x_j|, "n" the frame count of each row's statistics, "X" the windows."""
    w = np.asarray(w0, dtype=np.float64).reshape(512, 10)
    g, be = np.asarray(gn_w, np.float64), np.asarray(gn_b, np.float64)
    X = conv0_windows(wav)
    B, L0, _ = X.shape
    v = X @ w.T                                                       # [B, L0, 512]
    A = np.abs(X) @ np.abs(w).T
    n = np.full(B, L0) if rows is None else np.asarray(rows, dtype=np.int64)
    mean = np.stack([v[b, :n[b]].mean(0) for b in range(B)])
    var = np.stack([((v[b, :n[b]] - mean[b]) ** 2).mean(0) for b in range(B)])
    a = g[None] / np.sqrt(var + EPS)
    sh = be[None] - mean * a
    z = a[:, None] * v + sh[:, None]
    return {"v": v, "z": z, "y": gelu64(z), "scale": a, "shift": sh, "mean": mean, "var": var, "A": A, "X": X, "n": n,
            "S": np.abs(a)[:, None] * A + np.abs(sh)[:, None], "gn_w": g, "w": w}


def conv0_stats_bound(ref):
    """(d_scale, d_shift) [B, 512]: bounds on the kernel's fp32 table against ``ref``'s float64 scale / shift.

    conv0_stats_kernel sums the 10 strided sums and 55 lag products of the waveform in fp64 (a product of two fp32 values is exact in
    fp64), conv0_finalize_kernel forms mean = w . S / n and E[v^2] = w^T R w / n in fp64 and var = E[v^2] - mean^2.  With e = 2^-53
    and n + 128 fp64 roundings per accumulated quantity (n additions, ~100 for the quadratic form), and A_l = sum_j |w_j x_lj|:
        |d mean| <= (n + 128) e mean_l(A_l)
        |d var|  <= (n + 128) e (mean_l(A_l^2) + 2 |mean| mean_l(A_l))          -- the cancellation term of E[v^2] - mean^2
        |d a|    <= |gamma| |d var| / (2 (var + eps)^1.5)  +  2^-23 |a|          -- derivative of rsqrt, then the cast to fp32
        |d b|    <= |mean| |d a| + |a| |d mean|  +  2^-23 |b|
    (2^-23 relative covers the fp64 sqrt / divide / fma and the round to fp32, u = 2^-24, with room to spare.)"""
    e = 2.0 ** -53
    A, n, mean, var, a, sh = ref["A"], ref["n"], ref["mean"], ref["var"], ref["scale"], ref["shift"]
    B = A.shape[0]
    mA = np.stack([A[b, :n[b]].mean(0) for b in range(B)])
    mA2 = np.stack([(A[b, :n[b]] ** 2).mean(0) for b in range(B)])
    k = (n[:, None] + 128) * e
    d_mean = k * mA
    d_var = k * (mA2 + 2 * np.abs(mean) * mA)
    d_a = np.abs(ref["gn_w"])[None] * d_var / (2 * (var + EPS) ** 1.5) + 2.0 ** -23 * np.abs(a)
    d_b = np.abs(mean) * d_a + np.abs(a) * d_mean + 2.0 ** -23 * np.abs(sh)
    return d_a, d_b


def conv0_bound(ref, fmt, kernel):
    """Per-element bound [B, L0, 512] on |stored conv0 output - ref["y"]|.

    ``kernel``: "mfma" (conv0_mfma_kernel: bf16 / fp16), "valu" (conv0_gn_gelu_kernel<false, false>: bf16 / fp16 with
    SYLBER_OPT_CONV0_VALU = 1; GroupNorm scale folded into the taps, gelu_fast), "valu_ref" (the split16 and fp32 instantiations:
    conv, then scale and shift; gelu_erf7 resp. gelu_erf).

    1. Statistics: z = a v + b with the kernel's fp32 (a, b): |dz| <= |v| |d a| + |d b| (conv0_stats_bound).
    2. Arithmetic of z, with S = sum_j |a w_j x_j| + |b| and S' = S - |b|:
       VALU kernels: w' = fl(a w) (u relative), then a chain of 10 fmas starting from b ("valu"), or 10 fmas and one fma(v, a, b)
       ("valu_ref"): every rounding is u relative to a partial sum of magnitude <= S, 11 of them -> 12 u S (one spare).
       MFMA kernel: every operand p (a waveform sample x, a scaled tap w' = fl(a w)) enters as hi = half(p), lo = half(p - hi).  p - hi
       is exact in fp32; lo carries it to 11 more bits, so |p - hi - lo| <= 2^-22 |p| while lo is a normal half; once |p| < 2^-3 the
       lo half can drop below 2^-14, where halves sit on a 2^-24 grid, and the error is an ABSOLUTE 2^-25 instead (the same holds
       when hi itself is subnormal).  So |dp| <= 2^-22 |p| + [|p| < 2^-3] 2^-25 =: r|p| + s_p.  Three MFMAs compute hi.hi + lo.hi +
       hi.lo exactly (products of halves are exact in fp32), i.e. (w' - dw)(x - dx) - lo_w lo_x with |lo_p| <= 2^-11 |p| + 2^-25:
           |error| <= sum_j |w'| |dx| + |x| |dw| + |dw| |dx| + |lo_w| |lo_x|
                   <= (2 r + r^2 + 2^-22) S' + u S'                                   -- relative parts, and fl(a w)
                      + 2^-25 (1 + r + 2^-11) (|a| sum_j [.]|w_j|' + sum_j [.]|x_j|) + 10 (2^-50 + 2^-50)
       where the absolute part counts only the operands below 2^-3 (for |p| >= 2^-3 a subnormal lo still errs by at most 2^-25 <=
       2^-22 |p|); this bound charges it for the partner operand's full magnitude.  The accumulator starts at b and takes 3 x 16
       products: whatever the order inside the matrix pipe, 48 additions of partial sums <= S -> 48 u S.
    3. GELU: its Lipschitz constant (< 1.13) times the above, plus gelu_error of the kernel's variant.
    4. The store: store_error(fmt) at the kernel's own value, i.e. at |y| + the error so far."""
    assert kernel in ("mfma", "valu", "valu_ref")
    d_a, d_b = conv0_stats_bound(ref)
    S, sh, a, X, w = ref["S"], ref["shift"], ref["scale"], ref["X"], ref["w"]
    Sp = S - np.abs(sh)[:, None]
    ez = np.abs(ref["v"]) * d_a[:, None] + d_b[:, None]
    if kernel == "mfma":
        r = 2.0 ** -22
        small_x = (np.abs(X) < 0.125).astype(np.float64)                               # [B, L0, 10]
        wp = np.abs(a)[:, :, None] * np.abs(w)[None]                                   # |w'| [B, 512, 10]
        small_w = (wp < 0.125 * (1 + 2.0 ** -20)).astype(np.float64)         # (the kernel's own fl(a w) may sit a few ulps off)
        # sum_j |w'_j| s_x_j  +  sum_j |x_j| s_w_j
        absx = np.einsum("blj,bcj->blc", small_x, wp) + np.einsum("blj,bcj->blc", np.abs(X), small_w)
        ez = ez + (2 * r + r * r + 2.0 ** -22 + U) * Sp + 2.0 ** -25 * (1 + r + 2.0 ** -11) * absx + 20 * 2.0 ** -50 + 48 * U * S
        gk = "fast"
    else:
        ez = ez + 12 * U * S
        gk = "fast" if kernel == "valu" else ("erf7" if fmt == "split16" else "erf")
    ey = GELU_LIP * ez + gelu_error(ref["z"], gk, ez)
    return ey + store_error(np.abs(ref["y"]) + ey, fmt)


def conv0_kernel_of(fmt, valu=False):
    if fmt in ("bf16", "fp16"):
        return "valu" if valu else "mfma"
    return "valu_ref"


# ---- feature projection: LayerNorm(512) -> Linear(512 -> 768), padded frames zeroed ------------------------------------------------
def proj_ref(feats, valid, ln_w, ln_b, w, b, fmt):
    """feats [B, T, 512] (the stage-1 tap: the conv stack's stored output, exact), valid [B] frames -> float64
    x = Linear(LayerNorm(feats)) [B, T, 768] with frames t >= valid_b set to +0 (transformers zeroes them in front of the pos-conv).
    The weights are the kernel's operand, round_fmt(w) (rounded once at load time, deterministically); the LayerNorm output is NOT
    rounded here (proj_bound says why).
    Returns a dict with "x", the LayerNorm output "ln", its row statistics and "SW" = sum_k |w_nk| |ln_k|."""
    f = np.asarray(feats, np.float64)
    g, be = np.asarray(ln_w, np.float64), np.asarray(ln_b, np.float64)
    W, bb = round_fmt(np.asarray(w, np.float64), fmt), np.asarray(b, np.float64)
    mean = f.mean(-1, keepdims=True)
    var = ((f - mean) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + EPS)
    ln = (f - mean) * rstd * g + be
    x = ln @ W.T + bb
    keep = (np.arange(f.shape[1])[None, :] < np.asarray(valid)[:, None])
    x = np.where(keep[:, :, None], x, 0.0)
    return {"x": x, "ln": ln, "keep": keep, "SW": np.abs(ln) @ np.abs(W).T, "W": W, "b": bb, "rstd": rstd[..., 0], "mean": mean[..., 0],
            "fabs": np.abs(f).max(-1), "g": g, "be": be}


def proj_bound(ref, fmt):
    """Per-element bound [B, T, 768] on |tap -2 - ref["x"]|; exactly 0 on the zeroed frames (the kernel stores +0 there).

    The kernel normalises a row in fp32 (two-pass, one wave per row), ROUNDS the LayerNorm output to the 16-bit format, and runs the
    GEMM on 16-bit operands (weights rounded once at load time) with fp32 accumulation; the bias is added in fp32.
      * LayerNorm in fp32: mean and variance of 512 values by pairwise sums (<= 12 roundings each), x - mean, times rstd, fma with
        gamma / beta: |d ln_k| <= 16 u (|gamma_k| rstd (|x_k| + |mean| + max|x|) + |beta_k|), bounded with the row's max |x|.
      * operand rounding: the reference holds the rounded weights, so only |d ln_k| <= h |ln_k| + q remains: h sum_k |w_nk| |ln_k| +
        q sum_k |w_nk|.  split16 runs three passes hi.hi + lo.hi + hi.lo; the dropped lo.lo term is <= (2^-11 |w| + 2^-25)(2^-11 |ln| +
        2^-25), summed over K: 2^-22 sum |w| |ln| + 2^-36 (sum |w| + sum |ln|) + K 2^-50.
      * fp32 accumulation of K = 512 products (exact products of 16-bit operands; fp32 operands in the fp32 mode, one rounding more)
        and the bias: (K + 2) u (sum_k |w_nk| |ln_k| + |bias_n|), valid for any summation order.
    This bound is LOOSER than the conv0 and pos-conv ones: the reference is the unrounded LayerNorm output, so for bf16 / fp16 the
    half-ulp of that operand times sum_k |w_nk| |ln_k| (not times |x|) dominates -- about 5e-2 resp. 7e-3 at the synthetic
    checkpoint's scales.  Restating the rounding in the reference instead would put the reference itself one ulp of an operand off
    wherever float64 and fp32 LayerNorm round to different neighbours.  Far tighter than an O(1) zeroing or row-offset error."""
    h, q = HALF_ULP[fmt], SUB_Q[fmt]
    W = np.abs(ref["W"])
    SW = ref["SW"]
    dln = 16 * U * (np.abs(ref["g"])[None, None] * ref["rstd"][..., None] * (2 * ref["fabs"][..., None] + np.abs(ref["mean"])[..., None])
                    + np.abs(ref["be"])[None, None])
    e = dln @ W.T
    sw, sln = W.sum(1)[None, None], np.abs(ref["ln"]).sum(-1, keepdims=True)
    e = e + h * SW + q * sw
    if fmt == "split16":
        e = e + 2.0 ** -22 * SW + 2.0 ** -36 * (sw + sln) + 512 * 2.0 ** -50
    e = e + (512 + 2) * U * (SW + np.abs(ref["b"])[None, None])
    return np.where(ref["keep"][:, :, None], e, 0.0)


def layernorm_ref(f, g, be):
    """LayerNorm over the last axis in float64, and a bound on what an fp32 kernel (two-pass, tree sums; layernorm_kernel) returns
    instead: the mean and the variance take ~12 roundings each, rstd 8 u relative from them, then x - mean, the scaling and one fma:
    |d y_k| <= 16 u (|gamma_k| rstd (|x_k - mean| + max |x|) + |beta_k|), bounded with |x_k - mean| <= max |x| + |mean|"""
    f = np.asarray(f, np.float64)
    g, be = np.asarray(g, np.float64), np.asarray(be, np.float64)
    mean = f.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((f - mean) ** 2).mean(-1, keepdims=True) + EPS)
    y = (f - mean) * rstd * g + be
    return y, 16 * U * (np.abs(g) * rstd * (2 * np.abs(f).max(-1, keepdims=True) + np.abs(mean)) + np.abs(be))


# ---- positional convolution + GELU + residual --------------------------------------------------------------------------------------
def posconv_xpad(x, valid, fmt):
    """x [B, T, 768] (tap -2) -> the pos-conv's operand [B, 64 + T + 64, 768] float64: round_fmt(x) on frames [0, valid_b) at rows
    64 + t, zeros in the 64 halo rows in front, in the tail [valid_b, T) and behind"""
    x = np.asarray(x, np.float64)
    B, T, D = x.shape
    xp = np.zeros((B, T + 128, D))
    xr = round_fmt(x, fmt)
    for b in range(B):
        xp[b, 64:64 + int(valid[b])] = xr[b, :int(valid[b])]
    return xp


def posconv_weights(w_eff, fmt):
    """the weight-normed weight [768, 48, 128] as the kernel's operand: round_fmt, as [group][n][c][tap] (compute it once per format)"""
    return round_fmt(np.asarray(w_eff, np.float64), fmt).reshape(POS_G, POS_C, POS_C, POS_K)


def posconv_from_xpad(xpad, x, w_eff, bias, fmt, gelu=True, tap_shift=0, wr=None):
    """out[t][n] = x[t][n] + gelu(sum_tap sum_c xpad[t + tap + tap_shift][c] w[n][c][tap] + bias[n]) and, per element, P = sum |x| |w|.

    16 groups of 48 channels, 128 taps: frame t reaches input frames t - 64 .. t + 63 (xpad rows t .. t + 127) -- Conv1d(padding = 64)
    yields T + 1 frames and the reference drops the LAST one, so the extra tap of the symmetric padding is the one at t + 64.
    ``tap_shift`` (tests only) moves the window, as a kernel with an off-by-one window would."""
    xpad = np.asarray(xpad, np.float64)
    B, Tp, D = xpad.shape
    T = Tp - 128
    wr = posconv_weights(w_eff, fmt) if wr is None else wr                                       # [g][n][c][tap]
    xs = np.zeros((B, Tp + 2, D))
    xs[:, 1:Tp + 1] = xpad
    conv = np.empty((B, T, D))
    P = np.empty((B, T, D))
    Sx = np.empty((B, T, D))
    Sw = np.abs(wr).sum(axis=(2, 3)).reshape(D)
    from numpy.lib.stride_tricks import sliding_window_view
    for g in range(POS_G):
        win = sliding_window_view(xs[:, 1 + tap_shift:1 + tap_shift + T + POS_K - 1, g * POS_C:(g + 1) * POS_C], POS_K, axis=1)
        xg = np.ascontiguousarray(win).reshape(B * T, POS_C * POS_K)                              # [B, T, c, tap] -> rows of (c, tap)
        wg = np.ascontiguousarray(wr[g].reshape(POS_C, POS_C * POS_K).T)                          # [(c, tap), n]
        xa = np.abs(xg)
        conv[:, :, g * POS_C:(g + 1) * POS_C] = (xg @ wg).reshape(B, T, POS_C)
        P[:, :, g * POS_C:(g + 1) * POS_C] = (xa.astype(np.float32) @ np.abs(wg).astype(np.float32)).reshape(B, T, POS_C)
        Sx[:, :, g * POS_C:(g + 1) * POS_C] = xa.sum(1).reshape(B, T, 1)
    z = conv + np.asarray(bias, np.float64)[None, None]
    pos = gelu64(z) if gelu else z
    return {"out": np.asarray(x, np.float64) + pos, "z": z, "pos": pos, "P": P * (1 + 1e-5), "x": np.asarray(x, np.float64),
            "Sx": Sx, "Sw": Sw}


def posconv_ref(x, valid, w_eff, bias, fmt, wr=None):
    """x [B, T, 768] fp32 residual stream (tap -2, zero at t >= valid_b), w_eff the weight-normed weight [768, 48, 128]
    (oracle/hubert_ref.pos_conv_weight).  The operands are what the kernel reads: round_fmt of x and of w (fp32 mode: unrounded);
    everything else float64.  All T frames are returned, the padded ones too (their residual is +0, their pos-conv is not)."""
    return posconv_from_xpad(posconv_xpad(x, valid, fmt), x, w_eff, bias, fmt, wr=wr)


def posconv_bound(ref, fmt):
    """Per-element bound [B, T, 768] on |tap -3 - ref["out"]|.

    The reference already holds the rounded operands, and a product of two 16-bit operands (<= 11 + 11 significand bits) is exact in
    fp32, so the contraction's only error is the fp32 accumulation of K = 48 x 128 = 6144 terms: K u P with P = sum |x| |w|, for any
    summation order (the MFMA's included).  split16 reads hi / lo planes in three passes, hi.hi + lo.hi + hi.lo: 3 K accumulated
    products, and the dropped lo.lo with |lo_p| <= 2^-11 |p| + 2^-25 (the 2^-24 grid of subnormal halves), summed over K:
    2^-22 P + 2^-36 (sum |x| + sum |w|) + K 2^-50.  The fp32 mode multiplies fp32 operands: one rounding more per product,
    (K + 1) u P.  Then the bias add (u |z|), the GELU (Lipschitz < 1.13; gelu_fast for bf16 / fp16, gelu_erf7 for split16, gelu_erf for
    fp32) and the fp32 rounding of the residual add: u |out|."""
    K = POS_K * POS_C
    P, z = ref["P"], np.abs(ref["z"])
    if fmt == "split16":
        ez = (3 * K * U + 2.0 ** -22) * P + 2.0 ** -36 * (ref["Sx"] + ref["Sw"][None, None]) + K * 2.0 ** -50
        gk = "erf7"
    elif fmt == "fp32":
        ez, gk = (K + 1) * U * P, "erf"
    else:
        ez, gk = K * U * P, "fast"
    ez = ez + U * (z + ez)
    e = GELU_LIP * ez + gelu_error(z, gk, ez)
    return e + U * (np.abs(ref["out"]) + e)


# ---- the check every test uses -----------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, bound):
    """max over ALL elements of |got - ref| / bound (0 / 0 counts as 0, x / 0 as inf) and its index"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), i


# ---- the shapes both tiers run (tests/test_frontend_ref.py on the CPU, tests/test_gpu_frontend.py on the GPU) -----------------------
FMTS = ("bf16", "fp16", "split16", "fp32")
# (format, conv0 kernel): the matrix-pipe and the VALU kernel of the 16-bit modes, the reference-order VALU kernel of split16 / fp32
CONV0_COMBOS = (("bf16", "mfma"), ("fp16", "mfma"), ("bf16", "valu"), ("fp16", "valu"), ("split16", "valu_ref"), ("fp32", "valu_ref"))
# conv0 frame counts (Lmax = 5 (L0 - 1) + 10): one output frame's minimum, a 256-row block / 32-row sub-block edge, one or two chunks
# of the statistics pass; and an Lmax that is not of the form 5 k (trailing samples unused)
CONV0_LMAX = tuple(5 * (l0 - 1) + 10 for l0 in (79, 255, 256, 257, 2048, 2049)) + (1289,)
RAGGED_LMAX, RAGGED_LENS = 5 * 300 + 10, (5 * 300 + 10, 1203, 400)
# pos-conv shapes: (T, valid frames per utterance)
POSCONV_SHAPES = ((1, (1,)), (64, (64,)), (65, (65,)), (257, (257, 256, 193, 192, 65, 64, 1)), (385, (385, 384, 321)))


def conv0_weights(sd):
    return (sd["feature_extractor.conv_layers.0.conv.weight"].numpy().reshape(512, 10),
            sd["feature_extractor.conv_layers.0.layer_norm.weight"].numpy(), sd["feature_extractor.conv_layers.0.layer_norm.bias"].numpy())


def noise(B, n, seed, lens=None):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(B, n, generator=g, dtype=torch.float32)
    if lens is not None:
        for b, l in enumerate(lens):
            w[b, l:] = 0
    return w.numpy()
# projection shapes: (T, valid frames per utterance); 257 frames x 3 crosses every row tile of the projection GEMM
PROJ_SHAPES = ((9, (9, 6, 1)), (257, (257, 193, 1)))

"""Test-only float64 reference of conv layers 1-6 of the feature extractor (Conv1d(512, 512, k_i, stride 2, no bias) + GELU; k_i = 3
for i = 1..4, 2 for i = 5, 6) and a per-element error bound DERIVED from the arithmetic of the kernels that compute them: the six
implicit GEMMs of Forward::conv_stack / ForwardF32::conv_stack (csrc/forward.hip).  Built on tests/frontend_ref.py (formats, GELU
errors, store error, worst_ratio); plain numpy, written from the published algorithm (transformers' HubertModel, restated in
oracle/hubert_ref.py); never imported by ``sylber_amd``.

Every layer is computed FROM THE PREVIOUS TAP'S ACTUAL VALUES (SYLBER_TAP_CONV0 for layer 1, SYLBER_TAP_CONV(i - 1) else): a tap is
an exact fp32 widening of the stored operand, so the reference sees precisely what the kernel read and no operand-rounding term
exists.  The weights are the kernel's operand too: round_fmt of the checkpoint's, rounded once at load.

Geometry (restated here, checked against the library's plan in tests/test_conv_stack_ref.py): L_0 = (Lmax - 10) // 5 + 1 and
L_i = (L_(i-1) - k_i) // 2 + 1 valid rows per utterance -- of EVERY utterance of a padded batch: the reference model convolves the
padded waveform -- in a buffer of R_i = Tp 2^(6-i) rows per utterance, Tp = padded_frames(Lmax)."""
import numpy as np

import frontend_ref as fr
from frontend_ref import GELU_LIP, U, gelu64, gelu_error, round_fmt, store_error

CK = (10, 3, 3, 3, 3, 2, 2)
CS = (5, 2, 2, 2, 2, 2, 2)
CH = 512


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def conv_rows(Lmax):
    """[L_0 .. L_6]: valid output rows of every conv layer for Lmax samples"""
    L, n = [], int(Lmax)
    for k, s in zip(CK, CS):
        n = (n - k) // s + 1
        L.append(n)
    return L


def padded_frames(Lmax):
    """frame pitch Tp per utterance: the smallest multiple of 32 with L_i <= Tp 2^(6-i) for every layer"""
    need = max(-(-l // (1 << (6 - i))) for i, l in enumerate(conv_rows(Lmax)))
    return (need + 31) & ~31


def buffer_rows(Lmax):
    """[R_0 .. R_6]: rows per utterance of every layer's output buffer"""
    tp = padded_frames(Lmax)
    return [tp << (6 - i) for i in range(7)]


# ---- reference ----------------------------------------------------------------------------------------------------------------
def conv_weight(sd, i, fmt):
    """conv layer i's weight [512 out, 512 in, k_i] as the kernel's operand (round_fmt, float64), as k_i matrices [512 in, 512 out]"""
    w = round_fmt(sd["feature_extractor.conv_layers.%d.conv.weight" % i].numpy().astype(np.float64), fmt)
    assert w.shape == (CH, CH, CK[i])
    return [np.ascontiguousarray(w[:, :, t].T) for t in range(CK[i])]


def conv_rows_of(xflat, base, taps, n, shift=0, m0=0, with_S=True):
    """z [n, 512] = sum_t xflat[base + 2 m + t + shift] @ taps[t] for m0 <= m < m0 + n, and S = sum |x| |W| (float64 operands; S is
    accumulated in fp32 and inflated by its own worst-case summation error, so that it is an upper bound).  xflat [rows, 512]: a
    buffer's rows, every utterance's back to back, as the implicit GEMM sees them.  ``shift`` (tests only) moves the window"""
    z = np.zeros((n, CH))
    S = np.zeros((n, CH), np.float32)
    for t, w in enumerate(taps):
        a = base + 2 * m0 + t + shift
        x = xflat[a:a + 2 * n - 1:2]
        assert x.shape[0] == n, "the window leaves the buffer"
        z += x @ w
        if with_S:
            S += np.abs(x).astype(np.float32) @ np.abs(w).astype(np.float32)
    return z, S.astype(np.float64) * (1.0 + 2 * (len(taps) * CH + 2) * U)


def conv_layer_ref(x_prev, w, i, fmt, L_prev):
    """x_prev [B, R_(i-1), 512]: the stored output of the layer below (its tap, exact in fp32); w: conv_weight(sd, i, fmt); L_prev =
    L_(i-1).  Returns a dict: "y" = gelu(z) [B, L_i, 512] float64 with z[b, m, o] = sum_(t < k_i) sum_c x[b, 2 m + t, c] W[o, c, t] for
    m < L_i = (L_prev - k_i) // 2 + 1 (HuBERT-base has no conv bias), "z", "S" = sum |x| |W|, and for split16 "LL" = sum |lo_x| |lo_W|,
    the magnitude of the lo.lo products the three-pass kernel drops, from x's and W's own lo planes."""
    x = np.asarray(x_prev, np.float64)
    B, R, _ = x.shape
    k = CK[i]
    assert len(w) == k and L_prev <= R
    Li = (L_prev - k) // 2 + 1
    flat = x.reshape(B * R, CH)
    zs = [conv_rows_of(flat, b * R, w, Li) for b in range(B)]
    ref = {"z": np.stack([z for z, _ in zs]), "S": np.stack([s for _, s in zs]), "i": i, "k": k, "L": Li}
    ref["y"] = gelu64(ref["z"])
    if fmt == "split16":
        lx = np.abs(flat - round_fmt(flat, "fp16"))
        lw = [np.abs(m - round_fmt(m, "fp16")) for m in w]
        ref["LL"] = np.stack([sum(lx[b * R + t:b * R + t + 2 * Li - 1:2] @ lw[t] for t in range(k)) for b in range(B)])
    return ref


def gelu_kind(fmt):
    """the GELU of the layer's epilogue: gelu_fast (ACT_GELU_FAST) for bf16 / fp16, gelu_erf7 (ACT_GELU_ERF7) for split16; the fp32
    mode's launch_gemm_f32 applies gelu_erf for act = 1 (csrc/fp32_path.hip: `if (a.act == 1) x = gelu_erf(x)`, ocml's erff)"""
    return {"bf16": "fast", "fp16": "fast", "split16": "erf7", "fp32": "erf"}[fmt]


def conv_layer_bound(ref, fmt):
    """Per-element bound [B, L_i, 512] on |tap i - ref["y"]|, derived, not fitted.

      * Accumulation.  Both operands are exact (the tap, the rounded weights) and a product of two 16-bit operands (<= 11 + 11
        significand bits) is exact in fp32, so the contraction's only error is the fp32 accumulation of K = k_i 512 products:
        (K + 2) u S with S = sum |x| |W| and u = 2^-24, for ANY summation order -- the 32x32x16 and the 16x16x32 MFMA families, the
        chunk-major K order of the 3-tap layers (kpat) and the k-ordered fma chains of the fp32 mode alike.  The fp32 mode
        multiplies fp32 operands: one more rounding per product, u S more.
      * split16 only: the kernel runs three passes hi.hi + lo.hi + hi.lo and drops lo.lo: sum |lo_x| |lo_W| = ref["LL"], from the
        operands' own lo planes.  (Its three passes accumulate 3 K products; the lo passes' terms are 2^-11 of the hi ones, and the
        issue's (K + 2) u S is kept for them: the measured ratios say how far inside it the kernel sits.)
      * GELU: its Lipschitz constant (< 1.13) times the above, plus gelu_error of the mode's variant (gelu_kind) for an argument
        known to within the above.
      * The store: store_error(fmt) at the kernel's own value, i.e. at |y| + the error so far."""
    K = ref["k"] * CH
    ez = (K + 2) * U * ref["S"]
    if fmt == "fp32":
        ez = ez + U * ref["S"]
    if fmt == "split16":
        ez = ez + ref["LL"]
    ey = GELU_LIP * ez + gelu_error(ref["z"], gelu_kind(fmt), ez)
    return ey + store_error(np.abs(ref["y"]) + ey, fmt)


def check_layer(got, ref, fmt):
    """tap i [B, R_i, 512] against ``ref``: every element of rows [0, L_i) of every utterance.  -> (worst ratio, where, largest
    bound, rms |ref|)"""
    bound = conv_layer_bound(ref, fmt)
    r, at = fr.worst_ratio(np.asarray(got)[:, :ref["L"]], ref["y"], bound)
    return r, at, float(bound.max()), float(np.sqrt((ref["y"] ** 2).mean()))


# ---- the shapes both tiers run (tests/test_conv_stack_ref.py on the CPU, tests/test_gpu_conv_stack.py on the GPU) -------------------
def frames_to_samples(t):
    return 320 * t + 80


# name -> (B, Lmax, per-utterance sample counts or None, the layers checked).  What each reaches:
#   lone1        Tp = 32; L_1 .. L_6 = 39, 19, 9, 4, 2, 1: every launch below one tile; conv6 has M = 32
#   lone32_long  the longest waveform that still gives 32 frames: L_0 = 2126 needs 34 frames of pitch, so Tp must be 64, not 32
#   lone64       L_3 = 513 > 512, so Tp must be 96
#   seams        utterance seams at pitch 64 2^(6-i); rows [L_i, R_i) of utterances 0 and 1 feed nothing valid; ragged, zero padded
#   tiles        Tp = 288 = 256 + 32: M = 576 2^(6-i) is ragged against 128-, 192- and 256-row tiles
#   rounds       conv1 has M = 36864: at N = 512 that is 288 tiles of 256 x 256, more than one round of 256 persistent workgroups
CASES = {
    "lone1": (1, frames_to_samples(1), None, (1, 2, 3, 4, 5, 6)),
    "lone32_long": (1, 10639, None, (1, 2, 3, 4, 5, 6)),
    "lone64": (1, frames_to_samples(64), None, (1, 2, 3, 4, 5, 6)),
    "seams": (3, frames_to_samples(33), tuple(frames_to_samples(t) for t in (33, 32, 1)), (1, 2, 3, 4, 5, 6)),
    "tiles": (2, frames_to_samples(257), None, (1, 2, 3, 4, 5, 6)),
    "rounds": (4, frames_to_samples(257), None, (1, 2)),
}
CASE_FMTS = {"rounds": ("bf16", "fp16")}


def case_formats(name):
    return CASE_FMTS.get(name, fr.FMTS)


def case_wav(name):
    B, Lmax, lens, _ = CASES[name]
    return fr.noise(B, Lmax, 1000 + Lmax + B, lens)

"""CPU tier: the float64 reference of conv layers 1-6 (tests/conv_stack_ref.py) is pinned to the oracle, and its per-element bound is
shown to REJECT subtly wrong kernels at every shape and format tests/test_gpu_conv_stack.py runs on the GPU, for a 3-tap and for a
2-tap layer: the reference output, rounded as the kernel stores it, passes with no element excluded, and every planted defect
(exchanged taps, a window one row late, the wrong utterance pitch, a 64-channel chunk of K missing or doubled, a third tap on a 2-tap
layer, the next layer's weights, GELU omitted or applied twice, a last valid row without its last tap, the other ping-pong buffer)
fails.  Also host arithmetic: every layer's valid rows fit its buffer at every shape, and the library's plan agrees with the
restatement.  Nothing here needs a GPU, and nothing on the GPU has to misbehave for the bound to be trusted."""
import ctypes

import numpy as np
import pytest
import torch

import conv_stack_ref as cr
import frontend_ref as fr
from conv_stack_ref import CASES, CH, CK, case_formats
from oracle import hubert_ref
from sylber_amd.weights import synthetic_state_dict

TAP3_LAYER, TAP2_LAYER = 2, 5            # (layer 2: the deepest 3-tap layer case "rounds" checks, and layer 0 exists below its input)
WINDOW = 64                              # planted defects are recomputed for the last WINDOW valid rows of the last utterance


@pytest.fixture(scope="module")
def sd():
    return synthetic_state_dict(0, num_layers=1)


@pytest.fixture(scope="module")
def lib():
    from sylber_amd import build, _lib
    build.build()
    return _lib.load()


def plan_rows(lib, Lmax):
    L, R = (ctypes.c_int32 * 7)(), (ctypes.c_int32 * 7)()
    assert lib.sylber_debug_conv_rows(Lmax, L, R) == 0
    return list(L), list(R)


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def test_valid_rows_fit_every_buffer(lib):
    """L_i <= R_i for i = 0..6 with Tp = sylber_padded_frames(Lmax), at every shape of the GPU tier and over a sweep of lengths; the
    plan's L[] / R[] agree with the Python restatement"""
    lmaxes = sorted({c[1] for c in CASES.values()} | set(range(400, 12000)) | set(range(20000, 21000)) | {160000, 960000, 82000 + 7})
    for lmax in lmaxes:
        L, R = plan_rows(lib, lmax)
        tp = lib.sylber_padded_frames(lmax)
        assert L == cr.conv_rows(lmax) and R == cr.buffer_rows(lmax) and tp == cr.padded_frames(lmax) and tp % 32 == 0, lmax
        assert lib.sylber_num_frames(lmax) == L[6] and R[6] == tp
        assert all(l <= r for l, r in zip(L, R)), (lmax, L, R)
    assert lib.sylber_debug_conv_rows(399, (ctypes.c_int32 * 7)(), (ctypes.c_int32 * 7)()) != 0


def test_shapes_reach_what_they_claim():
    """the comments of conv_stack_ref.CASES, as arithmetic"""
    L, tp = cr.conv_rows, cr.padded_frames
    assert tp(CASES["lone1"][1]) == 32 and L(CASES["lone1"][1])[1:] == [39, 19, 9, 4, 2, 1]
    long32 = CASES["lone32_long"][1]
    assert L(long32)[6] == 32 and L(long32 + 1)[6] == 33 and L(long32)[0] == 2126 and tp(long32) == 64
    assert all(L(long32)[i] > 32 << (6 - i) for i in range(6))              # a pitch of 32 frames overflows layers 0-5
    assert L(CASES["lone64"][1])[6] == 64 and L(CASES["lone64"][1])[3] == 513 and tp(CASES["lone64"][1]) == 96
    B, lmax, lens, _ = CASES["seams"]
    assert tp(lmax) == 64 and [L(n)[6] for n in lens] == [33, 32, 1] and all(l < r for l, r in zip(L(lmax), cr.buffer_rows(lmax)))
    assert tp(CASES["tiles"][1]) == 288 and L(CASES["tiles"][1])[6] == 257
    B, lmax, _, layers = CASES["rounds"]
    M1 = B * cr.buffer_rows(lmax)[1]
    assert layers == (1, 2) and M1 == 36864 and (M1 // 256) * (CH // 256) == 288 > 256


# ---- the reference against the oracle -------------------------------------------------------------------------------------------
def test_reference_agrees_with_the_oracle(sd):
    """conv layers 1-6 chained in float64 from the oracle's conv0 output against oracle/hubert_ref.forward(collect=True) (fp32 torch) on
    a ragged batch: to the oracle's own fp32 noise"""
    lens = (4000, 3370, 1000)
    wav = fr.noise(3, 4000, 5, lens)
    o = hubert_ref.forward(sd, torch.from_numpy(wav), lens, num_layers=1, collect=True)
    x = o["conv0"].numpy().transpose(0, 2, 1).astype(np.float64)
    L = cr.conv_rows(4000)
    assert x.shape[1] == L[0]
    for i in range(1, 7):
        ref = cr.conv_layer_ref(x, cr.conv_weight(sd, i, "fp32"), i, "fp32", L[i - 1])
        assert ref["L"] == L[i]
        want = o["conv%d" % i].numpy().transpose(0, 2, 1)
        assert want.shape == ref["y"].shape and np.abs(ref["y"] - want).max() < 2e-5 * max(1.0, np.abs(want).max()), i
        x = ref["y"]


# ---- the bound can fail ---------------------------------------------------------------------------------------------------------
def stored_input(B, R, seed, fmt):
    """a layer's input buffer as the layer below leaves it: GELU outputs in the stored format in EVERY row (the rows past an utterance's
    valid ones hold values as well: a kernel that reads them must not get away with it)"""
    g = np.random.default_rng(seed)
    return fr.round_fmt(fr.gelu64(g.standard_normal((B, R, CH))), fmt)


def planted(x, other, w, w_next, i, fmt, L_prev, ref):
    """name -> (rows, values a wrong kernel would store there) for utterance b = B - 1, rows [m0, L_i)"""
    B, R, _ = x.shape
    k, Li, b = CK[i], ref["L"], B - 1
    n = min(WINDOW, Li)
    m0 = Li - n
    flat = x.reshape(B * R, CH)

    def z_of(xf, base, taps, shift=0):
        return cr.conv_rows_of(xf, base, taps, n, shift=shift, m0=m0, with_S=False)[0]

    z = z_of(flat, b * R, w)
    assert np.array_equal(z, ref["z"][b, m0:])
    rows = flat[b * R + 2 * m0:b * R + 2 * Li + k:1]                    # the window's input rows, from row 2 m0
    bad = {}
    bad["taps exchanged"] = z_of(flat, b * R, w[:-2] + [w[-1], w[-2]])
    bad["window one row late"] = z_of(flat, b * R, w, shift=1)
    if b >= 1:
        bad["input row pitch L instead of R"] = z_of(flat, b * L_prev, w)
    chunk = rows[1:2 * n:2, 64:128] @ w[1][64:128]                      # tap 1, channels 64 .. 127
    bad["a 64-channel chunk of K missing"] = z - chunk
    bad["a 64-channel chunk of K twice"] = z + chunk
    if k == 2:                                                          # K = 1536 on a 2-tap layer: the weight row runs into the next output channel's
        bad["a third tap"] = z + rows[2:2 * n + 1:2] @ np.roll(w[0], -1, axis=1)
    bad["the next layer's weights"] = z_of(flat, b * R, w_next)
    last = z.copy()
    last[-1] -= rows[2 * (n - 1) + k - 1] @ w[k - 1]
    bad["last valid row without its last tap"] = last
    bad["the other ping-pong buffer"] = z_of(other.reshape(B * R, CH), b * R, w)
    out = {name: fr.gelu64(v) for name, v in bad.items()}
    out["GELU omitted"] = z
    out["GELU twice"] = fr.gelu64(fr.gelu64(z))
    return b, m0, {name: fr.round_fmt(v, fmt) for name, v in out.items()}


@pytest.mark.parametrize("case", list(CASES))
def test_conv_bound_rejects_planted_defects(sd, case):
    B, lmax, _, layers = CASES[case]
    L, R = cr.conv_rows(lmax), cr.buffer_rows(lmax)
    for i in (TAP3_LAYER, TAP2_LAYER):
        if i not in layers:
            continue
        for fmt in case_formats(case):
            x = stored_input(B, R[i - 1], 10 * lmax + i, fmt)
            other = stored_input(B, R[i - 1], 10 * lmax + i + 5, fmt)
            w, w_next = cr.conv_weight(sd, i, fmt), cr.conv_weight(sd, i + 1, fmt)
            ref = cr.conv_layer_ref(x, w, i, fmt, L[i - 1])
            assert ref["L"] == L[i] and ref["y"].shape == (B, L[i], CH)
            bound = cr.conv_layer_bound(ref, fmt)
            # (a) the honest emulation: the float64 reference rounded as the kernel stores it, every valid element
            r, at = fr.worst_ratio(fr.round_fmt(ref["y"], fmt), ref["y"], bound)
            assert r <= 1.0, (case, i, fmt, "clean", r, at)
            # (b) every wrong kernel leaves the bound at some valid element
            b, m0, bad = planted(x, other, w, w_next, i, fmt, L[i - 1], ref)
            expect = {"taps exchanged", "window one row late", "a 64-channel chunk of K missing", "a 64-channel chunk of K twice", "the next layer's weights",
                      "last valid row without its last tap", "the other ping-pong buffer", "GELU omitted", "GELU twice"}
            expect |= {"a third tap"} if CK[i] == 2 else set()
            expect |= {"input row pitch L instead of R"} if B > 1 else set()
            assert set(bad) == expect
            for what, y in bad.items():
                r, _ = fr.worst_ratio(y, ref["y"][b, m0:], bound[b, m0:])
                assert r > 1.0, (case, i, fmt, what, r)

"""GPU tier: conv layers 1-6 of the feature extractor, each ALONE, against the float64 reference of tests/conv_stack_ref.py -- every
element of every utterance's valid rows inside a bound derived from the kernel's arithmetic (no element is left out, nothing is
averaged).  The layers are reached through the conv taps of sylber_set_stop_stage (SYLBER_TAP_CONV(i)), i.e. through the launches
every forward runs, and every layer is computed from the previous tap's actual values.  tests/test_conv_stack_ref.py shows on the
CPU that the bound rejects exchanged taps, a window one row late, the wrong utterance pitch, a missing or doubled 64-channel chunk of
K, a third tap on a 2-tap layer, the next layer's weights, a missing or doubled GELU, a last valid row without its last tap and the
other ping-pong buffer, at every shape used here."""
import ctypes

import numpy as np
import pytest
import torch

import conv_stack_ref as cr
import frontend_ref as fr
from conv_stack_ref import CASES, CK, case_formats, case_wav
from frontend_ref import FMTS
from sylber_amd import _lib
from sylber_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

# the smallest gain on a 0.05 grid that takes max |GELU argument| past 4.2 in EVERY layer at case "tiles" (float64 chain with bf16
# stores from the float64 conv0: max |z| of layers 1..6 = 8.1 6.3 5.5 5.2 6.5 5.9; at 1.05 layers 4 and 6 stay at 4.13 / 3.99).  The
# largest stored value is 6.9: nowhere near fp16's 65504 either
GAIN = 1.1
FMT_ID = {"bf16": 0, "fp16": 1, "split16": 2}


@pytest.fixture(scope="module")
def sds():
    sd = synthetic_state_dict(0, num_layers=1)
    gain = dict(sd)
    for i in range(1, 7):
        key = "feature_extractor.conv_layers.%d.conv.weight" % i
        gain[key] = sd[key] * GAIN
    return {"base": sd, "gain": gain}


@pytest.fixture(scope="module")
def encoders(sds):
    from sylber_amd import HubertEncoderHIP
    cache = {}

    def get(fmt, which="base"):
        if (fmt, which) not in cache:
            cache[(fmt, which)] = HubertEncoderHIP(sds[which], num_layers=1, precision=fmt)
        return cache[(fmt, which)]
    return get


@pytest.fixture(scope="module")
def weights(sds):
    """conv_weight per (state dict, layer, format), rounded once"""
    cache = {}

    def get(which, i, fmt):
        if (which, i, fmt) not in cache:
            cache[(which, i, fmt)] = cr.conv_weight(sds[which], i, fmt)
        return cache[(which, i, fmt)]
    return get


@pytest.fixture(scope="module")
def wavs():
    cache = {}

    def get(case):
        if case not in cache:
            lens = CASES[case][2]
            cache[case] = (torch.from_numpy(case_wav(case)).cuda(), None if lens is None else list(lens))
        return cache[case]
    return get


def conv_tap(enc, wav, lens, i):
    return enc.forward(wav, lens, stop_stage=_lib.TAP_CONV0 if i == 0 else _lib.TAP_CONV(i))


def read_taps(enc, wav, lens, layers):
    """{i: tap i on the device} for the layers and the layer below each"""
    return {i: conv_tap(enc, wav, lens, i) for i in sorted(set(layers) | {i - 1 for i in layers})}


def check_case(enc, weights, which, wavs, fmt, case, label, keep=None):
    """taps i - 1 and i of every layer of the case: every element of rows [0, L_i) of every utterance inside conv_layer_bound; the tap
    behind conv6 is bitwise stage 1.  -> ({layer: max err / bound}, {layer: max |GELU argument|})"""
    B, lmax, _, layers = CASES[case]
    wav, lens = wavs(case)
    L, R = cr.conv_rows(lmax), cr.buffer_rows(lmax)
    taps = read_taps(enc, wav, lens, layers)
    if 6 in layers:
        assert torch.equal(taps[6][:, :L[6]], enc.forward(wav, lens, stop_stage=1)), (case, "tap 6 is not stage 1")
    host = {i: t.cpu().numpy() for i, t in taps.items()}
    if keep is not None:
        keep.update(host)
    ratios, zmax = {}, {}
    for i in layers:
        assert host[i].shape == (B, R[i], 512) and host[i - 1].shape == (B, R[i - 1], 512) and R[i] == enc.padded_frames(lmax) << (6 - i)
        ref = cr.conv_layer_ref(host[i - 1], weights(which, i, fmt), i, fmt, L[i - 1])
        assert ref["L"] == L[i] <= R[i]
        r, at, bmax, rms = cr.check_layer(host[i], ref, fmt)
        zmax[i] = float(np.abs(ref["z"]).max())
        print("float64 check conv%d %s %s %s B %d L %d of R %d max err / bound %.3f at %s (largest bound %.2e, rms |ref| %.3f, max |gelu arg| %.1f)"
              % (i, fmt, label, case, B, L[i], R[i], r, at, bmax, rms, zmax[i]))
        ratios[i] = r
    return ratios, zmax


def resolve(lib, fmt, M, K, kpat, tile, model):
    """the kernel instantiation a conv layer's launch resolves to (sylber_debug_gemm_resolve: host arithmetic)"""
    buf = ctypes.create_string_buffer(4096)
    act = 3 if fmt == "split16" else 1
    n = lib.sylber_debug_gemm_resolve(M, 512, K, 0, act, FMT_ID[fmt], kpat, tile, model, 0, 0, 0, buf, len(buf))
    assert n == 1, (n, M, K, fmt, tile, model)
    m0, m1, name = buf.value.decode().strip().split(" ", 2)
    assert (int(m0), int(m1)) == (0, M)
    return name


def conv_launch(i, B, lmax, fmt):
    """(M, K, kpat) of conv layer i's launch"""
    return B * cr.buffer_rows(lmax)[i], CK[i] * 512, 1 if (CK[i] == 3 and fmt != "split16") else 0


# ---- 1. every layer against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_conv_layers_vs_float64(encoders, weights, wavs, fmt):
    """Every case of conv_stack_ref.CASES, every layer i = 1..6: tap i from tap i - 1, every valid element inside conv_layer_bound, and
    the tap behind conv6 bitwise stage 1.  bf16 / fp16 twice: SYLBER_OPT_GEMM_MFMA16 0 (the 16x16x32 family, the default) and -1 (the
    32x32x16 kernels), which agree only to fp32 rounding and so are each checked on their own; split16 has one family (asserted).
    Measured max err / bound on MI355X, the worst case per layer (conv1 .. conv6; bf16 / fp16: the same figures in both families, the
    worst element is one whose store rounds by nearly half an ulp either way):
      bf16     0.874 0.881 0.859 0.851 0.889 0.903
      fp16     0.497 0.477 0.423 0.444 0.577 0.551
      split16  0.004 0.004 0.004 0.004 0.006 0.004
      fp32     0.005 0.005 0.005 0.004 0.006 0.006
    (split16 / fp32: (K + 2) u S assumes every one of K roundings at its worst; the bound's largest value is still 3.5e-3, far below
    what any defect of tests/test_conv_stack_ref.py leaves.)"""
    enc = encoders(fmt)
    families = (0, -1) if fmt in ("bf16", "fp16") else (0,)
    if fmt == "split16":
        for i in range(1, 7):
            M, K, kpat = conv_launch(i, *CASES["tiles"][:2], fmt)
            assert resolve(enc.lib, fmt, M, K, kpat, -1, 0) == resolve(enc.lib, fmt, M, K, kpat, 1000999, 0)
    if len(families) == 2:                  # the two settings are different kernels at every layer (host arithmetic)
        for i in range(1, 7):
            M, K, kpat = conv_launch(i, *CASES["tiles"][:2], fmt)
            assert resolve(enc.lib, fmt, M, K, kpat, -1, 0) != resolve(enc.lib, fmt, M, K, kpat, 1000999, 0)
    worst, kept = {}, {}
    try:
        for fam in families:
            if fmt in ("bf16", "fp16"):
                enc.set_option(_lib.OPT_GEMM_MFMA16, fam)
            for case in CASES:
                if fmt not in case_formats(case):
                    continue
                ratios, _ = check_case(enc, weights, "base", wavs, fmt, case, "mfma16=%d" % fam, kept.setdefault(fam, {}) if case == "tiles" else None)
                for i, r in ratios.items():
                    worst[(fam, i)] = max(worst.get((fam, i), 0.0), r)
    finally:
        if fmt in ("bf16", "fp16"):
            enc.set_option(_lib.OPT_GEMM_MFMA16, 0)
    for fam in families:
        print("float64 check conv stack %s mfma16=%d worst max err / bound per layer: %s" % (fmt, fam, " ".join("%.3f" % worst[(fam, i)] for i in range(1, 7))))
    if len(families) == 2:                  # (information: how often the families' fp32 sums round to different stored values)
        print("float64 check conv stack %s stored values that differ between the families at case tiles, per layer: %s"
              % (fmt, " ".join("%d" % int((kept[0][i] != kept[-1][i]).sum()) for i in range(1, 7))))
    assert max(worst.values()) <= 1.0, worst


# ---- 2. outside the GELU's polynomial core -------------------------------------------------------------------------------------------
def test_conv_layers_outside_the_gelu_core(encoders, weights, wavs):
    """the conv weights of layers 1-6 times GAIN: the GELU's argument leaves gelu_fast's polynomial core |x| <= 4.2 in every layer
    (asserted on the reference), where the kernel freezes Phi.  bf16, case "tiles".
    Measured max err / bound on MI355X (conv1 .. conv6): 0.871 0.865 0.852 0.842 0.907 0.915 (max |GELU argument| 8.1 6.3 5.5 5.1 6.5 5.9)."""
    ratios, zmax = check_case(encoders("bf16", "gain"), weights, "gain", wavs, "bf16", "tiles", "gain%.2f" % GAIN)
    assert min(zmax.values()) > 4.2, zmax
    assert max(ratios.values()) <= 1.0, ratios


# ---- 3. every kernel the benchmark shapes run ------------------------------------------------------------------------------------------
# the benchmark shapes (B, Lmax): 32 x 10 s, 8 x 60 s and the ragged batch padded to Lmax = 10 s (the same launches as 32 x 10 s: the conv
# stack runs every utterance at the padded length)
BENCH_SHAPES = ((32, 160000), (8, 960000), (32, 160000))
# (layer, kernel instantiation with the operand format left open, forced SYLBER_OPT_GEMM_TILE id that reaches it at case "tiles" -- and at
# case "rounds" for conv1 / conv2 --, the (B, Lmax, SYLBER_OPT_GEMM_MODEL) benchmark launches whose automatic pick it is)
GEMMC = "gemmc_bf16_kernel[EPI = 0, ACT = 1, FMT = %d, TAP = %s, FMV = %d]"
GEMM16 = "gemm16_bf16_kernel[FM = 2, FN = 2, EPI = 0, ACT = 1, FMT = %d, NW = 8, NSTAGE = 2]"
PRODUCTION_KERNELS = (
    (1, GEMMC % (-1, "true", 4), 47, ((32, 160000, 0), (32, 160000, 5), (8, 960000, 0), (8, 960000, 5))),
    (2, GEMMC % (-1, "true", 4), 47, ((32, 160000, 0), (32, 160000, 5), (8, 960000, 0), (8, 960000, 5))),
    (3, GEMMC % (-1, "true", 4), 47, ((32, 160000, 0), (32, 160000, 5), (8, 960000, 0), (8, 960000, 5))),
    (4, GEMMC % (-1, "true", 4), 47, ((32, 160000, 0), (32, 160000, 5), (8, 960000, 0), (8, 960000, 5))),
    (5, GEMMC % (-1, "false", 4), 47, ((32, 160000, 0), (32, 160000, 5))),
    (5, GEMMC % (-1, "false", 3), 46, ((8, 960000, 0),)),
    (5, GEMM16 % -1, 15, ((8, 960000, 5),)),
    (6, GEMM16 % -1, 15, ((32, 160000, 0), (32, 160000, 5))),
    (6, GEMMC % (-1, "false", 3), 46, ((8, 960000, 0),)),
    (6, GEMMC % (-1, "false", 4), 47, ((8, 960000, 5),)),
)


def small_cases(i):
    return ("tiles", "rounds") if i in CASES["rounds"][3] else ("tiles",)


@pytest.mark.parametrize("fmt", ("bf16", "fp16"))
def test_conv_layers_every_production_kernel(encoders, wavs, fmt):
    """PRODUCTION_KERNELS lists every kernel instantiation conv1..conv6 resolve to at the benchmark shapes under SYLBER_OPT_GEMM_MODEL 0
    and 5 with the automatic tile, and a forced tile id that resolves to the same instantiation at the small shapes here (all of them are
    members of the 16x16x32 family, so none needs SYLBER_OPT_GEMM_MFMA16 = -1, and none is left unreached).  Both are asserted through
    sylber_debug_gemm_resolve, so that a retuning fails here instead of silently testing a fallback.  Under each forced id every
    conv tap equals, bit for bit, the automatic pick's tap (results do not depend on the tile within a family), which carries the float64
    check of test_conv_layers_vs_float64 over to every production kernel."""
    enc = encoders(fmt)
    lib = enc.lib
    table = [(i, name.replace("FMT = -1", "FMT = %d" % FMT_ID[fmt]), tile, where) for i, name, tile, where in PRODUCTION_KERNELS]
    # the table is complete: exactly the automatic picks of the benchmark shapes
    seen = {}
    for B, lmax in BENCH_SHAPES:
        for model in (0, 5):
            for i in range(1, 7):
                seen.setdefault((i, resolve(lib, fmt, *conv_launch(i, B, lmax, fmt), -1, model)), set()).add((B, lmax, model))
    assert seen == {(i, name): set(where) for i, name, _, where in table}, seen
    # ... and every forced id still reaches its kernel at the small shapes
    for i, name, tile, _ in table:
        for case in small_cases(i):
            assert resolve(lib, fmt, *conv_launch(i, *CASES[case][:2], fmt), tile, 0) == name, (i, case, tile)
    want = {}
    for case in ("tiles", "rounds"):
        wav, lens = wavs(case)
        want[case] = {i: conv_tap(enc, wav, lens, i) for i in CASES[case][3]}
    try:
        for tile in sorted({t for _, _, t, _ in table}):
            enc.set_option(_lib.OPT_GEMM_TILE, tile)
            for case in ("tiles", "rounds"):
                wav, lens = wavs(case)
                for i in CASES[case][3]:
                    assert torch.equal(conv_tap(enc, wav, lens, i), want[case][i]), (tile, case, i)
    finally:
        enc.set_option(_lib.OPT_GEMM_TILE, -1)


# ---- 4. stale workspace ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ("bf16", "fp32"))
def test_conv_taps_ignore_stale_workspace(encoders, wavs, fmt):
    """case "seams": after the workspace is filled with 0xFF / 0x7F bytes (NaN patterns / large finite values in every format), rows
    [0, L_i) of every conv tap are bitwise what they were: no valid row reads a row nobody wrote, the rows behind a neighbour's valid
    ones included.  Rows at or past L_i are not asserted."""
    enc = encoders(fmt)
    wav, lens = wavs("seams")
    L = cr.conv_rows(CASES["seams"][1])
    want = {i: conv_tap(enc, wav, lens, i)[:, :L[i]].clone() for i in range(1, 7)}
    for byte in (0xFF, 0x7F):
        for i in range(1, 7):
            _lib.check(enc.lib.sylber_debug_poison_workspace(enc.handle, byte), "poison")
            assert torch.equal(conv_tap(enc, wav, lens, i)[:, :L[i]], want[i]), (byte, i)


# ---- 5. the precisions that share a conv stack -----------------------------------------------------------------------------------------
def test_conv_taps_in_fp8_and_mixed16(encoders, wavs):
    """fp8 runs the bf16 conv stack and mixed16 the fp16 one: their conv taps return those handles' bits"""
    wav, lens = wavs("seams")
    for a, b in (("fp8", "bf16"), ("mixed16", "fp16")):
        for i in range(1, 7):
            assert torch.equal(conv_tap(encoders(a), wav, lens, i), conv_tap(encoders(b), wav, lens, i)), (a, i)


# ---- 6. refusals and hygiene -------------------------------------------------------------------------------------------------------------
def test_conv_taps_are_refused_where_they_do_not_apply(encoders):
    for fmt in ("bf16", "fp32"):
        enc = encoders(fmt)
        wav = torch.from_numpy(fr.noise(1, 400, 1)).cuda()
        for stage in (_lib.TAP_CONV(0), _lib.TAP_CONV(7)):
            with pytest.raises(_lib.SylberHipError):
                enc.forward(wav, None, stop_stage=stage)
            assert enc.forward(wav, None).shape == (1, 1, 768)          # (the refused stage left the handle at stage 0)
    enc = encoders("bf16")
    _lib.check(enc.lib.sylber_set_stop_stage(enc.handle, _lib.TAP_CONV(3)), "sylber_set_stop_stage")
    try:
        with pytest.raises(_lib.SylberHipError):
            enc.forward_packed([torch.from_numpy(fr.noise(1, 400, 1)[0])])
    finally:
        enc.lib.sylber_set_stop_stage(enc.handle, 0)


@pytest.mark.parametrize("fmt", FMTS)
def test_full_forward_is_unchanged_by_conv_taps(encoders, wavs, fmt):
    """a full forward after a round of all six conv taps returns the bits it returned before them"""
    enc = encoders(fmt)
    wav, lens = wavs("seams")
    before = enc.forward(wav, lens).clone()
    for i in range(1, 7):
        conv_tap(enc, wav, lens, i)
    assert torch.equal(enc.forward(wav, lens), before)

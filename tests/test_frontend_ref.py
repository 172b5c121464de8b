"""CPU tier: the float64 references of tests/frontend_ref.py are pinned to the oracle, and their per-element bounds are shown to
REJECT subtly wrong kernels: the reference output, rounded to the stored format, passes with no element excluded, and every planted
defect (an off-by-one window, a swapped 4-channel run, a row taken from the next 256-row block, GroupNorm statistics over one frame
too few, a zero tail that starts one frame late, a nonzero halo row) fails, at every shape tests/test_gpu_frontend.py runs on the GPU.
Nothing here needs a GPU, and nothing on the GPU has to misbehave for the bounds to be trusted."""
import numpy as np
import pytest
import torch

import frontend_ref as fr
from oracle import hubert_ref
from sylber_amd.weights import synthetic_state_dict

from frontend_ref import CONV0_COMBOS, CONV0_LMAX, FMTS, POSCONV_SHAPES, PROJ_SHAPES, RAGGED_LENS, RAGGED_LMAX, conv0_weights, noise


@pytest.fixture(scope="module")
def sd():
    return synthetic_state_dict(0, num_layers=1)


def test_round_fmt():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9, 3.0e-8, 1e5, -0.1])
    b = fr.round_fmt(x, "bf16")
    assert b[:3].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -7]                         # a tie goes to even; 0.75 ulp goes up
    assert (np.abs(b - x) <= fr.store_error(np.abs(x), "bf16")).all()
    h = fr.round_fmt(x, "fp16")
    assert h[3] == 2.0 ** -24 and h[4] == 65504.0                                 # the subnormal grid; saturation, not infinity
    assert (np.abs(h - x)[[0, 1, 2, 3, 5]] <= fr.store_error(np.abs(x), "fp16")[[0, 1, 2, 3, 5]]).all()
    s = fr.round_fmt(x, "split16")
    assert s[0] == 1.0 and abs(s[5] - np.float32(-0.1)) <= 2.0 ** -22 * 0.1 and abs(s[3] - 3.0e-8) <= 2.0 ** -25
    assert np.array_equal(fr.round_fmt(x, "fp32"), x.astype(np.float32).astype(np.float64))


def test_gelu_fast_stated_error():
    """csrc/common.h's gelu_fast, restated in fp32 numpy, sits inside the error frontend_ref.gelu_error derives from its comment"""
    x = np.linspace(-40, 40, 800001).astype(np.float32)
    xc = np.clip(x, np.float32(-4.2), np.float32(4.2))
    u = xc * xc
    q = np.float32(6.949803233e-11) * u + np.float32(-6.356798643e-09)
    for c in (2.570604920e-07, -6.139445304e-06, 9.818511899e-05, -1.133762766e-03, 9.886963293e-03, -6.643489748e-02, 3.989362717e-01):
        q = q * u + np.float32(c)
    y = x * (xc * q + np.float32(0.5))
    x64 = x.astype(np.float64)
    err = np.abs(y.astype(np.float64) - fr.gelu64(x64))
    stated = np.where(np.abs(x64) <= 4.2, 6.4e-5, 2.7e-5 * np.abs(x64))           # the comment's two figures, each on its own range
    assert (err <= stated).all(), float((err / stated).max())
    assert (err <= fr.gelu_error(x64, "fast")).all()
    assert np.array_equal(fr.gelu_error(x64, "fast"), stated + 2 * fr.U * np.abs(x64))
    # an argument known to +-dz only: the larger figure where the interval straddles 4.2
    assert fr.gelu_error(np.array([4.0]), "fast", 0.1)[0] < 6.5e-5 < 1.1e-4 < fr.gelu_error(np.array([4.15]), "fast", 0.1)[0] < 1.2e-4


def test_references_agree_with_the_oracle(sd):
    """conv0, the projection and the encoder LayerNorm's input against oracle/hubert_ref.forward(collect=True) (fp32 torch) on a ragged
    batch, to the oracle's own fp32 noise: sqrt(K) u times the magnitude of the accumulated terms, K = 10 / 512 / 6144"""
    lens = (4000, 3370, 1000)
    wav = noise(3, 4000, 5, lens)
    o = hubert_ref.forward(sd, torch.from_numpy(wav), lens, num_layers=1, collect=True)
    w0, gw, gb = conv0_weights(sd)
    c0 = fr.conv0_ref(wav, w0, gw, gb)
    assert np.abs(c0["y"] - o["conv0"].numpy().transpose(0, 2, 1)).max() < 2e-5
    valid = [hubert_ref.num_frames(n) for n in lens]
    pr = fr.proj_ref(o["conv6"].numpy().transpose(0, 2, 1), valid, sd["feature_projection.layer_norm.weight"].numpy(),
                     sd["feature_projection.layer_norm.bias"].numpy(), sd["feature_projection.projection.weight"].numpy(),
                     sd["feature_projection.projection.bias"].numpy(), "fp32")
    op = o["proj"].numpy()
    for b, nv in enumerate(valid):
        assert np.abs(pr["x"][b, :nv] - op[b, :nv]).max() < 1e-4 and not pr["x"][b, nv:].any()
    pc = fr.posconv_ref(pr["x"].astype(np.float32), valid, hubert_ref.pos_conv_weight(sd).numpy(), sd["encoder.pos_conv_embed.conv.bias"].numpy(), "fp32")
    pre = torch.from_numpy(pc["out"])
    ln = torch.nn.functional.layer_norm(pre, (768,), sd["encoder.layer_norm.weight"].double(), sd["encoder.layer_norm.bias"].double(), 1e-5)
    assert np.abs(ln.numpy() - o["enc_in"].numpy()).max() < 5e-4


# ---- conv0 -----------------------------------------------------------------------------------------------------------------------
def conv0_cases():
    for lmax in CONV0_LMAX:
        yield "L%d" % lmax, noise(1, lmax, lmax), None
    rows = [(n - 10) // 5 + 1 for n in RAGGED_LENS]
    yield "ragged", noise(3, RAGGED_LMAX, 7, RAGGED_LENS), None
    yield "ragged_per_utt", noise(3, RAGGED_LMAX, 7, RAGGED_LENS), rows


def with_zero_row(y):
    return np.concatenate([y, np.zeros_like(y[:, :1])], axis=1)


@pytest.mark.parametrize("fmt,kernel", CONV0_COMBOS)
def test_conv0_bound_rejects_planted_defects(sd, fmt, kernel):
    w0, gw, gb = conv0_weights(sd)
    for name, wav, rows in conv0_cases():
        ref = fr.conv0_ref(wav, w0, gw, gb, rows)
        L0 = ref["y"].shape[1]
        yref, bound = with_zero_row(ref["y"]), with_zero_row(fr.conv0_bound(ref, fmt, kernel))     # row L0: the first of the +0 rows
        clean = fr.round_fmt(yref, fmt)
        r, _ = fr.worst_ratio(clean, yref, bound)
        assert r <= 1.0, (name, "clean", r)
        a, sh = ref["scale"][:, None], ref["shift"][:, None]

        def stored(y):
            return fr.round_fmt(with_zero_row(y), fmt)
        bad = {}
        # the window read one sample late: x[5 l + j + 1]
        late = np.concatenate([wav[:, 1:], np.zeros_like(wav[:, :1])], axis=1)
        bad["taps shifted by one"] = stored(fr.gelu64(a * (fr.conv0_windows(late) @ ref["w"].T) + sh))
        # one row of the 32 x 32 block (rows 0 .. 31, channels 32 .. 63): two runs of 4 channels exchanged
        y = clean.copy()
        y[:, 5, 36:40], y[:, 5, 40:44] = clean[:, 5, 40:44], clean[:, 5, 36:40]
        bad["4-channel run swapped"] = y
        if L0 >= 256:                       # (no live row at a block edge below that)
            e = 256 * (L0 // 256) - 1
            y = clean.copy()
            y[:, e] = clean[:, e + 1]
            bad["block-edge row from the next block"] = y
        n1 = ref["n"] - 1
        bad["statistics over one frame too few"] = stored(fr.conv0_ref(wav, w0, gw, gb, n1)["y"])
        for what, y in bad.items():
            r, _ = fr.worst_ratio(y, yref, bound)
            assert r > 1.0, (name, what, r)


def test_conv0_stats_bound_rejects_wrong_frame_count(sd):
    """the scale / shift table itself: float64 statistics over n - 1 frames are outside conv0_stats_bound at every shape"""
    w0, gw, gb = conv0_weights(sd)
    for name, wav, rows in conv0_cases():
        ref = fr.conv0_ref(wav, w0, gw, gb, rows)
        da, db = fr.conv0_stats_bound(ref)
        a32, b32 = ref["scale"].astype(np.float32), ref["shift"].astype(np.float32)
        assert (np.abs(a32 - ref["scale"]) <= da).all() and (np.abs(b32 - ref["shift"]) <= db).all(), name
        off = fr.conv0_ref(wav, w0, gw, gb, ref["n"] - 1)
        assert (np.abs(off["scale"] - ref["scale"]) > da).any() and (np.abs(off["shift"] - ref["shift"]) > db).any(), name


# ---- projection ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PROJ_SHAPES, ids=lambda s: "T%d" % s[0])
@pytest.mark.parametrize("fmt", FMTS)
def test_proj_bound_rejects_planted_defects(sd, fmt, shape):
    T, valid = shape
    g = np.random.default_rng(T)
    feats = fr.round_fmt(np.abs(g.standard_normal((len(valid), T, 512))) * 0.5, fmt)          # (GELU outputs: mostly positive)
    W = sd["feature_projection.projection.weight"].numpy()
    bias = sd["feature_projection.projection.bias"].numpy() + 8.0
    ref = fr.proj_ref(feats, valid, sd["feature_projection.layer_norm.weight"].numpy(), sd["feature_projection.layer_norm.bias"].numpy(), W, bias, fmt)
    bound = fr.proj_bound(ref, fmt)
    # what the kernel computes: the 16-bit LayerNorm output times the 16-bit weights
    full = fr.round_fmt(ref["ln"], fmt) @ ref["W"].T + bias
    clean = np.where(ref["keep"][:, :, None], full, 0.0).astype(np.float32)
    r, _ = fr.worst_ratio(clean, ref["x"], bound)
    assert r <= 1.0, r
    assert bound.max() < 0.125           # (looser than the others, still far below the O(8) error of a zeroing off-by-one)
    b = 1                                 # an utterance with a zero tail
    late = clean.copy()
    late[b, valid[b]] = full[b, valid[b]]
    assert fr.worst_ratio(late, ref["x"], bound)[0] > 1.0, "zero tail one frame late"
    shifted = clean.copy()
    shifted[0, 1:] = clean[0, :-1]
    assert fr.worst_ratio(shifted, ref["x"], bound)[0] > 1.0, "rows shifted by one"
    y = clean.copy()
    y[0, 0, 36:40], y[0, 0, 40:44] = clean[0, 0, 40:44], clean[0, 0, 36:40]
    assert fr.worst_ratio(y, ref["x"], bound)[0] > 1.0, "4-channel run swapped"
    if T > 256:
        y = clean.copy()
        y[0, 255] = clean[0, 256]
        assert fr.worst_ratio(y, ref["x"], bound)[0] > 1.0, "block-edge row from the next block"


# ---- pos-conv --------------------------------------------------------------------------------------------------------------------
def posconv_input(T, valid, seed):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((len(valid), T, 768)) + 8.0).astype(np.float32)
    for b, nv in enumerate(valid):
        x[b, nv:] = 0
    return x


@pytest.mark.parametrize("shape", POSCONV_SHAPES, ids=lambda s: "T%d" % s[0])
@pytest.mark.parametrize("fmt", FMTS)
def test_posconv_bound_rejects_planted_defects(sd, fmt, shape):
    w = hubert_ref.pos_conv_weight(sd).numpy()
    bias = sd["encoder.pos_conv_embed.conv.bias"].numpy()
    wr = fr.posconv_weights(w, fmt)
    for T, valid in (shape,):
        x = posconv_input(T, valid, T)
        ref = fr.posconv_ref(x, valid, w, bias, fmt, wr=wr)
        bound = fr.posconv_bound(ref, fmt)
        clean = ref["out"].astype(np.float32)
        r, _ = fr.worst_ratio(clean, ref["out"], bound)
        assert r <= 1.0, (T, "clean", r)
        xpad = fr.posconv_xpad(x, valid, fmt)
        # defects that change the operand are planted in one utterance (the last: the shortest valid count) and recomputed for it alone
        b = len(valid) - 1
        nv = valid[b]
        sl = slice(b, b + 1)
        filler = fr.round_fmt(posconv_input(1, (1,), 99)[0, 0], fmt)

        def one(xp, **kw):
            return fr.posconv_from_xpad(xp, x[sl], w, bias, fmt, wr=wr, **kw)["out"].astype(np.float32)
        bad = {}
        bad["taps shifted by one"] = one(xpad[sl], tap_shift=1)
        xp = xpad[sl].copy()
        xp[0, 63] = filler
        bad["front halo row nonzero"] = one(xp)
        xp = xpad[sl].copy()
        xp[0, 64 + nv] = filler                     # frame valid_b: the first of the zero tail, or of the rear halo when valid_b = T
        bad["zero tail one frame late"] = one(xp)
        for what, y in bad.items():
            r, _ = fr.worst_ratio(y, ref["out"][sl], bound[sl])
            assert r > 1.0, (T, what, r)
        y = clean.copy()
        y[0, 0, 36:40], y[0, 0, 40:44] = clean[0, 0, 40:44], clean[0, 0, 36:40]
        assert fr.worst_ratio(y, ref["out"], bound)[0] > 1.0, (T, "4-channel run swapped")
        if T > 256:
            y = clean.copy()
            y[0, 255] = clean[0, 256]
            assert fr.worst_ratio(y, ref["out"], bound)[0] > 1.0, (T, "block-edge row from the next block")

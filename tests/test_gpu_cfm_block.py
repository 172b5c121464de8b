"""GPU tier: one decoder block per element against float64, launch by launch, through the decoder's taps (sylber_cfm_set_tap,
include/sylber_hip_dev.h).  Every stage is referenced from the ACTUAL values of the tap in front of it (tests/cfm_block_ref.py), so each
comparison tests one kernel with a bound derived from that kernel's arithmetic, and asserts max |tap - reference| / bound <= 1 over every
element of every row (slack excluded, padding included); tests/test_cfm_block_ref.py shows on the CPU that these bounds reject the
planted defects.  Exact checks ride along: the rows behind a clip in X0 are +0, the register rows are the checkpoint's bits, heads 8..11
of Q / K / V^T / CTX (and of QKVF) are +0, columns 1365..1407 of G are +0 (where the reference is 0 its bound is 0, so the ratio check holds them
as well; the bit patterns are compared on top).  Each distinct call's taps and float64 references are made once per module (Call.of), on
at most 16 CPU threads.

Measured max err / bound on MI355X, smallest .. largest over every test of this file (lone clips, the B = 3 batch's blocks 0 / 1 / 7,
frames=, packed, T = 2999, trained scale):
    stage    fp32              bf16              fp16
    GB       0.0001            0.0001            0.0001      (one fp32 kernel in every mode)
    CONDX    0.011 .. 0.023    0.003 .. 0.007    0.004 .. 0.007
    XE       0.23 .. 0.50      0.26 .. 0.51      0.26 .. 0.51
    X0       0.08 .. 0.68      0.07 .. 0.64      0.09 .. 0.76
    H_ATTN   0.54 .. 0.93      0.9994 .. 0.9999  0.998 .. 0.9995
    QKV      0.008 .. 0.012    0.002 .. 0.005    0.002 .. 0.004
    Q        -                 0.9994 .. 0.9997  0.9974 .. 0.9979
    K        -                 0.9994 .. 0.9997  0.9972 .. 0.9979
    VT       -                 0.9999 .. 1.0000  1.0000
    QKVF     0.21 .. 0.29      -                 -
    CTX      0.014 .. 0.023    0.45 .. 0.85      0.42 .. 0.60
    X_ATTN   0.006 .. 0.010    0.003 .. 0.005    0.003 .. 0.006
    H_FF     0.63 .. 0.91      0.9994 .. 0.9999  0.998 .. 0.9998
    FF       0.008 .. 0.015    0.003 .. 0.004    0.003 .. 0.005
    G        0.48 .. 0.56      0.9997 .. 0.9999  0.9990 .. 0.9995
    X_FF     0.004 .. 0.006    0.001 .. 0.003    0.001 .. 0.003
    final    0.014 .. 0.017    0.013 .. 0.019    0.017 .. 0.023
Above 0.9: H_ATTN, H_FF, Q, K, VT and G in the 16-bit modes are the store's half-ulp in the stage's format, which a round-to-nearest store
reaches (VT is that store and nothing else: a tie gives exactly 1); H_ATTN / H_FF in fp32 are the half-ulp of the last add where the
gamma term is small beside beta.  Below 0.001: GB -- its bound adds the absolute errors of two chains of 512 and 2048 terms and
SINCOS_ERR times sum |w| as if they all pointed one way, and the rounding errors of a sum that long mostly cancel.  The whole file
takes about 10 s on an MI355X host."""
import ctypes

import numpy as np
import pytest
import torch

import cfm_block_ref as cb
from cfm_block_ref import FI, FIP, Geom, LONE_T, RAGGED, REG, block_stages
from frontend_ref import worst_ratio
from guarded_alloc import three_runs

pytestmark = pytest.mark.gpu

PRECS = ("fp32", "bf16", "fp16")
T_EVAL = 0.37
DEV = "cuda:0"


def _stage_id(st, li=0):
    from sylber_amd import _lib
    front = {"condx": _lib.CFM_TAP_CONDX, "gb": _lib.CFM_TAP_GB, "xe": _lib.CFM_TAP_XE, "x0": _lib.CFM_TAP_X0}
    if st in front:
        return front[st]
    return _lib.CFM_TAP(li, getattr(_lib, "CFM_BTAP_" + st.upper()))


_SD, _DEC, _W, _GB, _CALLS, _REFS = {}, {}, {}, {}, {}, {}


@pytest.fixture(autouse=True)
def _at_most_16_threads():
    """the float64 references are numpy (BLAS) and torch products on the CPU: both pools are held to 16 threads while a test runs"""
    old = torch.get_num_threads()
    torch.set_num_threads(min(16, old))
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:                       # (then the BLAS pool's size is the environment's, OMP_NUM_THREADS and its like)
        threadpool_limits = None
    try:
        if threadpool_limits is None:
            yield
        else:
            with threadpool_limits(limits=16):
                yield
    finally:
        torch.set_num_threads(old)


def _sd(gamma=None):
    if gamma not in _SD:
        from sylber_amd.weights import synthetic_regressor_state_dict
        sd = synthetic_regressor_state_dict(0)
        _SD[gamma] = sd if gamma is None else cb.with_qk_gamma(sd, gamma)
    return _SD[gamma]


def _decoder(prec, gamma=None):
    from sylber_amd.synthesis import CfmDecoder
    if (prec, gamma) not in _DEC:
        _DEC[(prec, gamma)] = CfmDecoder(_sd(gamma), device=DEV, precision=prec)
    return _DEC[(prec, gamma)]


def _weights(prec, gamma=None):
    """the packed float64 weights, once per module and format"""
    if (prec, gamma) not in _W:
        _W[(prec, gamma)] = cb.pack_weights(_sd(gamma), prec)
    return _W[(prec, gamma)]


def _gb_ref(prec, t):
    if (prec, t) not in _GB:
        _GB[(prec, t)] = cb.gb_ref(_weights(prec), t)
    return _GB[(prec, t)]


def _plus_zero(a):
    return not np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).any()


class Call:
    """one decoder call that can be repeated with a tap: kind "eval" (t = T_EVAL or ``t``), "frames" (sample(frames=), steps 2) or
    "packed" (sample_packed, steps 2); the clips' inputs are cb.clip's, zero padded.  Call.of: one object per distinct call of the
    module, so that a tap is fetched and a stage's reference computed once however many tests look at it"""

    @classmethod
    def of(cls, prec, Ts, kind="eval", t=T_EVAL, gamma=None):
        key = (prec, tuple(Ts), kind, t if kind == "eval" else 0.0, gamma)
        if key not in _CALLS:
            _CALLS[key] = cls(prec, Ts, kind, t, gamma)
            _CALLS[key].key = key
        return _CALLS[key]

    def __init__(self, prec, Ts, kind="eval", t=T_EVAL, gamma=None):
        self.key = None
        self.prec, self.Ts, self.kind, self.gamma = prec, list(Ts), kind, gamma
        self.t = t if kind == "eval" else 0.0
        self.dec = _decoder(prec, gamma)
        self.g = Geom(self.Ts, {"eval": "padded", "frames": "frames", "packed": "packed"}[kind])
        cond, y = cb.padded(self.Ts)
        if kind == "packed":
            self.cond = [cond[b, :T] for b, T in enumerate(self.Ts)]
            self.y = [y[b, :T] for b, T in enumerate(self.Ts)]
        else:
            self.cond, self.y = list(cond), list(y)
        self._dev = (cond.to(DEV), y.to(DEV))
        self.taps = {}

    def run(self, tap=None):
        cond, y = self._dev
        if self.kind == "eval":
            return self.dec.eval(y, self.t, cond, tap=tap)
        if self.kind == "frames":
            return self.dec.sample(cond, steps=2, y0=y, pitch_amp=5, frames=self.Ts, tap=tap)
        return self.dec.sample_packed([c.to(DEV) for c in self.cond], steps=2, y0=torch.cat(self.y).to(DEV), pitch_amp=5, tap=tap)[0]

    def tap(self, st, li=0):
        """the tap of stage st of block li, split per clip (fetched once)"""
        if (st, li) not in self.taps:
            a = self.run(_stage_id(st, li)).cpu().numpy()
            self.taps[(st, li)] = a.reshape(16, 2, 512) if st == "gb" else self.g.split(st, a)
        return self.taps[(st, li)]

    def clip_taps(self, b, li, stages, x_in=None):
        """clip b's values around block li by name, as cfm_block_ref.stage_refs takes them"""
        t = {"cond": self.cond[b].numpy(), "y": self.y[b].numpy(), "gb": self.tap("gb")}
        names = set(stages) | ({"condx", "xe", "x0"} if li == 0 else set())
        for st in names:
            t[st] = self.tap(st, li)[b]
        t["x_in"] = t["x0"] if li == 0 else (self.tap("x_ff", li - 1)[b] if x_in is None else x_in)
        return t


def check_stages(call, li, stages, fails, front=None):
    """every stage of ``stages`` (and, for block 0, the front stages) of every clip against its reference: ratio <= 1; the exact checks"""
    prec, W = call.prec, _weights(call.prec, call.gamma)
    front = (li == 0) if front is None else front
    names = (cb.FRONT if front else ()) + tuple(stages)
    for b, c in enumerate(call.g.clips):
        t = call.clip_taps(b, li, names)
        rk = (call.key, b, li, names)
        if call.key is None or rk not in _REFS:
            _REFS[rk] = cb.stage_refs(t, W, c, li, prec, names)
        refs = _REFS[rk]
        for st in names:
            ref, bound = refs[st]
            r, at = worst_ratio(t[st], ref, bound)
            tag = "%s %s T=%s clip %d block %d %s" % (prec, call.kind, call.Ts, b, li, st)
            print("MEAS %s ratio %.4f at %s largest bound %.3e" % (tag, r, at, float(np.max(bound))))
            if not (np.isfinite(t[st]).all() and r <= 1.0):
                fails.append("%s: max err / bound %.4f at %s" % (tag, r, at))
        # ---- bit for bit
        nv, R = c["nv"], c["R"]
        if front:
            reg = _sd(call.gamma)["transformer.register_tokens"].float().numpy()
            if not np.array_equal(t["x0"][:REG].view(np.uint32), reg.view(np.uint32)):
                fails.append("%s clip %d: register rows of X0 differ from the checkpoint's bits" % (prec, b))
            if not _plus_zero(t["x0"][nv:R]):
                fails.append("%s clip %d: rows [%d, %d) of X0 are not +0" % (prec, b, nv, R))
        for st in names:
            if st in ("q", "k", "vt") and not _plus_zero(t[st][8:]):
                fails.append("%s clip %d block %d: heads 8..11 of %s are not +0" % (prec, b, li, st))
            if st == "ctx" and not _plus_zero(t[st][:, 512:]):
                fails.append("%s clip %d block %d: heads 8..11 of CTX are not +0" % (prec, b, li))
            if st == "qkvf" and not _plus_zero(t[st].reshape(R, 3, 12, 64)[:, :, 8:]):
                fails.append("%s clip %d block %d: heads 8..11 of QKVF are not +0" % (prec, b, li))
            if st == "g" and not _plus_zero(t[st][:, FI:FIP]):
                fails.append("%s clip %d block %d: columns 1365..1407 of G are not +0" % (prec, b, li))


def check_gb(call, fails):
    ref, bound = _gb_ref(call.prec, call.t)
    r, at = worst_ratio(call.tap("gb"), ref, bound)
    print("MEAS %s GB t=%.2f ratio %.4f at %s largest bound %.3e" % (call.prec, call.t, r, at, float(bound.max())))
    if not r <= 1.0:
        fails.append("%s GB t=%.2f: max err / bound %.4f at %s" % (call.prec, call.t, r, at))


# ---- block 0, every stage, lone clips --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", LONE_T)
@pytest.mark.parametrize("prec", PRECS)
def test_block0_lone_clip(prec, T):
    """eval at t = 0.37 of one clip: L = 16 + T of 17 .. 129, on both sides of the 32-row pitch, the 64-key tile and Tpv, the 128-query
    block; clips shorter than the conv's 31-tap window and of its half-width.  Measured: the module docstring's table."""
    call = Call.of(prec, [T])
    fails = []
    check_gb(call, fails)
    check_stages(call, 0, block_stages(prec), fails)
    assert not fails, fails


# ---- blocks 0, 1 and 7, every stage, plus the final launch -------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_blocks_0_1_7_and_final(prec):
    """one padded batch, B = 3, T = 113 (M = 480: ragged against the 128- and 256-row GEMM tiles): blocks 1 and 7 show a wrong per-block
    offset of the weights, biases, q / k gammas and norm index; the call's own output is referenced from X_FF of block 7"""
    call = Call.of(prec, RAGGED)
    fails = []
    for li in (0, 1, 7):
        check_stages(call, li, block_stages(prec), fails)
    out = call.g.split("final", call.run().cpu().numpy())
    W = _weights(prec)
    for b, c in enumerate(call.g.clips):
        ref, bound = cb.final_ref(call.tap("x_ff", 7)[b], W, c)
        r, at = worst_ratio(out[b], ref, bound)
        print("MEAS %s final clip %d ratio %.4f at %s largest bound %.3e" % (prec, b, r, at, float(bound.max())))
        if not r <= 1.0:
            fails.append("%s final clip %d: max err / bound %.4f at %s" % (prec, b, r, at))
    assert not fails, fails


# ---- frames= and packed -----------------------------------------------------------------------------------------------------------------------
def _clip_rows(st, a, c):
    """the clip's own part of one split tap: its 16 + Tb rows (frame stages: Tb frames; V^T: its keys in natural order)"""
    nv = c["nv"]
    if st in ("condx", "xe"):
        return a[:c["Tb"]]
    if st in ("q", "k"):
        return a[:, :nv]
    if st == "vt":
        import encoder_layer_ref as el
        return a[:, :, el.vt_key_permutation(c["R"])][:, :, :nv]
    return a[:nv]


@pytest.mark.parametrize("prec", PRECS)
def test_frames_and_packed(prec):
    """the clips (113, 48, 1), steps 2, the first evaluation (t = 0, state y0): every stage of block 0 inside its bound for the frames=
    call and (bf16 / fp16) the packed call, and each clip's rows in the packed taps bit for bit the frames= call's rows of that clip,
    stage by stage -- the library promises it for the output; here it holds at every launch"""
    fails = []
    fr = Call.of(prec, RAGGED, "frames")
    check_gb(fr, fails)
    check_stages(fr, 0, block_stages(prec), fails)
    if prec != "fp32":
        pk = Call.of(prec, RAGGED, "packed")
        check_stages(pk, 0, block_stages(prec), fails)
        if not np.array_equal(pk.tap("gb").view(np.uint32), fr.tap("gb").view(np.uint32)):
            fails.append("%s: GB differs between the packed and the frames= call" % prec)
        for st in cb.FRONT + block_stages(prec):
            for b, (cp, cf) in enumerate(zip(pk.g.clips, fr.g.clips)):
                a, f = _clip_rows(st, pk.tap(st)[b], cp), _clip_rows(st, fr.tap(st)[b], cf)
                if a.shape != f.shape or not np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(f).view(np.uint32)):
                    fails.append("%s %s clip %d: the packed rows are not the frames= rows bit for bit" % (prec, st, b))
    assert not fails, fails


# ---- the time conditioning ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_gb_table(prec):
    """the gamma / beta table [16, 2, 512] of time index 0 at t = 0, 0.37 and 1.0 through eval"""
    fails = []
    for t in (0.0, 0.37, 1.0):
        check_gb(Call.of(prec, [17], t=t), fails)
    assert not fails, fails


# ---- the long clip -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_long_clip_front_of_block0(prec):
    """T = 2999: the front and block 0 up to Q / K / V^T (QKVF): rotary angles near 3000 rad beside the registers' -10000"""
    call = Call.of(prec, [2999])
    fails = []
    check_stages(call, 0, ("h_attn", "qkv") + (("qkvf",) if prec == "fp32" else ("q", "k", "vt")), fails)
    assert not fails, fails


# ---- trained scale --------------------------------------------------------------------------------------------------------------------------------
def test_trained_scale_attention():
    """q / k gammas 1.0 (upstream's initial value), bf16, the T = 113 batch, stages Q, K, V^T and CTX of block 0: the reference's scores
    exceed 100 in log2 units (tests/test_cfm_block_ref.py shows the clip meets the condition on the CPU), where the decoder's OUTPUT is
    ill-conditioned (tests/test_gpu_decoder_ref.py) and each launch is not"""
    call = Call.of("bf16", RAGGED, gamma=1.0)
    for b, c in enumerate(call.g.clips):
        t = call.clip_taps(b, 0, ("q", "k", "vt"))
        s = cb.ctx_ref(t, "bf16", c)[2]["s"]
        assert np.abs(s[np.isfinite(s)]).max() > 100.0
    fails = []
    check_stages(call, 0, ("h_attn", "qkv", "q", "k", "vt", "ctx"), fails, front=False)
    assert not fails, fails


# ---- the facility ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_taps_leave_results_alone_and_refusals_hold(prec):
    """after a round of taps eval and sample return the bits they returned before; an unknown stage, a tap buffer that is too small and a
    tap on sample(steps=1) are refused with an error text, and the tap buffer is not touched"""
    from sylber_amd import _lib
    call = Call.of(prec, [49])
    dec, lib = call.dec, _lib.load()
    cond, y = call._dev
    before = (dec.eval(y, T_EVAL, cond).cpu(), dec.sample(cond, steps=3, y0=y, pitch_amp=5).cpu())
    for st in cb.FRONT + block_stages(prec):
        call.tap(st, 3)
    dec.sample(cond, steps=2, y0=y, tap=_stage_id("x_ff", 7))
    # ---- refusals
    for stage in (5, 15, 16 + 12, _lib.CFM_TAP(8, 0), -1, _stage_id("qkvf" if prec != "fp32" else "q")):
        assert lib.sylber_cfm_tap_floats(dec.handle, stage, 1, 49) == -1
        assert lib.sylber_cfm_set_tap(dec.handle, stage, ctypes.c_void_p(cond.data_ptr()), 1 << 20) != 0 and lib.sylber_last_error()
        with pytest.raises(ValueError):
            dec.eval(y, T_EVAL, cond, tap=stage)
    n = int(lib.sylber_cfm_tap_floats(dec.handle, _stage_id("x0"), 1, 49))
    assert n == call.g.M * 512
    buf = torch.full((n,), 7.0, device=DEV)
    assert lib.sylber_cfm_set_tap(dec.handle, _stage_id("x0"), ctypes.c_void_p(buf.data_ptr()), n - 1) == 0
    try:
        with pytest.raises(_lib.SylberHipError, match="too small"):
            dec.eval(y, T_EVAL, cond)
        assert lib.sylber_cfm_set_tap(dec.handle, _stage_id("x0"), ctypes.c_void_p(buf.data_ptr()), n) == 0
        with pytest.raises(_lib.SylberHipError, match="steps"):
            dec.sample(cond, steps=1, y0=y)
    finally:
        assert lib.sylber_cfm_set_tap(dec.handle, 0, None, 0) == 0
    with pytest.raises(_lib.SylberHipError, match="steps"):
        dec.sample(cond, steps=1, y0=y, tap=_stage_id("x0"))
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    after = (dec.eval(y, T_EVAL, cond).cpu(), dec.sample(cond, steps=3, y0=y, pitch_amp=5).cpu())
    for a, b in zip(before, after):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_tap_writes_exactly_its_floats(prec):
    """guard bands (tests/guarded_alloc.py) around the tap buffer, the inputs and the workspace: a tapped eval, frames= and packed call
    writes the floats its size query returns and nothing outside them, at T = 9 and T = 50 (B = 2)"""
    from sylber_amd import _lib
    dec, lib = _decoder(prec), _lib.load()
    gen = torch.Generator().manual_seed(15)
    stages = ["condx", "gb", "xe", "x0"] + (["qkvf"] if prec == "fp32" else ["q", "vt"]) + ["g", "x_ff"]
    for T in (9, 50):
        cond = torch.randn(2, T, 256, generator=gen).to(DEV)
        xs = torch.randn(2, T, 14, generator=gen).to(DEV)
        for st in stages:
            sid = _stage_id(st, 7 if st == "x_ff" else 0)
            n = int(lib.sylber_cfm_tap_floats(dec.handle, sid, 2, T))
            assert n > 0

            def run(g):
                c, x = (cond, xs) if g is None else (g.guarded_copy(cond, "cond_emb"), g.guarded_copy(xs, "x"))
                return dec.eval(x, 0.3, c, tap=sid), dec.sample(c, steps=2, y0=x, frames=[T, 7], tap=sid)
            plain, guarded = three_runs(run)
            for g, res in guarded:
                for a, b in zip(plain, res):
                    assert a.numel() == n and g.covers(b) and g.handed_out(4 * n)
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if prec == "bf16":
        packed = torch.randn(59, 256, generator=gen).to(DEV)
        farr = (ctypes.c_int32 * 2)(9, 50)
        for st in stages:
            sid = _stage_id(st, 7 if st == "x_ff" else 0)
            n = int(lib.sylber_cfm_tap_floats_packed(dec.handle, sid, farr, 2))
            assert n > 0

            def run(g):
                return dec.sample_packed((packed if g is None else g.guarded_copy(packed, "cond"), [9, 50]), steps=2, tap=sid)[0]
            plain, guarded = three_runs(run)
            for g, res in guarded:
                assert plain.numel() == n and g.covers(res) and g.handed_out(4 * n)
                assert torch.equal(plain.view(torch.int32), res.view(torch.int32))

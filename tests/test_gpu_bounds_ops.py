"""GPU tier, guard bands (tests/guarded_alloc.py) around the single-op entry points of include/sylber_hip.h, called through ctypes as
test_gpu_ops.py / test_gpu_fp8.py call them: sylber_op_linear (bf16, split16 and MXFP8 operands), sylber_op_linear16,
sylber_op_conv3, sylber_op_linear_resln (``pre`` is input and output), sylber_op_layernorm, sylber_op_attention (bf16 and fp8 cores)
and sylber_op_mx_quantize, at the smallest shapes with ragged row / column tails against every tile.

Every case runs once on plain ``torch.empty`` buffers and once per fill byte (0xFF, 0x00) with EVERY operand and output between
guards: ``check()`` finds any byte written before or after an operand or output, and the three outputs must be bit-identical -- so
every element is written, and none depends on what lies next to an operand.  No tolerances: the values themselves are
test_gpu_ops.py's and test_gpu_fp8.py's business.

Findings: none -- no guard was dirty and no result moved with the fill on an MI355X."""
import ctypes

import pytest
import torch

from guarded_alloc import FILLS, Guards

pytestmark = pytest.mark.gpu

BF16, FP8, SPLIT16 = 0, 2, 5
EVERY_TILE = [0, 1, 2, 3, 4, 5, 6, 10, 11, 40, 51, 57, 60, 80, 85, 90, 91, 95, 97]          # test_linear_every_tile_config
MFMA16 = [47, 97, 46, 13, 14, 15, 16, 17, 9047]                                              # test_mfma16_family
ROLE16 = [-1, 47, 46, 13, 14, 15, 16, 17, 1, 97, 57, 3, 4, 10, 85, 91, 1000097, 1000004, 1000999]   # test_mfma16_role_16bit_outputs
CONV3 = [-1, 47, 13, 14, 15, 16, 17, 1000097] + [1000000 + t for t in (9010, 97, 1, 2, 3, 4, 5, 6, 11, 40, 85, 999)]


@pytest.fixture(scope="module")
def lib():
    from sylber_amd import _lib
    assert torch.cuda.is_available(), "gpu tier needs the MI355X"
    return _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _Bufs:
    """operands and outputs of one run: plain torch buffers (``g`` None) or guarded ones"""

    def __init__(self, g):
        self.g = g
        self.outs = []

    def inp(self, t, name):
        if t is None:
            return None
        return t.cuda() if self.g is None else self.g.guarded_copy(t.cuda(), name)

    def out(self, shape, dtype, name):
        t = torch.empty(shape, dtype=dtype, device="cuda") if self.g is None else self.g.guarded(shape, dtype, "cuda", name)
        self.outs.append(t)
        return t


def _three(call):
    """``call(bufs) -> [outputs]`` plainly and under both fills; guards checked, outputs guarded and bit-identical"""
    plain = call(_Bufs(None))
    torch.cuda.synchronize()
    for fill in FILLS:
        g = Guards(fill)
        b = _Bufs(g)
        got = call(b)
        g.check()
        assert b.outs and all(g.covers(t) for t in b.outs) and all(g.covers(t) for t in got)
        assert len(got) == len(plain)
        for x, y in zip(got, plain):
            assert x.shape == y.shape and x.dtype == y.dtype
            assert torch.equal(x.view(-1).view(torch.uint8), y.view(-1).view(torch.uint8)), "fill 0x%02X" % fill


def test_the_check_sees_device_writes():
    """the positive control on the device itself: one byte written (by torch, inside the allocation) just before and just after a
    guarded buffer of an odd size is reported; the untouched buffer beside it is not"""
    for fill in FILLS:
        for side in ("front", "rear"):
            g = Guards(fill)
            g.guarded((5, 7), torch.float32, "cuda", "innocent")
            t = g.guarded((1003,), torch.uint8, "cuda", "victim")
            b = g.live[-1]
            assert t.is_cuda and t.data_ptr() % 256 == 0 and b.raw.data_ptr() + b.off == t.data_ptr()
            b.raw[b.off - 1 if side == "front" else b.off + b.nbytes] = 0x5A
            with pytest.raises(AssertionError) as e:
                g.check()
            msg = str(e.value)
            assert "%s guard of 'victim' (1003 bytes)" % side in msg and ("first at -1" if side == "front" else "first at +0") in msg
            assert "innocent" not in msg


def _operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)


@pytest.mark.parametrize("M,N,K", [(257, 768, 3072), (333, 3072, 768), (130, 512, 64), (200, 512, 192)])
def test_linear_fp32_out(lib, M, N, K):
    from sylber_amd import _lib
    a, w, bias = _operands(M, N, K, M + N + K)
    for tile in [-1] + EVERY_TILE + [t for t in MFMA16 if t not in EVERY_TILE]:
        if K < 256 and tile in (46, 47, 97, 9047):
            continue                                    # the generated loops need four K steps (test_mfma16_family)

        def call(b, tile=tile):
            ad, wd, bd = b.inp(a, "a"), b.inp(w, "w"), b.inp(bias, "bias")
            c = b.out((M, N), torch.float32, "c tile %d" % tile)
            _lib.check(lib.sylber_op_linear(_p(ad), _p(wd), _p(bd), _p(c), M, N, K, 1, BF16, tile, None), "op_linear")
            return [c]
        _three(call)


@pytest.mark.parametrize("tile", [-1, 3, 4, 10])
def test_linear_split16(lib, tile):
    from sylber_amd import _lib
    M, N, K = 257, 768, 3072
    a, w, bias = _operands(M, N, K, 5)

    def call(b):
        ad, wd, bd = b.inp(a, "a"), b.inp(w, "w"), b.inp(bias, "bias")
        c = b.out((M, N), torch.float32, "c")
        _lib.check(lib.sylber_op_linear(_p(ad), _p(wd), _p(bd), _p(c), M, N, K, 0, SPLIT16, tile, None), "op_linear split16")
        return [c]
    _three(call)


@pytest.mark.parametrize("M,N,K", [(257, 512, 1536), (1000, 512, 1024)])
def test_linear16(lib, M, N, K):
    from sylber_amd import _lib
    a, w, bias = _operands(M, N, K, 48)
    for tile in ROLE16:
        def call(b, tile=tile):
            ad, wd, bd = b.inp(a, "a"), b.inp(w, "w"), b.inp(bias, "bias")
            c = b.out((M, N), torch.int16, "c16 tile %d" % tile)
            _lib.check(lib.sylber_op_linear16(_p(ad), _p(wd), _p(bd), _p(c), M, N, K, 1, BF16, tile, None), "op_linear16")
            return [c]
        _three(call)


def test_conv3(lib):
    """M = 257 output rows from exactly the R = 2 M + 1 = 515 input rows the header asks for"""
    from sylber_amd import _lib
    M, R = 257, 515
    g = torch.Generator().manual_seed(77)
    x = torch.randn(R, 512, generator=g)
    wc = (torch.randn(512, 512, 3, generator=g) / (3 * 512) ** 0.5).contiguous()        # host memory
    for tile in CONV3:
        def call(b, tile=tile):
            xd = b.inp(x, "x")
            y = b.out((M, 512), torch.int16, "y16 tile %d" % tile)
            _lib.check(lib.sylber_op_conv3(_p(xd), ctypes.c_void_p(wc.data_ptr()), _p(y), R, M, tile, None), "op_conv3")
            return [y]
        _three(call)


@pytest.mark.parametrize("M,N,K", [(1000, 768, 768), (512, 384, 1152)])
def test_linear_resln(lib, M, N, K):
    """in place: ``pre`` is read and written, so it is a guarded copy in every run"""
    from sylber_amd import _lib
    g = torch.Generator().manual_seed(41)
    a = torch.randn(M, K, generator=g); w = torch.randn(N, K, generator=g) / K ** 0.5; bias = torch.randn(N, generator=g)
    pre = torch.randn(M, N, generator=g) * 2.0 + 0.3
    gamma = 1.0 + 0.2 * torch.randn(N, generator=g); beta = 0.1 * torch.randn(N, generator=g)
    stats = torch.stack([pre.mean(-1), (pre.var(-1, unbiased=False) + 1e-5).rsqrt()], -1).contiguous()
    for tile in (9004, 1, 2, 4, 5, 6, 51, 90, 91, 96):
        def call(b, tile=tile):
            ad, wd, bd, sd, gd, bed = (b.inp(t, n) for t, n in ((a, "a"), (w, "w"), (bias, "bias"), (stats, "stats"), (gamma, "gamma"), (beta, "beta")))
            c = b.inp(pre, "pre tile %d" % tile)
            b.outs.append(c)
            _lib.check(lib.sylber_op_linear_resln(_p(ad), _p(wd), _p(bd), _p(c), _p(sd), _p(gd), _p(bed), M, N, K, tile, None), "op_linear_resln")
            return [c]
        _three(call)


@pytest.mark.parametrize("D", [512, 768])
@pytest.mark.parametrize("res", [True, False])
def test_layernorm(lib, D, res):
    from sylber_amd import _lib
    g = torch.Generator().manual_seed(D)
    x = torch.randn(777, D, generator=g) * 3 + 0.5
    r = torch.randn(777, D, generator=g) if res else None
    gam, bet = torch.randn(D, generator=g), torch.randn(D, generator=g)

    def call(b):
        xd, rd, gd, bd = b.inp(x, "x"), b.inp(r, "res"), b.inp(gam, "gamma"), b.inp(bet, "beta")
        y = b.out((777, D), torch.float32, "y")
        _lib.check(lib.sylber_op_layernorm(_p(xd), _p(rd), _p(gd), _p(bd), _p(y), 777, D, None), "op_layernorm")
        return [y]
    _three(call)


@pytest.mark.parametrize("precision,qpw", [(BF16, 0), (BF16, 32), (BF16, 64), (FP8, 0)])
@pytest.mark.parametrize("B,T,valid", [(2, 1, None), (2, 33, [33, 32]), (3, 143, [143, 100, 1]), (3, 130, [130, 65, 64])])
def test_attention(lib, B, T, valid, precision, qpw):
    from sylber_amd import _lib
    g = torch.Generator().manual_seed(B * 1000 + T)
    q, k, v = (torch.randn(B, T, 768, generator=g) for _ in range(3))
    vt = torch.tensor(valid, dtype=torch.int32) if valid else None

    def call(b):
        qd, kd, vd, val = b.inp(q, "q"), b.inp(k, "k"), b.inp(v, "v"), b.inp(vt, "valid")
        o = b.out((B, T, 768), torch.float32, "o")
        _lib.check(lib.sylber_op_attention(_p(qd), _p(kd), _p(vd), _p(val), _p(o), B, T, precision, qpw, None), "op_attention")
        return [o]
    _three(call)


@pytest.mark.parametrize("R,K", [(257, 384), (1, 64), (130, 3072)])
def test_mx_quantize(lib, R, K):
    from sylber_amd import _lib
    g = torch.Generator().manual_seed(R + K)
    x = torch.randn(R, K, generator=g) * torch.exp(torch.rand(R, 1, generator=g) * 16 - 8)

    def call(b):
        xd = b.inp(x, "x")
        d = b.out((R, K), torch.uint8, "data")
        s = b.out((K // 64, R, 2), torch.uint8, "scales")
        _lib.check(lib.sylber_op_mx_quantize(_p(xd), R, K, _p(d), _p(s), None), "op_mx_quantize")
        return [d, s]
    _three(call)


# cfgs 0-3 take any shape; 85 / 91 (the hand-scheduled loop: whole 256-row tiles, K % 256 == 0, K >= 512) at the shapes
# test_mxfp8_asm_loop_tiles gives them
@pytest.mark.parametrize("M,N,K,act,cfg", [(300, 256, 128, 0, c) for c in (0, 1, 2, 3)] + [(515, 3072, 768, 1, c) for c in (0, 1, 2, 3)]
                         + [(256, 256, 512, 1, 85), (512, 768, 768, 1, 85), (512, 768, 768, 1, 91), (768, 384, 3072, 1, 91)])
def test_mxfp8_linear(lib, M, N, K, act, cfg):
    from sylber_amd import _lib
    g = torch.Generator().manual_seed(M + N)
    a = torch.randn(M, K, generator=g) * torch.exp(torch.rand(M, 1, generator=g) * 4 - 2)
    w = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g)

    def call(b):
        ad, wd, bd = b.inp(a, "a"), b.inp(w, "w"), b.inp(bias, "bias")
        c = b.out((M, N), torch.float32, "c")
        _lib.check(lib.sylber_op_linear(_p(ad), _p(wd), _p(bd), _p(c), M, N, K, act, FP8, cfg, None), "op_linear fp8")
        return [c]
    _three(call)

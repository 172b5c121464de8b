"""GPU tier, guard bands (tests/guarded_alloc.py) around the entry points behind the encoder: sylber_ingest; sylber_km_assign /
_decode and their residual forms; sylber_km_normalize, sylber_kmeans_assign / _update / _seed; the learned quantizer (sylber_lq_norm,
sylber_ffenc, sylber_rvq_prepare / _assign / _decode); sylber_condition, _packed, _features, _units, _units_packed and
sylber_expand_units; sylber_cfm_eval, sylber_cfm_sample, _sample_frames and _sample_packed.

Every case runs once plainly and once per fill byte (0xFF, 0x00) with the wrapper's allocations -- outputs AND the workspace of
exactly ``sylber_*_workspace_{bytes,floats}(...)`` -- and the device-resident inputs between guards.  ``check()`` finds any byte
written outside them; every returned tensor lies in a guarded buffer; a guarded buffer of exactly the size function's bytes was
handed out; and the defined results are bit-identical across the three runs.  No tolerances.

sylber_ingest is also called through ctypes: the wrapper rounds its workspace up to whole doubles, the direct call passes exactly
``sylber_ingest_workspace_bytes(sr)`` bytes.  sylber_flac_* work on host memory only and are not covered.

Findings: none -- no guard was dirty and no result moved with the fill on an MI355X."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import units_ref as U
from guarded_alloc import FILLS, Guards, three_runs
from sylber_amd import _lib
from sylber_amd.synth_states import syllable_states

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tier needs the MI355X"
    return _lib.load()


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _same(a, b, what=None):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(_bits(a), _bits(b)), what


def _check(plain, guarded, outputs=None, workspaces=(), defined=None):
    """every guarded run: the outputs lie in guarded buffers, buffers of exactly the workspace sizes were handed out, and the
    defined results equal the plain run's bit for bit"""
    outputs = outputs or (lambda r: [t for t in (r if isinstance(r, (tuple, list)) else [r]) if torch.is_tensor(t)])
    defined = defined or outputs
    want = defined(plain)
    assert want
    for g, r in guarded:
        outs = outputs(r)
        assert outs and all(g.covers(t) for t in outs), g.names()
        for nbytes in workspaces:
            assert nbytes > 0 and g.handed_out(nbytes), (nbytes, g.names())
        got = defined(r)
        assert len(got) == len(want)
        for x, y in zip(got, want):
            _same(x, y, "fill 0x%02X" % g.fill)


# ---- ingest --------------------------------------------------------------------------------------------------------------------------
def _pcm(sr, ch, width, n):
    from sylber_amd.ingest import PcmFile
    rng = np.random.default_rng(sr + ch)
    t = np.arange(n)[:, None] / 8000.0
    x = np.clip(0.4 * np.sin(2 * np.pi * (200 + 50 * np.arange(ch))[None, :] * t) + 0.1 * rng.standard_normal((n, ch)) + 0.05, -0.99, 0.99)
    if width == 2:
        raw = np.round(x * 32767).astype("<i2")
    elif width == 3:
        v = np.round(x * (2 ** 23 - 1)).astype(np.int64).reshape(-1)
        raw = np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], 1).astype(np.uint8)
    else:
        raw = x.astype("<f8")
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    return PcmFile(raw, sr, ch, width, n)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("sr,ch,width,n", [(16000, 1, 2, 5001), (44100, 2, 3, 3000), (48000, 1, -8, 3001)])
def test_ingest(lib, sr, ch, width, n, normalize):
    from sylber_amd.ingest import ingest_pcm, num_frames_16k
    pcm = _pcm(sr, ch, width, n)
    plain, guarded = three_runs(lambda g: ingest_pcm(pcm, DEV, normalize=normalize))
    _check(plain, guarded)
    # the C call itself, with a workspace of exactly the documented bytes and the PCM bytes between guards too
    n_out, wsb = num_frames_16k(n, sr), int(lib.sylber_ingest_workspace_bytes(sr))
    for fill in FILLS:
        g = Guards(fill)
        raw = g.guarded_copy(torch.from_numpy(pcm.data).to(DEV), "pcm")
        out = g.guarded((ch, n_out), torch.float32, DEV, "wav_out")
        ws = g.guarded((wsb,), torch.uint8, DEV, "workspace")
        _lib.check(lib.sylber_ingest(ctypes.c_void_p(raw.data_ptr()), width, ch, n, sr, 1 if normalize else 0, ctypes.c_void_p(out.data_ptr()),
                                     ctypes.c_void_p(ws.data_ptr()), None), "sylber_ingest")
        g.check()
        assert g.handed_out(wsb) and g.covers(out)
        _same(out, plain, "fill 0x%02X" % fill)


# ---- k-means tokens ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K", [(1, 64), (77, 1000), (50, 1002)])
def test_km_quantizers(lib, n, K):
    from sylber_amd.downstream import KMQuantizer, ResidualKMQuantizer
    rng = np.random.default_rng(n + K)
    c = rng.standard_normal((K, 768)).astype(np.float32)
    c2 = (0.3 * rng.standard_normal((K - 3, 768))).astype(np.float32)
    x = torch.from_numpy((c[rng.integers(0, K, n)] + 0.7 * rng.standard_normal((n, 768))).astype(np.float32)).to(DEV)
    for normalize in (False, True):
        q = KMQuantizer(c, normalize=normalize)

        def run(g):
            xd = x if g is None else g.guarded_copy(x, "x")
            idx = q.get_indices(xd)
            return idx, q.decode(idx if g is None else g.guarded_copy(idx, "ids"))
        plain, guarded = three_runs(run)
        _check(plain, guarded, outputs=lambda r: [r[1]], defined=lambda r: list(r),
               workspaces=[4 * int(lib.sylber_km_workspace_floats(n, K, 768)), 4 * n, 4 * n * 768])
    q = ResidualKMQuantizer(c, c2)

    def run(g):
        xd = x if g is None else g.guarded_copy(x, "x")
        idx = q.get_indices(xd)
        return idx, q.decode(idx if g is None else g.guarded_copy(idx, "ids"))
    plain, guarded = three_runs(run)
    _check(plain, guarded, outputs=lambda r: [r[1]], defined=lambda r: list(r),
           workspaces=[4 * int(lib.sylber_km_residual_workspace_floats(n, K, K - 3, 768)), 8 * n, 4 * n * 768])


@pytest.mark.parametrize("D", [16, 768])
@pytest.mark.parametrize("K", [1, 5, 4099])
def test_kmeans_fit_steps(lib, K, D):
    """n = 4200 rows (one more than 16 blocks of 256 and then some; more rows than the largest K), assigned 1000 at a time"""
    from sylber_amd import kmeans
    n = 4200
    gen = torch.Generator().manual_seed(K + D)
    x = torch.randn(n, D, generator=gen).to(DEV)
    cent = x[torch.randperm(n, generator=gen)[:K].to(DEV)].contiguous() + 0.01
    prev = torch.randint(0, K, (n,), generator=gen, dtype=torch.int32).to(DEV)
    u = np.random.default_rng(K).random(K)

    def run(g):
        xd, cd, pd = (x, cent.clone(), prev) if g is None else (g.guarded_copy(x, "x"), g.guarded_copy(cent, "centroids"), g.guarded_copy(prev, "prev"))
        y = kmeans._normalize(xd)
        labels, dmin, inertia, changed = kmeans.assign(xd, cd, prev=pd, row_chunk=1000)
        l1, d1, i1, _ = kmeans.assign(xd, cd)
        counts = kmeans.update(xd, labels, cd)                      # in place on cd
        chosen = kmeans.kmeans_plusplus(xd, K, u)
        return (y, labels, dmin, l1, d1, counts, cd, chosen), (inertia, changed, i1)
    plain, guarded = three_runs(run)
    assert torch.equal(plain[0][1], plain[0][3])
    ws = [4 * int(lib.sylber_kmeans_assign_workspace_floats(1000, K, D)), 4 * int(lib.sylber_kmeans_assign_workspace_floats(n, K, D)),
          int(lib.sylber_kmeans_update_workspace_bytes(n, K, D)), 4 * int(lib.sylber_kmeans_seed_workspace_floats(n))]
    _check(plain, guarded, outputs=lambda r: list(r[0][:7]), defined=lambda r: list(r[0]), workspaces=ws)
    for g, r in guarded:
        assert r[1] == plain[1], ("inertia / changed", g.fill)


# ---- learned quantizer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b"])
def test_learned_quantizer(lib, golden_dir, case):
    from sylber_amd import Quantizer
    from sylber_amd.weights import synthetic_quantizer_state_dict
    meta = json.loads(str(np.load(os.path.join(golden_dir, "quantizer.npz"))["meta_json"]))[case]
    sd = synthetic_quantizer_state_dict(meta["cfg"], meta["seed"], bias_std=meta["bias_std"])
    n = 333
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, meta["cfg"]["encoder_configs"]["input_dim"])) * rng.choice([0.1, 1.0, 10.0], (n, 1))
    x[[0, 77, n - 1]] = 0.0
    x = torch.from_numpy(x.astype(np.float32)).to(DEV)
    holder = {}

    def run(g):
        if g is None:
            q = holder["q"] = Quantizer(**meta["cfg"], state_dict=sd, device=DEV)
        else:
            q = Quantizer(**meta["cfg"], state_dict=sd, device=DEV)           # sylber_rvq_prepare's squared norms between guards too
        xd = x if g is None else g.guarded_copy(x, "tokens")
        o = q(xd)
        ids = o["indices"] if g is None else g.guarded_copy(o["indices"], "ids")
        return o["indices"], o["quantize"], o["non_quantized"], q.decode(ids), q.get_indices(xd), [sq for (_, sq, _, _, _) in q._books.values()]
    plain, guarded = three_runs(run)
    q = holder["q"]
    wsz = max(int(lib.sylber_ffenc_workspace_floats(n, len(q.config["hidden_dims"]), q._dims)),
              *[int(lib.sylber_rvq_workspace_floats(n, K, d)) for (_, _, _, K, d) in q._books.values()])
    flat = lambda r: [r[0], r[1], r[2], r[3], r[4]] + [sq[:, :K] for sq, (_, _, _, K, _) in zip(r[5], q._books.values())]   # noqa: E731
    _check(plain, guarded, outputs=lambda r: [r[1], r[2], r[3]] + list(r[5]), defined=flat, workspaces=[4 * wsz])


# ---- the conditioner -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def front():
    from sylber_amd import HubertEncoderHIP
    from sylber_amd.downstream import SegmentConditioner
    from sylber_amd.weights import synthetic_mlp_state_dict, synthetic_state_dict
    enc = HubertEncoderHIP(synthetic_state_dict(0, num_layers=1), num_layers=1)
    cond = SegmentConditioner(synthetic_mlp_state_dict(1))
    h = torch.from_numpy(np.stack([syllable_states(120, 3), syllable_states(120, 4), syllable_states(120, 5, mode="silence")])).to(DEV)
    return enc, cond, h


def test_condition(lib, front):
    from sylber_amd.downstream import KMQuantizer
    enc, cond, h = front
    B, T, D = h.shape
    seg, nseg, feats = enc.segment(h, 2.6, 0.8)
    nmax = int(nseg.max())
    assert 0 < nmax < T and int(nseg[2]) == 0
    q = KMQuantizer((np.random.default_rng(3).standard_normal((500, 768)) * 0.25).astype(np.float32))
    for S, quant in ((None, None), (nmax + 3, None), (nmax, q)):
        def run(g):
            hd, sg, ns, ft = (h, seg, nseg, feats) if g is None else (g.guarded_copy(h, "hidden"), g.guarded_copy(seg, "seg"),
                                                                    g.guarded_copy(nseg, "nseg"), g.guarded_copy(feats, "feats"))
            return cond(hd, sg, ns, ft, normthreshold=2.6, max_segments=S, quantizer=quant)
        plain, guarded = three_runs(run)
        _check(plain, guarded, workspaces=[4 * int(lib.sylber_condition_workspace_floats(cond.handle, B, S if S else nmax)), 4 * B * T * 256,
                                           4 * B * T * D])

    f = torch.randn(2, 37, 768, generator=torch.Generator().manual_seed(5))
    f[0, 3] = 0.0
    f = f.to(DEV)
    plain, guarded = three_runs(lambda g: cond.from_features(f if g is None else g.guarded_copy(f, "features")))
    _check(plain, guarded, workspaces=[4 * int(lib.sylber_condition_workspace_floats(cond.handle, 74, 1)), 4 * 74 * 256])


def test_condition_packed(lib, front):
    """the packed form on the tables of segment_packed: three clips of 120, 77 and 1 frames"""
    from sylber_amd.segmenter import packed_layout
    enc, cond, h = front
    lens = [320 * 120 + 80, 320 * 77 + 80, 400]
    offsets, frames = packed_layout(lens)
    assert [int(f) for f in frames] == [120, 77, 1]
    hidden = torch.zeros(int(offsets[-1]), 768, device=DEV)
    for b in range(3):
        hidden[int(offsets[b]):int(offsets[b]) + int(frames[b])] = h[b % 2, :int(frames[b])]
    seg, nseg, feats = enc.segment_packed(hidden, lens, 2.6, 0.8)
    S = max(1, int(nseg.max()))

    def run(g):
        hd, sg, ns, ft = (hidden, seg, nseg, feats) if g is None else (g.guarded_copy(hidden, "hidden"), g.guarded_copy(seg, "seg"),
                                                                         g.guarded_copy(nseg, "nseg"), g.guarded_copy(feats, "feats"))
        return cond.packed(hd, offsets, frames, sg, ns, ft, normthreshold=2.6)
    plain, guarded = three_runs(run)
    _check(plain, guarded, workspaces=[4 * int(lib.sylber_condition_packed_workspace_floats(cond.handle, 3, S)), 4 * 198 * 256])


@pytest.mark.parametrize("ncb", [1, 2])
def test_condition_units_and_expand(lib, front, golden_dir, ncb):
    from sylber_amd.downstream import expand_feature
    _, cond, _ = front
    gold = np.load(os.path.join(golden_dir, "units.npz"))
    T = int(gold["T"])
    books = [torch.from_numpy(gold[k]).to(DEV) for k in ("c1", "c2")[:ncb]]
    units = torch.from_numpy(gold["units"][..., :ncb].astype(np.int32)).to(DEV).contiguous()
    spans, nunits = torch.from_numpy(gold["spans"].astype(np.int32)).to(DEV), torch.from_numpy(gold["nunits"].astype(np.int32)).to(DEV)
    B, S = units.shape[:2]
    fr = torch.tensor([T, max(1, T - 7)][:B] + [T] * max(0, B - 2), dtype=torch.int32)

    def run(g):
        cb, un, sp, nu = (books, units, spans, nunits) if g is None else ([g.guarded_copy(c, "codebook") for c in books], g.guarded_copy(units, "units"),
                                                                          g.guarded_copy(spans, "spans"), g.guarded_copy(nunits, "nunits"))
        return (cond.from_units(cb, un, sp, nu, T), cond.from_units(cb, un, sp, nu, T, frames=fr), cond.from_units(cb, un, sp, nu, None, frames=fr))
    plain, guarded = three_runs(run)
    _check(plain, guarded, workspaces=[4 * int(lib.sylber_condition_units_workspace_floats(cond.handle, B, S)),
                                       4 * int(lib.sylber_condition_packed_workspace_floats(cond.handle, B, S)), 4 * B * T * 256])

    feats = U.decode(gold["units"][..., :ncb], [gold["c1"], gold["c2"]][:ncb])
    avg, dur = U.spans_to_durations(feats, gold["spans"], gold["nunits"], T)
    avg, dur = torch.from_numpy(avg).to(DEV), torch.from_numpy(dur)
    plain, guarded = three_runs(lambda g: expand_feature(avg if g is None else g.guarded_copy(avg, "avg_fts"), dur))
    _check(plain, guarded, workspaces=[4 * (avg.shape[0] * avg.shape[1] + 1), 4 * avg.shape[0] * T * 768])


# ---- the flow-matching decoder -------------------------------------------------------------------------------------------------------
_DEC = {}


def _decoder(prec):
    if prec not in _DEC:
        from sylber_amd.synthesis import CfmDecoder
        from sylber_amd.weights import synthetic_regressor_state_dict
        _DEC[prec] = CfmDecoder(synthetic_regressor_state_dict(0), device=DEV, precision=prec)
    return _DEC[prec]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_cfm(lib, prec):
    """B = 2, two steps: eval and sample at T = 9 and T = 50, the frames form on (50, 9) and, in bf16, the packed form on (9, 50)"""
    dec = _decoder(prec)
    gen = torch.Generator().manual_seed(14)
    for T in (9, 50):
        cond = torch.randn(2, T, 256, generator=gen).to(DEV)
        xs = torch.randn(2, T, 14, generator=gen).to(DEV)

        def run(g):
            c, x = (cond, xs) if g is None else (g.guarded_copy(cond, "cond_emb"), g.guarded_copy(xs, "x"))
            return dec.eval(x, 0.3, c), dec.sample(c, steps=2), dec.sample(c, steps=2, y0=x, pitch_amp=2.0)
        plain, guarded = three_runs(run)
        _check(plain, guarded, workspaces=[int(lib.sylber_cfm_workspace_bytes(dec.handle, 2, T)), 4 * 2 * T * 14])
    cond = torch.randn(2, 50, 256, generator=gen).to(DEV)

    def run(g):
        return dec.sample(cond if g is None else g.guarded_copy(cond, "cond_emb"), steps=2, frames=[50, 9])
    plain, guarded = three_runs(run)
    assert not plain[1, 9:].any()
    _check(plain, guarded, workspaces=[int(lib.sylber_cfm_workspace_bytes(dec.handle, 2, 50))])
    if prec == "bf16":
        packed = torch.cat([cond[1, :9], cond[0]]).contiguous()
        farr = (ctypes.c_int32 * 2)(9, 50)

        def run(g):
            return dec.sample_packed((packed if g is None else g.guarded_copy(packed, "cond"), [9, 50]), steps=2)[0]
        plain, guarded = three_runs(run)
        _check(plain, guarded, workspaces=[int(lib.sylber_cfm_workspace_bytes_packed(dec.handle, farr, 2)), 4 * 59 * 14])

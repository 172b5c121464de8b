"""GPU tier: the tokenizers and the conditioner (csrc/downstream.hip) and the 64x64 ``gemm_f32_kernel`` (csrc/fp32_path.hip) under them,
per element and per row against float64 (tests/tokenizer_ref.py), through the C entries ``sylber_ffenc``, ``sylber_lq_norm``,
``sylber_rvq_assign`` / ``sylber_rvq_decode``, ``sylber_km_assign`` / ``sylber_km_assign_residual``, ``sylber_condition_features`` and
``sylber_condition``.

* fp32 Linear launch and the FFEncoder chain: every element inside the Linear bound / the propagated bound;
* k-means ids (plain, normalised, residual): every row under the id rule on random rows, near ties (4x-16x their bound from a tie)
  and exact integer tables; duplicated centroids across the 256-thread stride and across the ragged K % 4 tail go to the smaller
  index; stage 2 of the residual form is judged on the residual of the device's own stage-1 id; K < 4 with K % 4 != 0 is refused;
* non-finite tokens: ids stay in [0, K), an all-NaN score row gets id 0, finite neighbours keep their bits, and
  ``synthesize_units(tokenize(x))`` survives a NaN segment mean; the fit's fused arg-min keeps its documented "no nearest
  centroid" label for such rows and the fits refuse them;
* ``sylber_lq_norm``: relative error <= (D + 4) u per element, exact zero padding, in place bitwise, blank rows zeroed;
* residual VQ: ids stage by stage on the device's own residual, ``z`` and ``decode`` bitwise the fp32 sum of the chosen rows, windows
  with strides wider than the widths, zero-padded codebook rows never returned, duplicated rows to the smaller index;
* conditioning MLP: per element relative to the row's max|y| within 4x the error the same restatement makes in float32 on the CPU
  (measured on the same inputs, printed with the ratio the device reached); silence decisions one ulp either side of both
  thresholds bitwise the float32 numpy evaluation.

Conditioning MLP, measured on an MI355X (rows 1 / 63 / 64 / 65 / 129): the float32 restatement on the CPU is 5.1e-7 / 7.7e-7 /
7.1e-7 / 7.2e-7 / 7.3e-7 of the row's max|y| from float64; the device reached 1.98 / 1.92 / 2.14 / 1.68 / 2.04 times that (limit 4)
(docs/HISTORY.md)."""
import ctypes

import numpy as np
import pytest
import torch

import tokenizer_ref as T
from oracle import downstream_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _lib():
    from sylber_amd import _lib as L
    return L, L.load()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _fmt(bad, k=5):
    return "%d failures, first: %s" % (len(bad), list(bad[:k]))


# ---- fp32 Linear launch / FFEncoder ----------------------------------------------------------------------------------------------
def _ffenc(x, dims, weights):
    L, lib = _lib()
    n = x.shape[0]
    cd = (ctypes.c_int32 * len(dims))(*dims)
    wt = [_dev(w) for w in weights]
    wp = (ctypes.c_void_p * len(wt))(*[t.data_ptr() for t in wt])
    xd = _dev(x)
    y = torch.full((n, dims[-1]), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(int(lib.sylber_ffenc_workspace_floats(n, len(dims) - 2, cd)), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        L.check(lib.sylber_ffenc(_vp(xd), n, len(dims) - 2, cd, wp, _vp(y), _vp(ws), _stream()), "sylber_ffenc")
    return y.cpu().numpy()


LIN_M = (1, 31, 33, 63, 64, 65, 129)


@pytest.mark.parametrize("K", [16, 48, 768])
@pytest.mark.parametrize("N", [16, 48, 80])
def test_linear_launch_per_element(N, K):
    worst = 0.0
    for M in LIN_M:
        x, W, b = T.linear_case(M, N, K)
        got = _ffenc(x, [K, N], [W, b])
        ref, bound = T.linear64(x, W, b), T.linear_bound(x, W, b)
        bad = T.judge_elements(got, ref, bound)
        worst = max(worst, float((np.abs(got - ref) / bound).max()))
        assert len(bad) == 0, "M=%d N=%d K=%d: %s" % (M, N, K, _fmt(bad))
    print("N=%d K=%d: largest |err| / bound %.3f" % (N, K, worst))


@pytest.mark.parametrize("M", LIN_M)
def test_ffenc_chain_per_element(M):
    dims = (48, 80, 32)
    x, weights = T.ffenc_case(M, dims)
    got = _ffenc(x, list(dims), weights)
    ref, bound = T.ffenc64(x, T.ffenc_layers(dims, weights))
    bad = T.judge_elements(got, ref, bound)
    print("M=%d: largest |err| / propagated bound %.3f" % (M, float((np.abs(got - ref) / bound).max())))
    assert len(bad) == 0, _fmt(bad)


# ---- k-means ids -------------------------------------------------------------------------------------------------------------------
def _km_assign(x, c, normalize, expect_fail=False):
    L, lib = _lib()
    n, D = x.shape
    K = c.shape[0]
    xd, cd = _dev(x), _dev(c)
    idx = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(lib.sylber_km_workspace_floats(n, K, D)), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        st = lib.sylber_km_assign(_vp(xd), n, _vp(cd), K, D, int(normalize), _vp(idx), _vp(ws), _stream())
    torch.cuda.synchronize()
    if expect_fail:
        return st, lib.sylber_last_error().decode(), idx.cpu().numpy()
    L.check(st, "sylber_km_assign")
    return idx.cpu().numpy()


def _km_residual(x, c1, c2, expect_fail=False):
    L, lib = _lib()
    n, D = x.shape
    K1, K2 = c1.shape[0], c2.shape[0]
    xd, c1d, c2d = _dev(x), _dev(c1), _dev(c2)
    idx = torch.full((n, 2), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(lib.sylber_km_residual_workspace_floats(n, K1, K2, D)), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        st = lib.sylber_km_assign_residual(_vp(xd), n, _vp(c1d), K1, _vp(c2d), K2, D, _vp(idx), _vp(ws), _stream())
    torch.cuda.synchronize()
    if expect_fail:
        return st, lib.sylber_last_error().decode(), idx.cpu().numpy()
    L.check(st, "sylber_km_assign_residual")
    return idx.cpu().numpy()


def _judge_residual(x, c1, c2, ids, exact=False):
    """stage 1 on x; stage 2 on the fp32 residual of the device's OWN stage-1 id, so a stage-1 tie does not excuse stage 2"""
    s1, b1 = T.km_bounds(x, c1, False)
    bad = [("stage 1",) + f for f in T.judge_ids(s1, 0.0 if exact else b1, ids[:, 0], exact)]
    i1 = np.clip(ids[:, 0], 0, len(c1) - 1)
    r = (x - c1[i1]).astype(np.float32)
    s2, b2 = T.km_bounds(r, c2, False)
    return bad + [("stage 2",) + f for f in T.judge_ids(s2, 0.0 if exact else b2, ids[:, 1], exact)]


@pytest.mark.parametrize("K", T.KM_K)
@pytest.mark.parametrize("D", T.KM_D)
def test_km_ids_every_row(D, K):
    for normalize in (0, 1):
        c, pool, dups = T.km_pool(D, K, bool(normalize))
        s, bnd = T.km_bounds(pool, c, bool(normalize))
        for n in T.KM_N:
            ids = _km_assign(pool[:n], c, normalize)
            bad = T.judge_ids(s[:n], bnd[:n], ids)
            assert bad == [], "D=%d K=%d n=%d normalize=%d: %s" % (D, K, n, normalize, _fmt(bad))
            for lo, hi in dups:                                   # bitwise equal scores: the smaller index wins
                assert not (ids == hi).any(), (D, K, n, normalize, hi)
            # row 0 is the last centroid (or its duplicate K - 5 across the ragged tail), row 1 centroid 3
            assert ids[0] == (K - 5 if K % 4 and K >= 5 else K - 1)
            if n > 1:
                assert ids[1] == 3
    c, pool, dups = T.km_pool(D, K, False)
    c2 = T.km_second_book(D, K)
    if K % 4 and K >= 5:
        c2[K - 1] = c2[K - 5]
    for n in T.KM_N:
        ids = _km_residual(pool[:n], c, c2, False)
        assert np.array_equal(ids[:, 0], _km_assign(pool[:n], c, 0))          # stage 1 is sylber_km_assign, bit for bit
        bad = _judge_residual(pool[:n], c, c2, ids)
        assert bad == [], "residual D=%d K=%d n=%d: %s" % (D, K, n, _fmt(bad))
        for lo, hi in dups:
            assert not (ids[:, 0] == hi).any()
        if K % 4 and K >= 5:
            assert not (ids[:, 1] == K - 1).any()


@pytest.mark.parametrize("K", T.KM_K)
@pytest.mark.parametrize("D", [16, 64])
def test_km_exact_integer_tables(D, K):
    """every dot product and norm is exact in fp32: the float64 arg-min on every row, ties to the smallest index"""
    rng = np.random.default_rng(31 * D + K)
    x, c = T.int_table(rng, 130, K, D)
    _, c2 = T.int_table(rng, 1, K, D)
    if K > 259:
        c[259] = c[3]
    if K % 4 and K >= 5:
        c[K - 1] = c[K - 5]; c2[K - 1] = c2[K - 5]
    x[0], x[1] = c[K - 1], c[3]
    x[2:12] = c[rng.integers(0, K, 10)]                            # exact hits, some of them on duplicated rows
    s = T.scores64(x, c)
    ties = 0
    for n in T.KM_N:
        ids = _km_assign(x[:n], c, 0)
        bad = T.judge_ids(s[:n], 0.0, ids, exact=True)
        assert bad == [], "D=%d K=%d n=%d: %s" % (D, K, n, _fmt(bad))
        ids2 = _km_residual(x[:n], c, c2)
        bad = _judge_residual(x[:n], c, c2, ids2, exact=True)
        assert bad == [], "residual D=%d K=%d n=%d: %s" % (D, K, n, _fmt(bad))
        ties = int((T.gaps(s[:n])[1] == 0).sum())
    print("D=%d K=%d: %d of 130 rows hold an exact tie for the best score" % (D, K, ties))


@pytest.mark.parametrize("K", [1, 2, 3])
def test_km_small_ragged_k_is_refused(K):
    rng = np.random.default_rng(K)
    x, c = rng.standard_normal((5, 16)).astype(np.float32), rng.standard_normal((K, 16)).astype(np.float32)
    for normalize in (0, 1):
        st, msg, ids = _km_assign(x, c, normalize, expect_fail=True)
        assert st == 1 and "K < 4 with K % 4 != 0 is not supported" in msg and "sylber_km_assign" in msg
        assert (ids == -7).all()                                   # no ids come back
    big = rng.standard_normal((8, 16)).astype(np.float32)
    for c1, c2 in ((c, big), (big, c)):
        st, msg, ids = _km_residual(x, c1, c2, expect_fail=True)
        assert st == 1 and "K < 4 with K % 4 != 0 is not supported" in msg and "sylber_km_assign_residual" in msg
        assert (ids[:, 1] == -7).all() and (c1 is big or (ids == -7).all())


# ---- non-finite tokens ------------------------------------------------------------------------------------------------------------
def _nonfinite_rows(x):
    """rows 1, 3 and 5 of a copy of x become: all NaN, all +inf, one NaN element"""
    y = x.copy()
    y[1] = np.nan
    y[3] = np.inf
    y[5, y.shape[1] // 2] = np.nan
    return y, [1, 3, 5]


@pytest.mark.parametrize("D,K", [(16, 5), (64, 257), (768, 1002)])
def test_km_nonfinite_tokens(D, K):
    c, pool, _ = T.km_pool(D, K, False)
    c2 = T.km_second_book(D, K)
    x, rows = _nonfinite_rows(pool[:65])
    finite = np.setdiff1d(np.arange(65), rows)
    for normalize in (0, 1):
        clean = _km_assign(pool[:65], c, normalize)
        ids = _km_assign(x, c, normalize)
        assert ((ids >= 0) & (ids < K)).all(), ids[rows]
        assert ids[1] == 0 and ids[5] == 0                         # every score NaN: id 0, upstream's argmax of an all-NaN row
        if normalize:
            assert ids[3] == 0                                     # inf / inf
        assert np.array_equal(ids[finite], clean[finite])
    clean = _km_residual(pool[:65], c, c2)
    ids = _km_residual(x, c, c2)
    assert ((ids >= 0) & (ids < K)).all(), ids[rows]
    assert (ids[[1, 5]] == 0).all()
    assert np.array_equal(ids[finite], clean[finite])


def test_fused_assign_refuses_rows_without_a_score():
    """``km_fused_assign_kernel`` (``sylber_kmeans_assign``) shares the arg-min's start value.  Its public paths: the fits refuse
    non-finite features before any launch; ``sylber_amd.kmeans.assign`` documents the label 2147483647 -- never one in [0, K) --
    for a row without a comparable score, which the inverted-file indexes read as "in no list" (tests/test_gpu_ivf.py).  Rows
    with a score get ``sylber_km_assign``'s ids bit for bit, whatever their neighbours hold, so a fitted ``KMQuantizer`` maps its
    training rows to the fit's labels."""
    from sylber_amd import kmeans
    c, pool, _ = T.km_pool(64, 257, False)
    x, rows = _nonfinite_rows(pool)
    labels, dmin = [t.cpu().numpy() for t in kmeans.assign(_dev(x), _dev(c))[:2]]
    ids = _km_assign(x, c, 0)
    scored = np.setdiff1d(np.arange(len(x)), rows)                  # rows 1, 3 and 5: every score NaN (the +inf row gives inf - inf)
    assert (labels[rows] == T.INT_MAX).all() and np.isinf(dmin[rows]).all() and (ids[rows] == 0).all()
    assert ((labels[scored] >= 0) & (labels[scored] < 257)).all()
    assert np.array_equal(labels[scored], ids[scored])
    assert np.array_equal(kmeans.assign(_dev(pool), _dev(c))[0].cpu().numpy(), _km_assign(pool, c, 0))
    with pytest.raises(ValueError, match="non-finite"):
        kmeans.fit_kmeans(x, 8, max_iter=2)
    fit = kmeans.fit_km_quantizer(pool, 8, max_iter=5)
    assert np.array_equal(fit.get_indices(_dev(pool)).cpu().numpy()[:, 0], fit.fit.labels.cpu().numpy().astype(np.int64))


def test_tokenize_then_synthesize_units_with_a_nan_segment_mean(monkeypatch):
    from sylber_amd import ResidualKMQuantizer, SegmentSynthesis
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_mlp_state_dict, synthetic_regressor_state_dict, synthetic_state_dict
    sd = {"speech_model." + k: v for k, v in synthetic_state_dict(0, num_layers=9).items()}
    sd.update({"input_model." + k: v for k, v in synthetic_mlp_state_dict(1).items()})
    sd.update({"regressor." + k: v for k, v in synthetic_regressor_state_dict(0).items()})
    g = torch.Generator().manual_seed(23)
    q = ResidualKMQuantizer(torch.randn(64, 768, generator=g) * 0.09, torch.randn(33, 768, generator=g) * 0.03, device=DEV)
    syn = SegmentSynthesis(model_ckpt=sd, device=DEV, precision="bf16", quantizer=q)
    w = syllable_wave(32000, 21)[0]
    x, mask = torch.as_tensor(w)[None].float().to(DEV), torch.ones(1, len(w), device=DEV)
    hidden = syn.speech_model.forward(x.contiguous(), [len(w)])
    thr = float(torch.quantile(torch.sqrt((hidden.double() ** 2).sum(-1) + 1e-8).flatten(), 0.4).item())
    plain = syn.tokenize(x, attention_mask=mask, normthreshold=thr)
    n = len(plain[0]["units"])
    assert n >= 3
    real = syn.speech_model.segment_batch

    def poisoned(*a, **k):
        out = list(real(*a, **k))
        feats = out[4].clone()
        feats[0, 0] = float("nan")                                  # a segment whose frames held a NaN
        feats[0, 1, 5] = float("inf")
        out[4] = feats
        return tuple(out)
    monkeypatch.setattr(syn.speech_model, "segment_batch", poisoned)
    toks = syn.tokenize(x, attention_mask=mask, normthreshold=thr)
    u = toks[0]["units"]
    assert u.shape == (n, 2) and (u >= 0).all() and (u[:, 0] < 64).all() and (u[:, 1] < 33).all(), u[:2]
    assert (u[0] == 0).all()
    assert np.array_equal(u[2:], plain[0]["units"][2:])
    art = syn.synthesize_units(toks, steps=2)
    assert art.shape[0] == 1 and bool(torch.isfinite(art).all())


# ---- sylber_lq_norm ------------------------------------------------------------------------------------------------------------------
def _lq_norm(x, ldx, n, D, split, y, ldy, Dy, blank=None, normalize=1):
    """x, y: device tensors (y may be x); blank: the device tensor the blank mask reads (width D, stride ldx)"""
    L, lib = _lib()
    with torch.cuda.device(DEV):
        L.check(lib.sylber_lq_norm(_vp(x), ldx, n, D, split, normalize, _vp(blank) if blank is not None else None, ldx, D, _vp(y), ldy, Dy,
                                   _stream()), "sylber_lq_norm")
    torch.cuda.synchronize()


@pytest.mark.parametrize("D", [1, 8, 63, 64, 65, 72, 130])
def test_lq_norm_per_element(D):
    rng = np.random.default_rng(D)
    n, Dy, ld = 67, D + 5, D + 9
    x = (rng.standard_normal((n, D)) * rng.choice([1e-4, 1.0, 1e3], (n, 1))).astype(np.float32)
    x[4] = 0.0
    x[9] = np.float32(2.0 ** -81) * rng.choice([-1.0, 1.0], D)     # every square underflows to 0 in fp32
    x[13] = np.nan
    blank_rows = [4, 9, 13]
    assert T.blank_rows32(x).nonzero()[0].tolist() == blank_rows
    for split in sorted({0, 1, D - 1}):
        ref = T.lq_norm64(x, split)
        src = torch.full((n, ld), 7.0, dtype=torch.float32, device=DEV)
        src[:, :D] = _dev(x)
        for blank in (False, True):
            out = torch.full((n, ld), -3.0, dtype=torch.float32, device=DEV)
            _lq_norm(src, ld, n, D, split, out, ld, Dy, src if blank else None)
            got = out.cpu().numpy()
            assert (got[:, Dy:] == -3.0).all() and (got[:, D:Dy] == 0.0).all() and not np.signbit(got[:, D:Dy]).any()
            rows = np.setdiff1d(np.arange(n), blank_rows if blank else [13])
            bad = T.judge_elements(got[rows, :D], ref[rows], T.NORM_REL(D) * np.abs(ref[rows]))
            assert len(bad) == 0, "D=%d split=%d blank=%d: %s" % (D, split, blank, _fmt(bad))
            if blank:
                assert (got[blank_rows, :Dy] == 0.0).all()
            else:
                assert np.isnan(got[13, :D]).all()
            inplace = src.clone()
            _lq_norm(inplace, ld, n, D, split, inplace, ld, Dy, src if blank else None)
            ip = inplace.cpu().numpy()
            assert np.array_equal(ip[:, :Dy].view(np.int32), got[:, :Dy].view(np.int32)) and (ip[:, Dy:] == 7.0).all()


# ---- residual VQ -----------------------------------------------------------------------------------------------------------------------
def _rvq_setup(books, K, d):
    L, lib = _lib()
    cb = _dev(T.pad_books(books))
    Q, Kp = cb.shape[0], cb.shape[1]
    sq = torch.empty(Q, Kp, dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        L.check(lib.sylber_rvq_prepare(_vp(cb), Q, K, d, _vp(sq), _stream()), "sylber_rvq_prepare")
    return cb, sq


def _rvq_assign(x, books, K, pad=(3, 2, 5), with_z=True):
    """x [n, d] placed as a column window of wider rows; -> (ids [n, Q], z [n, d] or None); the columns around every window must
    come back untouched"""
    L, lib = _lib()
    n, d = x.shape
    Q = len(books)
    cb, sq = _rvq_setup(books, K, d)
    px, pz, pi = pad
    xw = torch.full((n, d + 2 * px), 11.0, dtype=torch.float32, device=DEV); xw[:, px:px + d] = _dev(x)
    zw = torch.full((n, d + 2 * pz), 13.0, dtype=torch.float32, device=DEV)
    iw = torch.full((n, Q + 2 * pi), -9, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(lib.sylber_rvq_workspace_floats(n, K, d)), dtype=torch.float32, device=DEV)
    xw0 = xw.clone()
    with torch.cuda.device(DEV):
        L.check(lib.sylber_rvq_assign(ctypes.c_void_p(xw.data_ptr() + 4 * px), d + 2 * px, n, d, _vp(cb), _vp(sq), Q, K,
                                      ctypes.c_void_p(iw.data_ptr() + 4 * pi), Q + 2 * pi,
                                      ctypes.c_void_p(zw.data_ptr() + 4 * pz) if with_z else None, d + 2 * pz, _vp(ws), _stream()),
                "sylber_rvq_assign")
    torch.cuda.synchronize()
    assert torch.equal(xw, xw0)
    assert (iw[:, :pi] == -9).all() and (iw[:, pi + Q:] == -9).all()
    assert (zw[:, :pz] == 13.0).all() and (zw[:, pz + d:] == 13.0).all()
    if not with_z:
        assert (zw == 13.0).all()
    return iw[:, pi:pi + Q].cpu().numpy(), (zw[:, pz:pz + d].cpu().numpy() if with_z else None)


def _rvq_decode(ids, books, K, d, pad=(4, 6)):
    L, lib = _lib()
    n, Q = ids.shape
    cb, _ = _rvq_setup(books, K, d)
    pi, pz = pad
    iw = torch.full((n, Q + 2 * pi), 123456, dtype=torch.int32, device=DEV); iw[:, pi:pi + Q] = _dev(ids.astype(np.int32))
    zw = torch.full((n, d + 2 * pz), 17.0, dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        L.check(lib.sylber_rvq_decode(ctypes.c_void_p(iw.data_ptr() + 4 * pi), Q + 2 * pi, n, _vp(cb), Q, K, d,
                                      ctypes.c_void_p(zw.data_ptr() + 4 * pz), d + 2 * pz, _stream()), "sylber_rvq_decode")
    torch.cuda.synchronize()
    assert (zw[:, :pz] == 17.0).all() and (zw[:, pz + d:] == 17.0).all()
    return zw[:, pz:pz + d].cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("d,K,Q", [(8, 1024, 4), (64, 1024, 2), (5, 5, 3), (20, 64, 1)])
def test_rvq_ids_and_sums(d, K, Q):
    books, pool = T.rvq_case(d, K, Q)                               # the case tests/test_tokenizer_ref.py holds to its conditions
    rng = np.random.default_rng(Q)
    for n in (1, 65, 500):
        x = pool[:n] if n > 1 else pool[7:8]
        ids, z = _rvq_assign(x, books, K)
        assert ((ids >= 0) & (ids < K)).all(), "a zero-padded row came back: %s" % ids[(ids < 0).any(1) | (ids >= K).any(1)][:3]
        bad, decided = T.rvq_judge(x, books, ids)
        assert bad == [], "d=%d K=%d Q=%d n=%d: %s" % (d, K, Q, n, _fmt(bad))
        if K >= 64:                                                 # row K - 1 duplicates row 1 at every stage: never returned
            assert not (ids == K - 1).any()
        if n > 8:
            assert ids[8, 0] == 1
        assert np.array_equal(_bits(z), _bits(T.rvq_sum32(ids, books, K)))
        assert np.array_equal(_bits(_rvq_decode(ids, books, K, d)), _bits(z))
        ids_only, none = _rvq_assign(x, books, K, pad=(0, 1, 0), with_z=False)
        assert none is None and np.array_equal(ids_only, ids)
        print("d=%d K=%d Q=%d n=%d: %.2f %% of (row, stage) pairs decided" % (d, K, Q, n, 100 * decided))
    wild = rng.integers(-3, K + 3, (65, Q)).astype(np.int32)        # decode clamps ids < 0 to 0 and ids >= K to K - 1
    wild[0], wild[1] = -(2 ** 31), 2 ** 31 - 1
    assert np.array_equal(_bits(_rvq_decode(wild, books, K, d)), _bits(T.rvq_sum32(wild, books, K)))


# ---- conditioning MLP ----------------------------------------------------------------------------------------------------------------
_COND = {}


def _conditioner(seed):
    from sylber_amd.downstream import SegmentConditioner
    from sylber_amd.weights import synthetic_mlp_state_dict
    if seed not in _COND:
        sd = synthetic_mlp_state_dict(seed)
        _COND[seed] = (SegmentConditioner(sd, device=DEV), sd)
    return _COND[seed]


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 129])
def test_conditioning_mlp_per_element(rows):
    cond, sd = _conditioner(2)
    rng = np.random.default_rng(rows)
    x = (rng.standard_normal((rows, cond.input_dim)) * rng.choice([0.1, 1.0, 10.0], (rows, 1))).astype(np.float32)
    with torch.no_grad():
        ref = downstream_ref.mlp_forward({k: v.double() for k, v in sd.items()}, torch.from_numpy(x).double()).numpy()
        cpu32 = downstream_ref.mlp_forward({k: v.float() for k, v in sd.items()}, torch.from_numpy(x)).numpy().astype(np.float64)
    scale = np.abs(ref).max(1, keepdims=True)
    cpu_err = float((np.abs(cpu32 - ref) / scale).max())
    got = cond.from_features(_dev(x)).cpu().numpy().astype(np.float64)
    dev_err = float((np.abs(got - ref) / scale).max())
    print("rows=%d: float32 restatement on the CPU %.3e of the row's max|y|, device %.3e = %.2f x" % (rows, cpu_err, dev_err, dev_err / cpu_err))
    assert 0 < cpu_err < 1e-5                                       # fp32 arithmetic, not a looser class
    bad = np.argwhere(~(np.abs(got - ref) <= 4 * cpu_err * scale))
    assert len(bad) == 0, _fmt(bad)


def test_silence_decision_features_branch():
    """rows with one non-zero element within 3 ulps of where ``sqrtf(fl(v v))`` crosses 1e-4f"""
    cond, _ = _conditioner(2)
    v = T.ulp_neighbours(T.features_crossing(), 3)
    want = T.silent_features32(v)
    assert want.any() and not want.all()
    for col in (0, 63, 64, 767):
        x = np.zeros((len(v), cond.input_dim), np.float32)
        x[:, col] = v * np.where(np.arange(len(v)) % 2, -1, 1)
        got = cond.from_features(_dev(x)).cpu().numpy()
        assert np.array_equal((got == 0).all(1), want), (col, (got == 0).all(1), want)
        assert np.array_equal((got == 0).any(1), want)


@pytest.mark.parametrize("v0", [3e-4, 1e-4, 2.5])
def test_silence_decision_hidden_branch(v0):
    """``sylber_condition``: frames with one non-zero hidden element, thresholds ``sqrtf(fl(v v) + 1e-8f)`` and its two neighbours"""
    L, lib = _lib()
    cond, _ = _conditioner(2)
    D, O = cond.input_dim, cond.output_dim
    v = T.ulp_neighbours(np.float32(v0), 3)
    Tn = len(v)
    hidden = np.zeros((1, Tn, D), np.float32)
    hidden[0, np.arange(Tn), (np.arange(Tn) * 131) % D] = v
    feats = np.random.default_rng(3).standard_normal((1, Tn, D)).astype(np.float32)
    seg = np.stack([np.arange(Tn), np.arange(Tn) + 1], -1)[None].astype(np.int64)
    hd, fd, sg, ns = _dev(hidden), _dev(feats), _dev(seg), _dev(np.array([Tn], np.int32))
    centre = np.sqrt(v[3] * v[3] + np.float32(1e-8))
    seen = set()
    for thr in T.ulp_neighbours(centre, 1):
        out = torch.empty(1, Tn, O, dtype=torch.float32, device=DEV)
        ws = torch.empty(int(lib.sylber_condition_workspace_floats(cond.handle, 1, Tn)), dtype=torch.float32, device=DEV)
        with torch.cuda.device(DEV):
            L.check(lib.sylber_condition(cond.handle, _vp(hd), _vp(sg), _vp(ns), _vp(fd), 1, Tn, Tn, ctypes.c_float(float(thr)), None,
                                         _vp(out), _vp(ws), _stream()), "sylber_condition")
        got = out.cpu().numpy()[0]
        want = T.silent_hidden32(v, thr)
        assert np.array_equal((got == 0).all(1), want), (thr, (got == 0).all(1), want)
        assert np.array_equal((got == 0).any(1), want)
        seen.add(tuple(want.tolist()))
    assert len(seen) > 1                                            # the three thresholds do not all decide alike

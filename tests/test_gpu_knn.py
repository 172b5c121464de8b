"""GPU tier, exact k-nearest-neighbour syllable search (csrc/knn.hip behind sylber_amd.SyllableIndex):

* k = 1, L2: the ids are ``sylber_kmeans_assign``'s labels bit for bit and the scores max(0, ||q||^2 + d_min), N from 1 to 100 000;
* top-k against float64 (tests/knn_ref.py): ids equal wherever neighbouring float64 scores are further apart than the fp32 error
  bound of the score (``knn_ref.dot_error_bound``: gamma_D on the dot, one rounding for the add), scores within 1e-5 relative;
* ties by id, k = N and k > N, bitwise independence of the split count, query chunking and how the index was built;
* group exclusion, cosine (zero rows included), NaN rows and a NaN-poisoned workspace;
* end to end: Segmenter outputs -> ``SyllableIndex.from_outputs`` -> search across clips -> provenance, and a save / load round trip."""
import ctypes

import numpy as np
import pytest
import torch

import knn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _np(t):
    return t.cpu().numpy()


def _qsq(q):
    from sylber_amd import _lib
    from sylber_amd.kmeans import _stream, _vp
    out = torch.empty(q.shape[0], dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().sylber_knn_row_norms(_vp(q), q.shape[0], q.shape[1], _vp(out), _stream(q.device)), "sylber_knn_row_norms")
    return out


@pytest.mark.parametrize("D", [16, 768])
@pytest.mark.parametrize("N", [1, 5, 127, 128, 129, 4099, 100000])
def test_k1_l2_is_kmeans_assign_bitwise(N, D):
    from sylber_amd import SyllableIndex
    from sylber_amd import kmeans as KM
    rng = np.random.default_rng(N + D)
    n = 300
    x = rng.standard_normal((N, D)).astype(np.float32)
    q = (x[rng.integers(0, N, n)] + 0.5 * rng.standard_normal((n, D))).astype(np.float32)
    xd, qd = _t(x), _t(q)
    lab, dmin, _, _ = KM.assign(qd, xd)
    s, i = SyllableIndex(x, device=DEV).search(q, 1)
    assert torch.equal(i[:, 0], lab.to(torch.int64))
    assert torch.equal(s[:, 0], torch.clamp(_qsq(qd) + dmin, min=0.0))


def _check_against_f64(q, x, k, s, i, metric="l2", qg=None, xg=None):
    s64 = R.scores(q, x, metric)
    qq = R.unit_rows(q) if metric == "cosine" else q.astype(np.float64)
    xx = R.unit_rows(x) if metric == "cosine" else x.astype(np.float64)
    bound = np.nanmax(R.dot_error_bound(qq, xx), 1)           # NaN rows are never returned: their bound does not count
    N = x.shape[0]
    for r in range(q.shape[0]):
        adm = np.ones(N, bool) if qg is None else xg != qg[r]
        ref = R.order(s64[r], adm)
        v = s64[r, ref]
        m = min(k, len(ref))
        assert np.all(i[r, m:] == -1) and np.all(np.isinf(s[r, m:]))
        for p in range(m):
            sep_prev = p == 0 or v[p] - v[p - 1] > 2 * bound[r]
            sep_next = p + 1 >= len(ref) or v[p + 1] - v[p] > 2 * bound[r]
            if sep_prev and sep_next:
                assert i[r, p] == ref[p], (r, p)
        got = i[r, :m]
        assert np.all(adm[got]) and len(set(got.tolist())) == m
        if metric == "l2":
            exact = ((q[r].astype(np.float64) - x[got].astype(np.float64)) ** 2).sum(1)
            scale = (q[r].astype(np.float64) ** 2).sum() + (x[got].astype(np.float64) ** 2).sum(1)
        else:
            exact = (qq[r] * xx[got]).sum(1)
            scale = np.ones(m)
        assert np.all(np.abs(s[r, :m] - exact) <= 1e-5 * scale), r
        # the returned list is the best m under (s, j) up to the bound: nothing left out is clearly better
        if m < len(ref):
            worst = s64[r, got].max()
            assert v[m] >= worst - 2 * bound[r]


@pytest.mark.parametrize("k", [1, 2, 10, 100, 128])
def test_topk_against_float64(k):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(k)
    N, D, n = 6000, 768, 40
    x = rng.standard_normal((N, D)).astype(np.float32)
    q = (x[rng.integers(0, N, n)] + rng.standard_normal((n, D))).astype(np.float32)
    s, i = SyllableIndex(x, device=DEV).search(q, k)
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and tuple(s.shape) == (n, k)
    _check_against_f64(q, x, k, _np(s), _np(i))


def test_duplicates_full_order_and_padding():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(4)
    base = rng.standard_normal((7, 32)).astype(np.float32)
    x = base[rng.integers(0, 7, 90)]                         # every row repeated
    idx = SyllableIndex(x, device=DEV)
    q = base[:3]
    s, i = idx.search(q, 90)
    s, i = _np(s), _np(i)
    for r in range(3):
        assert sorted(i[r].tolist()) == list(range(90))
        for p in range(89):                                  # (s, j) order: equal scores ascend by id
            assert s[r, p] < s[r, p + 1] or (s[r, p] == s[r, p + 1] and i[r, p] < i[r, p + 1])
        same = np.nonzero((x == q[r]).all(1))[0]
        assert i[r, :len(same)].tolist() == same.tolist()
        assert np.all(s[r, :len(same)] <= 1e-5 * 2 * (q[r].astype(np.float64) ** 2).sum())
    s2, i2 = idx.search(q, 128)
    assert torch.equal(i2[:, :90].cpu(), torch.from_numpy(i)) and torch.equal(s2[:, :90].cpu(), torch.from_numpy(s))
    assert bool((i2[:, 90:] == -1).all()) and bool(torch.isinf(s2[:, 90:]).all())


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_bitwise_independent_of_splits_chunks_and_adds(metric):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(11)
    N, D, n, k = 20000, 128, 300, 17
    x = rng.standard_normal((N, D)).astype(np.float32)
    x[5000:5100] = x[4000:4100]                              # exact ties across splits
    q = rng.standard_normal((n, D)).astype(np.float32)
    q[:20] = x[4000:4020]
    one = SyllableIndex(x, metric=metric, device=DEV)
    many = SyllableIndex(metric=metric, device=DEV)
    for a, b in [(0, 1), (1, 129), (129, 7000), (7000, N)]:
        assert many.add(x[a:b]) == range(a, b)
    ref = one.search(q, k)
    for idx, splits, chunk in [(one, 1, 8192), (one, 2, 8192), (one, 7, 8192), (one, 0, 100), (one, 7, 1), (many, 0, 8192), (many, 3, 77)]:
        s, i = idx.search(q, k, splits=splits, query_chunk=chunk)
        assert torch.equal(i, ref[1]) and torch.equal(s, ref[0]), (splits, chunk)
    if metric == "l2":
        _check_against_f64(q, x, k, _np(ref[0]), _np(ref[1]))


def test_group_exclusion():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(12)
    N, D, n, k = 3000, 64, 50, 20
    x = rng.standard_normal((N, D)).astype(np.float32)
    xg = rng.integers(0, 5, N)
    q = x[:n] + 0.01 * rng.standard_normal((n, D)).astype(np.float32)
    qg = xg[:n]
    idx = SyllableIndex(x, groups=xg, device=DEV)
    s, i = idx.search(q, k, groups=qg, exclude_same_group=True)
    s, i = _np(s), _np(i)
    assert np.all(xg[i] != qg[:, None])
    _check_against_f64(q, x, k, s, i, qg=qg, xg=xg)
    for splits in (1, 5):
        s2, i2 = idx.search(q, k, groups=qg, exclude_same_group=True, splits=splits)
        assert np.array_equal(_np(i2), i) and np.array_equal(_np(s2), s)
    whole = SyllableIndex(x, groups=np.full(N, 9), device=DEV)
    s, i = whole.search(q[:3], 5, groups=[9, 9, 9], exclude_same_group=True)
    assert bool((i == -1).all()) and bool(torch.isinf(s).all())


def test_cosine_matches_normalised_float64_and_zero_rows():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(13)
    N, D, n, k = 2500, 768, 30, 10
    x = (rng.standard_normal((N, D)) * rng.uniform(0.1, 10, (N, 1))).astype(np.float32)
    x[[3, 700, 701]] = 0
    q = (x[rng.integers(0, N, n)] + 0.3 * rng.standard_normal((n, D))).astype(np.float32)
    idx = SyllableIndex(x, metric="cosine", device=DEV)
    s, i = idx.search(q, k)
    _check_against_f64(q, x, k, _np(s), _np(i), metric="cosine")
    # a query orthogonal to everything but the zero rows: similarity 0 everywhere ties by id
    y = np.zeros((5, 16), np.float32)
    y[1, 0] = 1
    y[3, 1] = 2
    s, i = SyllableIndex(y, metric="cosine", device=DEV).search(np.array([[0, 0, 1] + [0] * 13], np.float32), 5)
    assert _np(i).tolist() == [[0, 1, 2, 3, 4]]
    assert _np(s).tolist() == [[0.0] * 5] and not np.signbit(_np(s)).any()
    s, i = SyllableIndex(y, metric="cosine", device=DEV).search(np.array([[0, 3] + [0] * 14], np.float32), 2)
    assert _np(i).tolist() == [[3, 0]] and _np(s)[0, 0] == 1.0


def test_nan_rows_and_poisoned_workspace():
    from sylber_amd import SyllableIndex, _lib
    from sylber_amd.kmeans import _stream, _vp
    rng = np.random.default_rng(14)
    N, D, n, k = 1000, 32, 64, 8
    x = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((n, D)).astype(np.float32)
    clean_s, clean_i = SyllableIndex(x, device=DEV).search(q, k)
    xb = x.copy()
    xb[[int(v) for v in _np(clean_i)[:, 0][:5]]] = np.nan     # rows that were somebody's nearest
    s, i = SyllableIndex(xb, device=DEV).search(q, k)
    bad = set(np.nonzero(np.isnan(xb).any(1))[0].tolist())
    assert not (set(_np(i).ravel().tolist()) & bad)
    _check_against_f64(q, xb, k, _np(s), _np(i))
    qb = q.copy()
    qb[[2, 40]] = np.nan
    idx = SyllableIndex(x, device=DEV)
    s, i = idx.search(qb, k)
    assert bool((i[[2, 40]] == -1).all()) and bool(torch.isinf(s[[2, 40]]).all())
    keep = [r for r in range(n) if r not in (2, 40)]
    assert torch.equal(i[keep], clean_i[keep]) and torch.equal(s[keep], clean_s[keep])
    # the C entry with a workspace full of NaN gives the same bits
    lib = _lib.load()
    qd = _t(q)
    for splits in (0, 3):
        ws = torch.full((int(lib.sylber_knn_workspace_bytes(n, N, D, k, splits)) // 4,), float("nan"), device=DEV)
        so = torch.empty((n, k), dtype=torch.float32, device=DEV)
        io = torch.empty((n, k), dtype=torch.int64, device=DEV)
        _lib.check(lib.sylber_knn_search(_vp(qd), n, _vp(idx._x), N, D, _vp(idx._c), 0, k, None, None, splits, _vp(so), _vp(io), _vp(ws),
                                         _stream(qd.device)), "sylber_knn_search")
        assert torch.equal(io, clean_i) and torch.equal(so, clean_s)


def test_value_errors():
    from sylber_amd import SyllableIndex
    idx = SyllableIndex(np.ones((10, 16), np.float32), groups=np.arange(10), device=DEV)
    q = np.ones((2, 16), np.float32)
    for k in (0, 129, 1.5, True):
        with pytest.raises(ValueError):
            idx.search(q, k)
    with pytest.raises(ValueError):
        idx.search(np.ones((2, 32), np.float32), 1)
    with pytest.raises(ValueError):
        idx.search(np.ones((2, 16), np.complex64), 1)
    with pytest.raises(ValueError):
        idx.search(np.ones(16, np.float32), 1)
    with pytest.raises(ValueError):
        idx.search(q, 1, groups=[1, 2, 3], exclude_same_group=True)
    with pytest.raises(ValueError):
        idx.search(q, 1, exclude_same_group=True)
    with pytest.raises(ValueError):
        idx.add(np.ones((3, 16), np.float32), groups=[1, 2])
    with pytest.raises(ValueError):
        idx.add(np.ones((3, 32), np.float32))
    with pytest.raises(ValueError):
        SyllableIndex(np.ones((3, 24), np.float32), device=DEV)
    with pytest.raises(ValueError):
        SyllableIndex(metric="hamming", device=DEV)
    with pytest.raises(ValueError):
        SyllableIndex(device=DEV).search(q, 1)


def test_segmenter_outputs_end_to_end(tmp_path):
    from sylber_amd import Segmenter, SyllableIndex
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_state_dict
    seg = Segmenter(model_ckpt=synthetic_state_dict(0), device=DEV)
    wavs = [syllable_wave(int(m), s) for s, m in enumerate([32000, 24000, 40000, 28000], start=70)]
    outs = seg(wav=wavs, in_second=False)
    counts = [len(o["segments"]) for o in outs]
    assert sum(c > 0 for c in counts) >= 3, counts
    idx = SyllableIndex.from_outputs(outs)
    assert len(idx) == sum(counts)
    feats = np.concatenate([o["segment_features"] for o in outs if len(o["segments"])])
    clip = np.concatenate([np.full(c, ci) for ci, c in enumerate(counts)])
    k = 5
    s, i = idx.search(feats, k, groups=clip, exclude_same_group=True)
    s_np, i_np = _np(s), _np(i)
    for r in range(len(feats)):
        for j in i_np[r]:
            if j < 0:
                continue
            c, sg, st, en = idx.provenance([j])[0]
            assert c != clip[r]
            assert [st, en] == outs[c]["segments"][sg].tolist()
    _check_against_f64(feats, feats, k, s_np, i_np, qg=clip, xg=clip)
    p = str(tmp_path / "index.npz")
    idx.save(p)
    back = SyllableIndex.load(p, device=DEV)
    s2, i2 = back.search(feats, k, groups=clip, exclude_same_group=True)
    assert torch.equal(s2, s) and torch.equal(i2, i)
    assert back.provenance(i_np[0]) == idx.provenance(i_np[0])
    cos = SyllableIndex.from_outputs(outs, metric="cosine")
    p2 = str(tmp_path / "cos.npz")
    cos.save(p2)
    a = cos.search(feats, k, groups=clip, exclude_same_group=True)
    b = SyllableIndex.load(p2, device=DEV).search(feats, k, groups=clip, exclude_same_group=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

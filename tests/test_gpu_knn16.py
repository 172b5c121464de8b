"""GPU tier, two-stage syllable search (csrc/knn16.hip behind ``SyllableIndex.search_refined``):

* the pack kernel against torch's casts bit for bit, saturation counted, NaN kept;
* ``m >= N``: ``search_refined`` is ``search`` bit for bit (both metrics, both storages, padding, group exclusion);
* at scale every returned score carries ``search``'s bits, lists strictly ordered by (s, id) without duplicates;
* candidate validity against the float64 coarse scores of tests/knn16_ref.py within twice ``coarse_error_bound``;
* equality with ``search`` for every query where that bound decides it (at most 10 % may be undecided);
* bitwise independence of splits, query chunking, how the index was built and the workspace contents;
* NaN rows / queries, zero rows under cosine, ``k * refine == 128``, the fp16 range, the ValueErrors, ``n == 0``;
* end to end from Segmenter outputs, with provenance and a save / load round trip."""
import numpy as np
import pytest
import torch

import knn16_ref as R16
import knn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STORAGES = ["fp16", "bf16"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("storage", STORAGES)
def test_pack_is_torchs_cast_and_counts_saturation(storage):
    from sylber_amd import SyllableIndex, _lib
    from sylber_amd.kmeans import _stream, _vp
    from sylber_amd.search import STORAGES as ST
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((300, 48)) * 10.0 ** rng.integers(-7, 4, (300, 48))).astype(np.float32)
    x[0, :4] = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]       # ties of both formats
    x[1, :4] = [6e-8, 2.0 ** -25, 6.1e-5, -0.0]                                                           # fp16 subnormals
    assert np.abs(x).max() < 65504
    idx = SyllableIndex(x, device=DEV)
    plane = idx.half_rows(storage)
    code, dtype = ST[storage]
    assert plane.dtype == dtype and tuple(plane.shape) == x.shape and plane is idx.half_rows(storage)
    assert torch.equal(plane.view(torch.int16), _t(x).to(dtype).view(torch.int16))
    # out-of-range values and NaN through the C entry point
    y = x.copy()
    y[2, :6] = [1e5, -7e4, 65504.5, np.inf, np.nan, 65504.0]
    yd = _t(y)
    out = torch.empty(y.shape, dtype=dtype, device=DEV)
    sat = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    _lib.check(lib.sylber_knn16_pack(_vp(yd), y.shape[0], y.shape[1], code, _vp(out), _vp(sat), _stream(yd.device)), "sylber_knn16_pack")
    got = _np(out.to(torch.float32))
    assert np.isnan(got[2, 4])
    ref = R16.round16(y, storage)
    keep = ~np.isnan(y)
    assert np.array_equal(got[keep].view(np.uint32), ref[keep].view(np.uint32))
    if storage == "fp16":
        assert got[2, :4].tolist() == [65504.0, -65504.0, 65504.0, 65504.0] and int(sat.item()) == 3      # the finite ones beyond range
    else:
        assert int(sat.item()) == 0 and np.isinf(got[2, 3])


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D", [16, 768])
@pytest.mark.parametrize("N", [1, 5, 127, 128])
def test_m_at_least_N_is_search_bitwise(N, D, metric, storage):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(N * 1000 + D)
    n = 70
    x = rng.standard_normal((N, D)).astype(np.float32)
    q = (x[rng.integers(0, N, n)] + 0.5 * rng.standard_normal((n, D))).astype(np.float32)
    xg, qg = rng.integers(0, 3, N), rng.integers(0, 3, n)
    idx = SyllableIndex(x, metric=metric, groups=xg, device=DEV)
    for k, refine in ((128, 1), (32, 4), (1, 128)):
        if k * refine < N:
            continue
        assert _same(idx.search_refined(q, k, refine, storage), idx.search(q, k)), (k, refine)
        assert _same(idx.search_refined(q, k, refine, storage, groups=qg, exclude_same_group=True),
                     idx.search(q, k, groups=qg, exclude_same_group=True)), (k, refine)
    s, i, cand = idx.search_refined(q, 128, 1, storage, return_candidates=True)
    assert cand.dtype == torch.int64 and tuple(cand.shape) == (n, 128)
    assert bool((cand[:, N:] == -1).all()) and bool((torch.sort(cand[:, :N], 1).values == torch.arange(N, device=DEV)).all())
    assert bool((i[:, N:] == -1).all()) and bool(torch.isinf(s[:, N:]).all())


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("N", [20000, 100000])
def test_rerank_bits_at_scale(N, storage):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(N)
    D, n, k = 768, 200, 10
    x = rng.standard_normal((N, D)).astype(np.float32)
    q = (x[rng.integers(0, N, n)] + rng.standard_normal((n, D))).astype(np.float32)
    for metric in ("l2", "cosine"):
        idx = SyllableIndex(x, metric=metric, device=DEV)
        es, ei = (_np(t) for t in idx.search(q, 128))
        s, i = (_np(t) for t in idx.search_refined(q, k, 4, storage))
        hits = 0
        for r in range(n):
            assert len(set(i[r].tolist())) == k and i[r].min() >= 0
            ss = s[r] if metric == "l2" else -s[r]                       # cosine reports similarities, descending
            for p in range(k - 1):
                assert ss[p] < ss[p + 1] or (ss[p] == ss[p + 1] and i[r, p] < i[r, p + 1])
            pos = {int(j): p for p, j in enumerate(ei[r])}
            for p in range(k):
                if int(i[r, p]) in pos:
                    hits += 1
                    assert s[r, p].view(np.uint32) == es[r, pos[int(i[r, p])]].view(np.uint32), (r, p)
        assert hits > 0.9 * n * k                                       # the check above must have had something to check


def _clustered(seed, N, D, n):
    rng = np.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((100, D))
    x = (centres[rng.integers(0, 100, N)] + 0.3 * rng.standard_normal((N, D))).astype(np.float32)
    q = (x[rng.integers(0, N, n)] + 0.3 * rng.standard_normal((n, D))).astype(np.float32)
    return q, x


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_candidates_are_valid_against_float64(metric, storage):
    from sylber_amd import SyllableIndex
    q, x = _clustered(7, 6000, 128, 64)
    xg = np.random.default_rng(8).integers(0, 4, x.shape[0])
    qg = np.random.default_rng(9).integers(0, 4, q.shape[0])
    idx = SyllableIndex(x, metric=metric, groups=xg, device=DEV)
    m = 40
    _, _, cand = idx.search_refined(q, 10, 4, storage, groups=qg, exclude_same_group=True, return_candidates=True)
    cand = _np(cand)
    xs = _np(idx.features)                                             # the stored rows (unit rows for cosine) and the queries as scored
    qs = _np(idx._prep(_t(q)))
    t = R16.coarse_scores(qs, xs, storage, metric)
    b = R16.coarse_error_bound(qs, xs, storage, metric)               # per pair
    for r in range(q.shape[0]):
        adm = xg != qg[r]
        c = cand[r]
        assert c.min() >= 0 and len(set(c.tolist())) == m and adm[c].all()
        rest = adm.copy()
        rest[c] = False
        # no admissible non-candidate j is better than a candidate w by more than the two pairs' bounds, b(r, j) + b(r, w)
        assert (t[r, rest] + b[r, rest]).min() >= (t[r, c] - b[r, c]).max(), r
        tv, bv = t[r, c], b[r, c]                                      # stage-1 order, up to the bounds of the neighbours
        assert np.all(tv[1:] + bv[1:] >= tv[:-1] - bv[:-1])


@pytest.mark.parametrize("storage", STORAGES)
def test_equals_search_where_the_bound_decides(storage):
    """tests/test_knn16_ref.py: the float64 simulation finds 256 of 256 queries of these inputs checkable for both storages"""
    from sylber_amd import SyllableIndex
    q, x, k, refine = R16.checkable_inputs()
    ok = R16.checkable(q, x, k, refine, storage)
    assert (~ok).sum() <= 0.10 * len(ok)
    idx = SyllableIndex(x, device=DEV)
    es, ei = idx.search(q, k)
    s, i = idx.search_refined(q, k, refine, storage)
    sel = torch.from_numpy(np.nonzero(ok)[0]).to(DEV)
    print("checkable %s: %d of %d; rows equal to search: %d" % (storage, int(ok.sum()), len(ok), int((i == ei).all(1).sum())))
    assert torch.equal(i[sel], ei[sel]) and torch.equal(s[sel], es[sel])


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_bitwise_independent_of_splits_chunks_adds_and_workspace(metric, storage):
    from sylber_amd import SyllableIndex, _lib
    from sylber_amd._index import _pack16
    from sylber_amd.kmeans import _stream, _vp
    from sylber_amd.search import METRICS, STORAGES as ST
    rng = np.random.default_rng(11)
    N, D, n, k, refine = 20000, 128, 300, 8, 3
    x = rng.standard_normal((N, D)).astype(np.float32)
    x[5000:5100] = x[4000:4100]                              # exact ties across splits
    q = rng.standard_normal((n, D)).astype(np.float32)
    q[:20] = x[4000:4020]
    one = SyllableIndex(x, metric=metric, device=DEV)
    many = SyllableIndex(metric=metric, device=DEV)
    many.add(x[0:1])
    many.half_rows(storage)                                  # the plane exists before the later adds: they extend it
    for a, b in [(1, 129), (129, 7000), (7000, N)]:
        assert many.add(x[a:b]) == range(a, b)
    assert torch.equal(many.half_rows(storage).view(torch.int16), one.half_rows(storage).view(torch.int16))
    ref = one.search_refined(q, k, refine, storage, return_candidates=True)
    c = _np(ref[2])
    assert all(4000 + r in c[r] and 5000 + r in c[r] for r in range(20))        # both copies of a duplicated nearest row
    for idx, splits, chunk in [(one, 1, 8192), (one, 2, 8192), (one, 7, 8192), (one, 0, 100), (one, 7, 1), (many, 0, 8192), (many, 3, 77)]:
        assert _same(idx.search_refined(q, k, refine, storage, splits=splits, query_chunk=chunk, return_candidates=True), ref), (splits, chunk)
    # the C entry points with a workspace full of NaN
    lib = _lib.load()
    m = k * refine
    qd = one._prep(_t(q))
    q16 = _pack16(qd, storage, refuse=False)
    for splits in (0, 3):
        ws = torch.full((int(lib.sylber_knn16_workspace_bytes(n, N, D, m, splits)) // 4,), float("nan"), device=DEV)
        cand = torch.empty((n, m), dtype=torch.int32, device=DEV)
        so = torch.empty((n, k), dtype=torch.float32, device=DEV)
        io = torch.empty((n, k), dtype=torch.int64, device=DEV)
        _lib.check(lib.sylber_knn16_scan(_vp(q16), n, _vp(one.half_rows(storage)), N, D, _vp(one._c), ST[storage][0], m, None, None, splits,
                                         _vp(cand), _vp(ws), _stream(qd.device)), "sylber_knn16_scan")
        _lib.check(lib.sylber_knn_rerank(_vp(qd), n, _vp(one._x), N, D, _vp(one._c), METRICS[metric], _vp(cand), m, k, _vp(so), _vp(io),
                                         _stream(qd.device)), "sylber_knn_rerank")
        assert _same((so, io, cand.to(torch.int64)), ref), splits


def test_ragged_last_chunk_with_automatic_splits():
    """a shorter last chunk gets more automatic splits than a full one and needs a LARGER workspace: the buffer must serve both"""
    from sylber_amd import SyllableIndex, _lib
    from sylber_amd.search import _chunked_workspace_bytes
    lib = _lib.load()
    rng = np.random.default_rng(21)
    N, D, n, chunk, k, refine = 262144, 16, 1128, 1000, 10, 4
    m = k * refine
    tail = lib.sylber_knn16_workspace_bytes(n % chunk, N, D, m, 0)
    assert tail > lib.sylber_knn16_workspace_bytes(chunk, N, D, m, 0)           # the case exists at this shape
    assert _chunked_workspace_bytes(lib.sylber_knn16_workspace_bytes, n, chunk, N, D, m, 0) >= tail
    assert _chunked_workspace_bytes(lib.sylber_knn_workspace_bytes, n, chunk, N, D, k, 0) >= lib.sylber_knn_workspace_bytes(n % chunk, N, D, k, 0)
    x = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((n, D)).astype(np.float32)
    idx = SyllableIndex(x, device=DEV)
    for storage in STORAGES:
        ref = idx.search_refined(q, k, refine, storage, return_candidates=True)
        assert _same(idx.search_refined(q, k, refine, storage, query_chunk=chunk, return_candidates=True), ref)
    assert _same(idx.search(q, k, query_chunk=chunk), idx.search(q, k))


@pytest.mark.parametrize("storage", STORAGES)
def test_nan_zero_rows_and_limits(storage):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(14)
    N, D, n, k = 1000, 32, 64, 8
    x = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((n, D)).astype(np.float32)
    clean = SyllableIndex(x, device=DEV)
    clean_s, clean_i = clean.search_refined(q, k, 4, storage)
    xb = x.copy()
    xb[[int(v) for v in _np(clean_i)[:, 0][:5]]] = np.nan     # rows that were somebody's nearest
    s, i, cand = SyllableIndex(xb, device=DEV).search_refined(q, k, 4, storage, return_candidates=True)
    bad = set(np.nonzero(np.isnan(xb).any(1))[0].tolist())
    assert not (set(_np(i).ravel().tolist()) & bad) and not (set(_np(cand).ravel().tolist()) & bad)
    assert bool((i >= 0).all())
    qb = q.copy()
    qb[[2, 40]] = np.nan
    s, i, cand = clean.search_refined(qb, k, 4, storage, return_candidates=True)
    assert bool((i[[2, 40]] == -1).all()) and bool(torch.isinf(s[[2, 40]]).all()) and bool((cand[[2, 40]] == -1).all())
    keep = [r for r in range(n) if r not in (2, 40)]
    assert torch.equal(i[keep], clean_i[keep]) and torch.equal(s[keep], clean_s[keep])
    # zero rows under cosine: similarity 0 everywhere ties by id, exactly as search
    y = np.zeros((5, 16), np.float32)
    y[1, 0] = 1
    y[3, 1] = 2
    cos = SyllableIndex(y, metric="cosine", device=DEV)
    for qq, kk in ((np.array([[0, 0, 1] + [0] * 13], np.float32), 5), (np.array([[0, 3] + [0] * 14], np.float32), 2)):
        a, b = cos.search_refined(qq, kk, 1, storage), cos.search(qq, kk)
        assert _same(a, b) and not np.signbit(_np(a[0])).any()
    # k * refine == 128
    s, i, cand = clean.search_refined(q, 32, 4, storage, return_candidates=True)
    assert tuple(cand.shape) == (n, 128) and bool((cand >= 0).all()) and bool((i >= 0).all())
    for r in range(n):
        assert set(_np(i[r]).tolist()) <= set(_np(cand[r]).tolist())
    # n == 0
    s, i, cand = clean.search_refined(np.zeros((0, D), np.float32), k, 4, storage, return_candidates=True)
    assert tuple(s.shape) == (0, k) and tuple(i.shape) == (0, k) and tuple(cand.shape) == (0, 4 * k)
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and cand.dtype == torch.int64 and s.device == clean.features.device


def test_fp16_range_and_value_errors():
    from sylber_amd import SyllableIndex
    x = np.ones((10, 16), np.float32)
    x[3, 5] = 1e5
    big = SyllableIndex(x, device=DEV)
    q = np.ones((2, 16), np.float32)
    with pytest.raises(ValueError, match='storage="bf16"'):
        big.search_refined(q, 1, 4, "fp16")
    with pytest.raises(ValueError, match='storage="bf16"'):
        big.half_rows("fp16")
    assert _same(big.search_refined(q, 5, 2, "bf16"), big.search(q, 5))
    ok = SyllableIndex(np.ones((10, 16), np.float32), groups=np.arange(10), device=DEV)
    ok.half_rows("fp16")
    with pytest.raises(ValueError, match='storage="bf16"'):
        ok.add(x[3:4])                                        # the call that extends the plane refuses ...
    assert len(ok) == 10 and tuple(ok.half_rows("fp16").shape) == (10, 16)    # ... and leaves the index as it was
    s, i = ok.search_refined(np.full((1, 16), 1e6, np.float32), 3, 2, "fp16")          # queries saturate, they are never refused
    assert _same((s, i), ok.search(np.full((1, 16), 1e6, np.float32), 3))
    for k, refine in ((0, 1), (129, 1), (1.5, 1), (True, 1), (1, 0), (1, 1.5), (1, True), (1, 129), (33, 4), (128, 2)):
        with pytest.raises(ValueError):
            ok.search_refined(q, k, refine)
    with pytest.raises(ValueError):
        ok.search_refined(q, 1, 1, "fp8")
    with pytest.raises(ValueError):
        ok.half_rows("fp32")
    with pytest.raises(ValueError):
        ok.search_refined(np.ones((2, 32), np.float32), 1)
    with pytest.raises(ValueError):
        ok.search_refined(np.ones((2, 16), np.complex64), 1)
    with pytest.raises(ValueError):
        ok.search_refined(np.ones(16, np.float32), 1)
    with pytest.raises(ValueError):
        ok.search_refined(q, 1, groups=[1, 2, 3], exclude_same_group=True)
    with pytest.raises(ValueError):
        ok.search_refined(q, 1, exclude_same_group=True)
    with pytest.raises(ValueError):
        ok.search_refined(q, 1, splits=-1)
    with pytest.raises(ValueError):
        ok.search_refined(q, 1, query_chunk=0)
    with pytest.raises(ValueError):
        SyllableIndex(device=DEV).search_refined(q, 1)


def test_segmenter_outputs_end_to_end(tmp_path):
    from sylber_amd import Segmenter, SyllableIndex
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_state_dict
    seg = Segmenter(model_ckpt=synthetic_state_dict(0), device=DEV)
    wavs = [syllable_wave(int(m), s) for s, m in enumerate([32000, 24000, 40000, 28000], start=70)]
    outs = seg(wav=wavs, in_second=False)
    counts = [len(o["segments"]) for o in outs]
    assert sum(c > 0 for c in counts) >= 3, counts
    feats = np.concatenate([o["segment_features"] for o in outs if len(o["segments"])])
    clip = np.concatenate([np.full(c, ci) for ci, c in enumerate(counts)])
    k = 5
    for metric in ("l2", "cosine"):
        idx = SyllableIndex.from_outputs(outs, metric=metric)
        for storage in STORAGES:
            s, i, cand = idx.search_refined(feats, k, 4, storage, groups=clip, exclude_same_group=True, return_candidates=True)
            i_np, c_np = _np(i), _np(cand)
            for r in range(len(feats)):
                assert not (clip[c_np[r][c_np[r] >= 0]] == clip[r]).any()
                for j in i_np[r]:
                    if j < 0:
                        continue
                    c, sg, st, en = idx.provenance([j])[0]
                    assert c != clip[r] and [st, en] == outs[c]["segments"][sg].tolist()
            if len(idx) <= 4 * k:                                # every admissible row is a candidate: it is search
                assert _same((s, i), idx.search(feats, k, groups=clip, exclude_same_group=True))
            p = str(tmp_path / ("%s_%s.npz" % (metric, storage)))
            idx.save(p)
            back = SyllableIndex.load(p, device=DEV)
            assert _same(back.search_refined(feats, k, 4, storage, groups=clip, exclude_same_group=True, return_candidates=True), (s, i, cand))
            assert back.provenance(i_np[0]) == idx.provenance(i_np[0])

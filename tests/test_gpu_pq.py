"""GPU tier, product-quantized syllable search (csrc/pq.hip behind ``PQSyllableIndex``):

* codes = ``kmeans.assign``'s labels of every sliced sub-space bit for bit, = the float64 arg-min wherever tests/pq_ref.py's bound
  decides it (at most 1 % undecided); ``decode`` returns the codebook rows exactly;
* the table against float64 within the fmaf-chain bound, both metrics;
* the scan bitwise: ``t`` and the candidates from the GPU's own table, formed on the host with fp32 adds in ascending ``m``;
* ``rerank=True``: with ``k * refine >= N`` it is ``SyllableIndex.search`` bit for bit; at N = 1000 it is ``search`` restricted to the
  candidates, every score a ``search`` score, lists strictly ordered without duplicates;
* ``rerank=False``: the reported values from the scan's ``t``; the same after ``drop_rows()``, which frees ``4 N D`` bytes;
* bitwise independence of splits, query chunking, how the index was built and the workspace contents;
* training: codebook ``m`` is ``fit_kmeans`` of slice ``m`` with ``seed + m``, the codes of the training rows its labels;
* NaN rows / queries, zero rows under cosine, k = 128, padding, the ValueErrors, n = 0, save / load with and without rows;
* end to end from Segmenter outputs, with provenance."""
import functools

import numpy as np
import pytest
import torch

import pq_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEOMETRIES = [(32, 2), (64, 2), (768, 48)]
SIZES = [1, 5, 255, 256, 257, 1000]
# one scan tile is 1024 code rows: 2500 rows = three tiles with a partial last one, 7300 = eight (so that 7 splits are 7 splits)
SCAN_SIZES = SIZES + [2500, 7300]
NQ = 70


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Case:
    """one index with everything the tests share: inputs, the GPU's own table and the host's fp32 scan of it (computed once)"""

    def __init__(self, D, M, N, metric):
        from sylber_amd import PQSyllableIndex, SyllableIndex
        rng = np.random.default_rng(D * 10000 + M * 100 + N)
        self.q, self.x, self.C = P.clustered(D + M + N, N, D, M, NQ, noise=0.3)
        self.xg, self.qg = rng.integers(0, 3, N), rng.integers(0, 3, NQ)
        self.metric, self.N, self.D, self.M = metric, N, D, M
        self.index = SyllableIndex(self.x, metric=metric, groups=self.xg, device=DEV)
        self.pq = PQSyllableIndex.build(self.index, M, codebooks=self.C)
        self.qd = self.pq._prep(_t(self.q))
        self.lut_dev = gpu_lut(self.pq, self.qd, metric)
        self.codes = _np(self.pq.codes)
        self.t = P.scan_t(_np(self.lut_dev), self.codes)                 # [n, N] fp32: the contract's t, from the GPU's table


@functools.lru_cache(maxsize=None)
def case(D, M, N, metric="l2"):
    return Case(D, M, N, metric)


def gpu_lut(pq, qd, metric):
    from sylber_amd import _lib
    from sylber_amd.kmeans import _stream, _vp
    from sylber_amd.search import METRICS
    lib = _lib.load()
    lut = torch.empty((qd.shape[0], pq.M, 256), dtype=torch.float32, device=DEV)
    _lib.check(lib.sylber_pq_lut(_vp(qd), qd.shape[0], qd.shape[1], _vp(pq.codebooks), _vp(pq._cnorm), pq.M, METRICS[metric], _vp(lut),
                                 _stream(qd.device)), "sylber_pq_lut")
    return lut


def gpu_scan(pq, lut, mc, qg=None, splits=0, fill=None):
    from sylber_amd import _lib
    from sylber_amd.kmeans import _stream, _vp
    lib = _lib.load()
    n, N = lut.shape[0], len(pq)
    ws = torch.empty(int(lib.sylber_pq_workspace_bytes(n, N, pq.M, mc, splits)), dtype=torch.uint8, device=DEV)
    if fill is not None:
        ws.fill_(fill)
    t = torch.empty((n, mc), dtype=torch.float32, device=DEV)
    cand = torch.empty((n, mc), dtype=torch.int32, device=DEV)
    g = _t(qg, np.int32) if qg is not None else None
    _lib.check(lib.sylber_pq_scan(_vp(lut), n, _vp(pq.codes), _vp(pq._bad), N, pq.M, mc, _vp(g), _vp(pq._db_groups() if g is not None else None),
                                  splits, _vp(t), _vp(cand), _vp(ws), _stream(lut.device)), "sylber_pq_scan")
    return _np(t), _np(cand)


# ---- 1. encode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M", GEOMETRIES)
def test_codes_are_the_assign_labels_and_decode_is_exact(D, M):
    from sylber_amd import kmeans
    dsub = D // M
    for N in SIZES:
        for metric in ("l2", "cosine") if N == 257 else ("l2",):
            c = case(D, M, N, metric)
            rows = c.index.features                                      # the stored rows (unit rows under cosine)
            assert c.pq.codes.dtype == torch.uint8 and tuple(c.pq.codes.shape) == (N, M) and not bool(c.pq._bad.any())
            for m in range(M):
                lab = kmeans.assign(rows[:, m * dsub:(m + 1) * dsub].contiguous(), c.pq.codebooks[m])[0]
                assert torch.equal(c.pq.codes[:, m].to(torch.int32), lab), (N, m)
            ids = np.random.default_rng(N).permutation(N)[:50]
            assert np.array_equal(_bits(_np(c.pq.decode(ids))), _bits(P.decode(c.codes[ids], c.C)))
    assert tuple(case(D, M, 5).pq.decode([]).shape) == (0, D)


@pytest.mark.parametrize("D,M", GEOMETRIES)
def test_codes_are_the_float64_argmin_where_the_bound_decides(D, M):
    from sylber_amd import PQSyllableIndex
    rng = np.random.default_rng(D + M)
    N = 1000 if M == 2 else 250
    C = rng.standard_normal((M, 256, D // M)).astype(np.float32)
    x = rng.standard_normal((N, D)).astype(np.float32)                   # far from every centroid: near-ties are as likely as they get
    pq = PQSyllableIndex.build(x, M, codebooks=C, device=DEV)
    ref, bad = P.encode(x, C)
    ok = P.decided(x, C)
    print("undecided (D = %d, M = %d): %d of %d" % (D, M, int((~ok).sum()), ok.size))
    assert (~ok).sum() <= 0.01 * ok.size and not bad.any()
    assert np.array_equal(_np(pq.codes)[ok], ref[ok])


# ---- 2. table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,M", GEOMETRIES)
def test_table_against_float64(D, M, metric):
    c = case(D, M, 257, metric)
    qs = _np(c.qd)
    got = _np(c.lut_dev).astype(np.float64)
    ref = P.lut(qs, c.C, metric)
    bound = P.chain_bound(qs, c.C, with_norms=metric == "l2")
    err = np.abs(got - ref)
    print("table %s D = %d M = %d: max error / bound %.3f" % (metric, D, M, float((err / np.maximum(bound, 1e-300)).max())))
    assert got.shape == (NQ, M, 256) and np.all(err <= bound)


# ---- 3. scan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M", GEOMETRIES)
def test_scan_is_the_host_sum_of_the_gpu_table_bitwise(D, M):
    for N in SCAN_SIZES:
        if N > 1000 and D == 64:
            continue
        c = case(D, M, N)
        for mc in (1, 10, 128):
            for qg in (None, c.qg):
                kw = {} if qg is None else dict(q_group=qg, x_group=c.xg)
                et, ec = P.candidates(c.t, mc, None, **kw)
                gt, gc = gpu_scan(c.pq, c.lut_dev, mc, qg)
                assert np.array_equal(gc, ec), (N, mc, qg is not None)
                assert np.array_equal(_bits(gt), _bits(et)), (N, mc, qg is not None)


# ---- 4. rerank=True ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,M", GEOMETRIES)
def test_enough_candidates_is_search_bitwise(D, M, metric):
    for N in (1, 5, 100, 128):
        c = case(D, M, N, metric)
        for k, refine in ((128, 1), (32, 4), (1, 128), (5, 1), (10, 4)):
            if k * refine < N:
                continue
            assert _same(c.pq.search(c.q, k, refine), c.index.search(c.q, k)), (N, k, refine)
            assert _same(c.pq.search(c.q, k, refine, groups=c.qg, exclude_same_group=True),
                         c.index.search(c.q, k, groups=c.qg, exclude_same_group=True)), (N, k, refine)
        s, i, cand = c.pq.search(c.q, 128, 1, return_candidates=True)
        assert cand.dtype == torch.int64 and tuple(cand.shape) == (NQ, 128)
        assert bool((cand[:, N:] == -1).all()) and bool((torch.sort(cand[:, :N], 1).values == torch.arange(N, device=DEV)).all())
        assert bool((i[:, N:] == -1).all()) and bool(torch.isinf(s[:, N:]).all())


def _all_scores(c):
    """search's reported score of every (query, row) pair: a score's bits are a function of the pair alone, so searching the rows
    125 at a time with k = 125 lists them all"""
    from sylber_amd import SyllableIndex
    S = np.empty((NQ, c.N), np.float32)
    for r0 in range(0, c.N, 125):
        part = SyllableIndex(c.x[r0:r0 + 125], metric=c.metric, device=DEV)
        s, i = (_np(t) for t in part.search(c.q, len(part)))
        assert (i >= 0).all()
        np.put_along_axis(S[:, r0:r0 + 125], i, s, 1)
    return S


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,M", GEOMETRIES)
def test_rerank_is_search_restricted_to_the_candidates(D, M, metric):
    c = case(D, M, 1000, metric)
    k, refine = 10, 4
    S = _all_scores(c)
    es, ei = (_np(t) for t in c.index.search(c.q, k))
    for kw in ({}, dict(groups=c.qg, exclude_same_group=True)):
        s, i, cand = (_np(t) for t in c.pq.search(c.q, k, refine, return_candidates=True, **kw))
        et, ec = P.candidates(c.t, k * refine, None, **(dict(q_group=c.qg, x_group=c.xg) if kw else {}))
        assert np.array_equal(cand, ec)
        key = S if metric == "l2" else -S                                # cosine reports similarities, descending
        for r in range(NQ):
            assert len(set(i[r].tolist())) == k and i[r].min() >= 0
            assert np.array_equal(_bits(s[r]), _bits(S[r, i[r]]))        # every pair is a pair search produces
            want = cand[r][np.lexsort((cand[r], key[r, cand[r]]))][:k]   # search's (s, id) order over the candidate set
            assert i[r].tolist() == want.tolist()
            for p in range(k - 1):
                assert key[r, i[r, p]] < key[r, i[r, p + 1]] or (key[r, i[r, p]] == key[r, i[r, p + 1]] and i[r, p] < i[r, p + 1])
    s, i = (_np(t) for t in c.pq.search(c.q, k, refine))
    print("recall@10 of the re-ranked scan (%s, D = %d, M = %d): %.3f" % (metric, D, M, np.mean([len(set(i[r]) & set(ei[r])) / k for r in range(NQ)])))


# ---- 5. rerank=False --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,M", GEOMETRIES)
def test_scan_scores_and_dropped_rows(D, M, metric):
    from sylber_amd import PQSyllableIndex, _lib
    from sylber_amd.kmeans import _stream, _vp
    c = case(D, M, 1000, metric)
    k = 10
    pq = PQSyllableIndex.build(c.x, M, codebooks=c.C, groups=c.xg, metric=metric, device=DEV)      # its own rows: they get dropped
    qsq = torch.empty(NQ, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().sylber_knn_row_norms(_vp(c.qd), NQ, D, _vp(qsq), _stream(c.qd.device)), "sylber_knn_row_norms")
    want = {}
    for grouped in (False, True):
        et, ec = P.candidates(c.t, k, None, **(dict(q_group=c.qg, x_group=c.xg) if grouped else {}))
        want[grouped] = (P.report(et, ec, _np(qsq), metric), ec)
    before = pq.nbytes
    for dropped in (False, True):
        if dropped:
            pq.drop_rows()
            assert pq.index is None and before - pq.nbytes == 4 * c.N * D
            with pytest.raises(ValueError):
                pq.search(c.q, k, rerank=True)
            assert pq.provenance([0, -1]) == [None, None]
        for grouped in (False, True):
            kw = dict(groups=c.qg, exclude_same_group=True) if grouped else {}
            s, i, cand = (_np(t) for t in pq.search(c.q, k, return_candidates=True, **({} if dropped else dict(rerank=False)), **kw))
            assert np.array_equal(i, want[grouped][1]) and np.array_equal(cand, i)
            assert np.array_equal(_bits(s), _bits(want[grouped][0]))
    assert pq.nbytes == c.N * M + c.N + 4 * c.N + 4 * 256 * D + 4 * 256 * M


# ---- 6. independence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1000, 7300])
@pytest.mark.parametrize("D,M", [(32, 2), (768, 48)])
def test_bitwise_independent_of_splits_chunks_adds_and_workspace(D, M, N):
    from sylber_amd import PQSyllableIndex
    c = case(D, M, N)
    k, refine = 10, 4
    kw = dict(groups=c.qg, exclude_same_group=True, return_candidates=True)
    ref = c.pq.search(c.q, k, refine, **kw)
    ref_scan = c.pq.search(c.q, k, rerank=False, **kw)
    cut = 600 * N // 1000
    two = PQSyllableIndex.build(c.x[:cut], M, codebooks=c.C, groups=c.xg[:cut], device=DEV)
    assert two.add(c.x[cut:], groups=c.xg[cut:]) == range(cut, N) and len(two) == N == len(two.index)
    assert torch.equal(two.codes, c.pq.codes)
    for pq, splits, chunk, fill in [(c.pq, 1, None, None), (c.pq, 3, None, None), (c.pq, 7, None, None), (c.pq, 0, 1, None),
                                    (c.pq, 0, 33, None), (c.pq, 7, 33, 0xFF), (c.pq, 0, None, 0xFF), (two, 0, None, None), (two, 3, 33, 0xFF)]:
        a = pq.search(c.q, k, refine, splits=splits, query_chunk=chunk, _workspace_fill=fill, **kw)
        assert _same(a, ref), (splits, chunk, fill)
        if chunk != 1:
            b = pq.search(c.q, k, rerank=False, splits=splits, query_chunk=chunk, _workspace_fill=fill, **kw)
            assert _same(b, ref_scan), (splits, chunk, fill)
    # the C entry point: every split count against the host's scan, the workspace full of 0xFF (a NaN pattern)
    for splits in (1, 3, 7):
        et, ec = P.candidates(c.t, 40)
        gt, gc = gpu_scan(c.pq, c.lut_dev, 40, None, splits, 0xFF)
        assert np.array_equal(gc, ec) and np.array_equal(_bits(gt), _bits(et)), splits


# ---- 7. training ------------------------------------------------------------------------------------------------------------------
def test_training_is_fit_kmeans_per_sub_space():
    from sylber_amd import PQSyllableIndex, fit_kmeans
    q, x, _ = P.clustered(77, 2000, 32, 2, 4, noise=0.3)
    for metric in ("l2", "cosine"):
        pq = PQSyllableIndex.build(x, 2, seed=5, max_iter=5, metric=metric, device=DEV)
        rows = pq.index.features
        for m in range(2):
            fit = fit_kmeans(rows[:, m * 16:(m + 1) * 16].contiguous(), 256, seed=5 + m, max_iter=5, tol=1e-4, device=DEV)
            assert torch.equal(pq.codebooks[m], fit.centroids), m
            assert torch.equal(pq.codes[:, m].to(torch.int64), fit.labels), m
        assert tuple(pq.codebooks.shape) == (2, 256, 16) and pq.M == 2 and len(pq) == 2000 and pq.metric == metric
        s, i = pq.search(q, 3)
        assert bool((i >= 0).all())


# ---- 8. edges ---------------------------------------------------------------------------------------------------------------------
def test_nan_rows_nan_queries_zero_rows_and_padding():
    from sylber_amd import PQSyllableIndex
    c = case(32, 2, 1000)
    k = 8
    clean_s, clean_i = c.pq.search(c.q, k)
    scan_s, scan_i = c.pq.search(c.q, k, rerank=False)
    xb = c.x.copy()
    hit = sorted({int(v) for v in _np(scan_i)[:, 0][:5]})                # rows that were somebody's best
    xb[hit[0], 3] = np.nan                                               # one sub-row only: the other one still gets its code
    xb[hit[1:]] = np.nan
    pq = PQSyllableIndex.build(xb, 2, codebooks=c.C, device=DEV)
    bad = np.isnan(xb).any(1)
    assert np.array_equal(_np(pq._bad).astype(bool), bad)
    assert (_np(pq.codes)[hit[0]] == [0, c.codes[hit[0], 1]]).all() and (_np(pq.codes)[hit[1:]] == 0).all()
    for kw in (dict(refine=4), dict(rerank=False)):
        s, i, cand = pq.search(c.q, k, return_candidates=True, **kw)
        assert not (set(_np(i).ravel().tolist()) & set(hit)) and not (set(_np(cand).ravel().tolist()) & set(hit)) and bool((i >= 0).all())
    qb = c.q.copy()
    qb[[2, 40]] = np.nan
    keep = [r for r in range(NQ) if r not in (2, 40)]
    for kw, (cs, ci) in ((dict(refine=4), (clean_s, clean_i)), (dict(rerank=False), (scan_s, scan_i))):
        s, i, cand = c.pq.search(qb, k, return_candidates=True, **kw)
        assert bool((i[[2, 40]] == -1).all()) and bool(torch.isinf(s[[2, 40]]).all()) and bool((cand[[2, 40]] == -1).all())
        assert torch.equal(i[keep], ci[keep]) and torch.equal(s[keep], cs[keep])
    # a zero row under cosine stays zero: similarity 0 with every query, exactly as search
    y = c.x[:100].copy()
    y[7] = 0
    small = PQSyllableIndex.build(y, 2, codebooks=c.C, metric="cosine", device=DEV)
    a, b = small.search(c.q, 100, 1), small.index.search(c.q, 100)
    assert _same(a, b) and bool((a[1] == 7).any(1).all())
    assert bool((a[0][a[1] == 7] == 0).all()) and not np.signbit(_np(a[0][a[1] == 7])).any()
    # k = 128 and N < k
    s, i, cand = c.pq.search(c.q, 128, 1, return_candidates=True)
    assert tuple(cand.shape) == (NQ, 128) and bool((cand >= 0).all()) and bool((i >= 0).all())
    s, i = c.pq.search(c.q, 128, rerank=False)
    assert bool((i >= 0).all()) and bool((s[:, 1:] >= s[:, :-1]).all())
    few = case(32, 2, 5)
    for kw in (dict(refine=1), dict(rerank=False)):
        s, i = few.pq.search(few.q, 9, **kw)
        assert bool((i[:, 5:] == -1).all()) and bool(torch.isinf(s[:, 5:]).all()) and bool((i[:, :5] >= 0).all())
    # n == 0
    s, i, cand = c.pq.search(np.zeros((0, 32), np.float32), k, 4, return_candidates=True)
    assert tuple(s.shape) == (0, k) and tuple(i.shape) == (0, k) and tuple(cand.shape) == (0, 4 * k)
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and cand.dtype == torch.int64 and s.device == c.pq.codes.device


def test_value_errors():
    from sylber_amd import PQSyllableIndex, SyllableIndex
    c = case(32, 2, 1000)
    x, C, q = c.x, c.C, c.q
    for M in (0, 65, 3, 4, 1.5, True, -1):                               # 32 / 3 is no integer, 32 / 4 = 8 is no multiple of 16
        with pytest.raises(ValueError):
            PQSyllableIndex.build(x, M, device=DEV)
    with pytest.raises(ValueError):
        PQSyllableIndex.build(np.ones((10, 2048), np.float32), 128, device=DEV)          # a legal split, but M > 64
    with pytest.raises(ValueError):
        PQSyllableIndex.build(x[:255], 2, device=DEV)                    # training needs 256 rows
    with pytest.raises(ValueError):
        PQSyllableIndex.build(np.ones((300, 32), np.float32), 2, device=DEV)             # fit_kmeans: fewer than 256 distinct rows
    with pytest.raises(ValueError):
        PQSyllableIndex.build(SyllableIndex(device=DEV), 2)
    with pytest.raises(ValueError):
        PQSyllableIndex.build(x, 2, codebooks=C[:, :255], device=DEV)
    with pytest.raises(ValueError):
        PQSyllableIndex.build(x, 2, codebooks=C[:1], device=DEV)
    Cn = C.copy()
    Cn[1, 3, 2] = np.inf
    with pytest.raises(ValueError):
        PQSyllableIndex.build(x, 2, codebooks=Cn, device=DEV)
    with pytest.raises(ValueError):
        PQSyllableIndex.build(x, 2, codebooks=C, metric="dot", device=DEV)
    pq = c.pq
    for k, refine in ((0, 1), (129, 1), (1.5, 1), (True, 1), (1, 0), (1, 1.5), (1, True), (1, 129), (33, 4), (128, 2)):
        with pytest.raises(ValueError):
            pq.search(q, k, refine)
    for k in (0, 129, 1.5, True):
        with pytest.raises(ValueError):
            pq.search(q, k, rerank=False)
    assert tuple(pq.search(q, 128, 50, rerank=False)[0].shape) == (NQ, 128)             # refine plays no part without re-ranking
    with pytest.raises(ValueError):
        pq.search(np.ones((2, 64), np.float32), 1)
    with pytest.raises(ValueError):
        pq.search(np.ones(32, np.float32), 1)
    with pytest.raises(ValueError):
        pq.search(q, 1, groups=[1, 2, 3], exclude_same_group=True)
    with pytest.raises(ValueError):
        pq.search(q, 1, exclude_same_group=True)
    with pytest.raises(ValueError):
        pq.search(q, 1, splits=-1)
    with pytest.raises(ValueError):
        pq.search(q, 1, query_chunk=0)
    with pytest.raises(ValueError):
        pq.decode([len(pq)])
    # a refused add leaves everything unchanged, with and without the rows
    own = PQSyllableIndex.build(x[:300], 2, codebooks=C, device=DEV)
    for dropped in (False, True):
        if dropped:
            own.drop_rows()
        for bad_add in (dict(features=np.ones((3, 64), np.float32)), dict(features=x[:3], groups=[1, 2])):
            with pytest.raises(ValueError):
                own.add(**bad_add)
        held = 310 if dropped else 300                               # the first round's accepted add of ten rows stays
        assert len(own) == held and tuple(own.codes.shape) == (held, 2) and tuple(own._bad.shape) == (held,)
        assert dropped or len(own.index) == 300
        if dropped:
            assert own.add(x[310:320]) == range(310, 320)
        else:
            assert own.add(x[300:310], groups=np.arange(10)) == range(300, 310) and len(own.index) == 310
    assert len(own) == 320 and torch.equal(own.codes, c.pq.codes[:320])
    # the C entry points refuse bad arguments without a launch
    from sylber_amd import _lib
    lib = _lib.load()
    assert lib.sylber_pq_workspace_bytes(1, 1, 65, 1, 0) == -1 and lib.sylber_pq_workspace_bytes(1, 1, 2, 129, 0) == -1
    assert lib.sylber_pq_workspace_bytes(70, 1000, 48, 40, 0) > 0
    assert lib.sylber_pq_scan(None, 1, None, None, 1, 2, 1, None, None, 0, None, None, None, None) != 0
    assert lib.sylber_pq_encode(None, 1, 32, None, None, 2, None, None, None) != 0
    assert lib.sylber_pq_lut(None, 1, 32, None, None, 2, 0, None, None) != 0
    assert lib.sylber_pq_decode(None, 1, None, 2, 32, None, None) != 0


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_save_load_round_trips(tmp_path, metric):
    from sylber_amd import PQSyllableIndex
    c = case(64, 2, 1000, metric)
    pq = PQSyllableIndex.build(c.x, 2, codebooks=c.C, groups=c.xg, metric=metric, device=DEV)
    kw = dict(groups=c.qg, exclude_same_group=True, return_candidates=True)
    p = str(tmp_path / "held.npz")
    pq.save(p)
    back = PQSyllableIndex.load(p, device=DEV)
    assert back.index is not None and back.metric == metric and len(back) == 1000 and back.nbytes == pq.nbytes
    assert torch.equal(back.codes, pq.codes) and torch.equal(back.codebooks, pq.codebooks) and torch.equal(back.index.features, pq.index.features)
    assert _same(back.search(c.q, 10, 4, **kw), pq.search(c.q, 10, 4, **kw))
    assert _same(back.search(c.q, 10, rerank=False, **kw), pq.search(c.q, 10, rerank=False, **kw))
    ref = pq.search(c.q, 10, rerank=False, **kw)
    pq.drop_rows()
    p = str(tmp_path / "dropped.npz")
    pq.save(p)
    back = PQSyllableIndex.load(p, device=DEV)
    assert back.index is None and back.nbytes == pq.nbytes and len(back) == 1000
    assert _same(back.search(c.q, 10, **kw), ref) and _same(pq.search(c.q, 10, **kw), ref)
    with pytest.raises(ValueError):
        back.search(c.q, 10, rerank=True)
    assert back.add(c.x[:7], groups=c.xg[:7]) == range(1000, 1007) and torch.equal(back.codes[1000:], pq.codes[:7])
    with pytest.raises(ValueError):
        from sylber_amd import SyllableIndex
        q = str(tmp_path / "plain.npz")
        SyllableIndex(c.x[:10], device=DEV).save(q)
        PQSyllableIndex.load(q, device=DEV)


# ---- 9. end to end ----------------------------------------------------------------------------------------------------------------
def test_segmenter_outputs_end_to_end(tmp_path):
    from sylber_amd import PQSyllableIndex, Segmenter, SyllableIndex
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_state_dict
    seg = Segmenter(model_ckpt=synthetic_state_dict(0), device=DEV)
    wavs = [syllable_wave(int(m), s) for s, m in enumerate([32000, 24000, 40000, 28000], start=70)]
    outs = seg(wav=wavs, in_second=False)
    counts = [len(o["segments"]) for o in outs]
    assert sum(c > 0 for c in counts) >= 3, counts
    feats = np.concatenate([o["segment_features"] for o in outs if len(o["segments"])])
    clip = np.concatenate([np.full(c, ci) for ci, c in enumerate(counts)])
    C = np.random.default_rng(9).standard_normal((48, 256, 16)).astype(np.float32)      # a handful of syllables cannot train 256 centroids
    k = 5
    for metric in ("l2", "cosine"):
        idx = SyllableIndex.from_outputs(outs, metric=metric)
        pq = PQSyllableIndex.build(idx, M=48, codebooks=C)
        assert pq.index is idx and len(pq) == len(feats) and pq.M == 48 and tuple(pq.codes.shape) == (len(feats), 48)
        for kw in (dict(refine=4), dict(rerank=False)):
            s, i, cand = pq.search(feats, k, groups=clip, exclude_same_group=True, return_candidates=True, **kw)
            i_np, c_np = _np(i), _np(cand)
            for r in range(len(feats)):
                assert not (clip[c_np[r][c_np[r] >= 0]] == clip[r]).any()
                for j in i_np[r]:
                    if j < 0:
                        continue
                    cl, sg, st, en = pq.provenance([j])[0]
                    assert cl != clip[r] and [st, en] == outs[cl]["segments"][sg].tolist()
            if "refine" in kw and len(idx) <= 4 * k:                     # every admissible row is a candidate: it is search
                assert _same((s, i), idx.search(feats, k, groups=clip, exclude_same_group=True))
        p = str(tmp_path / ("%s.npz" % metric))
        pq.save(p)
        back = PQSyllableIndex.load(p, device=DEV)
        got = back.search(feats, k, 4, groups=clip, exclude_same_group=True, return_candidates=True)
        assert _same(got, pq.search(feats, k, 4, groups=clip, exclude_same_group=True, return_candidates=True))
        assert back.provenance(i_np[0]) == pq.provenance(i_np[0])
        pq.drop_rows()
        assert pq.provenance(i_np[0]) == back.provenance(i_np[0])

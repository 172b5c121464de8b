"""GPU tier, compressed inverted-file search (csrc/pq.hip ``sylber_ivfpq_scan`` behind ``IVFPQSyllableIndex``):

* with every list probed a search is ``PQSyllableIndex.search`` on the same codebooks bit for bit (scores, ids, candidates; both
  metrics, both ``rerank`` settings, with and without groups), the codes are the same codes;
* the scan bitwise: ``t`` and the candidates from the GPU's own table, summed on the host (``pq_ref.scan_t``) and restricted to the
  probed lists by ``labels`` / ``probe`` (tests/ivfpq_ref.py);
* ``rerank=True`` is ``SyllableIndex.search`` restricted to the returned candidates;
* lists of 0, 1, 63 ... 1 025 rows (every power-of-two tile up to 1 024, the 512-row scan tile among them), queries that probe only empty lists, fewer rows than
  ``k * refine``;
* bitwise independence of splits, query chunking, the workspace's contents and ``build`` against ``build`` + ``add`` + ``add``;
* group exclusion, NaN queries, NaN rows, a zero row under cosine, ties in ``t`` across two lists;
* ``drop_rows``, save / load with and without rows, the ValueErrors, n = 0;
* end to end from Segmenter outputs."""
import functools

import numpy as np
import pytest
import torch

import ivfpq_ref as F
import pq_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEOMETRIES = [(32, 2), (64, 4), (256, 16)]              # code rows of 2, 4 and 16 bytes: the 1-, 4- and 16-byte code loads
BIG = (768, 48)
NLIST = 8
NQ = 40
FORCED_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 511, 512, 513]       # the last three: the scan's own tile is 512 rows


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu_lut(ix, qd):
    from sylber_amd import _lib
    from sylber_amd.kmeans import _stream, _vp
    from sylber_amd.search import METRICS
    lut = torch.empty((qd.shape[0], ix.M, 256), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().sylber_pq_lut(_vp(qd), qd.shape[0], qd.shape[1], _vp(ix.codebooks), _vp(ix._cnorm), ix.M, METRICS[ix.metric],
                                         _vp(lut), _stream(qd.device)), "sylber_pq_lut")
    return lut


def gpu_scan(ix, lut, probe, mc, qg=None, splits=0, fill=None):
    """the C entry point on the index's own device arrays -> (t [n, mc], cand [n, mc]) as numpy"""
    from sylber_amd import _lib
    from sylber_amd.kmeans import _stream, _vp
    lib = _lib.load()
    n, nprobe = probe.shape
    ws = torch.empty(int(lib.sylber_ivfpq_workspace_bytes(n, nprobe, mc, splits)), dtype=torch.uint8, device=DEV)
    if fill is not None:
        ws.fill_(fill)
    t = torch.empty((n, mc), dtype=torch.float32, device=DEV)
    cand = torch.empty((n, mc), dtype=torch.int32, device=DEV)
    pd = _t(probe, np.int32)
    g = _t(qg, np.int32) if qg is not None else None
    _lib.check(lib.sylber_ivfpq_scan(_vp(lut), n, _vp(pd), nprobe, _vp(ix._off), ix.nlist, _vp(ix._codes), _vp(ix._rbad), _vp(ix._rid),
                                     ix._listed, ix.M, mc, _vp(g), _vp(ix._rg if g is not None else None), splits, _vp(t), _vp(cand), _vp(ws),
                                     _stream(lut.device)), "sylber_ivfpq_scan")
    return _np(t), _np(cand)


class Case:
    """one index with everything the tests share: inputs, the PQ index on the same codebooks, the GPU's own table and the host's fp32
    scan of it (computed once)"""

    def __init__(self, D, M, N, metric):
        from sylber_amd import IVFPQSyllableIndex, PQSyllableIndex, SyllableIndex
        rng = np.random.default_rng(D * 10000 + M * 100 + N)
        self.q, self.x, self.C = P.clustered(D + M + N, N, D, M, NQ, noise=0.3)
        self.xg, self.qg = rng.integers(0, 3, N), rng.integers(0, 3, NQ)
        self.metric, self.N, self.D, self.M = metric, N, D, M
        self.index = SyllableIndex(self.x, metric=metric, groups=self.xg, device=DEV)
        # centroids near stored rows (unit rows under cosine), so that every list gets rows and the queries' probe order varies
        self.cent = _np(self.index.features)[rng.permutation(N)[:NLIST]] * (1 + 0.01 * rng.standard_normal((NLIST, D)).astype(np.float32))
        self.ix = IVFPQSyllableIndex.build(self.index, NLIST, M, centroids=self.cent, codebooks=self.C)
        self.pq = PQSyllableIndex.build(self.index, M, codebooks=self.ix.codebooks)
        self.qd = self.pq._prep(_t(self.q))
        self.lut_dev = gpu_lut(self.ix, self.qd)
        self.codes = _np(self.ix.codes)
        self.labels = _np(self.ix.labels)
        self.t = P.scan_t(_np(self.lut_dev), self.codes)                 # [n, N] fp32: the contract's t, from the GPU's table


@functools.lru_cache(maxsize=None)
def case(D, M, N=2000, metric="l2"):
    return Case(D, M, N, metric)


# ---- 1. every list probed ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,M", GEOMETRIES + [BIG])
def test_every_list_probed_is_the_pq_search_bitwise(D, M, metric):
    c = case(D, M, 1500 if (D, M) == BIG else 2000, metric)
    sizes = _np(c.ix.list_sizes)
    assert sizes.sum() == c.N and (sizes > 0).all() and c.ix.nlist == NLIST and c.ix.M == M and len(c.ix) == c.N and c.ix.metric == metric
    assert c.ix.codes.dtype == torch.uint8 and torch.equal(c.ix.codes, c.pq.codes)
    assert c.ix.index is c.index
    for kw in ({}, dict(groups=c.qg, exclude_same_group=True)):
        for k, refine, rerank in ((10, 4, True), (10, 4, False), (128, 1, True), (128, 1, False), (1, 1, None)):
            a = c.ix.search(c.q, k, NLIST, refine, rerank=rerank, return_candidates=True, **kw)
            b = c.pq.search(c.q, k, refine, rerank=rerank, return_candidates=True, **kw)
            assert _same(a, b), (k, refine, rerank, bool(kw))
            assert a[0].dtype == torch.float32 and a[1].dtype == torch.int64 and a[2].dtype == torch.int64
    ls = c.ix.last_search
    assert ls["pairs"] == NQ * c.N and ls["fraction"] == 1.0 and ls["workspace_bytes"] > 0


# ---- 2. the scan ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M", GEOMETRIES)
def test_scan_is_the_host_sum_over_the_probed_lists_bitwise(D, M):
    c = case(D, M)
    for nprobe in (1, 3):
        probe = _np(c.ix.probe(c.q, nprobe))
        assert probe.shape == (NQ, nprobe) and probe.dtype == np.int64 and probe.min() >= 0 and probe.max() < NLIST
        assert len(np.unique(probe[:, 0])) > 1
        for mc in (1, 10, 128):
            for qg in (None, c.qg):
                kw = {} if qg is None else dict(q_group=qg, x_group=c.xg)
                et, ec = F.candidates(c.t, mc, c.labels, probe, None, **kw)
                gt, gc = gpu_scan(c.ix, c.lut_dev, probe, mc, qg)
                assert np.array_equal(gc, ec), (nprobe, mc, qg is not None)
                assert np.array_equal(_bits(gt), _bits(et)), (nprobe, mc, qg is not None)
        # the class takes the same lists
        s, i, cand = c.ix.search(c.q, 10, nprobe, rerank=False, return_candidates=True)
        et, ec = F.candidates(c.t, 10, c.labels, probe)
        assert np.array_equal(_np(cand), ec) and np.array_equal(_np(i), ec)
        ls = c.ix.last_search
        want = int(_np(c.ix.list_sizes)[probe].sum())
        assert ls["pairs"] == want and ls["fraction"] == want / (NQ * c.N) and 0 < ls["fraction"] < 1


# ---- 3. rerank=True ---------------------------------------------------------------------------------------------------------------
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
@pytest.mark.parametrize("D,M", [(32, 2), (256, 16)])
def test_rerank_is_search_restricted_to_the_candidates(D, M, metric):
    c = case(D, M, 2000, metric)
    k, refine, nprobe = 10, 4, 3
    S = _all_scores(c)
    probe = _np(c.ix.probe(c.q, nprobe))
    for kw in ({}, dict(groups=c.qg, exclude_same_group=True)):
        s, i, cand = (_np(t) for t in c.ix.search(c.q, k, nprobe, refine, return_candidates=True, **kw))
        et, ec = F.candidates(c.t, k * refine, c.labels, probe, None, **(dict(q_group=c.qg, x_group=c.xg) if kw else {}))
        assert np.array_equal(cand, ec) and (cand >= 0).sum() > NQ * k
        key = S if metric == "l2" else -S                                # cosine reports similarities, descending
        for r in range(NQ):
            cr = cand[r][cand[r] >= 0]
            assert np.isin(c.labels[cr], probe[r]).all()
            want = cr[np.lexsort((cr, key[r, cr]))][:k]                  # search's (s, id) order over the candidate set
            assert i[r].tolist() == want.tolist() + [-1] * (k - len(want))
            assert np.array_equal(_bits(s[r, :len(want)]), _bits(S[r, want])) and np.isinf(s[r, len(want):]).all()      # search's own scores


# ---- 4. forced list sizes ---------------------------------------------------------------------------------------------------------
def _forced(seed, D, metric, n=48):
    """lists of exactly FORCED_SIZES rows around far-apart centroids (list 0 stays empty); the rows of the lists are interleaved.
    Query l < len(FORCED_SIZES) is centroid l itself."""
    rng = np.random.default_rng(seed)
    nl = len(FORCED_SIZES)
    cent = np.zeros((nl, D), np.float32)
    cent[np.arange(nl), np.arange(nl)] = 1.0 if metric == "cosine" else 40.0
    lab = rng.permutation(np.repeat(np.arange(nl), FORCED_SIZES))
    scale = 0.02 if metric == "cosine" else 1.0
    x = cent[lab] + scale * rng.standard_normal((len(lab), D)).astype(np.float32)
    a, b = rng.integers(0, nl, n), rng.integers(0, nl, n)
    w = rng.uniform(0, 1, (n, 1)).astype(np.float32)
    q = w * cent[a] + (1 - w) * cent[b] + scale * rng.standard_normal((n, D)).astype(np.float32)
    q[:nl] = cent
    return x.astype(np.float32), q.astype(np.float32), cent, lab


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_forced_list_sizes_empty_lists_and_short_lists(metric):
    from sylber_amd import IVFPQSyllableIndex
    D, M = 32, 2
    x, q, cent, lab = _forced(5, D, metric)
    C = np.random.default_rng(6).standard_normal((M, 256, D // M)).astype(np.float32) * (0.3 if metric == "cosine" else 10.0)
    ix = IVFPQSyllableIndex.build(x, None, M, centroids=cent, codebooks=C, metric=metric, device=DEV)
    assert _np(ix.list_sizes).tolist() == FORCED_SIZES and np.array_equal(_np(ix.labels), lab) and ix.nlist == len(FORCED_SIZES)
    for l in range(ix.nlist):
        assert np.array_equal(_np(ix.list_ids(l)), np.nonzero(lab == l)[0])
    from sylber_amd.pq import _prep
    lut = gpu_lut(ix, _prep(_t(q), metric, ix.device))
    t = P.scan_t(_np(lut), _np(ix.codes))
    for nprobe in (1, 2, ix.nlist):
        probe = _np(ix.probe(q, nprobe))
        assert probe[:ix.nlist, 0].tolist() == list(range(ix.nlist))
        for mc, splits in ((1, 0), (40, 0), (128, 1), (128, 2)):
            et, ec = F.candidates(t, mc, lab, probe)
            gt, gc = gpu_scan(ix, lut, probe, mc, None, splits)
            assert np.array_equal(gc, ec) and np.array_equal(_bits(gt), _bits(et)), (nprobe, mc, splits)
        for rerank in (True, False):
            s, i, cand = (_np(v) for v in ix.search(q, 5, nprobe, 4, rerank=rerank, return_candidates=True))
            mc = 20 if rerank else 5
            assert np.array_equal(cand, F.candidates(t, mc, lab, probe)[1])
            if nprobe == 1:
                # query 0 probes the empty list alone: only padding; query 1 probes the list of one row: that row, then padding
                assert (cand[0] == -1).all() and (i[0] == -1).all() and np.isinf(s[0]).all()
                one = int(np.nonzero(lab == 1)[0][0])
                assert cand[1].tolist() == [one] + [-1] * (mc - 1) and i[1].tolist() == [one, -1, -1, -1, -1]
                assert np.isfinite(s[1, 0]) and np.isinf(s[1, 1:]).all()
            if nprobe == 2:
                # fewer rows in the probed lists than k * refine: every one of them, then padding
                rows = np.isin(lab, probe[1]).sum()
                if rows < mc:
                    assert (cand[1, :rows] >= 0).all() and (cand[1, rows:] == -1).all()
    # 128 candidates from the lists of 63 and 64 rows: 127 rows, one slot of padding
    probe = np.array([[2, 3]])
    gt, gc = gpu_scan(ix, lut[:1], probe, 128)
    assert sorted(gc[0, :127].tolist()) == np.nonzero((lab == 2) | (lab == 3))[0].tolist() and gc[0, 127] == -1 and np.isinf(gt[0, 127])
    # probe slots that name no list cost nothing and change nothing
    gt2, gc2 = gpu_scan(ix, lut[:1], np.array([[-1, 2, -1, 3, 0]]), 128)
    assert np.array_equal(gc2, gc) and np.array_equal(_bits(gt2), _bits(gt))


# ---- 5. independence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M", [(64, 4), BIG])
def test_bitwise_independent_of_splits_chunks_adds_and_workspace(D, M):
    from sylber_amd import IVFPQSyllableIndex
    c = case(D, M, 1500 if (D, M) == BIG else 2000)
    k, refine, nprobe = 10, 4, 3
    kw = dict(groups=c.qg, exclude_same_group=True, return_candidates=True)
    ref = c.ix.search(c.q, k, nprobe, refine, **kw)
    ref_scan = c.ix.search(c.q, k, nprobe, rerank=False, **kw)
    a, b = c.N * 5 // 10, c.N * 8 // 10
    two = IVFPQSyllableIndex.build(c.x[:a], NLIST, M, centroids=c.cent, codebooks=c.C, groups=c.xg[:a], device=DEV)
    assert two.add(c.x[a:b], groups=c.xg[a:b]) == range(a, b) and two.add(c.x[b:], groups=c.xg[b:]) == range(b, c.N)
    assert len(two) == c.N == len(two.index)
    assert torch.equal(two.codes, c.ix.codes) and torch.equal(two.labels, c.ix.labels) and torch.equal(two.list_sizes, c.ix.list_sizes)
    assert torch.equal(two._rid, c.ix._rid) and torch.equal(two._codes, c.ix._codes) and torch.equal(two._rg, c.ix._rg)
    for ix, splits, chunk, fill in [(c.ix, 1, 8192, None), (c.ix, 2, 8192, None), (c.ix, nprobe, 8192, None), (c.ix, 0, 1, None),
                                    (c.ix, 0, 7, None), (c.ix, 2, 7, 0xFF), (c.ix, 0, 8192, 0xFF), (two, 0, 8192, None), (two, nprobe, 7, 0xFF)]:
        got = ix.search(c.q, k, nprobe, refine, splits=splits, query_chunk=chunk, _workspace_fill=fill, **kw)
        assert _same(got, ref), (splits, chunk, fill)
        got = ix.search(c.q, k, nprobe, rerank=False, splits=splits, query_chunk=chunk, _workspace_fill=fill, **kw)
        assert _same(got, ref_scan), (splits, chunk, fill)
    # the C entry point: every split count against the host's scan, the workspace full of 0xFF (a NaN pattern)
    probe = _np(c.ix.probe(c.q, nprobe))
    et, ec = F.candidates(c.t, 40, c.labels, probe)
    for splits in (1, 2, 3, 9):
        gt, gc = gpu_scan(c.ix, c.lut_dev, probe, 40, None, splits, 0xFF)
        assert np.array_equal(gc, ec) and np.array_equal(_bits(gt), _bits(et)), splits


# ---- 6. admissibility -------------------------------------------------------------------------------------------------------------
def test_groups_nan_queries_nan_rows_and_zero_rows():
    from sylber_amd import IVFPQSyllableIndex, PQSyllableIndex
    c = case(32, 2)
    k, nprobe = 8, 3
    for kw in (dict(refine=4), dict(rerank=False)):
        s, i, cand = c.ix.search(c.q, k, nprobe, groups=c.qg, exclude_same_group=True, return_candidates=True, **kw)
        for v in (_np(cand), _np(i)):
            assert (v >= 0).any(1).all() and not ((c.xg[np.maximum(v, 0)] == c.qg[:, None]) & (v >= 0)).any()
    # a NaN query probes no list: only padding; the other queries are not touched
    qb = c.q.copy()
    qb[[2, 30], 5] = np.nan
    keep = [r for r in range(NQ) if r not in (2, 30)]
    assert bool((c.ix.probe(qb, nprobe)[[2, 30]] == -1).all())
    for kw in (dict(refine=4), dict(rerank=False)):
        clean = c.ix.search(c.q, k, nprobe, return_candidates=True, **kw)
        s, i, cand = c.ix.search(qb, k, nprobe, return_candidates=True, **kw)
        assert bool((i[[2, 30]] == -1).all()) and bool(torch.isinf(s[[2, 30]]).all()) and bool((cand[[2, 30]] == -1).all())
        assert _same((s[keep], i[keep], cand[keep]), tuple(v[keep] for v in clean))
    # a NaN row is in no list, keeps the PQ rule's code and mask, and is never returned
    scan_i = _np(c.ix.search(c.q, 1, nprobe, rerank=False)[1])
    hit = sorted({int(v) for v in scan_i[:, 0][:5]})                     # rows that were somebody's best
    xb = c.x.copy()
    xb[hit[0], 3] = np.nan                                               # one sub-row only: the other one still gets its code
    xb[hit[1:]] = np.nan
    ix = IVFPQSyllableIndex.build(xb, NLIST, 2, centroids=c.cent, codebooks=c.C, device=DEV)
    pq = PQSyllableIndex.build(xb, 2, codebooks=c.C, device=DEV)
    lab = _np(ix.labels)
    assert (lab[hit] == -1).all() and (np.delete(lab, hit) == np.delete(c.labels, hit)).all() and int(ix.list_sizes.sum()) == c.N - len(hit)
    assert torch.equal(ix.codes, pq.codes) and ix._listed == c.N - len(hit) and sorted(_np(ix._rid[ix._listed:]).tolist()) == hit
    for kw in (dict(refine=4), dict(rerank=False)):
        s, i, cand = ix.search(c.q, k, nprobe, return_candidates=True, **kw)
        assert not (set(_np(i).ravel().tolist()) & set(hit)) and not (set(_np(cand).ravel().tolist()) & set(hit)) and bool((i >= 0).all())
        assert _same(ix.search(c.q, k, NLIST, return_candidates=True, **kw), pq.search(c.q, k, return_candidates=True, **kw))
    # a zero row under cosine stays zero: similarity 0 with every query, exactly as search
    y = c.x[:100].copy()
    y[7] = 0
    small = IVFPQSyllableIndex.build(y, 4, 2, centroids=y[[1, 30, 60, 90]], codebooks=c.C, metric="cosine", device=DEV)
    assert int(small.labels[7]) >= 0
    a, b = small.search(c.q, 100, 4, 1), small.index.search(c.q, 100)
    assert _same(a, b) and bool((a[1] == 7).any(1).all())
    assert bool((a[0][a[1] == 7] == 0).all()) and not np.signbit(_np(a[0][a[1] == 7])).any()


def test_ties_across_lists_go_to_the_smaller_original_id():
    """two rows with the same code in two different lists tie in t; the list that holds the LARGER id is the nearer one and is scanned
    first, so an order on positions (or on arrival) would return it first"""
    from sylber_amd import IVFPQSyllableIndex
    D, M = 32, 2
    rng = np.random.default_rng(21)
    _, x, C = P.clustered(21, 600, D, M, 1, noise=0.3)
    base = P.decode(rng.integers(0, 256, (1, M)), C)[0]
    d = rng.standard_normal(D).astype(np.float32)
    d *= 0.05 / np.linalg.norm(d)
    x[10] = base + 0.4 * d                                               # nearer centroid 0
    x[200] = base - 0.4 * d                                              # nearer centroid 1
    cent = np.stack([base + d, base - d])
    q = (base - d)[None]                                                 # centroid 1 itself: list 1 is probed first
    ix = IVFPQSyllableIndex.build(x, 2, M, centroids=cent, codebooks=C, device=DEV)
    codes, lab = _np(ix.codes), _np(ix.labels)
    assert (codes[10] == codes[200]).all() and lab[10] == 0 and lab[200] == 1 and _np(ix.probe(q, 2)).tolist() == [[1, 0]]
    assert ((codes == codes[10]).all(1).sum()) == 2
    pos = {int(j): p for p, j in enumerate(_np(ix._rid).tolist())}
    assert pos[10] < pos[200]                                            # list 0 lies first in memory, list 1 is walked first
    for splits in (1, 2):
        for k in (1, 2, 5):
            s, i = ix.search(q, k, 2, rerank=False, splits=splits)
            assert _np(i)[0, :2].tolist() == [10, 200][:k], (splits, k)
            if k > 1:
                assert _bits(_np(s))[0, 0] == _bits(_np(s))[0, 1]
                assert _np(s)[0, 2:].min(initial=np.inf) > _np(s)[0, 0]
        s, i, cand = ix.search(q, 1, 2, 2, return_candidates=True, splits=splits)
        assert _np(cand)[0].tolist() == [10, 200]
    assert _np(ix.search(q, 1, 1, rerank=False)[1]).tolist() == [[200]]  # list 1 alone


# ---- 7. persistence and limits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_drop_rows_and_save_load_round_trips(tmp_path, metric):
    from sylber_amd import IVFPQSyllableIndex, PQSyllableIndex, SyllableIndex
    c = case(64, 4, 2000, metric)
    ix = IVFPQSyllableIndex.build(c.x, NLIST, 4, centroids=c.cent, codebooks=c.C, groups=c.xg, metric=metric, device=DEV)     # its own rows
    kw = dict(groups=c.qg, exclude_same_group=True, return_candidates=True)
    ref = c.ix.search(c.q, 10, 3, 4, **kw)
    ref_scan = c.ix.search(c.q, 10, 3, rerank=False, **kw)
    assert _same(ix.search(c.q, 10, 3, 4, **kw), ref)
    N, D, M = c.N, 64, 4
    assert ix.nbytes == N * (M + 9) + 4 * (NLIST + 1) + 4 * NLIST * D + 4 * NLIST + 4 * 256 * D + 4 * 256 * M + 4 * N * D
    p = str(tmp_path / "held.npz")
    ix.save(p)
    back = IVFPQSyllableIndex.load(p, device=DEV)
    assert back.index is not None and back.metric == metric and len(back) == N and back.nbytes == ix.nbytes and back.nlist == NLIST
    assert torch.equal(back.codes, ix.codes) and torch.equal(back.codebooks, ix.codebooks) and torch.equal(back.centroids, ix.centroids)
    assert torch.equal(back.labels, ix.labels) and torch.equal(back.index.features, ix.index.features)
    assert _same(back.search(c.q, 10, 3, 4, **kw), ref) and _same(back.search(c.q, 10, 3, rerank=False, **kw), ref_scan)
    ids = np.random.default_rng(1).permutation(N)[:50]
    assert np.array_equal(_bits(_np(ix.decode(ids))), _bits(P.decode(c.codes[ids], c.C))) and tuple(ix.decode([]).shape) == (0, D)
    prov = ix.provenance([0, -1])
    before = ix.nbytes
    ix.drop_rows()
    assert ix.index is None and before - ix.nbytes == 4 * N * D and ix.provenance([0, -1]) == prov
    assert _same(ix.search(c.q, 10, 3, **kw), ref_scan) and _same(ix.search(c.q, 10, 3, rerank=False, **kw), ref_scan)
    with pytest.raises(ValueError):
        ix.search(c.q, 10, 3, rerank=True)
    p = str(tmp_path / "dropped.npz")
    ix.save(p)
    back = IVFPQSyllableIndex.load(p, device=DEV)
    assert back.index is None and back.nbytes == ix.nbytes and len(back) == N
    assert _same(back.search(c.q, 10, 3, **kw), ref_scan)
    with pytest.raises(ValueError):
        back.search(c.q, 10, 3, rerank=True)
    # add without the rows: the same codes and lists as the first rows have
    assert back.add(c.x[:7], groups=c.xg[:7]) == range(N, N + 7)
    assert torch.equal(back.codes[N:], ix.codes[:7]) and torch.equal(back.labels[N:], ix.labels[:7]) and len(back) == N + 7
    for other in (SyllableIndex(c.x[:10], device=DEV), PQSyllableIndex.build(c.x[:300], 4, codebooks=c.C, device=DEV)):
        with pytest.raises(ValueError):
            q = str(tmp_path / "other.npz")
            other.save(q)
            IVFPQSyllableIndex.load(q, device=DEV)


def test_value_errors_and_empty_queries():
    from sylber_amd import IVFPQSyllableIndex, SyllableIndex, _lib
    c = case(32, 2)
    x, C, q, ix = c.x, c.C, c.q, c.ix
    for M in (0, 65, 3, 4, 1.5, True, -1):                               # 32 / 3 is no integer, 32 / 4 = 8 is no multiple of 16
        with pytest.raises(ValueError):
            IVFPQSyllableIndex.build(x, NLIST, M, centroids=c.cent, device=DEV)
    for bad in (dict(nlist=0), dict(nlist=None), dict(nlist=1.5), dict(nlist=len(x) + 1), dict(nlist=3, centroids=c.cent),
                dict(nlist=None, centroids=c.cent[:, :16]), dict(nlist=None, centroids=np.full((2, 32), np.inf, np.float32)),
                dict(nlist=NLIST, centroids=c.cent, codebooks=C[:, :255]), dict(nlist=NLIST, centroids=c.cent, codebooks=C[:1]),
                dict(nlist=NLIST, centroids=c.cent, metric="dot")):
        with pytest.raises(ValueError):
            IVFPQSyllableIndex.build(x, M=2, device=DEV, **dict(dict(codebooks=C), **bad))
    with pytest.raises(ValueError):
        IVFPQSyllableIndex.build(x[:255], 2, 2, centroids=c.cent[:2], device=DEV)      # training the codebooks needs 256 rows
    with pytest.raises(ValueError):
        IVFPQSyllableIndex.build(SyllableIndex(device=DEV), 2, 2)
    for k, refine in ((0, 1), (129, 1), (1.5, 1), (True, 1), (1, 0), (1, 1.5), (1, True), (1, 129), (33, 4), (128, 2)):
        with pytest.raises(ValueError):
            ix.search(q, k, 3, refine)
    for k in (0, 129, 1.5, True):
        with pytest.raises(ValueError):
            ix.search(q, k, 3, rerank=False)
    assert tuple(ix.search(q, 128, 3, 50, rerank=False)[0].shape) == (NQ, 128)         # refine plays no part without re-ranking
    for nprobe in (0, NLIST + 1, 129, 1.5, True, -1):
        with pytest.raises(ValueError):
            ix.search(q, 1, nprobe)
        with pytest.raises(ValueError):
            ix.probe(q, nprobe)
    for bad in (dict(queries=np.ones((2, 64), np.float32)), dict(queries=np.ones(32, np.float32)),
                dict(queries=q, groups=[1, 2, 3], exclude_same_group=True), dict(queries=q, exclude_same_group=True),
                dict(queries=q, groups=[1, 2, 3]), dict(queries=q, splits=-1), dict(queries=q, query_chunk=0)):
        with pytest.raises(ValueError):
            ix.search(k=1, nprobe=3, **bad)
    with pytest.raises(ValueError):
        ix.probe(np.ones((2, 64), np.float32), 1)
    with pytest.raises(ValueError):
        ix.decode([len(ix)])
    # n == 0: empty outputs, no launch
    s, i, cand = ix.search(np.zeros((0, 32), np.float32), 8, 3, 4, return_candidates=True)
    assert tuple(s.shape) == (0, 8) and tuple(i.shape) == (0, 8) and tuple(cand.shape) == (0, 32)
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and cand.dtype == torch.int64 and s.device == ix.codebooks.device
    assert ix.last_search == {"pairs": 0, "fraction": 0.0, "workspace_bytes": 0}
    # a refused add leaves everything unchanged, with and without the rows
    own = IVFPQSyllableIndex.build(x[:300], 4, 2, centroids=c.cent[:4], codebooks=C, device=DEV)
    assert own.last_search is None
    for dropped in (False, True):
        if dropped:
            own.drop_rows()
        codes, labels, rid = own.codes, own.labels, own._rid
        for bad_add in (dict(features=np.ones((3, 64), np.float32)), dict(features=x[:3], groups=[1, 2])):
            with pytest.raises(ValueError):
                own.add(**bad_add)
        assert len(own) == 300 and torch.equal(own.codes, codes) and torch.equal(own.labels, labels) and torch.equal(own._rid, rid)
        assert dropped or len(own.index) == 300
        assert own.add(np.zeros((0, 32), np.float32)) == range(300, 300) and len(own) == 300
    # the C entry points refuse bad arguments without a launch
    lib = _lib.load()
    assert lib.sylber_ivfpq_workspace_bytes(1, 129, 1, 0) == -1 and lib.sylber_ivfpq_workspace_bytes(NQ, 3, 40, 0) > 0
    assert lib.sylber_ivfpq_scan(None, 1, None, 1, None, 1, None, None, None, 1, 2, 1, None, None, 0, None, None, None, None) == 1


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------------
def test_segmenter_outputs_end_to_end(tmp_path):
    from sylber_amd import IVFPQSyllableIndex, PQSyllableIndex, Segmenter, SyllableIndex
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
        cent = _np(idx.features)[[0, len(idx) // 2]]
        ix = IVFPQSyllableIndex.build(idx, 2, M=48, centroids=cent, codebooks=C)
        pq = PQSyllableIndex.build(idx, M=48, codebooks=C)
        assert ix.index is idx and len(ix) == len(feats) and ix.M == 48 and tuple(ix.codes.shape) == (len(feats), 48)
        lab = _np(ix.labels)
        for kw in (dict(refine=4), dict(rerank=False)):
            for nprobe in (1, 2):
                s, i, cand = ix.search(feats, k, nprobe, groups=clip, exclude_same_group=True, return_candidates=True, **kw)
                i_np, c_np = _np(i), _np(cand)
                probe = _np(ix.probe(feats, nprobe))
                for r in range(len(feats)):
                    got = c_np[r][c_np[r] >= 0]
                    assert not (clip[got] == clip[r]).any() and np.isin(lab[got], probe[r]).all()
                    for j in i_np[r]:
                        if j < 0:
                            continue
                        cl, sg, st, en = ix.provenance([j])[0]
                        assert cl != clip[r] and [st, en] == outs[cl]["segments"][sg].tolist()
            # both lists probed: the product-quantized search
            assert _same((s, i, cand), pq.search(feats, k, groups=clip, exclude_same_group=True, return_candidates=True, **kw))
        p = str(tmp_path / ("%s.npz" % metric))
        ix.save(p)
        back = IVFPQSyllableIndex.load(p, device=DEV)
        got = back.search(feats, k, 1, 4, groups=clip, exclude_same_group=True, return_candidates=True)
        assert _same(got, ix.search(feats, k, 1, 4, groups=clip, exclude_same_group=True, return_candidates=True))
        assert back.provenance(i_np[0]) == ix.provenance(i_np[0])
        ix.drop_rows()
        assert ix.provenance(i_np[0]) == back.provenance(i_np[0])

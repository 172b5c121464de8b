"""GPU tier, residual codes behind the inverted file (``IVFPQSyllableIndex.build(..., residual=True)``; csrc/pq.hip
``sylber_ivfpq_scan_residual``, ``sylber_ivfpq_list_terms``, ``sylber_ivfpq_recon_norms``, ``sylber_ivfpq_decode``):

* the scan bitwise: from the GPU's own table, ``a`` and ``nrm`` numpy forms the fp32 ``(u + a) + nrm`` and the candidates under
  ``(t, id)`` over the probed lists (tests/ivfpq_residual_ref.py); ``rerank=False`` reports them;
* ``a`` and ``nrm`` against float64 within the bound of their fp32 chains;
* the codes are ``sylber_pq_encode``'s of torch-formed residual rows and the float64 reference's on every decided entry; with one
  list at the origin they are ``PQSyllableIndex``'s; ``decode`` is centroid + codebook rows;
* with at least as many candidates as probed rows a re-ranked search is ``IVFSyllableIndex.search``;
* bitwise independence of splits, query chunking, the workspace's contents and ``build`` against ``build`` + ``add`` + ``add``;
* lists of 0, 1, 63 ... 1 025 rows, NaN rows and queries, groups, ``k`` above the admissible count, ties across lists;
* ``drop_rows``, save / load, a file from before the flag, the errors, and the reconstruction error against today's codes."""
import functools

import numpy as np
import pytest
import torch

import ivfpq_ref as F
import ivfpq_residual_ref as Q
import knn_ref as R
import pq_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEOMETRIES = [(32, 2), (64, 4), (256, 16)]              # code rows of 2, 4 and 16 bytes: the 1-, 4- and 16-byte code loads
BIG = (768, 48)
NLIST = 8
NQ = 40
FORCED_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]       # the scan's tile is 512 positions


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu_lut(ix, qd):
    """the inner-product table, whatever the metric"""
    from sylber_amd import _lib
    from sylber_amd.kmeans import _stream, _vp
    from sylber_amd.search import METRICS
    lut = torch.empty((qd.shape[0], ix.M, 256), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().sylber_pq_lut(_vp(qd), qd.shape[0], qd.shape[1], _vp(ix.codebooks), None, ix.M, METRICS["cosine"], _vp(lut),
                                         _stream(qd.device)), "sylber_pq_lut")
    return lut


def gpu_list_terms(ix, qd, probe):
    from sylber_amd import _lib
    from sylber_amd.kmeans import _stream, _vp
    pd = _t(probe, np.int32)
    a = torch.empty(pd.shape, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().sylber_ivfpq_list_terms(_vp(qd), qd.shape[0], qd.shape[1], _vp(ix.centroids), ix.nlist, _vp(pd), pd.shape[1], _vp(a),
                                                   _stream(qd.device)), "sylber_ivfpq_list_terms")
    return a


def raw_scan(lut, probe, off, nlist, codes, bad, rid, listed, M, mc, a, nrm, qg=None, rg=None, splits=0, fill=None):
    """the C entry point on device arrays -> (t [n, mc], cand [n, mc]) as numpy"""
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
    _lib.check(lib.sylber_ivfpq_scan_residual(_vp(lut), n, _vp(pd), nprobe, _vp(off), nlist, _vp(codes), _vp(bad), _vp(rid), listed, M, mc,
                                              _vp(g), _vp(rg if g is not None else None), splits, _vp(a), _vp(nrm), _vp(t), _vp(cand), _vp(ws),
                                              _stream(lut.device)), "sylber_ivfpq_scan_residual")
    return _np(t), _np(cand)


def gpu_scan(ix, lut, probe, a, mc, qg=None, splits=0, fill=None):
    return raw_scan(lut, probe, ix._off, ix.nlist, ix._codes, ix._rbad, ix._rid, ix._listed, ix.M, mc, a, ix._nrm, qg, ix._rg, splits, fill)


def host_t(ix, lut, a, probe):
    """[n, N] fp32: the contract's t from the GPU's own table, a and nrm"""
    nrm = _np(ix._by_id(ix._nrm)) if ix._nrm is not None else None
    return Q.scan_t(_np(lut), _np(ix.codes), _np(a), nrm, _np(ix.labels), probe)


def _centroids(cent, metric):
    return R.unit_rows(cent).astype(np.float32) if metric == "cosine" else cent


class Case:
    """one residual index with everything the tests share: inputs, codebooks sampled from the residuals, the GPU's own table"""

    def __init__(self, D, M, N, metric):
        from sylber_amd import IVFPQSyllableIndex, SyllableIndex
        from sylber_amd.pq import _prep
        rng = np.random.default_rng(D * 10000 + M * 100 + N)
        self.q, self.x, cent, self.lists = Q.clustered_lists(D + M + N, N, D, M, NLIST, NQ)
        self.cent = _centroids(cent, metric)
        self.xg, self.qg = rng.integers(0, 3, N), rng.integers(0, 3, NQ)
        self.metric, self.N, self.D, self.M = metric, N, D, M
        self.index = SyllableIndex(self.x, metric=metric, groups=self.xg, device=DEV)
        self.xs = _np(self.index.features)                               # the stored rows (unit rows under cosine)
        self.C = Q.sampled_codebooks(Q.residuals(self.xs, self.cent, self.lists), M, 1)
        self.ix = IVFPQSyllableIndex.build(self.index, NLIST, M, centroids=self.cent, codebooks=self.C, residual=True)
        self.qd = _prep(_t(self.q), metric, self.ix.device)
        self.lut_dev = gpu_lut(self.ix, self.qd)
        self.codes = _np(self.ix.codes)
        self.labels = _np(self.ix.labels)


@functools.lru_cache(maxsize=None)
def case(D, M, N=2000, metric="l2"):
    return Case(D, M, N, metric)


# ---- 1. the scan ------------------------------------------------------------------------------------------------------------------
def _check_scan(c, nprobes, mcs):
    from sylber_amd._index import _row_norms
    ix = c.ix
    assert ix.residual is True and np.array_equal(c.labels, c.lists) and (ix._nrm is not None) == (c.metric == "l2")
    qsq = _np(_row_norms(c.qd))
    for nprobe in nprobes:
        probe = _np(ix.probe(c.q, nprobe))
        assert probe.shape == (NQ, nprobe) and probe.min() >= 0 and len(np.unique(probe[:, 0])) > 1
        a = gpu_list_terms(ix, c.qd, probe)
        t = host_t(ix, c.lut_dev, a, probe)
        assert t.dtype == np.float32 and np.array_equal(~np.isnan(t), F.member(c.labels, probe))
        for mc in mcs:
            for qg in (None, c.qg):
                kw = {} if qg is None else dict(q_group=qg, x_group=c.xg)
                et, ec = Q.candidates(t, mc, None, **kw)
                gt, gc = gpu_scan(ix, c.lut_dev, probe, a, mc, qg)
                assert np.array_equal(gc, ec), (nprobe, mc, qg is not None)
                assert np.array_equal(_bits(gt), _bits(et)), (nprobe, mc, qg is not None)
        # the class takes the same lists and reports the scan's own t
        s, i, cand = c.ix.search(c.q, 10, nprobe, rerank=False, return_candidates=True)
        et, ec = Q.candidates(t, 10, None)
        assert np.array_equal(_np(cand), ec) and np.array_equal(_np(i), ec)
        assert np.array_equal(_bits(_np(s)), _bits(P.report(et, ec, qsq, c.metric)))
        assert ix.last_search["pairs"] == int(_np(ix.list_sizes)[probe].sum())


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,M", GEOMETRIES)
def test_scan_is_the_host_sum_over_the_probed_lists_bitwise(D, M, metric):
    _check_scan(case(D, M, 2000, metric), (1, 3), (1, 10, 128))


def test_scan_bitwise_at_the_flagship_geometry():
    _check_scan(case(*BIG, 3000), (3,), (10, 128))


# ---- 2. a and nrm -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,M", GEOMETRIES)
def test_list_terms_and_norms_against_float64(D, M, metric):
    c = case(D, M, 2000, metric)
    ix = c.ix
    probe = _np(ix.probe(c.q, 3))
    probe[5, 1] = -1                                                     # a slot without a list: 0, never read
    qd = _np(c.qd)
    a = _np(gpu_list_terms(ix, c.qd, probe))
    want, bound = Q.list_terms(qd, c.cent, probe), Q.list_term_bound(qd, c.cent, probe)
    assert a[5, 1] == 0 and not np.signbit(a[5, 1])
    assert (np.abs(a - want) <= bound).all() and np.abs(want).min(initial=np.inf, where=probe >= 0) > 0
    if metric == "l2":
        xhat = Q.reconstruct(c.codes, c.labels, c.cent, c.C)             # fp32, one addition per element
        n64 = Q.recon_norms(xhat)
        got = _np(ix._by_id(ix._nrm))
        assert (np.abs(got - n64) <= (D + 2) * 2.0 ** -24 * n64).all() and n64.min() > 0
    else:
        assert ix._nrm is None


# ---- 3. codes and decode ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,M", GEOMETRIES)
def test_codes_are_the_encode_of_the_residual_rows(D, M, metric):
    from sylber_amd.pq import _encode
    c = case(D, M, 2000, metric)
    ix = c.ix
    r = (c.index._x - ix.centroids.index_select(0, ix.labels)).contiguous()
    codes, bad = _encode(r, ix.codebooks, ix._cnorm)
    assert torch.equal(ix.codes, codes) and not bool(bad.any()) and not bool(ix._rbad.any()) and ix.codes.dtype == torch.uint8
    rr = Q.residuals(c.xs, c.cent, c.labels)
    assert np.array_equal(_bits(_np(r)), _bits(rr))                      # one fp32 subtraction per element
    want, wbad = Q.encode(c.xs, c.cent, c.labels, c.C)
    dec = P.decided(rr, c.C)
    assert 1.0 - dec.mean() <= 0.01 and not wbad.any()
    assert (c.codes == want)[dec].all()
    # decode: the list's centroid plus the codebook rows, one fp32 addition per element
    ids = np.random.default_rng(1).permutation(c.N)[:50]
    assert np.array_equal(_bits(_np(ix.decode(ids))), _bits(Q.reconstruct(c.codes[ids], c.labels[ids], c.cent, c.C)))
    assert tuple(ix.decode([]).shape) == (0, D)
    assert ix.nbytes == c.N * (M + (13 if metric == "l2" else 9)) + 4 * (NLIST + 1) + 4 * NLIST * D + 4 * NLIST + 4 * 256 * D + 4 * 256 * M \
        + 4 * c.N * D


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_zero_centroids_one_list_gives_the_pq_codes(metric):
    from sylber_amd import IVFPQSyllableIndex, PQSyllableIndex
    q, x, C = P.clustered(17, 1500, 64, 4, NQ, noise=0.3)
    ix = IVFPQSyllableIndex.build(x, None, 4, centroids=np.zeros((1, 64), np.float32), codebooks=C, metric=metric, device=DEV, residual=True)
    pq = PQSyllableIndex.build(x, 4, codebooks=C, metric=metric, device=DEV)
    assert ix.residual and ix.nlist == 1 and int(ix.list_sizes[0]) == 1500
    assert torch.equal(ix.codes, pq.codes) and torch.equal(ix._by_id(ix._rbad), pq._bad) and not bool(pq._bad.any())
    ids = np.arange(0, 1500, 7)
    assert torch.equal(ix.decode(ids), pq.decode(ids))


# ---- 4. re-rank -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_rerank_with_every_probed_row_a_candidate_is_the_ivf_search(metric):
    from sylber_amd import IVFPQSyllableIndex, IVFSyllableIndex, SyllableIndex
    q, x, cent, lists = Q.clustered_lists(23, 100, 32, 2, 4, NQ)
    cent = _centroids(cent, metric)
    rng = np.random.default_rng(23)
    xg, qg = rng.integers(0, 3, 100), rng.integers(0, 3, NQ)
    C = (0.5 * rng.standard_normal((2, 256, 16)) / (np.sqrt(32) * 4 if metric == "cosine" else 1)).astype(np.float32)
    index = SyllableIndex(x, metric=metric, groups=xg, device=DEV)
    ix = IVFPQSyllableIndex.build(index, None, 2, centroids=cent, codebooks=C, residual=True)
    ivf = IVFSyllableIndex.build(index, centroids=cent)
    assert torch.equal(ix.labels, ivf.labels) and int(ix.list_sizes.min()) > 0
    for kw in ({}, dict(groups=qg, exclude_same_group=True)):
        for k, refine in ((32, 4), (128, 1), (10, 10)):
            s, i, cand = ix.search(q, k, 2, refine, return_candidates=True, **kw)
            assert _same((s, i), ivf.search(q, k, 2, **kw)), (k, refine, bool(kw))
            assert bool(((cand >= 0).sum(1) <= 100).all()) and bool((cand[:, -1] == -1).all())


# ---- 5. independence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M", [(64, 4), BIG])
def test_bitwise_independent_of_splits_chunks_adds_and_workspace(D, M):
    from sylber_amd import IVFPQSyllableIndex
    c = case(D, M, 3000 if (D, M) == BIG else 2000)
    k, refine, nprobe = 10, 4, 3
    kw = dict(groups=c.qg, exclude_same_group=True, return_candidates=True)
    ref = c.ix.search(c.q, k, nprobe, refine, **kw)
    ref_scan = c.ix.search(c.q, k, nprobe, rerank=False, **kw)
    a, b = c.N * 5 // 10, c.N * 8 // 10
    two = IVFPQSyllableIndex.build(c.x[:a], NLIST, M, centroids=c.cent, codebooks=c.C, groups=c.xg[:a], device=DEV, residual=True)
    assert two.add(c.x[a:b], groups=c.xg[a:b]) == range(a, b) and two.add(c.x[b:], groups=c.xg[b:]) == range(b, c.N)
    assert len(two) == c.N == len(two.index) and two.residual
    assert torch.equal(two.codes, c.ix.codes) and torch.equal(two.labels, c.ix.labels) and torch.equal(two.list_sizes, c.ix.list_sizes)
    assert torch.equal(two._rid, c.ix._rid) and torch.equal(two._codes, c.ix._codes) and torch.equal(two._rg, c.ix._rg)
    assert np.array_equal(_bits(_np(two._nrm)), _bits(_np(c.ix._nrm)))
    for ix, splits, chunk, fill in [(c.ix, 1, 8192, None), (c.ix, 2, 8192, None), (c.ix, nprobe, 8192, None), (c.ix, 0, 1, None),
                                    (c.ix, 0, 7, None), (c.ix, 2, 7, 0xFF), (c.ix, 0, 8192, 0xFF), (two, 0, 8192, None), (two, nprobe, 7, 0xFF)]:
        got = ix.search(c.q, k, nprobe, refine, splits=splits, query_chunk=chunk, _workspace_fill=fill, **kw)
        assert _same(got, ref), (splits, chunk, fill)
        got = ix.search(c.q, k, nprobe, rerank=False, splits=splits, query_chunk=chunk, _workspace_fill=fill, **kw)
        assert _same(got, ref_scan), (splits, chunk, fill)
    # nrm does not depend on the launch either: row by row it is what the whole build gave
    from sylber_amd.pq import _recon_norms
    lab32 = c.ix.labels.to(torch.int32)
    for lo, hi in ((0, 1), (255, 257), (c.N - 3, c.N)):
        part = _recon_norms(c.ix.codes[lo:hi].contiguous(), lab32[lo:hi].contiguous(), c.ix.centroids, c.ix.codebooks)
        assert np.array_equal(_bits(_np(part)), _bits(_np(c.ix._by_id(c.ix._nrm)[lo:hi])))


# ---- 6. forced list sizes and admissibility ---------------------------------------------------------------------------------------
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
def test_forced_list_sizes_nan_rows_nan_queries_and_groups(metric):
    from sylber_amd import IVFPQSyllableIndex
    from sylber_amd.pq import _prep
    D, M = 32, 2
    x, q, cent, lab = _forced(5, D, metric)
    rng = np.random.default_rng(6)
    nan_rows = [3, 700, len(x) - 1] if metric == "l2" else []            # "cosine" stores a NaN row as a zero row: there are none
    if nan_rows:
        x[3, 5] = np.nan                                                 # one sub-row only: still code 0 in both, in no list
        x[[700, len(x) - 1]] = np.nan
    lab = lab.copy()
    lab[nan_rows] = -1
    sizes = np.bincount(lab[lab >= 0], minlength=len(FORCED_SIZES))
    xg = rng.integers(0, 3, len(x))
    C = (rng.standard_normal((M, 256, D // M)) * (0.02 if metric == "cosine" else 1.0)).astype(np.float32)
    ix = IVFPQSyllableIndex.build(x, None, M, centroids=cent, codebooks=C, groups=xg, metric=metric, device=DEV, residual=True)
    assert _np(ix.list_sizes).tolist() == sizes.tolist() and np.array_equal(_np(ix.labels), lab) and sizes[0] == 0
    assert sizes[1] == 1 and sizes.sum() == len(x) - len(nan_rows)       # "l2": three lists lost a row to the NaNs; the clean sizes run below
    codes = _np(ix.codes)
    assert (codes[nan_rows] == 0).all() and _np(ix._by_id(ix._rbad))[nan_rows].all() and ix._listed == len(x) - len(nan_rows)
    assert np.array_equal(_bits(_np(ix.decode(nan_rows))), _bits(np.tile(np.concatenate([C[m][0] for m in range(M)]), (len(nan_rows), 1))))
    qd = _prep(_t(q), metric, ix.device)
    lut = gpu_lut(ix, qd)
    for nprobe in (1, 2, ix.nlist):
        probe = _np(ix.probe(q, nprobe))
        assert probe[:ix.nlist, 0].tolist() == list(range(ix.nlist))
        a = gpu_list_terms(ix, qd, probe)
        t = host_t(ix, lut, a, probe)
        for mc, splits in ((1, 0), (40, 0), (128, 1), (128, 2)):
            et, ec = Q.candidates(t, mc, None)
            gt, gc = gpu_scan(ix, lut, probe, a, mc, None, splits)
            assert np.array_equal(gc, ec) and np.array_equal(_bits(gt), _bits(et)), (nprobe, mc, splits)
            assert not np.isin(nan_rows, gc).any()
        qg = rng.integers(0, 3, len(q))
        et, ec = Q.candidates(t, 40, None, qg, xg)
        gt, gc = gpu_scan(ix, lut, probe, a, 40, qg)
        assert np.array_equal(gc, ec) and np.array_equal(_bits(gt), _bits(et))
        assert not ((xg[np.maximum(gc, 0)] == qg[:, None]) & (gc >= 0)).any()
        for rerank in (True, False):
            s, i, cand = (_np(v) for v in ix.search(q, 5, nprobe, 4, rerank=rerank, return_candidates=True))
            mc = 20 if rerank else 5
            assert np.array_equal(cand, Q.candidates(t, mc, None)[1])
            if nprobe == 1:
                # query 0 probes the empty list alone: only padding; query 1 probes the list of one row: k is above the admissible count
                assert (cand[0] == -1).all() and (i[0] == -1).all() and np.isinf(s[0]).all()
                one = int(np.nonzero(lab == 1)[0][0])
                assert cand[1].tolist() == [one] + [-1] * (mc - 1) and i[1].tolist() == [one, -1, -1, -1, -1]
                assert np.isfinite(s[1, 0]) and np.isinf(s[1, 1:]).all()
    if metric == "cosine":                                               # a NaN query is scored as a zero row there
        return
    # NaN queries probe nothing: only padding; the other queries are not touched
    qb = q.copy()
    qb[[2, 30], 5] = np.nan
    keep = [r for r in range(len(q)) if r not in (2, 30)]
    for kw in (dict(refine=4), dict(rerank=False)):
        clean = ix.search(q, 8, 3, return_candidates=True, **kw)
        s, i, cand = ix.search(qb, 8, 3, return_candidates=True, **kw)
        assert bool((i[[2, 30]] == -1).all()) and bool(torch.isinf(s[[2, 30]]).all()) and bool((cand[[2, 30]] == -1).all())
        assert _same((s[keep], i[keep], cand[keep]), tuple(v[keep] for v in clean))


def test_clean_forced_list_sizes():
    """every size of FORCED_SIZES itself (no row lost to a NaN): the lists end one short of, at, and one past the 512-position tile"""
    from sylber_amd import IVFPQSyllableIndex
    from sylber_amd.pq import _prep
    D, M = 32, 2
    x, q, cent, lab = _forced(7, D, "l2")
    C = np.random.default_rng(8).standard_normal((M, 256, D // M)).astype(np.float32)
    ix = IVFPQSyllableIndex.build(x, None, M, centroids=cent, codebooks=C, device=DEV, residual=True)
    assert _np(ix.list_sizes).tolist() == FORCED_SIZES and np.array_equal(_np(ix.labels), lab)
    qd = _prep(_t(q), "l2", ix.device)
    lut = gpu_lut(ix, qd)
    for nprobe in (1, ix.nlist):
        probe = _np(ix.probe(q, nprobe))
        a = gpu_list_terms(ix, qd, probe)
        t = host_t(ix, lut, a, probe)
        for mc, splits in ((1, 0), (128, 0), (128, 2)):
            et, ec = Q.candidates(t, mc, None)
            gt, gc = gpu_scan(ix, lut, probe, a, mc, None, splits)
            assert np.array_equal(gc, ec) and np.array_equal(_bits(gt), _bits(et)), (nprobe, mc, splits)
    # 128 candidates from the lists of 63 and 64 rows: 127 rows, one slot of padding; slots that name no list change nothing
    probe = np.array([[2, 3]])
    a = gpu_list_terms(ix, qd[:1], probe)
    gt, gc = gpu_scan(ix, lut[:1], probe, a, 128)
    assert sorted(gc[0, :127].tolist()) == np.nonzero((lab == 2) | (lab == 3))[0].tolist() and gc[0, 127] == -1 and np.isinf(gt[0, 127])
    probe2 = np.array([[-1, 2, -1, 3, 0]])
    gt2, gc2 = gpu_scan(ix, lut[:1], probe2, gpu_list_terms(ix, qd[:1], probe2), 128)
    assert np.array_equal(gc2, gc) and np.array_equal(_bits(gt2), _bits(gt))


def test_ties_across_lists_go_to_the_smaller_original_id():
    """equal codes, a = 0 and nrm = 0: every row ties in t.  The list that is walked first holds the LARGER ids, so an order on
    positions (or on arrival) would return them first."""
    M = 4
    rng = np.random.default_rng(31)
    lut = _t(rng.standard_normal((1, M, 256)))
    codes = torch.full((6, M), 7, dtype=torch.uint8, device=DEV)
    off = _t([0, 3, 6], np.int32)
    rid = _t([3, 4, 5, 0, 1, 2], np.int32)                               # list 0 = rows 3, 4, 5; list 1 = rows 0, 1, 2
    bad = torch.zeros(6, dtype=torch.uint8, device=DEV)
    a = torch.zeros((1, 2), dtype=torch.float32, device=DEV)
    nrm = torch.zeros(6, dtype=torch.float32, device=DEV)
    want_t = P.scan_t(_np(lut), _np(codes))[0, 0]
    for splits in (1, 2):
        for mc in (1, 4, 6, 8):
            for r in (nrm, None):
                gt, gc = raw_scan(lut, np.array([[0, 1]]), off, 2, codes, bad, rid, 6, M, mc, a, r, splits=splits)
                assert gc[0].tolist() == (list(range(6)) + [-1, -1])[:mc], (splits, mc)
                assert (_bits(gt[0, :min(mc, 6)]) == _bits(want_t)).all() and np.isinf(gt[0, 6:]).all()
    gt, gc = raw_scan(lut, np.array([[0]]), off, 2, codes, bad, rid, 6, M, 4, a, nrm)
    assert gc[0].tolist() == [3, 4, 5, -1]                               # list 0 alone


# ---- 7. persistence, errors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_drop_rows_and_save_load_round_trips(tmp_path, metric):
    from sylber_amd import IVFPQSyllableIndex
    c = case(64, 4, 2000, metric)
    ix = IVFPQSyllableIndex.build(c.x, NLIST, 4, centroids=c.cent, codebooks=c.C, groups=c.xg, metric=metric, device=DEV, residual=True)
    kw = dict(groups=c.qg, exclude_same_group=True, return_candidates=True)
    ref = c.ix.search(c.q, 10, 3, 4, **kw)
    ref_scan = c.ix.search(c.q, 10, 3, rerank=False, **kw)
    assert _same(ix.search(c.q, 10, 3, 4, **kw), ref)
    p = str(tmp_path / "held.npz")
    ix.save(p)
    back = IVFPQSyllableIndex.load(p, device=DEV)
    assert back.residual is True and back.index is not None and back.metric == metric and len(back) == c.N and back.nbytes == ix.nbytes
    assert torch.equal(back.codes, ix.codes) and torch.equal(back.labels, ix.labels) and torch.equal(back.centroids, ix.centroids)
    assert (back._nrm is None) == (metric == "cosine") and (metric == "cosine" or np.array_equal(_bits(_np(back._nrm)), _bits(_np(ix._nrm))))
    assert _same(back.search(c.q, 10, 3, 4, **kw), ref) and _same(back.search(c.q, 10, 3, rerank=False, **kw), ref_scan)
    before = ix.nbytes
    ix.drop_rows()
    assert ix.index is None and ix.residual is True and before - ix.nbytes == 4 * c.N * 64
    assert ix.nbytes - 4 * (NLIST + 1) - 4 * NLIST * 64 - 4 * NLIST - 4 * 256 * 64 - 4 * 256 * 4 == c.N * (4 + (13 if metric == "l2" else 9))
    assert _same(ix.search(c.q, 10, 3, **kw), ref_scan) and _same(ix.search(c.q, 10, 3, rerank=False, **kw), ref_scan)
    with pytest.raises(ValueError):
        ix.search(c.q, 10, 3, rerank=True)
    ids = np.arange(0, c.N, 41)
    assert torch.equal(ix.decode(ids), c.ix.decode(ids))
    p = str(tmp_path / "dropped.npz")
    ix.save(p)
    back = IVFPQSyllableIndex.load(p, device=DEV)
    assert back.index is None and back.residual is True and back.nbytes == ix.nbytes
    assert _same(back.search(c.q, 10, 3, **kw), ref_scan)
    # add without the rows: the same codes, lists and norms as the first rows have
    assert back.add(c.x[:7], groups=c.xg[:7]) == range(c.N, c.N + 7)
    assert torch.equal(back.codes[c.N:], ix.codes[:7]) and torch.equal(back.labels[c.N:], ix.labels[:7]) and len(back) == c.N + 7
    assert torch.equal(back.decode(np.arange(c.N, c.N + 7)), ix.decode(np.arange(7)))
    # a file from before the flag (no "residual" entry) loads as today's index
    plain = IVFPQSyllableIndex.build(c.x, NLIST, 4, centroids=c.cent, codebooks=c.C, groups=c.xg, metric=metric, device=DEV)
    assert plain.residual is False and plain._nrm is None
    p = str(tmp_path / "plain.npz")
    plain.save(p)
    assert "residual" not in np.load(p, allow_pickle=False).files        # the file of an index without residual codes has not changed
    back = IVFPQSyllableIndex.load(p, device=DEV)
    assert back.residual is False and back.nbytes == plain.nbytes
    assert _same(back.search(c.q, 10, 3, 4, **kw), plain.search(c.q, 10, 3, 4, **kw))
    # ... and the flag of a residual file is what makes it one: without it the same arrays load as today's index
    z = dict(np.load(str(tmp_path / "held.npz"), allow_pickle=False))
    assert bool(z.pop("residual"))
    old = str(tmp_path / "old.npz")
    np.savez(old, **z)
    assert IVFPQSyllableIndex.load(old, device=DEV).residual is False
    assert not _same(plain.search(c.q, 10, 3, rerank=False, **kw), ref_scan) and not torch.equal(plain.codes, c.ix.codes)


def test_value_errors_and_refused_adds():
    from sylber_amd import IVFPQSyllableIndex, _lib
    c = case(32, 2)
    for bad in (1, 0, None, "yes", 1.0, np.array([True])):
        with pytest.raises(ValueError):
            IVFPQSyllableIndex.build(c.x, NLIST, 2, centroids=c.cent, codebooks=c.C, device=DEV, residual=bad)
    with pytest.raises(ValueError):                                      # training needs 256 rows in a list
        IVFPQSyllableIndex.build(c.x[:255], None, 2, centroids=c.cent[:2], device=DEV, residual=True)
    y = c.x[:300].copy()
    y[:60] = np.nan                                                      # 300 rows, 240 of them in a list
    with pytest.raises(ValueError):
        IVFPQSyllableIndex.build(y, None, 2, centroids=c.cent, device=DEV, residual=True)
    # a refused add leaves everything unchanged, with and without the rows
    own = IVFPQSyllableIndex.build(c.x[:300], None, 2, centroids=c.cent[:4], codebooks=c.C, device=DEV, residual=True)
    for dropped in (False, True):
        if dropped:
            own.drop_rows()
        codes, labels, rid, nrm = own.codes, own.labels, own._rid, own._nrm
        for bad_add in (dict(features=np.ones((3, 64), np.float32)), dict(features=c.x[:3], groups=[1, 2])):
            with pytest.raises(ValueError):
                own.add(**bad_add)
        assert len(own) == 300 and torch.equal(own.codes, codes) and torch.equal(own.labels, labels) and torch.equal(own._rid, rid)
        assert torch.equal(own._nrm, nrm) and own.add(np.zeros((0, 32), np.float32)) == range(300, 300) and len(own) == 300
    # the C entry points refuse bad arguments without a launch
    lib = _lib.load()
    assert lib.sylber_ivfpq_scan_residual(None, 1, None, 1, None, 1, None, None, None, 1, 2, 1, None, None, 0, None, None, None, None, None,
                                          None) == 1
    assert lib.sylber_last_error().decode().startswith("sylber_ivfpq_scan_residual: ")
    assert lib.sylber_ivfpq_list_terms(None, 1, 32, None, 1, None, 1, None, None) == 1
    assert lib.sylber_ivfpq_recon_norms(None, 1, None, None, 1, None, 2, 32, None, None) == 1
    assert lib.sylber_ivfpq_decode(None, 1, None, None, 1, None, 2, 32, None, None) == 1
    assert lib.sylber_last_error().decode().startswith("sylber_ivfpq_decode: ")


# ---- 8. what it is for ------------------------------------------------------------------------------------------------------------
def test_trained_residual_codes_halve_the_reconstruction_error():
    """512 lists given as the true centres, codebooks trained by ``build`` in both modes: the residual codes' mean squared
    reconstruction error is below half of that of the codes of the rows themselves (the float64 restatement reads 8x with trained
    codebooks, 43x with sampled ones: the half is a condition, not a measurement)"""
    from sylber_amd import IVFPQSyllableIndex, SyllableIndex
    from sylber_amd.kmeans import fit_kmeans
    N, D, M, nlist = 4096, 64, 4, 512
    q, x, cent, lists = Q.clustered_lists(11, N, D, M, nlist, NQ)
    index = SyllableIndex(x, device=DEV)
    res = IVFPQSyllableIndex.build(index, None, M, centroids=cent, seed=3, residual=True)
    plain = IVFPQSyllableIndex.build(index, None, M, centroids=cent, seed=3)
    assert np.array_equal(_np(res.labels), lists) and torch.equal(res.labels, plain.labels)
    # the codebooks are those of the residuals
    r = index._x - res.centroids.index_select(0, res.labels)
    for m in (0, 3):
        fit = fit_kmeans(r[:, 16 * m:16 * m + 16].contiguous(), 256, seed=3 + m, max_iter=25, tol=1e-4, device=DEV)
        assert torch.equal(res.codebooks[m], fit.centroids)
    ids = np.arange(N)
    e_res, e_plain = Q.recon_error(x, _np(res.decode(ids))), Q.recon_error(x, _np(plain.decode(ids)))
    print("reconstruction error: residual %.3f, codes of the rows themselves %.3f" % (e_res, e_plain))
    assert e_res < 0.5 * e_plain, (e_res, e_plain)
    # and the scan finds the rows: every query is a row plus a quarter of the lists' spread
    s, i = res.search(q, 1, 4, rerank=False)
    assert bool((i >= 0).all())

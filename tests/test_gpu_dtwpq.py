"""GPU tier, compressed phrase search (csrc/dtwpq.hip behind ``PQSyllableIndex.search_phrases``).

* rows dropped, "l2": the whole call equals ``search_phrases_refined`` of a ``SyllableIndex`` over the decoded rows, bit for bit;
* stage 1 equals ``sylber_dtw16_scan`` on the materialised plane ``pack16(decode(all codes))`` with the reconstruction norms, bit for
  bit, both metrics, masked rows included;
* rows held: ``pq.index.search_phrases`` restricted to the candidates, and that search itself once m covers the sequences or the bound
  of tests/dtwpq_ref.py decides the candidate set;
* bitwise invariance under the split / chunk / packing hooks, stale workspace contents, how the index was built, a save /
  load round trip and ``drop_rows()``;
* tile, K-step and sub-space edges; admissibility and padding; the fp16 range, the refusals (the C entry's too) and ``P = 0``;
* stage 1 within ``coarse_cost_error_bound`` of the float64 restatement on the decoded rows."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dtw16_ref as R16
import dtwpq_ref as R
import pq_ref as PQ

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COMBOS = [(m, s) for m in ("l2", "cosine") for s in R.STORAGES]


def _np(t):
    return t.cpu().numpy()


def _groups_of(offsets):
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets)).astype(np.int32)


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _assert_equal(got, want, what=""):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, what
        if a.dtype == torch.float32:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what
        else:
            assert torch.equal(a, b), what


@functools.lru_cache(maxsize=None)
def _index(metric):
    from sylber_amd import SyllableIndex
    x, offsets, phrases, k, refine = R16.checkable_inputs()
    assert x.shape == (1337, 64) and len(offsets) == 61 and len(phrases) == 24
    return SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)


@functools.lru_cache(maxsize=None)
def _codebooks(metric, M):
    """explicit codebooks cut from the rows as the index holds them: no k-means"""
    return R.codebooks_from_rows(_np(_index(metric).features), M)


def _pq(metric, M=4):
    """a fresh PQSyllableIndex over the shared rows (the rows are not copied; ``drop_rows`` on it leaves ``_index`` alone)"""
    from sylber_amd import PQSyllableIndex
    return PQSyllableIndex.build(_index(metric), M, codebooks=_codebooks(metric, M))


def _decoded_index(pq, groups, nan_masked=False):
    """the oracle of rerank=False under "l2": a SyllableIndex over the decoded rows (masked rows as NaN rows on request)"""
    from sylber_amd import SyllableIndex
    xh = pq.decode(torch.arange(len(pq), device=DEV))
    if nan_masked:
        xh = torch.where((pq._bad != 0)[:, None], torch.full_like(xh, float("nan")), xh)
    return SyllableIndex(xh, metric="l2", groups=groups, device=DEV)


def _dtw16_scan_on_decoded(pq, phrases, m, storage, offsets, pgrp=None):
    """(cand int32 [P, m], coarse [P, m]) of ``sylber_dtw16_scan`` driven through ``_lib`` on the materialised plane
    pack16(decode(all codes)) (a NaN row for a masked one) with db_norm = the reconstruction norms (NaN for a masked row)"""
    from sylber_amd import _index as IX
    from sylber_amd import _lib
    from sylber_amd.kmeans import _stream, _vp
    lib = _lib.load()
    dev = pq.device
    N, D = len(pq), pq.dim
    xh = pq.decode(torch.arange(N, device=dev))
    masked = (pq._bad != 0)
    xh = torch.where(masked[:, None], torch.full_like(xh, float("nan")), xh).contiguous()
    plane = IX._pack16(xh, storage, refuse=True)
    c = IX._row_norms(xh) if pq.metric == "l2" else None
    lens = np.array([len(p) for p in phrases], np.int64)
    qd = IX._prep(torch.cat([torch.as_tensor(p) for p in phrases]), pq.metric, dev)
    P = len(phrases)
    seq_id, seq_grp = IX._sequence_tables(offsets, pq._db_groups() if pgrp is not None else None, dev)
    b = IX._phrase_blocks(lib, dev, qd, lens, 0, P, offsets, m, 0, 0, pgrp)
    qn = IX._row_norms(b.qp) if pq.metric == "l2" else None
    q16 = IX._pack16(b.qp, storage, refuse=False)
    ws = torch.empty(int(lib.sylber_dtw16_workspace_bytes(P, m, b.C)), dtype=torch.uint8, device=dev)
    cand = torch.empty((P, m), dtype=torch.int32, device=dev)
    coarse = torch.empty((P, m), dtype=torch.float32, device=dev)
    meta_d, sp_d, br_d, cut_d, pg_d = b.tables()
    with torch.cuda.device(dev):
        _lib.check(lib.sylber_dtw16_scan(_vp(q16), b.nb, _vp(meta_d), _vp(sp_d), _vp(br_d), P, b.slots, _vp(plane), N, D, _vp(c), _vp(qn),
                                         IX.METRICS[pq.metric], IX.STORAGES[storage][0], m, _vp(seq_id), _vp(cut_d), b.C, _vp(pg_d),
                                         _vp(seq_grp), _vp(cand), _vp(coarse), _vp(ws), _stream(dev)), "sylber_dtw16_scan")
    return cand.to(torch.int64), coarse


# ---- 1, 2: the bitwise oracles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", R.STORAGES)
@pytest.mark.parametrize("M", (4, 2, 1))
def test_rows_dropped_l2_equals_the_refined_search_on_the_decoded_rows(storage, M):
    x, offsets, phrases, k, refine = R16.checkable_inputs()
    ph = list(phrases)
    pq = _pq("l2", M)
    oracle = _decoded_index(pq, _groups_of(offsets))
    for kk, rf in ((k, refine), (16, 8)):
        want = oracle.search_phrases_refined(ph, kk, rf, storage, return_candidates=True)
        got = pq.search_phrases(ph, kk, rf, storage, rerank=False, return_candidates=True)
        assert len(got) == 5
        _assert_equal(got, want, (M, kk, rf))
        _assert_equal(pq.search_phrases(ph, kk, rf, storage, rerank=False), want[:3])
    assert (_np(got[1]) >= 0).sum() == 24 * 16


@pytest.mark.parametrize("metric,storage", COMBOS)
def test_stage_one_equals_dtw16_scan_on_the_materialised_plane(metric, storage):
    from sylber_amd import PQSyllableIndex, SyllableIndex
    x, offsets, phrases, k, refine = R16.checkable_inputs()
    ph = list(phrases)
    pq = _pq(metric)
    for m_k, m_r in ((k, refine), (32, 4)):
        cand, coarse = _dtw16_scan_on_decoded(pq, ph, m_k * m_r, storage, offsets)
        for rerank in (True, False):
            got = pq.search_phrases(ph, m_k, m_r, storage, rerank=rerank, return_candidates=True)
            _assert_equal(got[3:], (cand, coarse), (m_k, m_r, rerank))
    assert (_np(cand)[:, :60] >= 0).all() and (_np(cand)[:, 60:] == -1).all()
    # masked rows and the exclusion go through the same comparison
    xm = x.copy()
    xm[offsets[3] + 2] = np.nan
    xm[offsets[40]:offsets[41]] = np.nan
    grp = _groups_of(offsets) % 7
    pqm = PQSyllableIndex.build(SyllableIndex(xm, metric=metric, groups=grp, device=DEV), 4, codebooks=_codebooks(metric, 4))
    if metric == "cosine":                                   # a NaN row is stored as a zero row under "cosine": mask the same rows by hand
        pqm._bad[torch.from_numpy(np.isnan(xm[:, 0]).nonzero()[0]).to(DEV)] = 1
    assert int(pqm._bad.sum()) == 1 + offsets[41] - offsets[40]
    pgrp = (np.arange(24) % 7).astype(np.int32)
    cand, coarse = _dtw16_scan_on_decoded(pqm, ph, 64, storage, offsets, pgrp)
    got = pqm.search_phrases(ph, 16, 4, storage, groups=pgrp, exclude_same_group=True, sequences=offsets, return_candidates=True)
    _assert_equal(got[3:], (cand, coarse), "masked")
    assert 40 not in _np(cand)


# ---- 3, 4: rows held ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,storage", COMBOS)
def test_rows_held_is_search_phrases_restricted_to_the_candidates(metric, storage):
    x, offsets, phrases, k, refine = R16.checkable_inputs()
    ph = list(phrases)
    pq = _pq(metric)
    S = 60
    full = pq.index.search_phrases(ph, S)
    _assert_equal(pq.search_phrases(ph, 15, 4, storage), pq.index.search_phrases(ph, 15))       # m = 60 >= S: it is search_phrases
    got = pq.search_phrases(ph, k, refine, storage, return_candidates=True)                    # rerank defaults to True: rows are held
    _assert_equal(got, pq.search_phrases(ph, k, refine, storage, rerank=True, return_candidates=True))
    fc, fs, fsp = (_np(t) for t in full)
    c, s, sp, cand, _ = (_np(t) for t in got)
    assert (fs >= 0).all() and (cand >= 0).all()
    for p in range(24):
        keep = np.isin(fs[p], cand[p])                       # the (cost, sequence) ranking of the candidate set
        assert keep.sum() == k * refine
        assert np.array_equal(s[p], fs[p][keep][:k]) and np.array_equal(sp[p], fsp[p][keep][:k])
        assert np.array_equal(c[p].view(np.uint32), fc[p][keep][:k].view(np.uint32))


@functools.lru_cache(maxsize=None)
def _stage1_reference(metric, storage):
    """float64 coarse costs and bounds [24, 60] on the rows decoded from the index's own codes, and what they decide"""
    x, offsets, phrases, k, refine = R16.checkable_inputs()
    pq = _pq(metric)
    C = _codebooks(metric, 4)
    xh = R.decoded(None, C, _np(pq.codes), _np(pq._bad))[0]
    assert np.array_equal(xh, _np(pq.decode(np.arange(len(pq)))))
    qs = [_np(pq._prep(torch.from_numpy(p))) for p in phrases]
    cc, cb = R16.coarse_costs(qs, xh, offsets, storage, metric, bounds=True)
    decided, _, top = R16.checkable(qs, xh, offsets, k, refine, storage, metric, coarse=(cc, cb), exact=(np.zeros_like(cc), None, None))
    return cc, cb, decided, top


@pytest.mark.parametrize("metric,storage", COMBOS)
def test_equals_search_phrases_where_the_bound_decides_it(metric, storage):
    x, offsets, phrases, k, refine = R16.checkable_inputs()
    cc, cb, decided, top = _stage1_reference(metric, storage)
    pq = _pq(metric)
    # the index's codes are the restatement's wherever its bound settles them
    xs = _np(pq.index.features)
    ref_codes, ref_bad = PQ.encode(xs, _codebooks(metric, 4))
    settled = PQ.decided(xs, _codebooks(metric, 4))
    assert settled.mean() > 0.9 and not ref_bad.any() and not _np(pq._bad).any()
    assert (_np(pq.codes) == ref_codes)[settled].all()
    want = [_np(t) for t in pq.index.search_phrases(list(phrases), k)]
    got = [_np(t) for t in pq.search_phrases(list(phrases), k, refine, storage, rerank=True)]
    checked = 0
    for p in range(24):
        if not (decided[p] and np.isin(want[1][p], top[p]).all()):
            continue
        checked += 1
        assert np.array_equal(got[1][p], want[1][p]) and np.array_equal(got[2][p], want[2][p]), p
        assert np.array_equal(got[0][p].view(np.uint32), want[0][p].view(np.uint32)), p
    print("compressed two-stage equals search_phrases on", checked, "of 24 phrases", metric, storage)
    assert checked >= (17 if metric == "l2" else 19)


# ---- 9: stage 1 against the float64 restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,storage", COMBOS)
def test_stage_one_against_the_restatement(metric, storage):
    x, offsets, phrases, k, refine = R16.checkable_inputs()
    cc, cb, decided, top = _stage1_reference(metric, storage)
    cand, coarse = (_np(t) for t in _pq(metric).search_phrases(list(phrases), k, refine, storage, return_candidates=True)[3:])
    m = k * refine
    assert cand.shape == (24, m) and (cand >= 0).all() and np.isfinite(coarse).all()
    worst = 0.0
    for p in range(24):
        err = np.abs(coarse[p].astype(np.float64) - cc[p, cand[p]])
        worst = max(worst, float((err / cb[p, cand[p]]).max()))
        assert (err <= cb[p, cand[p]]).all(), p
        assert len(set(cand[p].tolist())) == m
        c0, c1 = coarse[p, :-1], coarse[p, 1:]
        assert ((c0 < c1) | ((c0 == c1) & (cand[p, :-1] < cand[p, 1:]))).all(), p
        if decided[p]:
            assert set(cand[p].tolist()) == set(top[p].tolist()), p
    print("compressed stage 1", metric, storage, "decided", int(decided.sum()), "of 24; max err / bound", worst)


# ---- 5: invariance -----------------------------------------------------------------------------------------------------------------
def test_invariance_is_bitwise(tmp_path):
    from sylber_amd import PQSyllableIndex, SyllableIndex
    x, offsets, phrases, k, refine = R16.checkable_inputs()
    ph = list(phrases)
    grp = _groups_of(offsets)
    hooks = ({"splits": 1}, {"splits": 2}, {"splits": 5}, {"phrase_chunk": 1}, {"block_phrases": 1}, {"_workspace_fill": 0xFF},
             {"_workspace_fill": 0xFF, "splits": 5, "phrase_chunk": 7, "block_phrases": 3})
    for metric, storage in (("l2", "fp16"), ("cosine", "bf16")):
        pq = _pq(metric)
        for rerank in (False, True):
            base = pq.search_phrases(ph, k, refine, storage, rerank=rerank, return_candidates=True)
            for kw in hooks:
                _assert_equal(pq.search_phrases(ph, k, refine, storage, rerank=rerank, return_candidates=True, **kw), base, (rerank, kw))
        held = pq.search_phrases(ph, k, refine, storage, rerank=True, return_candidates=True)
        base = pq.search_phrases(ph, k, refine, storage, rerank=False, return_candidates=True)
        # one build against a build plus three adds; the lazy state exists before the adds and is extended by them
        cuts = [int(offsets[s]) for s in (0, 20, 31, 47, 60)]
        C = _codebooks(metric, 4)
        grown = PQSyllableIndex.build(SyllableIndex(x[:cuts[1]], metric=metric, groups=grp[:cuts[1]], device=DEV), 4, codebooks=C)
        grown.search_phrases(ph[:2], 1, 1, storage, rerank=False)
        bytes_before = grown.nbytes
        for a, b in zip(cuts[1:-1], cuts[2:]):
            grown.add(x[a:b], groups=grp[a:b])
        assert grown.nbytes > bytes_before and np.array_equal(grown.sequence_offsets(), offsets)
        _assert_equal(grown.search_phrases(ph, k, refine, storage, rerank=False, return_candidates=True), base, "three adds")
        _assert_equal(grown.search_phrases(ph, k, refine, storage, return_candidates=True), held, "three adds, rows held")
        # a save / load round trip, rows held and rows dropped
        path = str(tmp_path / ("pq_%s.npz" % metric))
        pq.save(path)
        back = PQSyllableIndex.load(path, device=DEV)
        _assert_equal(back.search_phrases(ph, k, refine, storage, return_candidates=True), held, "load")
        _assert_equal(back.search_phrases(ph, k, refine, storage, rerank=False, return_candidates=True), base, "load")
        # before and after drop_rows
        n0 = pq.nbytes
        pq.drop_rows()
        assert pq.index is None and pq.nbytes == n0 - 4 * 1337 * 64 and np.array_equal(pq.sequence_offsets(), offsets)
        _assert_equal(pq.search_phrases(ph, k, refine, storage, rerank=False, return_candidates=True), base, "dropped")
        _assert_equal(pq.search_phrases(ph, k, refine, storage, return_candidates=True), base, "dropped, rerank by default False")
        with pytest.raises(ValueError, match="rerank=True"):
            pq.search_phrases(ph, k, refine, storage, rerank=True)
        pq.save(path)
        back = PQSyllableIndex.load(path, device=DEV)
        assert back.index is None
        _assert_equal(back.search_phrases(ph, k, refine, storage, return_candidates=True), base, "load, dropped")
        grown.drop_rows()
        grown.add(x[:7], groups=np.full(7, 99, np.int32))
        assert len(grown.sequence_offsets()) == 62 and len(grown._rnorm if metric == "l2" else grown._codes) == 1337 + 7


def test_lazy_state_counts_in_nbytes():
    pq = _pq("l2", 4)
    n0 = pq.nbytes
    pq.search_phrases([R16.checkable_inputs()[2][0]], 1, 1, "fp16")
    assert pq.nbytes == n0 + 2 * 4 * 256 * 16 + 4 * 1337                  # one 16-bit copy of the codebooks and c [N]
    pq.search_phrases([R16.checkable_inputs()[2][0]], 1, 1, "bf16")
    assert pq.nbytes == n0 + 2 * 2 * 4 * 256 * 16 + 4 * 1337
    pc = _pq("cosine", 4)
    n0 = pc.nbytes
    pc.search_phrases([R16.checkable_inputs()[2][0]], 1, 1, "fp16")
    assert pc.nbytes == n0 + 2 * 4 * 256 * 16                              # no norms under "cosine"


# ---- 6: edges ----------------------------------------------------------------------------------------------------------------------
EDGE_LENS = [127, 1, 128, 129, 300, 7, 64, 33]                # 127 + 1 and + 128 end on 128-row tile edges; 300 crosses two
EDGES = [(48, 3, EDGE_LENS),                                  # D % 32 == 16: the last K step is half empty
         (64, 1, EDGE_LENS),                                  # dsub = 64: a sub-space crosses K steps
         (32, 2, [100, 27]), (32, 2, [100, 28]), (32, 2, [100, 29]), (32, 2, [128, 129]),          # N = 127, 128, 129, 257
         (16, 1, [100, 28])]                                  # D = 16: one K step, half empty; every code byte comes from global memory


@pytest.mark.parametrize("D,M,lens", EDGES)
def test_tile_k_step_and_sub_space_edges(D, M, lens):
    from sylber_amd import PQSyllableIndex
    rng = np.random.default_rng(5)
    offsets = _offsets(lens)
    N, S = int(offsets[-1]), len(lens)
    C = rng.standard_normal((M, 256, D // M)).astype(np.float32)
    x = (PQ.decode(rng.integers(0, 256, (N, M)), C) + 0.3 * rng.standard_normal((N, D))).astype(np.float32)
    grp = _groups_of(offsets)
    spots = ((40, 60), (30, 10), (1, 126), (64, 20), (20, 3), (2, 90), (63, 0)) if N < 300 else \
        ((40, 100), (30, 250), (1, 127), (64, 300), (20, 380), (2, 255), (63, 500))              # 40 + 30 > 64: both halves of block 0
    ph = [(x[a:a + m] + 0.2 * rng.standard_normal((m, D))).astype(np.float32) for m, a in spots]
    assert {len(p) for p in ph} >= {1, 64} and (min(lens) < 64 or N < 300)                       # m_p > L: vertical steps
    for metric in ("l2", "cosine"):
        pq = PQSyllableIndex.build(x, M, codebooks=C, groups=grp, metric=metric, device=DEV)
        oracle = _decoded_index(pq, grp) if metric == "l2" else None
        for storage in R.STORAGES:
            for k, refine in ((S, 1), (1, 2)):
                m = k * refine
                got = pq.search_phrases(ph, k, refine, storage, rerank=False, return_candidates=True)
                _assert_equal(got[3:], _dtw16_scan_on_decoded(pq, ph, m, storage, offsets), (metric, storage, m))
                if oracle is not None:
                    _assert_equal(got, oracle.search_phrases_refined(ph, k, refine, storage, return_candidates=True), (storage, m))
                # cuts fall on sequence starts, here on tile edges too
                _assert_equal(pq.search_phrases(ph, k, refine, storage, rerank=False, return_candidates=True, splits=5), got, "splits")
            _assert_equal(pq.search_phrases(ph, S, 1, storage), pq.index.search_phrases(ph, S), (metric, storage))   # m = S: exact
            one = pq.search_phrases([ph[2]], S, 1, storage, rerank=False, return_candidates=True)                    # a lone 1-row phrase
            assert sorted(_np(one[3])[0].tolist()) == list(range(S))


# ---- 7: admissibility and padding --------------------------------------------------------------------------------------------------
def test_admissibility_and_padding():
    from sylber_amd import PQSyllableIndex
    rng = np.random.default_rng(9)
    D, M = 32, 2
    lens = [5, 9, 130, 4, 7, 3]
    offsets = _offsets(lens)
    N = int(offsets[-1])
    C = rng.standard_normal((M, 256, D // M)).astype(np.float32)
    x = (PQ.decode(rng.integers(0, 256, (N, M)), C) + 0.3 * rng.standard_normal((N, D))).astype(np.float32)
    x[offsets[1] + 4, 20] = np.nan                            # a masked row inside sequence 1: a path avoids it or the cost is +inf
    x[offsets[4]:offsets[5], 3] = np.nan                      # sequence 4 is masked throughout
    grp = np.array([0] * 5 + [1] * 9 + [0] * 130 + [2] * 4 + [3] * 7 + [1] * 3, np.int32)
    phrases = [rng.standard_normal((m, D)).astype(np.float32) for m in (3, 1, 10, 2)]
    phrases[3][1] = np.nan                                    # a NaN phrase row
    pgrp = np.array([0, 1, 2, 0], np.int32)
    a = int(offsets[1])
    for metric, storage in COMBOS:
        pq = PQSyllableIndex.build(x[:a], M, codebooks=C, groups=grp[:a], metric=metric, device=DEV)
        pq.add(x[a:], groups=grp[a:])                         # the masked rows arrive by a NaN in add
        if metric == "cosine":                                # ... under "l2": "cosine" stores a NaN row as a zero row, so mask them by hand
            pq._bad[torch.from_numpy(np.isnan(x).any(1).nonzero()[0]).to(DEV)] = 1
        exact = metric == "l2"                                # whether pq.index sees those rows as the codes do
        assert _np(pq._bad).nonzero()[0].tolist() == [a + 4] + list(range(offsets[4], offsets[5]))
        k, refine = 8, 1                                      # more than the 6 sequences
        for rerank in (True, False):
            got = pq.search_phrases(phrases, k, refine, storage, rerank=rerank, return_candidates=True)
            c, q, sp, cand, co = (_np(t) for t in got)
            assert 4 not in cand and 4 not in q               # +inf under both stages: never a candidate
            if metric == "l2":                                # the NaN phrase: all padding ("cosine" scores it as a zero row)
                assert (cand[3] == -1).all() and np.isinf(co[3]).all()
                assert (q[3] == -1).all() and np.isinf(c[3]).all() and (sp[3] == -1).all()
            assert (cand[0, :5] >= 0).all() and (cand[0, 5:] == -1).all() and np.isinf(co[0, 5:]).all() and np.isfinite(co[0, :5]).all()
            assert (q[0, :5] >= 0).all() and (q[0, 5:] == -1).all() and np.isinf(c[0, 5:]).all() and (sp[0, 5:] == -1).all()
            if rerank and exact:
                _assert_equal(got[:3], pq.index.search_phrases(phrases, k), metric)
            elif metric == "l2":
                want = _decoded_index(pq, grp, nan_masked=True).search_phrases_refined(phrases, k, refine, storage, return_candidates=True)
                _assert_equal(got, want, "masked rows as NaN rows")
            at = np.nonzero(q[0] == 1)[0]                     # the match in sequence 1 stays on one side of its masked row
            assert at.size == 1 and (rerank and not exact or sp[0, at[0], 1] <= a + 4 or sp[0, at[0], 0] > a + 4)
            gx = pq.search_phrases(phrases, k, refine, storage, rerank=rerank, groups=pgrp, exclude_same_group=True, return_candidates=True)
            c, q, sp, cand, co = (_np(t) for t in gx)
            for p, own in ((0, [0, 2]), (1, [1, 5]), (2, [3]), (3, [0, 2])):
                assert not np.isin(cand[p], own).any() and not np.isin(q[p], own).any()
            n_adm = int((cand[0] >= 0).sum())                 # fewer than k admissible sequences: (+inf, -1, (-1, -1))
            assert 0 < n_adm < 5 and (cand[0, n_adm:] == -1).all() and np.isinf(co[0, n_adm:]).all()
            assert (q[0, n_adm:] == -1).all() and np.isinf(c[0, n_adm:]).all() and (sp[0, n_adm:] == -1).all() and (q[0, :n_adm] >= 0).all()
            if rerank and exact:
                _assert_equal(gx[:3], pq.index.search_phrases(phrases, k, groups=pgrp, exclude_same_group=True), metric)
        # all sequences masked
        allbad = PQSyllableIndex.build(np.full((12, D), np.nan, np.float32), M, codebooks=C, groups=np.repeat(np.arange(3), 4), metric=metric,
                                       device=DEV)
        allbad._bad.fill_(1)                                  # already so under "l2"
        for rerank in (True, False):
            c, q, sp, cand, co = (_np(t) for t in allbad.search_phrases(phrases[:2], 2, 2, storage, rerank=rerank, return_candidates=True))
            assert (cand == -1).all() and np.isinf(co).all() and (q == -1).all() and np.isinf(c).all() and (sp == -1).all()
        # P = 0
        for rc in (False, True):
            for rerank in (True, False):
                out = pq.search_phrases([], 4, 3, storage, rerank=rerank, return_candidates=rc)
                assert len(out) == (5 if rc else 3)
                c, s, sp = out[:3]
                assert c.shape == (0, 4) and s.shape == (0, 4) and sp.shape == (0, 4, 2)
                assert c.dtype == torch.float32 and s.dtype == torch.int64 and sp.dtype == torch.int64 and c.device.type == "cuda"
                if rc:
                    assert out[3].shape == (0, 12) and out[3].dtype == torch.int64 and out[4].shape == (0, 12) and out[4].dtype == torch.float32
                    assert out[3].device.type == "cuda" and out[4].device.type == "cuda"


# ---- 8: the storage range and the refusals -----------------------------------------------------------------------------------------
def test_storage_range():
    from sylber_amd import PQSyllableIndex
    rng = np.random.default_rng(12)
    D, M = 32, 2
    offsets = _offsets([6, 40, 9, 12])
    N = int(offsets[-1])
    C = rng.standard_normal((M, 256, D // M)).astype(np.float32)
    x = PQ.decode(rng.integers(0, 255, (N, M)), C).astype(np.float32)       # code 255 is not used: its value never enters a score
    C[1, 255, 3] = 1.0e5
    ph = [x[3:6] + np.float32(0.1), x[20:31] + np.float32(0.1)]
    pq = PQSyllableIndex.build(x, M, codebooks=C, groups=_groups_of(offsets), device=DEV)
    for rerank in (True, False):
        with pytest.raises(ValueError, match="65504"):
            pq.search_phrases(ph, 2, 2, "fp16", rerank=rerank)
    _assert_equal(pq.search_phrases(ph, 2, 2, "bf16"), pq.index.search_phrases(ph, 2))         # m = 4 = S; the index is still usable
    with pytest.raises(ValueError, match="65504"):
        pq.search_phrases(ph, 2, 2, "fp16")
    # a phrase value beyond the range is saturated, not refused
    C[1, 255, 3] = 1.0
    pq = PQSyllableIndex.build(x, M, codebooks=C, groups=_groups_of(offsets), device=DEV)
    ph[1] = ph[1].copy()
    ph[1][4, 2] = 1.0e5
    ph[1][5, 7] = -3.0e5
    for storage in R.STORAGES:
        _assert_equal(pq.search_phrases(ph, 2, 2, storage), pq.index.search_phrases(ph, 2), storage)


def test_every_refusal_comes_before_a_launch(monkeypatch):
    from sylber_amd import PQSyllableIndex, _lib
    rng = np.random.default_rng(10)
    C = rng.standard_normal((1, 256, 16)).astype(np.float32)
    x = rng.standard_normal((40, 16)).astype(np.float32)
    grp = np.repeat(np.arange(4), 10)
    pq = PQSyllableIndex.build(x, 1, codebooks=C, groups=grp, device=DEV)
    dropped = PQSyllableIndex.build(x, 1, codebooks=C, groups=grp, device=DEV)
    dropped.drop_rows()
    far = C.copy()
    far[0, 7, 7] = -1.0e6
    wide = PQSyllableIndex.build(x, 1, codebooks=far, groups=grp, device=DEV)
    big = PQSyllableIndex.build(np.zeros((65537, 16), np.float32), 1, codebooks=C, device=DEV)
    lib = _lib.load()
    launched = []
    spied = ("sylber_dtwpq_scan", "sylber_dtw16_scan", "sylber_dtw_rerank", "sylber_dtw_rerank_codes", "sylber_dtw_search")

    def spy(name):
        real = getattr(lib, name)

        def call(*a):
            launched.append(name)
            return real(*a)
        return call
    spies = {n: spy(n) for n in spied}
    monkeypatch.setattr(_lib, "_LIB", type("L", (), {"__getattr__": lambda self, n: spies[n] if n in spies else getattr(lib, n)})())
    p = [x[:3]]
    bad = [dict(phrases=p, k=0), dict(phrases=p, k=129), dict(phrases=p, k=1.5), dict(phrases=[x[:0]], k=1), dict(phrases=[np.zeros((65, 16), np.float32)], k=1),
           dict(phrases=[np.zeros((3, 32), np.float32)], k=1), dict(phrases=p, k=1, exclude_same_group=True),
           dict(phrases=p, k=1, groups=[0, 1], exclude_same_group=True), dict(phrases=x[:5], k=1), dict(phrases=x[:5], k=1, lengths=[2, 2]),
           dict(phrases=x[:5], k=1, lengths=[5, 0]), dict(phrases=x[:5], k=1, lengths=[[5]]), dict(phrases=x[:5], k=1, lengths=[2.5, 2.5]),
           dict(phrases=p, k=1, sequences=[0, 10, 10, 40]), dict(phrases=p, k=1, sequences=[1, 40]), dict(phrases=p, k=1, sequences=[0, 30]),
           dict(phrases=p, k=1, sequences=[0, 25, 20, 40]), dict(phrases=p, k=1, sequences=[40]), dict(phrases=p, k=1, splits=-1),
           dict(phrases=p, k=1, phrase_chunk=0), dict(phrases=p, k=1, block_phrases=-1),
           # the two-stage call's own limits: they hold in both modes, m = k * refine
           dict(phrases=p, k=1, refine=0), dict(phrases=p, k=1, refine=-2), dict(phrases=p, k=1, refine=1.5), dict(phrases=p, k=1, refine=True),
           dict(phrases=p, k=True), dict(phrases=p, k=33, refine=4), dict(phrases=p, k=128, refine=2), dict(phrases=p, k=1, refine=129),
           dict(phrases=p, k=1, storage="fp32"), dict(phrases=p, k=1, storage="fp8"), dict(phrases=p, k=1, storage=None)]
    for kw in bad:
        for ix, rerank in ((pq, True), (pq, False), (dropped, False)):
            kw2 = dict(kw)
            with pytest.raises(ValueError):
                ix.search_phrases(kw2.pop("phrases"), kw2.pop("k"), rerank=rerank, **kw2)
    with pytest.raises(ValueError, match="rerank=True"):
        dropped.search_phrases(p, 1, rerank=True)
    for ix in (pq, dropped):
        with pytest.raises(TypeError):
            ix.search_phrases(p, 1, scratch_rows=1)          # there is no scratch to bound
    for rerank in (True, False):
        with pytest.raises(ValueError, match="sequences="):
            big.search_phrases(p, 1, rerank=rerank)
        with pytest.raises(ValueError, match="65504"):
            wide.search_phrases(p, 1, 1, "fp16", rerank=rerank)
    pq.index.add(x[:2])                                      # rows added behind the index's back
    with pytest.raises(ValueError, match="pq.add"):
        pq.search_phrases(p, 1)
    assert not launched
    # 65 536 rows in one sequence is legal
    got = big.search_phrases(p, 1, 2, sequences=[0, 65536, 65537], return_candidates=True)
    assert launched == ["sylber_dtwpq_scan", "sylber_dtw_rerank"]
    _assert_equal(got[:3], big.index.search_phrases(p, 1, sequences=[0, 65536, 65537]))
    assert _np(got[3]).tolist() == [[0, 1]]
    launched.clear()
    dropped.search_phrases(p, 2, 2)                          # the exact DTW straight from the codes
    assert launched == ["sylber_dtwpq_scan", "sylber_dtw_rerank_codes"]
    launched.clear()
    assert len(dropped.search_phrases([], 4, 3)) == 3 and not launched


def test_the_entry_refuses_by_itself():
    """every bad argument returns 1 with ``sylber_last_error`` naming the entry: no device call is made for them"""
    from sylber_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    ptr = ctypes.c_void_p(buf.data_ptr())
    names = ("q16", "n_blocks", "row_meta", "slot_phrase", "block_rows", "n_phrases", "block_phrases", "codes", "bad", "codebooks16", "N", "D",
             "M", "recon_norm", "q_norm", "metric", "storage", "m", "seq_id", "cut_rows", "cuts", "phrase_group", "seq_group", "cand", "coarse",
             "workspace", "stream")
    good = dict.fromkeys(names, ptr)
    good.update(n_blocks=1, n_phrases=1, block_phrases=1, N=8, D=64, M=4, metric=0, storage=0, m=4, cuts=1, phrase_group=None, seq_group=None,
                stream=None)
    assert len(names) == len(_lib.EXPORTS["sylber_dtwpq_scan"][1])
    cases = [dict(q16=None), dict(codes=None), dict(codebooks16=None), dict(cand=None), dict(coarse=None), dict(workspace=None),
             dict(seq_id=None), dict(cut_rows=None), dict(n_blocks=0), dict(n_phrases=0), dict(N=0), dict(D=0), dict(D=24, M=1),
             dict(M=0), dict(M=65, D=65 * 16), dict(M=3), dict(M=8), dict(D=96, M=4), dict(m=0), dict(m=129), dict(block_phrases=0),
             dict(block_phrases=129), dict(m=128, block_phrases=33), dict(cuts=0), dict(cuts=65536), dict(metric=2), dict(storage=2),
             dict(recon_norm=None), dict(q_norm=None), dict(phrase_group=ptr), dict(seq_group=ptr), dict(n_phrases=1 << 20, cuts=65535, m=128)]
    for kw in cases:
        a = dict(good)
        a.update(kw)
        assert lib.sylber_dtwpq_scan(*[a[n] for n in names]) == 1, kw
        assert "sylber_dtwpq_scan" in lib.sylber_last_error().decode(), kw
    ip = dict(good, metric=1, recon_norm=None, q_norm=None, bad=None, n_blocks=0)      # the norms and the mask may be null under IP
    assert lib.sylber_dtwpq_scan(*[ip[n] for n in names]) == 1 and "n_blocks" in lib.sylber_last_error().decode()
    torch.cuda.synchronize()

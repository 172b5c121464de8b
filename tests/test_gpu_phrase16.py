"""GPU tier, two-stage phrase search (csrc/dtw16.hip behind ``SyllableIndex.search_phrases_refined``).

* with every sequence a candidate the result is ``search_phrases`` bit for bit (both metrics, both storages; tile and chunk edges,
  vertical steps, both 64-row halves of a block, a lone 1-row phrase; NaN rows; saturated phrase values);
* stage 1 against tests/dtw16_ref.py: every coarse cost within ``coarse_cost_error_bound`` of its float64 value, the candidate set
  equal to the float64 top-m wherever the bound decides it, the stage-1 order;
* the result equals ``search_phrases`` for every decided phrase whose exact top-k lies inside that top-m;
* ``cand``, ``coarse``, costs, seqs and spans are bitwise invariant under the split / chunk / packing hooks, stale workspace contents
  and how the index was built;
* admissibility and padding, the fp16 range, the refusals and ``P = 0``."""
import functools

import numpy as np
import pytest
import torch

import dtw16_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COMBOS = [(m, s) for m in ("l2", "cosine") for s in R.STORAGES]


def _np(t):
    return t.cpu().numpy()


def _groups_of(offsets):
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets)).astype(np.int32)


def _assert_equal(got, want, what=""):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        if a.dtype == torch.float32:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what
        else:
            assert torch.equal(a, b), what


@functools.lru_cache(maxsize=None)
def _index(metric):
    from sylber_amd import SyllableIndex
    x, offsets, phrases, k, refine = R.checkable_inputs()
    return SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)


@functools.lru_cache(maxsize=None)
def _stage1_reference(metric, storage):
    """float64 coarse costs and bounds [24, 60] from the rows as the index holds them, and ``checkable`` on them"""
    x, offsets, phrases, k, refine = R.checkable_inputs()
    idx = _index(metric)
    if metric == "l2":                                       # the index holds the fp32 rows as given: the CPU tier's reference serves
        cc, cb, _ = R.checkable_reference(storage, metric)
        qs, xs = R.stored(phrases, x, metric)
    else:
        xs = _np(idx.features)
        qs = [_np(idx._prep(torch.from_numpy(p))) for p in phrases]
        cc, cb = R.coarse_costs(qs, xs, offsets, storage, metric, bounds=True)
    # the exact top-k comes from the library in the test; here only what the coarse costs decide
    exact = (np.zeros_like(cc), None, None)
    decided, _, top = R.checkable(qs, xs, offsets, k, refine, storage, metric, coarse=(cc, cb), exact=exact)
    return cc, cb, decided, top


@pytest.mark.parametrize("metric,storage", COMBOS)
def test_equals_search_phrases_when_every_sequence_is_a_candidate(metric, storage):
    x, offsets, phrases, _, _ = R.checkable_inputs()
    S, N = len(offsets) - 1, x.shape[0]
    assert (S, N) == (60, 1337)
    rng = np.random.default_rng(1)
    lens = np.diff(offsets)
    assert lens.min() == 5                                   # the 64-row phrase meets a 5-row sequence: vertical steps
    more = [(x[a:a + m] + 0.3 * rng.standard_normal((m, 64))).astype(np.float32) for m, a in ((33, 100), (64, 700))]
    s5 = int(np.argmin(lens))
    more.append(np.repeat(x[offsets[s5]:offsets[s5 + 1]], 13, 0)[:64] + np.float32(0.1))
    ph = list(phrases) + more
    idx = _index(metric)
    k, refine = 16, 8                                        # m = 128 >= S
    want = idx.search_phrases(ph, k)
    got = idx.search_phrases_refined(ph, k, refine, storage, return_candidates=True)
    _assert_equal(got[:3], want)
    cand, coarse = _np(got[3]), _np(got[4])
    assert got[3].dtype == torch.int64 and got[4].dtype == torch.float32 and cand.shape == coarse.shape == (len(ph), 128)
    assert (np.sort(cand[:, :S], 1) == np.arange(S)).all() and (cand[:, S:] == -1).all()
    assert np.isfinite(coarse[:, :S]).all() and np.isinf(coarse[:, S:]).all()
    assert _np(want[1])[-1, 0] == s5                         # the stretched copy of the 5-row sequence finds it
    _assert_equal(idx.search_phrases_refined(ph, k, refine, storage), want)


@pytest.mark.parametrize("metric,storage", COMBOS)
def test_stage_one_against_the_restatement(metric, storage):
    x, offsets, phrases, k, refine = R.checkable_inputs()
    cc, cb, decided, top = _stage1_reference(metric, storage)
    idx = _index(metric)
    cand, coarse = (_np(t) for t in idx.search_phrases_refined(list(phrases), k, refine, storage, return_candidates=True)[3:])
    m = k * refine
    assert cand.shape == (24, m) and (cand >= 0).all() and np.isfinite(coarse).all()
    worst = 0.0
    for p in range(24):
        err = np.abs(coarse[p].astype(np.float64) - cc[p, cand[p]])
        worst = max(worst, float((err / cb[p, cand[p]]).max()))
        assert (err <= cb[p, cand[p]]).all(), p
        assert len(set(cand[p].tolist())) == m
        c0, c1 = coarse[p, :-1], coarse[p, 1:]
        assert ((c0 < c1) | ((c0 == c1) & (cand[p, :-1] < cand[p, 1:]))).all(), p      # ordered by the returned (coarse, sequence)
        if decided[p]:
            assert set(cand[p].tolist()) == set(top[p].tolist()), p
    print("stage 1", metric, storage, "decided", int(decided.sum()), "of 24; max err / bound", worst)
    assert decided.sum() >= 22


@pytest.mark.parametrize("metric,storage", COMBOS)
def test_equals_search_phrases_where_the_bound_decides_it(metric, storage):
    x, offsets, phrases, k, refine = R.checkable_inputs()
    cc, cb, decided, top = _stage1_reference(metric, storage)
    idx = _index(metric)
    want = [_np(t) for t in idx.search_phrases(list(phrases), k)]
    got = [_np(t) for t in idx.search_phrases_refined(list(phrases), k, refine, storage)]
    checked = 0
    for p in range(24):
        if not (decided[p] and np.isin(want[1][p], top[p]).all()):
            continue
        checked += 1
        assert np.array_equal(got[1][p], want[1][p]) and np.array_equal(got[2][p], want[2][p]), p
        assert np.array_equal(got[0][p].view(np.uint32), want[0][p].view(np.uint32)), p
    print("two-stage equals search_phrases on", checked, "of 24 phrases", metric, storage)
    assert checked >= 22


def test_invariance_is_bitwise():
    from sylber_amd import SyllableIndex
    x, offsets, phrases, k, refine = R.checkable_inputs()
    ph = list(phrases)
    grp = _groups_of(offsets)
    for metric, storage in (("l2", "fp16"), ("cosine", "bf16")):
        idx = _index(metric)
        base = idx.search_phrases_refined(ph, k, refine, storage, return_candidates=True)
        for kw in ({"splits": 1}, {"splits": 2}, {"splits": 5}, {"phrase_chunk": 1}, {"phrase_chunk": 7}, {"block_phrases": 1},
                   {"block_phrases": 3}, {"_workspace_fill": 0xFF}, {"_workspace_fill": 0xFF, "splits": 5, "phrase_chunk": 7, "block_phrases": 3}):
            _assert_equal(idx.search_phrases_refined(ph, k, refine, storage, return_candidates=True, **kw), base, str(kw))
        two = SyllableIndex(x[:offsets[31]], metric=metric, groups=grp[:offsets[31]], device=DEV)      # one add against two
        two.half_rows(storage)                               # the plane exists before the second add and is extended by it
        two.add(x[offsets[31]:], groups=grp[offsets[31]:])
        _assert_equal(two.search_phrases_refined(ph, k, refine, storage, return_candidates=True), base, "two adds")


def _check_tile_edges(metric, storage, D, lens, spots):
    """m >= S: the two-stage call returns search_phrases' results; a lone 1-row phrase's candidates are every sequence"""
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(5)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N, S = int(offsets[-1]), len(lens)
    x = rng.standard_normal((N, D)).astype(np.float32)
    idx = SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)
    ph = [(x[a:a + m] + 0.2 * rng.standard_normal((m, D))).astype(np.float32) for m, a in spots]
    what = "D = %d, N = %d" % (D, N)
    for k, refine in ((S, 1), (2, 4)):                       # m = 8 >= S
        _assert_equal(idx.search_phrases_refined(ph, k, refine, storage), idx.search_phrases(ph, k), what)
    one = [ph[2]]                                            # a lone 1-row phrase
    got = idx.search_phrases_refined(one, S, 1, storage, return_candidates=True)
    _assert_equal(got[:3], idx.search_phrases(one, S), what)
    assert sorted(_np(got[3])[0].tolist()) == list(range(S)), what


@pytest.mark.parametrize("metric,storage", COMBOS)
def test_tile_and_chunk_edges(metric, storage):
    from sylber_amd.search import RERANK_CHUNK
    lens = [127, 1, 128, 129, 300, 7, 64, 33]                # 127 + 1 and + 128 end on 128-row tile edges
    offsets = np.cumsum(lens)
    assert offsets[1] == 128 and offsets[2] == 256 and max(lens) > RERANK_CHUNK and RERANK_CHUNK + 1 in lens
    _check_tile_edges(metric, storage, 32, lens,
                      ((40, 100), (30, 250), (1, 127), (64, 300), (20, 380), (2, 255), (63, 500)))     # 40 + 30 > 64: both halves of block 0
    # D = 16: one K step whose upper half is zero-filled; D = 48: the last of two is.  N = 127, 128, 129: a tile short of one row,
    # full, and a second tile of one row
    for D in (16, 48):
        for last in (27, 28, 29):
            _check_tile_edges(metric, storage, D, [100, last], ((40, 60), (30, 10), (1, 126), (64, 20), (20, 3), (2, 90), (63, 0)))


def test_admissibility_and_padding():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(9)
    D = 16
    lens = [5, 9, 130, 4, 7, 3]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(offsets[-1])
    x = rng.standard_normal((N, D)).astype(np.float32)
    x[offsets[1] + 4] = np.nan                                # a NaN row inside sequence 1: a path avoids it or the cost is +inf
    x[offsets[4]:offsets[5]] = np.nan                         # sequence 4 is NaN throughout
    grp = np.array([0] * 5 + [1] * 9 + [0] * 130 + [2] * 4 + [3] * 7 + [1] * 3, np.int32)
    phrases = [rng.standard_normal((m, D)).astype(np.float32) for m in (3, 1, 10, 2)]
    phrases[3][1] = np.nan                                    # a NaN phrase row
    pgrp = np.array([0, 1, 2, 0], np.int32)
    for metric, storage in COMBOS:
        idx = SyllableIndex(x, metric=metric, groups=grp, device=DEV)
        k, refine = 8, 1                                      # more than the 6 sequences
        want = idx.search_phrases(phrases, k)
        got = idx.search_phrases_refined(phrases, k, refine, storage, return_candidates=True)
        _assert_equal(got[:3], want, metric)
        c, q, sp, cand, co = (_np(t) for t in got)
        if metric == "l2":
            assert 4 not in cand and 4 not in q               # +inf under both stages: never a candidate
            assert (cand[3] == -1).all() and np.isinf(co[3]).all()                 # the NaN phrase: all padding
            assert (q[3] == -1).all() and np.isinf(c[3]).all() and (sp[3] == -1).all()
            assert (cand[0, :5] >= 0).all() and (cand[0, 5:] == -1).all() and np.isinf(co[0, 5:]).all() and np.isfinite(co[0, :5]).all()
        want = idx.search_phrases(phrases, k, groups=pgrp, exclude_same_group=True)
        got = idx.search_phrases_refined(phrases, k, refine, storage, groups=pgrp, exclude_same_group=True, return_candidates=True)
        _assert_equal(got[:3], want, metric)
        c, q, sp, cand, co = (_np(t) for t in got)
        for p, own in ((0, [0, 2]), (1, [1, 5]), (2, [3]), (3, [0, 2])):
            assert not np.isin(cand[p], own).any() and not np.isin(q[p], own).any()
        # fewer than k admissible sequences: (+inf, -1, (-1, -1)); cand ends in -1 and coarse in +inf
        n_adm = int((cand[0] >= 0).sum())
        assert 0 < n_adm < k and (cand[0, n_adm:] == -1).all() and np.isinf(co[0, n_adm:]).all()
        assert (q[0, n_adm:] == -1).all() and np.isinf(c[0, n_adm:]).all() and (sp[0, n_adm:] == -1).all() and (q[0, :n_adm] >= 0).all()
        # a smaller candidate list is still a restriction of search_phrases: every returned triple is one of its triples
        full = [_np(t) for t in idx.search_phrases(phrases, 6)]
        c, q, sp = (_np(t) for t in idx.search_phrases_refined(phrases, 2, 1, storage))
        for p in range(len(phrases)):
            for e in range(2):
                if q[p, e] < 0:
                    continue
                at = np.nonzero(full[1][p] == q[p, e])[0]
                assert at.size == 1 and c[p, e] == full[0][p, at[0]] and np.array_equal(sp[p, e], full[2][p, at[0]])


def test_storage_range():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(12)
    D = 16
    lens = [6, 40, 9, 12]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = rng.standard_normal((int(offsets[-1]), D)).astype(np.float32)
    ph = [x[3:6] + np.float32(0.1), x[20:31] + np.float32(0.1)]
    big = x.copy()
    big[10, 3] = 70000.0
    idx = SyllableIndex(big, groups=_groups_of(offsets), device=DEV)
    with pytest.raises(ValueError, match="65504"):
        idx.search_phrases_refined(ph, 2, 2, "fp16")
    want = idx.search_phrases(ph, 2)                          # the index is still usable
    _assert_equal(idx.search_phrases_refined(ph, 2, 2, "bf16"), want)
    with pytest.raises(ValueError, match="65504"):
        idx.search_phrases_refined(ph, 2, 2, "fp16")
    # a phrase value beyond the range is saturated, not refused
    idx = SyllableIndex(x, groups=_groups_of(offsets), device=DEV)
    ph[1] = ph[1].copy()
    ph[1][4, 2] = 1.0e5
    ph[1][5, 7] = -3.0e5
    for storage in R.STORAGES:
        _assert_equal(idx.search_phrases_refined(ph, 2, 2, storage), idx.search_phrases(ph, 2), storage)


def test_every_refusal_comes_before_a_launch_and_no_phrases(monkeypatch):
    from sylber_amd import SyllableIndex, _lib
    rng = np.random.default_rng(10)
    x = rng.standard_normal((40, 16)).astype(np.float32)
    idx = SyllableIndex(x, groups=np.repeat(np.arange(4), 10), device=DEV)
    lib = _lib.load()
    launched = []
    spied = ("sylber_dtw16_scan", "sylber_dtw_rerank", "sylber_dtw_search")

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
           # the two-stage call's own limits
           dict(phrases=p, k=1, refine=0), dict(phrases=p, k=1, refine=-2), dict(phrases=p, k=1, refine=1.5), dict(phrases=p, k=1, refine=True),
           dict(phrases=p, k=True), dict(phrases=p, k=33, refine=4), dict(phrases=p, k=128, refine=2), dict(phrases=p, k=1, refine=129),
           dict(phrases=p, k=1, storage="fp32"), dict(phrases=p, k=1, storage="fp8"), dict(phrases=p, k=1, storage=None)]
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(ValueError):
            idx.search_phrases_refined(kw.pop("phrases"), kw.pop("k"), **kw)
    with pytest.raises(ValueError):
        SyllableIndex(device=DEV).search_phrases_refined(p, 1)
    big = SyllableIndex(np.zeros((65537, 16), np.float32), device=DEV)
    with pytest.raises(ValueError, match="sequences="):
        big.search_phrases_refined(p, 1)
    far = x.copy()
    far[7, 7] = -1.0e6
    with pytest.raises(ValueError, match="65504"):
        SyllableIndex(far, groups=np.repeat(np.arange(4), 10), device=DEV).search_phrases_refined(p, 1, 1, "fp16")
    assert not launched
    # 65 536 rows in one sequence is legal: only the chunk loop depends on the length
    got = big.search_phrases_refined(p, 1, 2, sequences=[0, 65536, 65537], return_candidates=True)
    assert launched == ["sylber_dtw16_scan", "sylber_dtw_rerank"]
    _assert_equal(got[:3], big.search_phrases(p, 1, sequences=[0, 65536, 65537]))
    assert _np(got[3]).tolist() == [[0, 1]]
    launched.clear()
    for rc in (False, True):
        out = idx.search_phrases_refined([], 4, 3, return_candidates=rc)
        assert len(out) == (5 if rc else 3)
        c, s, sp = out[:3]
        assert c.shape == (0, 4) and s.shape == (0, 4) and sp.shape == (0, 4, 2)
        assert c.dtype == torch.float32 and s.dtype == torch.int64 and sp.dtype == torch.int64 and c.device.type == "cuda"
        if rc:
            assert out[3].shape == (0, 12) and out[3].dtype == torch.int64 and out[4].shape == (0, 12) and out[4].dtype == torch.float32
            assert out[3].device.type == "cuda" and out[4].device.type == "cuda"
    assert not launched

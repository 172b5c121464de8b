"""GPU tier, every occurrence of a phrase (csrc/dtw.hip and csrc/dtw16.hip behind ``SyllableIndex.search_occurrences`` /
``search_occurrences_refined``), bitwise against tests/occ_ref.py: the local costs are taken from the library itself
(``SyllableIndex.search`` on pieces of at most 128 rows, as tests/test_gpu_phrase.py takes them), the fp32 recurrence and the
one-pass rule of occ_ref run over them, and the calls must return exactly those costs, sequences, spans and that order."""
import numpy as np
import pytest
import torch

import occ_ref as O
from test_gpu_phrase import _corpus, _groups_of, _local_costs, _np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _reference(x, offsets, phrases, metric, k, phrase_groups=None, seq_groups=None, only=None):
    rows = np.concatenate(phrases)
    d = _local_costs(x, offsets, rows, metric)
    r0 = np.concatenate([[0], np.cumsum([len(p) for p in phrases])])
    return O.search_occurrences(lambda p, s: d[r0[p]:r0[p + 1], offsets[s]:offsets[s + 1]], len(phrases), offsets, k, np.float32,
                                phrase_groups, seq_groups, only)


def _assert_same(got, ref, k=None):
    c, q, sp = (_np(t) for t in got[:3])
    rc, rq, rsp = (r[:, :k] for r in ref[:3])
    assert np.array_equal(sp, rsp)
    assert np.array_equal(q, rq)
    assert np.array_equal(c.view(np.uint32), rc.astype(np.float32).view(np.uint32))


def _equal(a, b, what=None):
    for s, t in zip(a, b):
        assert torch.equal(s, t), what


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,integer", [(16, True), (16, False), (768, False)])
def test_bitwise_against_the_contract(D, integer, metric):
    from sylber_amd import SyllableIndex
    x, offsets, phrases = _corpus(D, integer, D + integer)
    idx = SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)
    ref = _reference(x, offsets, phrases, metric, 128)
    assert (ref[3] > len(offsets) - 1).any()                  # more occurrences than sequences: more than one per sequence is in play
    _assert_same(idx.search_occurrences(phrases, 128), ref)
    _assert_same(idx.search_occurrences(phrases, 5), ref, 5)
    _assert_same(idx.search_occurrences(phrases, 5, splits=len(x)), ref, 5)      # a cut at every sequence start


def test_a_phrase_planted_three_times_in_one_sequence():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(21)
    D, m = 32, 7
    offsets = np.array([0, 50, 750, 780], np.int64)
    x = rng.standard_normal((780, D)).astype(np.float32)
    phrase = rng.standard_normal((m, D)).astype(np.float32)
    planted = [125, 300, 640]                                 # rows 125 .. 131 straddle the edge of the first 128-row tile
    for a in planted:
        x[a:a + m] = phrase
    want = sorted((a, a + m) for a in planted)
    ref = _reference(x, offsets, [phrase], "l2", 10)
    assert sorted(map(tuple, ref[2][0, :3].tolist())) == want and (ref[1][0, :3] == 1).all()       # on the reference first
    assert ref[0][0, 3] > 100 * max(ref[0][0, 2], 1e-6)       # and nothing else comes near
    idx = SyllableIndex(x, metric="l2", groups=_groups_of(offsets), device=DEV)
    for splits in (1, 0):
        got = idx.search_occurrences([phrase], 10, splits=splits)
        _assert_same(got, ref)
        assert sorted(map(tuple, _np(got[2])[0, :3].tolist())) == want and (_np(got[1])[0, :3] == 1).all()
    assert (_np(idx.search_phrases([phrase], 3)[1])[0] == 1).sum() == 1      # where search_phrases has one entry for the sequence


def _small_corpus(seed, D=16, integer=False):
    rng = np.random.default_rng(seed)
    lens = [9, 1, 20, 3, 14, 2, 17, 6, 11, 12]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(offsets[-1])
    x = rng.integers(-2, 3, (N, D)).astype(np.float32) if integer else rng.standard_normal((N, D)).astype(np.float32)
    phrases = []
    for mm in (1, 3, 8, 20):
        a = int(rng.integers(0, N - mm))
        phrases.append(x[a:a + mm].copy() if integer else x[a:a + mm] + 0.3 * rng.standard_normal((mm, D)).astype(np.float32))
    return x, offsets, phrases


@pytest.mark.parametrize("metric,integer", [("l2", True), ("cosine", False)])
def test_consequence_a_the_first_entry_of_each_sequence_is_search_phrases(metric, integer):
    from sylber_amd import SyllableIndex
    x, offsets, phrases = _small_corpus(5, integer=integer)
    S = len(offsets) - 1
    ref = _reference(x, offsets, phrases, metric, 128)
    assert (ref[3] <= 128).all() and (ref[3] > S).any()       # nothing is cut off at k = 128
    idx = SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)
    got = idx.search_occurrences(phrases, 128)
    _assert_same(got, ref)
    c, q, sp = (_np(t) for t in got)
    pc, pq, psp = (_np(t) for t in idx.search_phrases(phrases, S))
    for p in range(len(phrases)):
        live = np.nonzero(q[p] >= 0)[0]
        first = live[np.unique(q[p, live], return_index=True)[1]]
        first.sort()                                          # each sequence's first entry, in list order
        n = int((pq[p] >= 0).sum())
        assert n == first.size
        assert np.array_equal(q[p, first], pq[p, :n]) and np.array_equal(sp[p, first], psp[p, :n])
        assert np.array_equal(c[p, first].view(np.uint32), pc[p, :n].view(np.uint32))


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_consequence_b_one_row_phrases_are_search(metric):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3000, 32)).astype(np.float32)
    grp = np.sort(rng.integers(0, 90, 3000)).astype(np.int32)
    idx = SyllableIndex(x, metric=metric, groups=grp, device=DEV)
    q = rng.standard_normal((150, 32)).astype(np.float32)
    k = 9
    c, s, sp = idx.search_occurrences(q, k, lengths=[1] * 150)
    sc, ids = idx.search(q, k)
    want = sc if metric == "l2" else torch.clamp(1.0 - sc, min=0.0)
    assert torch.equal(sp[:, :, 0], ids) and torch.equal(sp[:, :, 1], ids + 1)
    assert torch.equal(c, want)
    off = idx.sequence_offsets()
    assert np.array_equal(_np(s), np.searchsorted(off, _np(ids), side="right") - 1)
    pq = torch.from_numpy(grp[::20].copy())                   # with the exclusion: search's own
    c, s, sp = idx.search_occurrences(q, k, lengths=[1] * 150, groups=pq, exclude_same_group=True)
    sc, ids = idx.search(q, k, groups=pq, exclude_same_group=True)
    assert torch.equal(sp[:, :, 0], ids) and torch.equal(c, sc if metric == "l2" else torch.clamp(1.0 - sc, min=0.0))


def test_invariance_is_bitwise():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(8)
    D = 32
    lens = rng.integers(1, 300, 40)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N, grp = int(offsets[-1]), _groups_of(offsets)
    x = np.round(rng.standard_normal((N, D)) * 2).astype(np.float32) / 2
    phrases = [x[a:a + m] + np.float32(0.5) * rng.integers(-1, 2, (m, D)).astype(np.float32)
               for m, a in zip(rng.integers(1, 65, 40), rng.integers(0, N - 64, 40))]
    idx = SyllableIndex(x, metric="l2", groups=grp, device=DEV)
    k = 12
    base = idx.search_occurrences(phrases, k)
    for kw in ({"splits": 1}, {"splits": 2}, {"splits": 3}, {"splits": N}, {"phrase_chunk": 1}, {"phrase_chunk": 7}, {"block_phrases": 1},
               {"block_phrases": 5, "splits": 4, "phrase_chunk": 33}, {"_workspace_fill": 0xFF}, {"_workspace_fill": 0xFF, "splits": 9}):
        _equal(base, idx.search_occurrences(phrases, k, **kw), kw)
    for p in (0, 13, 39):                                     # alone against in a batch of others
        _equal([t[p:p + 1] for t in base], idx.search_occurrences([phrases[p]], k))
    many = SyllableIndex(metric="l2", device=DEV)             # one add against many
    for s in range(len(lens)):
        many.add(x[offsets[s]:offsets[s + 1]], groups=grp[offsets[s]:offsets[s + 1]])
    _equal(base, many.search_occurrences(phrases, k))
    _assert_same([t[:4] for t in base], _reference(x, offsets, phrases[:4], "l2", k))
    # the refined call, whose stage 2 is another kernel: the same answer when the candidates cover every sequence, under its hooks too
    k, refine = 3, 40
    base = idx.search_occurrences(phrases, k)
    for kw in ({}, {"splits": 3}, {"phrase_chunk": 7, "block_phrases": 2}, {"_workspace_fill": 0xFF}, {"storage": "bf16"}):
        _equal(base, idx.search_occurrences_refined(phrases, k, refine, **kw), kw)


def test_exclusion_nan_rows_and_lists_shorter_than_k():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(9)
    D = 16
    lens = [5, 9, 130, 4, 7, 3]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(offsets[-1])
    x = rng.standard_normal((N, D)).astype(np.float32)
    x[offsets[1] + 4] = np.nan                                # a NaN row inside sequence 1: a hole in every E
    x[offsets[2] + 60:offsets[2] + 63] = np.nan               # and a run of them inside the long one
    x[offsets[4]:offsets[5]] = np.nan                         # sequence 4 is NaN throughout: never returned
    grp = np.array([0] * 5 + [1] * 9 + [0] * 130 + [2] * 4 + [3] * 7 + [1] * 3, np.int32)
    phrases = [rng.standard_normal((m, D)).astype(np.float32) for m in (3, 1, 10, 2)]
    phrases[3][1] = np.nan                                    # a NaN phrase row: no occurrence anywhere
    pgrp = np.array([0, 1, 2, 0], np.int32)
    sgrp = grp[offsets[:-1]]
    idx = SyllableIndex(x, metric="l2", groups=grp, device=DEV)
    k = 128
    ref = _reference(x, offsets, phrases, "l2", k)
    got = idx.search_occurrences(phrases, k)
    _assert_same(got, ref)
    c, q, sp = (_np(t) for t in got)
    assert (q[3] == -1).all() and np.isinf(c[3]).all() and (sp[3] == -1).all()
    assert 4 not in q and (q[:3, 0] >= 0).all() and (q[[0, 2, 3], -1] == -1).all()       # lists shorter than k
    assert (q[1] >= 0).all() and N - 11 > k                   # the one-row phrase: every row that is not NaN is an occurrence
    short = SyllableIndex(x[:14], metric="l2", groups=grp[:14], device=DEV).search_occurrences(phrases[1:2], 128)
    assert sorted(_np(short[2])[0, :, 0].tolist()) == [-1] * (128 - 13) + [j for j in range(14) if j != 9]      # ... each of them once
    ref = _reference(x, offsets, phrases, "l2", k, pgrp, sgrp)
    got = idx.search_occurrences(phrases, k, groups=pgrp, exclude_same_group=True)
    _assert_same(got, ref)
    q = _np(got[1])
    assert not np.isin(q[0], [0, 2]).any() and not np.isin(q[1], [1, 5]).any() and not np.isin(q[2], [3]).any()
    idc = SyllableIndex(x, metric="cosine", groups=grp, device=DEV)
    _assert_same(idc.search_occurrences(phrases, 6, groups=pgrp, exclude_same_group=True),
                 _reference(x, offsets, phrases, "cosine", 6, pgrp, sgrp))


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_refined_is_the_reference_restricted_to_its_candidates(metric):
    from sylber_amd import SyllableIndex
    x, offsets, phrases = _corpus(16, False, 3)
    S = len(offsets) - 1
    grp = _groups_of(offsets)
    idx = SyllableIndex(x, metric=metric, groups=grp, device=DEV)
    # k * refine covers every sequence: search_occurrences itself
    _equal(idx.search_occurrences(phrases, 8), idx.search_occurrences_refined(phrases, 8, 3))
    _equal(idx.search_occurrences(phrases, 128), idx.search_occurrences_refined(phrases, 128, 1))
    # fewer candidates than sequences: the reference restricted to cand, which is search_phrases_refined's
    k, refine = 3, 2
    c, q, sp, cand, coarse = idx.search_occurrences_refined(phrases, k, refine, return_candidates=True)
    want = idx.search_phrases_refined(phrases, k, refine, return_candidates=True)
    assert torch.equal(cand, want[3]) and torch.equal(coarse, want[4])
    assert cand.shape == (len(phrases), k * refine) and k * refine < S
    _assert_same((c, q, sp), _reference(x, offsets, phrases, metric, k, only=_np(cand)))
    pg = np.array([0, 3, 9, 11, 20, 11, 9], np.int32)         # with the exclusion, which stage 1 applies
    c, q, sp, cand, _ = idx.search_occurrences_refined(phrases, 5, 2, groups=pg, exclude_same_group=True, return_candidates=True)
    assert not (_np(cand) == pg[:, None]).any()
    _assert_same((c, q, sp), _reference(x, offsets, phrases, metric, 5, pg, grp[offsets[:-1]], only=_np(cand)))


def test_every_refusal_comes_before_a_launch(monkeypatch):
    from sylber_amd import SyllableIndex, _lib
    rng = np.random.default_rng(10)
    x = rng.standard_normal((40, 16)).astype(np.float32)
    idx = SyllableIndex(x, groups=np.repeat(np.arange(4), 10), device=DEV)
    lib = _lib.load()
    entries = ("sylber_dtw_occurrences", "sylber_dtw_rerank_occurrences", "sylber_dtw16_scan")

    def fail(*a):
        raise AssertionError("launched")
    monkeypatch.setattr(_lib, "_LIB", type("L", (), {"__getattr__": lambda self, n: fail if n in entries else getattr(lib, n)})())
    p = [x[:3]]
    bad = [dict(phrases=p, k=0), dict(phrases=p, k=129), dict(phrases=p, k=1.5), dict(phrases=[x[:0]], k=1), dict(phrases=[np.zeros((65, 16), np.float32)], k=1),
           dict(phrases=[np.zeros((3, 32), np.float32)], k=1), dict(phrases=p, k=1, exclude_same_group=True),
           dict(phrases=p, k=1, groups=[0, 1], exclude_same_group=True), dict(phrases=x[:5], k=1), dict(phrases=x[:5], k=1, lengths=[2, 2]),
           dict(phrases=x[:5], k=1, lengths=[5, 0]), dict(phrases=x[:5], k=1, lengths=[[5]]), dict(phrases=x[:5], k=1, lengths=[2.5, 2.5]),
           dict(phrases=p, k=1, sequences=[0, 10, 10, 40]), dict(phrases=p, k=1, sequences=[1, 40]), dict(phrases=p, k=1, sequences=[0, 30]),
           dict(phrases=p, k=1, sequences=[0, 25, 20, 40]), dict(phrases=p, k=1, sequences=[40]), dict(phrases=p, k=1, splits=-1),
           dict(phrases=p, k=1, phrase_chunk=0)]
    for call in (idx.search_occurrences, idx.search_occurrences_refined):
        for kw in bad:
            kw = dict(kw)
            with pytest.raises(ValueError):
                call(kw.pop("phrases"), kw.pop("k"), **kw)
    for kw in (dict(k=33, refine=4), dict(k=2, refine=0), dict(k=2, refine=1.5), dict(k=2, storage="fp8")):
        with pytest.raises(ValueError):
            idx.search_occurrences_refined(p, **kw)
    for name in ("search_occurrences", "search_occurrences_refined"):
        with pytest.raises(ValueError):
            getattr(SyllableIndex(device=DEV), name)(p, 1)
    big = SyllableIndex(np.zeros((65537, 16), np.float32), device=DEV)
    with pytest.raises(ValueError, match="sequences="):
        big.search_occurrences(p, 1)
    with pytest.raises(ValueError, match="sequences="):
        big.search_occurrences_refined(p, 1)
    c, s, sp = idx.search_occurrences([], 4)                  # P = 0: empty outputs without a launch
    assert c.shape == (0, 4) and s.shape == (0, 4) and sp.shape == (0, 4, 2)
    assert c.dtype == torch.float32 and s.dtype == torch.int64 and sp.dtype == torch.int64 and c.device.type == "cuda"
    out = idx.search_occurrences_refined([], 4, 2, return_candidates=True)
    assert out[0].shape == (0, 4) and out[2].shape == (0, 4, 2) and out[3].shape == (0, 8) and out[4].shape == (0, 8)
    monkeypatch.undo()
    c, s, sp = big.search_occurrences(p, 1, sequences=[0, 65536, 65537])      # and the same arguments made legal do launch
    assert s.shape == (1, 1) and int(s[0, 0]) == 0

"""GPU tier, phrase search through the inverted file (``IVFSyllableIndex.search_phrases`` = ``ivf.search`` seeds, the vote of
csrc/phrase_vote.hip, the exact re-rank; ``SyllableIndex.search_phrases_seeded`` holds the last two).

(a) full coverage (``nprobe == nlist``, every row a seed, every sequence a candidate): ``search_phrases`` bit for bit, both metrics;
(b) the general case: the candidates are the numpy vote (tests/phrase_vote_ref.py) on the library's own ``ivf.search`` output, and
    costs, seqs and spans are ``search_phrases`` restricted to those candidates;
(c) at ``nprobe == nlist`` every bound is at most the exact cost of its candidate;
(d) the planted phrases, which the reference recovers (tests/test_phrase_vote_ref.py asserts that), are recovered;
(e) bitwise invariance under the chunk and tile hooks, stale workspaces, ``build`` + ``add`` and ``save`` / ``load``;
(f) exclusion with default and explicit sequences, a NaN row in the corpus;
(g) the refusals and ``P = 0``."""
import functools

import numpy as np
import pytest
import torch

import phrase_vote_ref as V

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K, REFINE = 3, 4


def _np(t):
    return t.cpu().numpy()


def _assert_equal(got, want, what=""):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        if a.dtype == torch.float32:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what
        else:
            assert torch.equal(a, b), what


def _restrict(full, cand, k):
    """(costs [P, k], seqs, spans) of a full ``search_phrases`` list (numpy, every sequence listed) restricted to ``cand [P, m]``"""
    fc, fs, fsp = full
    P = fc.shape[0]
    c = np.full((P, k), np.inf, np.float32)
    s = np.full((P, k), -1, np.int64)
    sp = np.full((P, k, 2), -1, np.int64)
    for p in range(P):
        keep = np.nonzero((fs[p] >= 0) & np.isin(fs[p], cand[p][cand[p] >= 0]))[0][:k]
        c[p, :keep.size], s[p, :keep.size], sp[p, :keep.size] = fc[p, keep], fs[p, keep], fsp[p, keep]
    return c, s, sp


def _same_as_restriction(got, full, cand, k, what=""):
    c, s, sp = _restrict(full, cand, k)
    assert np.array_equal(_np(got[0]).view(np.uint32), c.view(np.uint32)), what
    assert np.array_equal(_np(got[1]), s) and np.array_equal(_np(got[2]), sp), what


@functools.lru_cache(maxsize=None)
def _case():
    c = V.planted_case()
    rng = np.random.default_rng(11)
    x, D = c["x"], c["x"].shape[1]
    extra = [rng.standard_normal((1, D)).astype(np.float32), (x[200:264] + 0.2 * rng.standard_normal((64, D))).astype(np.float32),
             (x[900:933] * 1.1).astype(np.float32)]
    c["all_phrases"] = list(c["phrases"]) + extra
    return c


@functools.lru_cache(maxsize=None)
def _ivf(metric):
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    c = _case()
    idx = SyllableIndex(c["x"], metric=metric, groups=c["groups"], device=DEV)
    if metric == "l2":
        return IVFSyllableIndex.build(idx, centroids=c["centroids"])
    return IVFSyllableIndex.build(idx, V.PLANTED["nlist"], seed=0)


@functools.lru_cache(maxsize=None)
def _full(metric):
    """``search_phrases`` with every sequence listed (S = 60 <= 128), as numpy: the reference of (b), (c) and (f), computed once"""
    c = _case()
    return tuple(_np(t) for t in _ivf(metric).index.search_phrases(c["all_phrases"], c["offsets"].size - 1))


def _lens_rows(phrases):
    lens = np.array([len(p) for p in phrases])
    return lens, np.cumsum(lens) - lens


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_full_coverage_is_search_phrases(metric):
    from sylber_amd import IVFSyllableIndex
    rng = np.random.default_rng(2)
    lens = np.array([3, 14, 5, 9, 8, 7, 10, 6, 12, 4, 11, 7])
    assert lens.sum() == 96
    off = np.concatenate([[0], np.cumsum(lens)])
    x = rng.standard_normal((96, 32)).astype(np.float32)
    groups = np.repeat(np.arange(12), lens).astype(np.int32)
    ivf = IVFSyllableIndex.build(x, 4, groups=groups, metric=metric, device=DEV)
    ph = [np.repeat(x[0:3], 22, 0)[:64] + np.float32(0.05),               # 64 rows against (among others) the 3-row sequence
          rng.standard_normal((1, 32)).astype(np.float32),
          (x[20:27] + 0.1 * rng.standard_normal((7, 32))).astype(np.float32),
          rng.standard_normal((64, 32)).astype(np.float32),
          rng.standard_normal((2, 32)).astype(np.float32)]
    want = ivf.index.search_phrases(ph, 4)
    got = ivf.search_phrases(ph, 4, 4, seeds=128, refine=3, return_candidates=True)
    _assert_equal(got[:3], want, metric)
    cand = _np(got[3])
    assert got[3].dtype == torch.int64 and got[4].dtype == torch.float32 and cand.shape == (5, 12)
    assert (np.sort(cand, 1) == np.arange(12)).all()
    assert _np(want[1])[0, 0] == 0 and ivf.last_search["seen"] == 12.0
    assert np.array_equal(ivf.sequence_offsets(), off)


# ---- (b), (c) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,nprobe,seeds", [("l2", 1, 4), ("l2", 1, 32), ("l2", 3, 4), ("l2", 3, 32), ("cosine", 3, 32), ("l2", 8, 4),
                                                 ("l2", 8, 32), ("cosine", 8, 7)])
def test_candidates_are_the_vote_and_the_result_its_restriction(metric, nprobe, seeds):
    c, ivf = _case(), _ivf(metric)
    ph, off = c["all_phrases"], c["offsets"]
    m = K * REFINE
    got = ivf.search_phrases(ph, K, nprobe, seeds=seeds, refine=REFINE, return_candidates=True)
    stats = dict(ivf.last_search)
    sc, ids = ivf.search(np.concatenate(ph), seeds, nprobe)
    lens, rows = _lens_rows(ph)
    cand, bound, seen = V.vote(_np(sc), _np(ids), rows, lens, off, metric, m, return_seen=True)
    assert np.array_equal(_np(got[3]), cand.astype(np.int64)), (metric, nprobe, seeds)
    assert np.array_equal(_np(got[4]).view(np.uint32), bound.view(np.uint32))
    assert stats["seen"] == pytest.approx(seen.mean()) and stats["pairs"] == ivf.last_search["pairs"] > 0
    full = _full(metric)
    _same_as_restriction(got, full, cand, K)
    # the seeded entry on the same seeds, given as host arrays, is the same search
    again = ivf.index.search_phrases_seeded(ph, _np(sc), _np(ids), K, REFINE, return_candidates=True)
    _assert_equal(again, got)
    if nprobe == ivf.nlist:                                                 # (c): the lower bound, against the exact costs
        fc, fs = full[0], full[1]
        for p in range(len(ph)):
            for s, b in zip(cand[p], bound[p]):
                if s >= 0:
                    cost = fc[p][fs[p] == s]
                    assert cost.size == 1 and b <= cost[0], (p, s, b, cost)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
def test_planted_phrases_are_recovered():
    c, P, ivf = _case(), V.PLANTED, _ivf("l2")
    costs, seqs, spans = ivf.search_phrases(c["phrases"], P["k"], P["nprobe"], seeds=P["seeds"], refine=P["refine"])
    assert np.array_equal(_np(seqs)[:, 0], c["truth"])
    sp = _np(spans)[:, 0]
    assert ((sp[:, 0] >= c["offsets"][c["truth"]]) & (sp[:, 1] <= c["offsets"][c["truth"] + 1])).all()


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
def test_invariance(tmp_path):
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    c, ivf = _case(), _ivf("l2")
    ph = c["all_phrases"]
    args = dict(seeds=32, refine=REFINE, return_candidates=True)
    base = ivf.search_phrases(ph, K, 3, **args)
    for hook in (dict(query_chunk=1), dict(phrase_chunk=1), dict(item_tiles=1), dict(_workspace_fill=0xFF), dict(_workspace_fill=0x7F),
                 dict(query_chunk=5, phrase_chunk=4)):
        _assert_equal(ivf.search_phrases(ph, K, 3, **args, **hook), base, str(hook))
    # one [sum m, D] array with lengths= is the same input
    lens, _ = _lens_rows(ph)
    _assert_equal(ivf.search_phrases(np.concatenate(ph), K, 3, lengths=lens, **args), base, "lengths=")
    # build + add
    n0 = int(c["offsets"][31])
    part = IVFSyllableIndex.build(SyllableIndex(c["x"][:n0], groups=c["groups"][:n0], device=DEV), centroids=c["centroids"])
    part.add(c["x"][n0:], groups=c["groups"][n0:])
    _assert_equal(part.search_phrases(ph, K, 3, **args), base, "build + add")
    # save / load
    path = str(tmp_path / "ivf.npz")
    ivf.save(path)
    _assert_equal(IVFSyllableIndex.load(path, device=DEV).search_phrases(ph, K, 3, **args), base, "save / load")


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------
def test_exclusion_with_default_sequences():
    c, ivf = _case(), _ivf("l2")
    ph, off = c["phrases"], c["offsets"]
    pg = c["truth"].astype(np.int32)                                        # group = sequence number: each phrase's own clip is excluded
    m = K * REFINE
    got = ivf.search_phrases(ph, K, 3, seeds=32, refine=REFINE, groups=pg, exclude_same_group=True, return_candidates=True)
    lens, rows = _lens_rows(ph)
    sc, ids = ivf.search(np.concatenate(ph), 32, 3, groups=np.repeat(pg, lens), exclude_same_group=True)
    assert not (_np(ivf.index._g)[np.maximum(_np(ids), 0)] == np.repeat(pg, lens)[:, None])[_np(ids) >= 0].any()   # no seed spent there
    cand, bound = V.vote(_np(sc), _np(ids), rows, lens, off, "l2", m, pg, np.arange(off.size - 1))
    assert np.array_equal(_np(got[3]), cand.astype(np.int64)) and np.array_equal(_np(got[4]).view(np.uint32), bound.view(np.uint32))
    full = tuple(_np(t) for t in ivf.index.search_phrases(ph, off.size - 1, groups=pg, exclude_same_group=True))
    _same_as_restriction(got, full, cand, K)
    assert not (_np(got[1]) == c["truth"][:, None]).any() and (_np(got[1])[:, 0] >= 0).all()


def test_exclusion_with_explicit_sequences():
    c, ivf = _case(), _ivf("l2")
    ph, off = c["phrases"], c["offsets"]
    mid = (off[:-1] + off[1:]) // 2
    cut = np.unique(np.concatenate([off, mid[::2]]))                        # every other sequence cut in two
    S2 = cut.size - 1
    assert 60 < S2 <= 128
    pg = c["truth"].astype(np.int32)
    m = K * REFINE
    got = ivf.search_phrases(ph, K, 3, seeds=32, refine=REFINE, groups=pg, exclude_same_group=True, sequences=cut, return_candidates=True)
    lens, rows = _lens_rows(ph)
    sc, ids = ivf.search(np.concatenate(ph), 32, 3)                         # stage 1a excludes nothing; the vote does
    cand, bound = V.vote(_np(sc), _np(ids), rows, lens, cut, "l2", m, pg, c["groups"][cut[:-1]])
    assert np.array_equal(_np(got[3]), cand.astype(np.int64)) and np.array_equal(_np(got[4]).view(np.uint32), bound.view(np.uint32))
    full = tuple(_np(t) for t in ivf.index.search_phrases(ph, S2, groups=pg, exclude_same_group=True, sequences=cut))
    _same_as_restriction(got, full, cand, K)
    assert not (c["groups"][cut[:-1]][np.maximum(_np(got[1]), 0)] == pg[:, None])[_np(got[1]) >= 0].any()


def test_nan_row_in_the_corpus():
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    c = _case()
    x = c["x"].copy()
    t = int(c["truth"][0])
    bad = int(c["offsets"][t]) + 1
    x[bad, 5] = np.nan                                                      # inside the first planted phrase's sequence
    ivf = IVFSyllableIndex.build(SyllableIndex(x, groups=c["groups"], device=DEV), centroids=c["centroids"])
    assert int(ivf.labels[bad]) == -1
    ph = c["phrases"]
    got = ivf.search_phrases(ph, K, 3, seeds=32, refine=REFINE, return_candidates=True)
    full = tuple(_np(t_) for t_ in ivf.index.search_phrases(ph, c["offsets"].size - 1))
    lens, rows = _lens_rows(ph)
    sc, ids = ivf.search(np.concatenate(ph), 32, 3)
    cand, bound = V.vote(_np(sc), _np(ids), rows, lens, c["offsets"], "l2", K * REFINE)
    assert not (_np(ids) == bad).any()
    assert np.array_equal(_np(got[3]), cand.astype(np.int64)) and np.array_equal(_np(got[4]).view(np.uint32), bound.view(np.uint32))
    _same_as_restriction(got, full, cand, K)
    assert np.isfinite(_np(got[0])[1:, 0]).all()


# ---- (g) ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_input():
    c, ivf = _case(), _ivf("l2")
    ph = c["phrases"][:2]
    R = sum(len(p) for p in ph)
    N = len(ivf)
    for kw in (dict(seeds=0), dict(seeds=129), dict(seeds=2.5), dict(refine=0), dict(refine=64), dict(phrase_chunk=0), dict(query_chunk=0),
               dict(exclude_same_group=True), dict(sequences=[0, 5])):
        with pytest.raises(ValueError):
            ivf.search_phrases(ph, K, 3, **kw)
    for k, nprobe in ((0, 3), (129, 3), (K, 0), (K, 9)):
        with pytest.raises(ValueError):
            ivf.search_phrases(ph, k, nprobe)
    with pytest.raises(ValueError):
        ivf.search_phrases([np.zeros((65, 32), np.float32)], K, 3)
    with pytest.raises(ValueError):
        ivf.search_phrases([np.zeros((3, 16), np.float32)], K, 3)
    idx = ivf.index
    sc, ids = np.zeros((R, 4), np.float32), np.zeros((R, 4), np.int64)
    for s_, i_ in ((sc[:-1], ids[:-1]), (sc, ids[:, :3]), (sc.astype(np.float64), ids), (sc, ids.astype(np.int32)), (sc[0], ids[0]),
                   (np.zeros((R, 129), np.float32), np.zeros((R, 129), np.int64)), (np.zeros((R, 0), np.float32), np.zeros((R, 0), np.int64)),
                   (sc, ids - 2), (sc, ids + N)):
        with pytest.raises(ValueError):
            idx.search_phrases_seeded(ph, s_, i_, K)
    with pytest.raises(ValueError):
        idx.search_phrases_seeded(ph, sc, ids, K, 64)
    idx.search_phrases_seeded(ph, sc, ids + (N - 1), K)                     # the largest id is legal, and so is -1
    idx.search_phrases_seeded(ph, sc, ids - 1, K)
    # P = 0
    got = ivf.search_phrases([], K, 3, return_candidates=True)
    assert [tuple(t.shape) for t in got] == [(0, K), (0, K), (0, K, 2), (0, K * 4), (0, K * 4)]
    assert [t.dtype for t in got] == [torch.float32, torch.int64, torch.int64, torch.int64, torch.float32]
    assert ivf.last_search["seen"] == 0.0
    got = idx.search_phrases_seeded(np.zeros((0, 32), np.float32), np.zeros((0, 4), np.float32), np.zeros((0, 4), np.int64), K, lengths=[])
    assert [tuple(t.shape) for t in got] == [(0, K), (0, K), (0, K, 2)]

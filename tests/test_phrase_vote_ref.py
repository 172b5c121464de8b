"""The vote of the seeded phrase search, checked on the CPU in the numpy restatement (tests/phrase_vote_ref.py): the lower bound, the
tie order, the padding, what ignored / duplicate / unsorted seeds may change, and that the planted case shared with
tests/test_gpu_ivf_phrase.py is recovered by the reference alone."""
import numpy as np
import pytest

import phrase_vote_ref as V

F = np.float32


def _corpus(rng, n_seq=9, D=8, lo=1, hi=9):
    lens = rng.integers(lo, hi, n_seq)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rng.standard_normal((int(off[-1]), D)).astype(F), off


@pytest.mark.parametrize("seeds", [1, 3, 8, 1000])
def test_lower_bound_on_true_nearest_seeds(seeds):
    """seeds = each row's nearest rows of the full fp32 distance matrix: bound <= the fp32 DTW cost on that matrix, exactly"""
    rng = np.random.default_rng(seeds)
    x, off = _corpus(rng)
    phrases = [rng.standard_normal((m, 8)).astype(F) for m in (1, 2, 5, 11)]
    q = np.concatenate(phrases)
    dm = V.l2_matrix(q, x)
    seeds = min(seeds, x.shape[0])
    sc, ids = V.nearest_seeds(dm, seeds)
    lens = np.array([len(p) for p in phrases])
    rows = np.cumsum(lens) - lens
    S = off.size - 1
    cand, bound = V.vote(sc, ids, rows, lens, off, "l2", S)
    checked = 0
    for p in range(len(phrases)):
        for s, b in zip(cand[p], bound[p]):
            if s < 0:
                assert b == np.inf
                continue
            cost = V.dtw_cost(dm[rows[p]:rows[p] + lens[p], off[s]:off[s + 1]])
            assert b <= cost, (p, s, b, cost)
            checked += 1
        if seeds == x.shape[0]:                                             # every row is a seed: every sequence is seen
            assert (cand[p] >= 0).all()
    assert checked >= len(phrases)


def test_full_seeds_single_row_phrase_bound_is_the_cost():
    """a one-row phrase with every row a seed: the bound of a sequence is its smallest distance, which is its DTW cost"""
    rng = np.random.default_rng(0)
    x, off = _corpus(rng)
    q = rng.standard_normal((1, 8)).astype(F)
    dm = V.l2_matrix(q, x)
    sc, ids = V.nearest_seeds(dm, x.shape[0])
    cand, bound = V.vote(sc, ids, [0], [1], off, "l2", off.size - 1)
    for s, b in zip(cand[0], bound[0]):
        assert b == dm[0, off[s]:off[s + 1]].min()
    assert np.array_equal(np.lexsort((cand[0], bound[0])), np.arange(off.size - 1))


def test_tie_order_and_padding():
    off = np.array([0, 2, 4, 6, 8])
    # one row; seeds in sequences 3, 1, 2 with equal cost 1, sequence 0 with cost 2
    sc = np.array([[1, 1, 2, 1]], F)
    ids = np.array([[6, 2, 0, 5]], np.int64)
    cand, bound = V.vote(sc, ids, [0], [1], off, "l2", 6)
    assert cand.dtype == np.int32 and bound.dtype == F
    assert cand[0].tolist() == [1, 2, 3, 0, -1, -1]
    assert bound[0].tolist() == [1, 1, 1, 2, np.inf, np.inf]
    cand, bound = V.vote(sc, ids, [0], [1], off, "l2", 2)                   # m below the number of seen sequences
    assert cand[0].tolist() == [1, 2] and bound[0].tolist() == [1, 1]


def test_floor_and_rows_without_seeds():
    off = np.array([0, 4, 8])
    # row 0: seeds in sequence 0 (0.5) and 1 (3); row 1: no valid seed (floor 0); row 2: seed in sequence 1 only (2), floor 2
    sc = np.array([[0.5, 3], [np.inf, np.nan], [2, np.inf]], F)
    ids = np.array([[1, 5], [-1, 3], [6, -1]], np.int64)
    cand, bound = V.vote(sc, ids, [0], [3], off, "l2", 3)
    assert cand[0].tolist() == [0, 1, -1]
    assert bound[0].tolist() == [F(F(F(0.5) + F(0)) + F(2)), F(F(F(3) + F(0)) + F(2)), np.inf]
    # a phrase with no valid seed at all
    cand, bound = V.vote(np.full((2, 3), np.nan, F), np.full((2, 3), 4, np.int64), [0], [2], off, "l2", 2)
    assert (cand == -1).all() and (bound == np.inf).all()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_ignored_duplicate_and_unsorted_seeds(metric):
    rng = np.random.default_rng(3)
    off = np.array([0, 3, 7, 8, 15, 20])
    R, seeds = 7, 6
    ids = rng.integers(0, 20, (R, seeds)).astype(np.int64)
    sc = (rng.random((R, seeds)) * (1 if metric == "cosine" else 4)).astype(F)
    lens, rows = np.array([3, 4]), np.array([0, 3])
    base = V.vote(sc, ids, rows, lens, off, metric, 5)
    # shuffled within each row
    perm = np.stack([rng.permutation(seeds) for _ in range(R)])
    sh = V.vote(np.take_along_axis(sc, perm, 1), np.take_along_axis(ids, perm, 1), rows, lens, off, metric, 5)
    # every seed twice, and ignored seeds appended: id -1, NaN score, d = +inf
    bad_s = np.array([0.25, np.nan, -np.inf if metric == "cosine" else np.inf], F)
    bad_i = np.array([-1, 2, 9], np.int64)
    sc2 = np.concatenate([sc, np.tile(bad_s, (R, 1)), sc], 1)
    ids2 = np.concatenate([ids, np.tile(bad_i, (R, 1)), ids], 1)
    dup = V.vote(sc2, ids2, rows, lens, off, metric, 5)
    for other in (sh, dup):
        assert np.array_equal(base[0], other[0]) and np.array_equal(base[1].view(np.uint32), other[1].view(np.uint32))
    # group exclusion drops exactly the sequences of the phrase's group
    sg, pg = np.array([0, 1, 0, 2, 1]), np.array([0, 1])
    ex = V.vote(sc, ids, rows, lens, off, metric, 5, pg, sg)
    for p in range(2):
        keep = [(s, b) for s, b in zip(base[0][p], base[1][p]) if s >= 0 and sg[s] != pg[p]]
        got = [(s, b) for s, b in zip(ex[0][p], ex[1][p]) if s >= 0]
        assert got == keep and len(keep) < (base[0][p] >= 0).sum()


def test_cosine_local_cost():
    d = V.local_cost(np.array([1.5, 1.0, 0.25, -1.0], F), "cosine")
    assert d.tolist() == [0.0, 0.0, 0.75, 2.0]


def test_planted_phrases_are_recovered_by_the_reference():
    """the case of tests/test_gpu_ivf_phrase.py (d): numpy inverted-file seeds, the vote and the exact fp32 DTW of the candidates put
    the planted sequence first for every phrase, at the parameters the GPU test uses"""
    c, P = V.planted_case(), V.PLANTED
    q = np.concatenate(c["phrases"])
    sc, ids = V.ivf_seeds(q, c["x"], c["centroids"], P["nprobe"], P["seeds"])
    costs, seqs, cand, bound = V.seeded_search(c["phrases"], c["x"], c["offsets"], sc, ids, P["k"], P["k"] * P["refine"])
    assert 1200 <= c["x"].shape[0] <= 1400 and c["offsets"].size - 1 == P["n_seq"]
    assert np.array_equal(seqs[:, 0], c["truth"]), (seqs[:, 0], c["truth"])
    # the runner-up is far behind: the recovery does not hang on a rounding
    assert (costs[:, 1] > 4 * costs[:, 0]).all(), costs

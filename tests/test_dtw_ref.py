"""CPU tier, phrase search: the numpy restatement of the subsequence-DTW contract (tests/dtw_ref.py) against brute force, its tie
rules and corner cases, and the host-only planner of the built library (``sylber_dtw_plan``): every row of every sequence covered
exactly once, cuts on sequence starts only, a phrase never straddling a query block (nor a 64-row half), and its refusals."""
import ctypes
import itertools

import numpy as np
import pytest

import dtw_ref as R

INF = np.inf


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dp_is_the_minimum_over_all_warping_paths(dtype):
    rng = np.random.default_rng(5)
    for m, L in itertools.product(range(1, 5), range(1, 7)):
        for rep in range(4):
            d = rng.random((m, L)) * 10.0 ** rng.integers(-3, 4)
            if rep == 3:
                d = np.round(d * 4) / 4                      # many equal sums
            c, s, e, A = R.dtw_loop(d, dtype)
            assert c == R.brute_force(d, dtype), (m, L, rep)
            assert R.dtw(d, dtype) == (c, s, e)
            assert 0 <= s <= e < L


def test_anti_diagonal_evaluation_equals_the_cell_loop():
    rng = np.random.default_rng(6)
    for m, L in ((1, 1), (1, 9), (7, 1), (7, 3), (13, 40), (64, 5), (64, 130)):
        d = rng.random((m, L)).astype(np.float32)
        d[rng.random((m, L)) < 0.05] = INF
        d = np.round(d * 8) / 8 if m == 13 else d
        c, s, e, _ = R.dtw_loop(d, np.float32)
        assert R.dtw(d, np.float32) == (c, s, e), (m, L)


def test_tie_rules():
    # predecessor order: diagonal before (i-1, j) before (i, j-1)
    d = np.zeros((2, 3))
    c, s, e, A = R.dtw_loop(d, np.float32)
    assert (c, s, e) == (0.0, 0, 0)                          # smallest end on ties; at j = 0 only the vertical step exists
    d = np.array([[0.0, 0.0, 5.0], [9.0, 9.0, 1.0]])         # row 1 best at j = 2: predecessors (0,1) diag = 0, (0,2) up = 5, (1,1) left = 9
    assert R.dtw_loop(d, np.float32)[:3] == (1.0, 1, 2)
    d = np.array([[1.0, 1.0], [7.0, 2.0]])                   # (1,1): diagonal (0,0) = 1 and up (0,1) = 1 tie: the diagonal's start wins
    assert R.dtw_loop(d, np.float32)[:3] == (3.0, 0, 1)
    d = np.array([[4.0, 1.0], [0.0, 2.0]])                   # (1,1): diag 4, up 1, left 4: up wins, start 1
    assert R.dtw_loop(d, np.float32)[:3] == (3.0, 1, 1)
    d = np.array([[1.0, 3.0], [0.0, 0.0]])                   # (1,1): diag 1, up 3, left 1: the diagonal before the left on a tie; both start 0
    assert R.dtw_loop(d, np.float32)[:3] == (1.0, 0, 0)
    # order of a list: (cost, sequence); +inf never returned; padding
    c, q, sp = R.rank(np.array([2.0, 1.0, INF, 1.0], np.float32), [0, 1, 0, 0], [0, 2, 0, 1], [0, 3, 10, 12], 5)
    assert q.tolist() == [1, 3, 0, -1, -1] and c.tolist() == [1.0, 1.0, 2.0, INF, INF]
    assert sp.tolist() == [[4, 6], [12, 14], [0, 1], [-1, -1], [-1, -1]]
    c, q, sp = R.rank(np.array([2.0, 1.0], np.float32), [0, 0], [0, 0], [0, 1], 1, admissible=[True, False])
    assert q.tolist() == [0]


def test_infinite_and_nan_costs():
    d = np.array([[1.0, np.nan, 1.0], [1.0, 1.0, INF]])
    c, s, e, A = R.dtw_loop(d, np.float32)
    assert A[0, 1] == INF and (c, s, e) == (2.0, 0, 0)
    assert R.dtw(d, np.float32) == (c, s, e)
    c, s, e = R.dtw(np.full((3, 4), np.nan), np.float32)
    assert c == INF                                          # a NaN phrase has no result: rank drops it
    assert R.rank(np.array([c]), [s], [e], [0, 4], 2)[1].tolist() == [-1, -1]
    # a NaN column inside a sequence can be stepped over only by paths that avoid it: none does for m = 1 spans, some do around it
    d = np.array([[0.0, np.nan, 0.0], [5.0, np.nan, 0.0]])
    assert R.dtw(d, np.float32) == (0.0, 2, 2)


def test_phrase_longer_than_sequence_and_single_column():
    d = np.array([[1.0], [2.0], [4.0]])
    assert R.dtw(d, np.float32) == (7.0, 0, 0)               # L = 1: vertical steps only
    d = np.arange(10.0).reshape(5, 2)
    c, s, e, _ = R.dtw_loop(d, np.float64)
    assert c == R.brute_force(d) and R.dtw(d, np.float64) == (c, s, e)


def test_default_sequences_from_groups():
    assert R.sequences_from_groups([]).tolist() == [0]
    assert R.sequences_from_groups([3]).tolist() == [0, 1]
    assert R.sequences_from_groups([0, 0, 1, 1, 1, 0, 2, 2, -1, -1]).tolist() == [0, 2, 5, 6, 8, 10]      # group 0 twice: two sequences


def test_error_bound_is_positive_and_grows_with_the_path():
    rng = np.random.default_rng(1)
    q, x = rng.standard_normal((4, 16)), rng.standard_normal((9, 16))
    b1 = R.cost_error_bound(q, x[:3], 1.0)
    b2 = R.cost_error_bound(q, x, 1.0)
    assert 0 < b1 < b2 < 1e-2


# ---- the host-only planner of the built library --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sylber_amd import build, _lib
    build.build()
    return _lib.load()


def _plan(lib, offsets, lens, k=10, splits=0, block_phrases=0):
    i32p = ctypes.POINTER(ctypes.c_int32)
    off = np.ascontiguousarray(offsets, np.int32)
    ln = np.ascontiguousarray(lens, np.int32)
    nb, ph = ctypes.c_int32(-7), ctypes.c_int32(-7)
    place = np.full(ln.size, -1, np.int32)
    a = (off.ctypes.data_as(i32p), off.size - 1, ln.ctypes.data_as(i32p), ln.size, k, splits, block_phrases)
    C = lib.sylber_dtw_plan(*a, None, 0, place.ctypes.data_as(i32p), ctypes.byref(nb), ctypes.byref(ph))
    if C < 0:
        return C, None, None, None, None
    cuts = np.full(C + 1, -1, np.int32)
    assert lib.sylber_dtw_plan(*a, cuts.ctypes.data_as(i32p), C + 1, None, None, None) == C
    assert lib.sylber_dtw_plan(*a, cuts.ctypes.data_as(i32p), C, None, None, None) == -1      # one entry short
    return C, cuts, place, nb.value, ph.value


def _check_plan(offsets, lens, C, cuts, place, nb, ph):
    offsets, lens = np.asarray(offsets), np.asarray(lens)
    N = offsets[-1]
    # cuts: ascending from 0 to N, on sequence starts only, so every row of every sequence lies in exactly one cut, with its sequence
    assert cuts[0] == 0 and cuts[-1] == N and np.all(np.diff(cuts) > 0) and len(cuts) == C + 1
    assert np.isin(cuts[:-1], offsets[:-1]).all()
    covered = np.zeros(N, np.int64)
    for c in range(C):
        covered[cuts[c]:cuts[c + 1]] += 1
    assert (covered == 1).all()
    # phrases: in order, inside one block and one 64-row half of it, not overlapping, at most ph per block
    used = np.zeros(nb * 128, np.int64)
    for p, m in zip(place, lens):
        assert p // 128 == (p + m - 1) // 128 and p // 64 == (p + m - 1) // 64
        used[p:p + m] += 1
    assert used.max() == 1 and np.all(np.diff(place) > 0)
    assert np.bincount(place // 128, minlength=nb).max() <= ph and np.bincount(place // 128, minlength=nb).min() >= 1


def test_planner_covers_rows_and_packs_phrases(lib):
    rng = np.random.default_rng(2)
    for trial in range(30):
        S = int(rng.integers(1, 400))
        offsets = np.concatenate([[0], np.cumsum(rng.integers(1, [3, 70, 700][trial % 3], S))])
        lens = rng.integers(1, 65, int(rng.integers(1, 300)))
        if trial % 5 == 0:
            lens[:] = [1, 63, 64, 32, 33][trial // 5 % 5]
        k = int(rng.choice([1, 10, 33, 128]))
        for splits in (0, 1, 2, 7, S, int(offsets[-1]), 100000):
            for bp in (0, 1, 5):
                C, cuts, place, nb, ph = _plan(lib, offsets, lens, k, splits, bp)
                assert 1 <= C <= min(S, max(splits, 1) if splits else S)
                assert ph == (min(128, 4096 // k) if bp == 0 else min(bp, 128, 4096 // k))
                _check_plan(offsets, lens, C, cuts, place, nb, ph)
                if 65535 >= splits >= offsets[-1]:
                    assert C == S and cuts.tolist() == offsets.tolist()         # every admissible cut
                if splits == 1:
                    assert cuts.tolist() == [0, offsets[-1]]


def test_planner_automatic_cuts_fill_the_chip(lib):
    offsets = np.arange(0, 4_000_001, 40)
    C, cuts, place, nb, ph = _plan(lib, offsets, [8] * 128, 10, 0, 0)
    assert nb == 8 and C == 64                               # 8 query blocks x 64 cuts = 512 workgroups
    _check_plan(offsets, [8] * 128, C, cuts, place, nb, ph)
    assert np.diff(cuts).min() >= 4 * 128
    C, cuts, place, nb, ph = _plan(lib, [0, 100, 300], [8], 10, 0, 0)
    assert C == 1                                            # fewer than 4 tiles: no cut


def test_planner_refusals(lib):
    ok = [0, 10, 20]
    assert _plan(lib, ok, [0])[0] == -2
    assert _plan(lib, ok, [65])[0] == -2
    assert _plan(lib, ok, [64, 1])[0] == 1
    assert _plan(lib, [0, 65537], [3])[0] == -3
    assert _plan(lib, [0, 65536], [3])[0] == 1
    assert _plan(lib, [1, 10], [3])[0] == -4
    assert _plan(lib, [0, 10, 10], [3])[0] == -4
    assert _plan(lib, [0, 10, 5], [3])[0] == -4
    assert _plan(lib, ok, [3], k=0)[0] == -1 and _plan(lib, ok, [3], k=129)[0] == -1
    assert _plan(lib, ok, [3], splits=-1)[0] == -1

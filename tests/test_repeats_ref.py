"""CPU tier: tests/repeats_ref.py, the numpy restatement of the "Embedding repeats" contract (``SyllableIndex.search_repeats`` /
``find_repeats``), against itself: the cell loop against the anti-diagonal evaluation with the kernel's gather, both against a brute
force over every path, exact ties, +inf cells, the two facts the contract states, the window theorem, the derived error bound
between the fp32 and the float64 run, and that the entry is exported and checks its arguments before any device call."""
import numpy as np
import pytest

import dtw_ref
import knn_ref
import repeats_ref as R

F = np.float32


def _cases(rng, n, half_integers, max_m=9, max_L=14):
    for _ in range(n):
        m, L = int(rng.integers(1, max_m)), int(rng.integers(1, max_L))
        d = (rng.integers(0, 7, (m, L)) * 0.5).astype(F) if half_integers else rng.gamma(2.0, 1.0, (m, L)).astype(F)
        d[rng.random((m, L)) < 0.1] = np.inf
        if rng.random() < 0.3:
            d[rng.random((m, L)) < 0.05] = np.nan                    # a NaN d counts as +inf
        radius = F(rng.integers(1, 5) * 0.5) if half_integers else F(rng.uniform(0.5, 3.0))
        gap = [F(0), radius, F(2) * radius, F(rng.integers(0, 5) * 0.5)][int(rng.integers(0, 4))]
        yield d, radius, gap


def _same(a, b):
    return np.asarray(a[0], F).view(np.uint32) == np.asarray(b[0], F).view(np.uint32) and a[1] == b[1] and a[2] == b[2]


@pytest.mark.parametrize("half_integers", [False, True])
def test_cell_loop_equals_the_anti_diagonals(half_integers):
    rng = np.random.default_rng(1 + half_integers)
    some = 0
    for d, radius, gap in _cases(rng, 150, half_integers):
        a, b = R.local_loop(d, radius, gap)[:3], R.local(d, radius, gap)
        assert _same(a, b), (d, radius, gap)
        some += a[0] > 0
    assert some > 75


def test_float64_runs_agree_too():
    rng = np.random.default_rng(3)
    for d, radius, gap in _cases(rng, 60, False):
        a, b = R.local_loop(d, radius, gap, np.float64)[:3], R.local(d, radius, gap, np.float64)
        assert a[0] == b[0] and a[1:] == b[1:]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_against_every_path(dtype):
    rng = np.random.default_rng(4)
    for half in (False, True):
        for d, radius, gap in _cases(rng, 40, half, max_m=4, max_L=5):
            assert R.local(d, radius, gap, dtype)[0] == R.brute_force(d, radius, gap, dtype)


def test_exact_ties_by_hand():
    d = np.zeros((2, 2), F)
    # gap = radius: every step earns 1 diagonally, 0 otherwise
    assert R.local(d, F(1), F(1)) == (F(2), (0, 2), (0, 2))
    # gap = 0: H = [[1, 2], [2, 3]]; the last cell takes (i-1, j) before (i, j-1), whose path began in (0, 0)
    sc, pa, pb, H, _ = R.local_loop(d, F(1), F(0))
    assert H.tolist() == [[1, 2], [2, 3]] and (sc, pa, pb) == (F(3), (0, 2), (0, 2))
    # equal best cells: the smallest i, then the smallest j
    d = np.full((3, 5), 9, F)
    d[2, 0] = d[1, 3] = d[1, 4] = 0
    assert R.local(d, F(1), F(2)) == (F(1), (1, 2), (3, 4)) == R.local_loop(d, F(1), F(2))[:3]
    # half-integers: a diagonal of 1.5 + 1.5 against a detour 1.5 + (2.5 - 1) + ... stays exact
    d = np.array([[0.5, 0.0], [9, 0.5]], F)
    assert R.local(d, F(2), F(1)) == (F(3), (0, 2), (0, 2))


def test_inf_cells_and_no_result():
    d = np.full((3, 4), np.inf, F)
    assert R.local(d, F(1), F(0)) == (F(0), None, None) and R.local_loop(d, F(1), F(0))[:3] == (F(0), None, None)
    assert R.local(np.full((2, 2), 5, F), F(1), F(0))[0] == 0          # nothing closer than the radius
    d[1, 2] = 0.25
    assert R.local(d, F(1), F(0)) == (F(0.75), (1, 2), (2, 3))
    d[:] = 0
    d[1, 1] = np.nan                                                   # a wall: paths go round it or end before it
    sc, pa, pb = R.local(d, F(1), F(2))
    assert sc == 3 and R.brute_force(d, F(1), F(2), F) == 3 and (pa, pb) == ((0, 3), (1, 4))


def test_a_start_is_only_read_from_a_positive_cell():
    rng = np.random.default_rng(5)
    for half in (False, True):
        for d, radius, gap in _cases(rng, 80, half):
            sc, pa, pb, H, read = R.local_loop(d, radius, gap)
            assert (read > 0).all()
            if sc > 0:
                assert pa[0] < pa[1] and pb[0] < pb[1]                 # both spans are non-empty
                d0 = d[pa[0], pb[0]]
                assert radius - d0 > 0                                 # the first cell of the path earns


def test_a_sub_range_of_the_probe_never_scores_higher_and_keeps_the_bits_of_a_path_inside():
    rng = np.random.default_rng(6)
    kept = 0
    for half in (False, True):
        for d, radius, gap in _cases(rng, 120, half, max_m=12):
            full = R.local(d, radius, gap)
            m = d.shape[0]
            a = int(rng.integers(0, m))
            b = int(rng.integers(a + 1, m + 1))
            sub = R.local(d[a:b], radius, gap)
            assert sub[0] <= full[0]
            if full[0] > 0 and a <= full[1][0] and full[1][1] <= b:
                assert _same(sub, (full[0], (full[1][0] - a, full[1][1] - a), full[2]))
                kept += 1
    assert kept > 30


def test_windows():
    assert R.windows(10, 64, 32) == [0] and R.windows(64, 64, 32) == [0] and R.windows(65, 64, 32) == [0, 1]
    assert R.windows(150, 64, 32) == [0, 32, 64, 86] and R.windows(128, 64, 32) == [0, 32, 64]
    assert R.windows(5, 2, 1) == [0, 1, 2, 3] and R.windows(5, 2, 2) == [0, 2, 3]


def _planted(rng, a, b, n, L=150):
    """d [2 L, 2 L] of two sequences of L rows: far everywhere (d in [4, 6]) but close (d in [0, 0.5]) on the diagonal of n cells
    from (a, b) of the block (sequence 0, sequence 1)"""
    d = rng.uniform(4, 6, (2 * L, 2 * L)).astype(F)
    k = np.arange(n)
    d[a + k, L + b + k] = rng.uniform(0, 0.5, n).astype(F)
    return d


@pytest.mark.parametrize("window,hop", [(64, 32), (64, 64), (40, 1), (64, 17)])
def test_the_window_theorem(window, hop):
    rng = np.random.default_rng(window + hop)
    L, off = 150, np.array([0, 150, 300])
    width = window - hop + 1
    radius, gap = F(1), F(2)
    cases = ((0, 0, width), (hop - 1 if hop > 1 else 7, 20, width), (L - width, 3, width), (L - window + 5, 100, min(width, 20)),
                (31, 60, width), (70, 1, 1), (10, 10, min(64, width + 20)), (50, 90, 60))
    for a, b, n in (cases[1:3] + cases[-1:] if hop == 1 else cases):  # hop = 1 has 111 windows: fewer cases
        d = _planted(rng, a, b, n)
        full = R.local(d[:L, L:], radius, gap)
        assert full[0] > 0
        sc, pairs, spans = R.find_repeats(d, off, 3, radius, gap, F(0.5), window, hop)
        assert pairs.tolist() == [[0, 1], [-1, -1], [-1, -1]] and sc[1] == 0 and (spans[1:] == -1).all()
        if full[1][1] - full[1][0] <= width:
            assert sc[0].view(np.uint32) == F(full[0]).view(np.uint32)
            assert spans[0].tolist() == [list(full[1]), [full[2][0] + L, full[2][1] + L]]
        else:
            assert n > width and 0 < sc[0] <= full[0]


def test_find_repeats_reduces_per_pair_and_orders():
    rng = np.random.default_rng(8)
    off = np.array([0, 30, 70, 80, 150])
    d = rng.uniform(4, 6, (150, 150)).astype(F)
    for (a, b, n) in ((2, 40, 6), (5, 100, 6), (33, 120, 4), (72, 85, 8)):
        d[a + np.arange(n), b + np.arange(n)] = 0
    sc, pairs, spans = R.find_repeats(d, off, 5, F(1), F(2), F(3), 16, 8)
    assert sc.tolist() == [8, 6, 6, 4, 0] and pairs.tolist() == [[2, 3], [0, 1], [0, 3], [1, 3], [-1, -1]]
    assert spans[0].tolist() == [[72, 80], [85, 93]] and spans[2].tolist() == [[5, 11], [100, 106]]
    grp = np.repeat([0, 1, 2, 0], np.diff(off))
    sc, pairs, _ = R.find_repeats(d, off, 5, F(1), F(2), F(3), 16, 8, groups=grp)
    assert pairs.tolist()[:4] == [[2, 3], [0, 1], [1, 3], [-1, -1]]
    assert R.find_repeats(d, off, 2, F(1), F(2), F(5), 16, 8)[1].tolist() == [[2, 3], [0, 1]]


def test_rank_and_search_repeats():
    off = np.array([0, 4, 10, 12])
    res = [(F(2), (0, 1), (1, 2)), (F(5), (1, 3), (0, 2)), (F(2), (0, 2), (0, 2))]
    sc, sq, sp = R.rank(res, off, 4, F(1))
    assert sc.tolist() == [5, 2, 2, 0] and sq.tolist() == [1, 0, 2, -1]
    assert sp[0].tolist() == [[1, 3], [4, 6]] and sp[2].tolist() == [[0, 2], [10, 12]] and (sp[3] == -1).all()
    assert R.rank(res, off, 4, F(3))[1].tolist() == [1, -1, -1, -1]
    assert R.rank(res, off, 1, F(1), [True, False, True])[1].tolist() == [0]
    d = np.full((2, 12), 9, F)
    d[0, 5] = d[1, 6] = d[0, 10] = 0
    got = R.search_repeats(lambda p, s: d[:, off[s]:off[s + 1]], 1, off, 3, F(1), F(2), F(1))
    assert got[0].tolist() == [[2, 1, 0]] and got[1].tolist() == [[1, 2, -1]] and got[3].tolist() == [[False, True, True]]
    assert got[2][0, 0].tolist() == [[0, 2], [5, 7]]
    got = R.search_repeats(lambda p, s: d[:, off[s]:off[s + 1]], 1, off, 3, F(1), F(2), F(1), after=[1])
    assert got[1].tolist() == [[2, -1, -1]]


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_score_error_bound_holds_between_the_fp32_and_the_float64_run(metric):
    x, offsets, probes, radii = R.float64_case()
    radius = radii[metric]
    if metric == "cosine":
        x = knn_ref.unit_rows(x).astype(F)
        probes = [knn_ref.unit_rows(p).astype(F) for p in probes]
    worst, positive = 0.0, 0
    for gap in (F(0), F(2) * radius):
        for q in probes:
            for s in range(len(offsets) - 1):
                xr = x[offsets[s]:offsets[s + 1]]
                s32 = R.local(R.local_costs32(q, xr, metric), radius, gap, np.float32)[0]
                s64 = R.local(dtw_ref.local_costs(q, xr, metric), radius, gap, np.float64)[0]
                bound = R.score_error_bound(q, xr, s64, radius, gap, metric)
                assert abs(float(s32) - float(s64)) <= bound
                assert bound < float(radius)                                   # and the bound says something
                worst = max(worst, abs(float(s32) - float(s64)) / bound)
                positive += s64 > 0
    print("fp32 against float64", metric, "worst error / bound", worst, "positive pairs", positive)
    assert positive >= 8


def test_the_entry_is_declared_exported_and_checks_its_arguments():
    from sylber_amd import _lib
    assert "sylber_dtw_local" in set(_lib.EXPORTS)
    lib = _lib.load()
    x = 64                                                              # a non-null pointer that is never followed
    good = [x, 1, x, x, x, 1, 1, x, 1, 16, x, 0, 1, 1.0, 2.0, 3.0, x, x, 1, None, None, None, x, x, x, x, None]
    for at, bad, msg in ((0, None, b"null"), (1, 0, b"n_blocks"), (9, 24, b"multiple of 16"), (12, 129, b"k <= 128"), (6, 129, b"block_phrases"),
                         (18, 0, b"cuts"), (11, 7, b"metric"), (10, None, b"db_norm_dev"), (19, x, b"go together"),
                         (13, 0.0, b"radius"), (13, float("nan"), b"radius"), (13, float("inf"), b"radius"), (13, -1.0, b"radius"),
                         (14, -0.5, b"gap"), (14, float("inf"), b"gap"), (14, float("nan"), b"gap"),
                         (15, 0.0, b"min_score"), (15, float("inf"), b"min_score"), (15, float("nan"), b"min_score")):
        a = list(good)
        a[at] = bad
        assert lib.sylber_dtw_local(*a) == 1, (at, bad)
        err = lib.sylber_last_error()
        assert b"sylber_dtw_local" in err and msg in err, (at, bad, err)
    a = list(good)
    a[5], a[12], a[18] = 70000, 128, 128
    assert lib.sylber_dtw_local(*a) == 1 and b"use smaller phrase chunks" in lib.sylber_last_error()

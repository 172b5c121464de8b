"""CPU tier: the warping-path contract of tests/align_ref.py and the theorem that lets ``align_phrases`` work after the fact --
recomputing the DP on nothing but a returned span's columns and backtracking from its last cell reproduces the full scan's path,
its start and its cost bit for bit -- on random, tied and +inf-holed matrices; the ``rows`` representation; pinned examples whose
paths are written out by hand."""
import numpy as np
import pytest

import align_ref as A
import dtw_ref as R


def _matrices(n, seed):
    """n local-cost matrices of 1..8 x 1..13 cells: small integers (ties everywhere), uniform reals, and either with 15 % +inf holes"""
    rng = np.random.default_rng(seed)
    for t in range(n):
        m, L = (1 if t % 40 == 0 else int(rng.integers(1, 9))), int(rng.integers(1, 14))
        kind = t % 3
        d = rng.integers(0, 3, (m, L)).astype(np.float32) if kind == 0 or (kind == 2 and t % 2) else rng.random((m, L), np.float32)
        if kind == 2:
            d[rng.random((m, L)) < 0.15] = np.inf
        yield d


def test_the_theorem_window_dp_reproduces_the_full_scan():
    finite = ones = 0
    for d in _matrices(4200, 0):
        m = d.shape[0]
        full = A.full_scan(d)
        if full is None:
            assert not (R.dtw_loop(d)[0] < np.inf)
            continue
        finite += 1
        ones += m == 1
        cost, start, end, cells = full
        assert cells[0] == (0, start) and cells[-1] == (m - 1, end)       # the tracked start is the path's
        got = A.align(d[:, start:end + 1])
        assert got is not None
        wcost, steps, runs, wcells = got
        assert [(i, j + start) for i, j in wcells] == cells               # the window path is the full DP's path
        assert wcells[0] == (0, 0)                                        # it starts at the span start
        assert np.float32(wcost).view(np.uint32) == np.float32(cost).view(np.uint32)
        assert A.fold(d, cells).view(np.uint32) == np.float32(cost).view(np.uint32)
        assert steps == len(cells) and m <= steps <= m + (end - start)
        assert runs[0, 0] == 0 and runs[m - 1, 1] == end - start + 1
    assert finite >= 3000 and ones >= 50


def test_rows_round_trip_to_the_cell_list():
    n = 0
    for d in _matrices(600, 1):
        got = A.align(d)
        if got is None:
            continue
        _, steps, runs, cells = got
        m = d.shape[0]
        assert A.cells_of(runs) == cells and np.array_equal(A.runs_of(A.cells_of(runs), m), runs)
        assert int((runs[:, 1] - runs[:, 0]).sum()) == steps              # every cell of the path lies in exactly one run
        assert (runs[:, 1] > runs[:, 0]).all() and runs[0, 1] - runs[0, 0] == 1      # row 0 holds one cell: the start is free
        nxt = runs[1:, 0] - (runs[:-1, 1] - 1)                            # lo[i+1] is hi[i] (a vertical step) or hi[i] + 1 (a diagonal)
        assert np.isin(nxt, (0, 1)).all()
        n += 1
    assert n > 400


def test_a_window_that_is_no_span_may_start_inside_it():
    d = np.zeros((2, 3), np.float32)                                      # every comparison ties
    cost, steps, runs, cells = A.align(d)
    assert cells == [(0, 1), (1, 2)] and cost == 0 and steps == 2         # the diagonal first: the path starts in column 1, not 0
    assert A.full_scan(d)[1:3] == (0, 0)                                  # where the scan itself reports the span [0, 1)


@pytest.mark.parametrize("d,cells,cost", [
    # A = [[1, 1, 1, 1], [2, 1, 1, 2], [3, 2, 1, 1]]: (2, 3) ties diagonal with left, (1, 2) ties all three: the diagonal both times
    ([[1, 1, 1, 1], [1, 0, 0, 1], [1, 1, 0, 0]], [(0, 1), (1, 2), (2, 3)], 1),
    # m > W forces a vertical step: (2, 1) ties diagonal with up -> diagonal; (1, 0) has only up
    ([[0, 5], [0, 0], [5, 0]], [(0, 0), (1, 0), (2, 1)], 0),
    # a step to the left: (1, 2) takes (1, 1) at 0 against 9 and 9; (1, 1) takes the diagonal
    ([[0, 9, 9], [9, 0, 0]], [(0, 0), (1, 1), (1, 2)], 0),
    # a hole: the only finite way into (1, 2) is from above
    ([[3, np.inf, 1], [np.inf, np.inf, 2]], [(0, 2), (1, 2)], 3),
])
def test_pinned_paths_written_out_by_hand(d, cells, cost):
    d = np.array(d, np.float32)
    got = A.align(d)
    assert got[3] == cells and got[0] == np.float32(cost) and got[1] == len(cells)
    assert np.array_equal(got[2], A.runs_of(cells, d.shape[0]))


def test_an_infinite_last_cell_is_padding_and_align_phrases_places_the_rest():
    inf = np.float32(np.inf)
    d = np.array([[0, 1, inf], [1, 0, inf]], np.float32)
    assert A.align(d) is None and A.align(d[:, :2]) is not None
    rows, steps, costs = A.align_phrases(lambda p, a, b: d[:, a - 10:b - 10], [2], np.array([[[10, 13], [10, 12], [-1, -1]]]))
    assert rows.shape == (1, 3, 2, 2) and (rows[0, [0, 2]] == -1).all() and steps.tolist() == [[0, 2, 0]]
    assert rows[0, 1].tolist() == [[10, 11], [11, 12]] and costs[0, 1] == 0 and np.isinf(costs[0, [0, 2]]).all()

"""CPU tier: tests/dtw_strings_ref.py, the restatement of the "Embedding strings" contract, against brute force, against the window
DP of tests/align_ref.py (the theorem of include/sylber_hip.h) and against the strip-wise decomposition that csrc/dtw_strings.hip
relies on.  No GPU, no library."""
import numpy as np

import align_ref as A
import dtw_strings_ref as G


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


def test_the_dp_is_the_minimum_over_every_monotone_path():
    rng = np.random.default_rng(0)
    for m, L in G.shapes_up_to(5):
        for d in G.tied_matrices(rng, m, L):
            want, counts = G.brute_force(d, np.float64)
            got = G.align(d, np.float64, loop=True)
            if not want < np.inf:
                assert got is None
                continue
            cost, steps, runs, cells = got
            assert cost == want and steps in counts and steps == len(cells), (m, L)
            assert A.fold(d, cells, np.float64) == cost             # the path's own left fold is the cost
            assert cells[0] == (0, 0) and cells[-1] == (m - 1, L - 1)
            assert all((c - a, e - b) in ((1, 1), (1, 0), (0, 1)) for (a, b), (c, e) in zip(cells, cells[1:]))


def test_the_anti_diagonal_form_is_the_loop():
    rng = np.random.default_rng(1)
    for m, L in ((1, 1), (1, 9), (9, 1), (7, 12), (12, 7), (20, 20)):
        for d in G.tied_matrices(rng, m, L):
            a, b = G.global_loop(d), G.global_diag(d)
            assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_identities_of_steps_and_runs():
    rng = np.random.default_rng(2)
    for m, L in ((1, 1), (1, 6), (6, 1), (5, 9), (9, 5), (17, 17), (3, 40)):
        for d in G.tied_matrices(rng, m, L):
            got = G.align(d)
            if got is None:
                assert not G.global_loop(d)[0][m - 1, L - 1] < np.inf
                continue
            cost, steps, runs, cells = got
            assert max(m, L) <= steps <= m + L - 1
            assert runs[0, 0] == 0 and runs[m - 1, 1] == L and (runs[:, 1] > runs[:, 0]).all()
            nxt, hi = runs[1:, 0], runs[:-1, 1]
            assert ((nxt == hi - 1) | (nxt == hi)).all()              # lo[i+1] is hi[i] - 1 (a vertical step) or hi[i] (a diagonal one)
            assert steps == int((runs[:, 1] - runs[:, 0]).sum())      # the runs are the path
            assert _bits(A.fold(d, cells)) == _bits(cost)


def test_the_theorem_against_the_window_dp():
    """when the window DP's path (free start, forced end) starts in column 0, the global alignment has its cost bits, its steps and
    its runs; always the global cost is at least the window's"""
    rng = np.random.default_rng(3)
    held = 0
    for m, L in ((1, 1), (1, 7), (2, 5), (5, 5), (7, 4), (6, 11), (12, 9), (3, 30)):
        for rep in range(12):
            for d in G.tied_matrices(rng, m, L):
                if rep % 2:
                    d[0, 1:] += np.float32(rep)                       # a dear first row behind column 0: the free start takes column 0 more often
                win, glob = A.align(d), G.align(d)
                if win is None:
                    assert glob is None                               # no path to (m-1, L-1) at all
                    continue
                if glob is not None:
                    assert glob[0] >= win[0]
                if win[3][0] != (0, 0):
                    continue
                held += 1
                assert glob is not None
                assert _bits(glob[0]) == _bits(win[0]) and glob[1] == win[1] and np.array_equal(glob[2], win[2]) and glob[3] == win[3]
    assert held > 100


def test_the_strip_wise_form_has_the_same_bits():
    """64-row strips, 128-column tiles, carried (A, n) rows: one strip, two, three with a short last one; one tile, two, three"""
    rng = np.random.default_rng(4)
    for m, L in ((1, 1), (33, 40), (64, 128), (65, 129), (128, 128), (129, 127), (150, 257)):
        mats = [rng.random((m, L)).astype(np.float32), rng.integers(0, 3, (m, L)).astype(np.float32)]
        h = mats[1].copy()
        h[rng.random((m, L)) < 0.05] = np.inf
        for d in mats + [h]:
            Af, nf, _ = G.global_diag(d)
            cost, steps = G.align_strips(d)
            assert _bits(cost) == _bits(Af[m - 1, L - 1]), (m, L)
            if cost < np.inf:
                assert steps == nf[m - 1, L - 1], (m, L)


def test_padding_and_the_workspace_formula():
    assert G.align(np.zeros((0, 5), np.float32)) is None and G.align(np.zeros((3, 0), np.float32)) is None
    d = np.ones((3, 3), np.float32)
    d[1] = np.nan                                                     # a NaN row of x: every path crosses it
    assert G.align(d) is None
    rows, costs, steps, xo = G.align_sequences(lambda s: [d, np.ones((2, 4), np.float32)][s], [3, 2], [3, 4])
    assert (rows[:3] == -1).all() and np.isposinf(costs[0]) and steps[0] == 0 and xo.tolist() == [0, 3, 5]
    assert rows[3:].tolist() == [[0, 3], [3, 4]] and steps[1] == 4 and costs[1] == 4      # all ties: the diagonal first, so it is taken last on the way back
    assert G.workspace_bytes(128, 1000, False) == 0 and G.workspace_bytes(129, 1000, False) == 16128
    assert G.workspace_bytes(129, 0, True) == 0 and G.workspace_bytes(0, 9, True) == 0
    assert G.workspace_bytes(65, 129, True) == 2 * 2 * 2048 and G.workspace_bytes(300, 257, True) == 4352 + 5 * 3 * 2048
    assert G.workspace_bytes(65536, 65536, False) == 1 << 20

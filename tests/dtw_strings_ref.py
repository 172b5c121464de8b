"""numpy restatement of the "Embedding strings" contract of include/sylber_hip.h: sylber_amd.align_sequences /
SyllableIndex.align_sequences / csrc/dtw_strings.hip, on top of tests/dtw_ref.py (whose local costs these are) and tests/align_ref.py
(whose predecessor order this is).

A pair is a sequence x of m rows and a sequence y of L rows; ``d [m, L]`` are the local costs of ``search_phrases`` with x in the role
of the phrase.  Global DTW, all additions in the dtype given (float32 restates the device bit for bit), one per cell::

    A[0][0] = d[0][0]                                     n[0][0] = 1
    A[i][j] = d[i][j] + min(A[i-1][j-1], A[i-1][j], A[i][j-1])      terms outside the matrix are +inf
              the first smallest in that order (diagonal, up, left)
    n[i][j] = n[the predecessor taken] + 1

``cost = A[m-1][L-1]``, ``steps = n[m-1][L-1]``, ``rows[i] = (lo, hi)``: the run of columns the path visits in row i, hi exclusive.
A pair whose cost is not below +inf, and a pair with an empty side, is padding: cost +inf, steps 0, rows (-1, -1)."""
import itertools

import numpy as np

import dtw_ref as R

DIAG, UP, LEFT = 0, 1, 2
STRIP_ROWS, TILE_COLS, SUPER_ROWS = 64, 128, 128


def global_loop(d, dtype=np.float32):
    """the recurrence cell by cell, as the contract writes it -> (A [m, L], n int64 [m, L], code int8 [m, L]: the predecessor taken)"""
    d = R._clean(d, dtype)
    m, L = d.shape
    inf = dtype(np.inf)
    A = np.full((m, L), inf, dtype)
    n = np.zeros((m, L), np.int64)
    code = np.zeros((m, L), np.int8)
    for i in range(m):
        for j in range(L):
            if i == 0 and j == 0:
                A[0, 0], n[0, 0] = d[0, 0], 1
                continue
            best, nb, c = (A[i - 1, j - 1], n[i - 1, j - 1], DIAG) if i > 0 and j > 0 else (inf, 0, DIAG)
            if i > 0 and A[i - 1, j] < best:
                best, nb, c = A[i - 1, j], n[i - 1, j], UP
            if j > 0 and A[i, j - 1] < best:
                best, nb, c = A[i, j - 1], n[i, j - 1], LEFT
            A[i, j], n[i, j], code[i, j] = dtype(d[i, j] + best), nb + 1, c
    return A, n, code


def global_diag(d, dtype=np.float32, top=None):
    """the same recurrence, the same additions, one anti-diagonal at a time (cells of one anti-diagonal do not depend on each other)
    -> (A, n, code) as ``global_loop``.  ``top = (A [L], n [L])``: the row above row 0 instead of +inf -- a strip of a longer x, which
    then has no origin cell."""
    d = R._clean(d, dtype)
    m, L = d.shape
    inf = dtype(np.inf)
    A = np.full((m + 1, L + 1), inf, dtype)                 # row 0 and column 0 of the padded arrays: outside the matrix
    n = np.zeros((m + 1, L + 1), np.int64)
    code = np.zeros((m, L), np.int8)
    if top is not None:
        A[0, 1:], n[0, 1:] = top
    for t in range(m + L - 1):
        i = np.arange(max(0, t - L + 1), min(m, t + 1))
        j = t - i
        best, nb, c = A[i, j].copy(), n[i, j].copy(), np.zeros(i.size, np.int8)
        up = A[i, j + 1]
        mk = up < best
        best[mk], nb[mk], c[mk] = up[mk], n[i, j + 1][mk], UP
        left = A[i + 1, j]
        mk = left < best
        best[mk], nb[mk], c[mk] = left[mk], n[i + 1, j][mk], LEFT
        cur, cn = (d[i, j] + best).astype(dtype), nb + 1
        if t == 0 and top is None:
            cur[0], cn[0] = d[0, 0], 1
        A[i + 1, j + 1], n[i + 1, j + 1], code[i, j] = cur, cn, c
    return A[1:, 1:], n[1:, 1:], code


def walk(code, m, L):
    """follow the predecessor codes from (m-1, L-1) to (0, 0), a step out of the matrix bent along its edge as the kernel bends it
    -> the path's cells in ascending order"""
    i, j = m - 1, L - 1
    cells = [(i, j)]
    while i > 0 or j > 0:
        c = LEFT if i == 0 else UP if j == 0 else int(code[i, j])
        if c == LEFT:
            j -= 1
        elif c == UP:
            i -= 1
        else:
            i, j = i - 1, j - 1
        cells.append((i, j))
    return cells[::-1]


def runs_of(cells, m):
    """the cell list of a path -> int64 [m, 2]: (first column, one past the last column) visited in each row of x"""
    runs = np.full((m, 2), -1, np.int64)
    for i, j in cells:
        if runs[i, 0] < 0:
            runs[i] = (j, j + 1)
        else:
            assert j == runs[i, 1]
            runs[i, 1] = j + 1
    return runs


def align(d, dtype=np.float32, loop=False):
    """one pair from its local costs d [m, L] -> (cost, steps, runs int64 [m, 2], cells), or None for padding"""
    d = np.asarray(d)
    if d.ndim != 2 or d.shape[0] == 0 or d.shape[1] == 0:
        return None
    A, n, code = (global_loop if loop else global_diag)(d, dtype)
    m, L = A.shape
    if not A[m - 1, L - 1] < np.inf:
        return None
    cells = walk(code, m, L)
    return A[m - 1, L - 1], int(n[m - 1, L - 1]), runs_of(cells, m), cells


def align_strips(d, dtype=np.float32):
    """the decomposition csrc/dtw_strings.hip relies on: x in strips of 64 rows, each walked tile by tile of 128 columns with only
    the lane state (a strip's last two columns) kept between tiles, the strip's last row carried to the next strip as its upper row
    -> (cost, steps) of the cell (m-1, L-1), +inf cells included.  Every cell makes the additions of ``global_loop``."""
    d = R._clean(d, dtype)
    m, L = d.shape
    inf = dtype(np.inf)
    top_a, top_n = np.full(L, inf, dtype), np.zeros(L, np.int64)
    for s0 in range(0, m, STRIP_ROWS):
        rows = min(STRIP_ROWS, m - s0)
        a_cur, a_prev = np.full(rows, inf, dtype), np.full(rows, inf, dtype)       # A[i][last column done], A[i][the one before]
        n_cur, n_prev = np.zeros(rows, np.int64), np.zeros(rows, np.int64)
        pa, pn = inf, 0                                          # the row above at the previous column: lane 0's diagonal
        out_a, out_n = np.full(L, inf, dtype), np.zeros(L, np.int64)
        for n0 in range(0, L, TILE_COLS):
            ncol = min(TILE_COLS, L - n0)
            for t in range(ncol + rows - 1):                    # the wavefront drains at the tile's edge
                ua, uap = np.concatenate([[inf], a_cur[:-1]]).astype(dtype), np.concatenate([[inf], a_prev[:-1]]).astype(dtype)
                un, unp = np.concatenate([[0], n_cur[:-1]]), np.concatenate([[0], n_prev[:-1]])
                lane = np.arange(rows)
                j = t - lane
                ok = (j >= 0) & (j < ncol)
                if ok[0]:
                    ua[0], un[0], uap[0], unp[0] = top_a[n0 + j[0]], top_n[n0 + j[0]], pa, pn
                    pa, pn = ua[0], un[0]
                best, nb = uap.copy(), unp.copy()
                mk = ua < best
                best[mk], nb[mk] = ua[mk], un[mk]
                mk = a_cur < best
                best[mk], nb[mk] = a_cur[mk], n_cur[mk]
                dv = d[s0 + lane, n0 + np.clip(j, 0, ncol - 1)]
                cur, cn = (dv + best).astype(dtype), nb + 1
                if s0 == 0 and n0 == 0 and t == 0:
                    cur[0], cn[0] = dv[0], 1
                a_prev, n_prev = np.where(ok, a_cur, a_prev), np.where(ok, n_cur, n_prev)
                a_cur, n_cur = np.where(ok, cur, a_cur).astype(dtype), np.where(ok, cn, n_cur)
                if ok[rows - 1]:
                    out_a[n0 + j[rows - 1]], out_n[n0 + j[rows - 1]] = a_cur[rows - 1], n_cur[rows - 1]
        top_a, top_n = out_a, out_n
    return top_a[L - 1], int(top_n[L - 1])


def brute_force(d, dtype=np.float64):
    """every monotone path from (0, 0) to (m-1, L-1) (steps (1,1), (1,0), (0,1)) -> (the smallest sum, accumulated cell by cell from
    (0, 0) in ``dtype``, the set of cell counts of the paths that reach it).  Tiny cases only."""
    d = R._clean(d, dtype)
    m, L = d.shape
    best, counts = [dtype(np.inf)], [set()]

    def go(i, j, acc, cells):
        if i == m - 1 and j == L - 1:
            if acc < best[0]:
                best[0], counts[0] = acc, {cells}
            elif acc == best[0]:
                counts[0].add(cells)
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            a, b = i + di, j + dj
            if a < m and b < L:
                go(a, b, dtype(acc + d[a, b]), cells + 1)

    go(0, 0, d[0, 0], 1)
    return best[0], counts[0]


def workspace_bytes(m, L, path):
    """what a pair adds to ``sylber_dtw_strings_workspace_bytes`` beyond its 64 B of table, written out from the header's formula"""
    al = lambda b: (b + 255) // 256 * 256
    rows = al(2 * 8 * L) if m > SUPER_ROWS and L > 0 else 0
    codes = -(-m // STRIP_ROWS) * -(-L // TILE_COLS) * 2048 if path and m > 0 and L > 0 else 0
    return rows + codes


def align_sequences(d_of, lens_x, lens_y, dtype=np.float32):
    """the whole contract from a function ``d_of(s) -> d [m_s, L_s]`` -> (rows int64 [sum m, 2], costs [S], steps int32 [S],
    x_offsets int64 [S + 1])"""
    S = len(lens_x)
    xo = np.concatenate([[0], np.cumsum(lens_x)]).astype(np.int64)
    rows = np.full((int(xo[-1]), 2), -1, np.int64)
    costs, steps = np.full(S, np.inf, dtype), np.zeros(S, np.int32)
    for s in range(S):
        got = align(d_of(s), dtype) if lens_x[s] and lens_y[s] else None
        if got is not None:
            costs[s], steps[s] = got[0], got[1]
            rows[xo[s]:xo[s + 1]] = got[2]
    return rows, costs, steps, xo


def cost_error_bound(x, y, cost64, metric="l2"):
    """an upper bound on |cost32 - cost64| of one pair (rows x [m, D], y [L, D], both as the kernel reads them: unit rows under
    "cosine").  ``dtw_ref.cost_error_bound``'s derivation carries over word for word, because it uses of the DP only that the cost is
    a minimum, over some set of monotone paths, of left folds of d -- here the paths from (0, 0) to (m-1, L-1) instead of the
    paths from row 0 to row m-1:
      * each cell's d is off by at most e_d = the rounding of the chain (knn_ref.dot_error_bound on the score s) + gamma_D ||x_i||^2
        (the fp32 row norm, L2 only) + one rounding u (d + e) of dt_cost's last operation; max(0, .) is 1-Lipschitz;
      * a path has ``steps`` <= n = m + L - 1 cells, and each DP addition rounds once, so along a path
        |f32 - f64| <= E + gamma_n (f64 + E) with E = n e_d;
      * min over paths is 1-Lipschitz in those errors, taken at the float64-optimal path one way and at the fp32-optimal path the
        other way, whose float64 sum is at most (cost64 + E (1 + gamma_n)) / (1 - gamma_n).
    The bound is evaluated with n = m + L - 1 >= steps, so it holds whichever path either DP takes."""
    return R.cost_error_bound(x, y, cost64, metric)


def tied_matrices(rng, m, L):
    """local costs for the reference tests: random, small integers (ties everywhere), constant, and integers with +inf holes"""
    yield rng.random((m, L)).astype(np.float32)
    yield rng.integers(0, 3, (m, L)).astype(np.float32)
    yield np.ones((m, L), np.float32)
    h = rng.integers(0, 3, (m, L)).astype(np.float32)
    h[rng.random((m, L)) < 0.25] = np.inf
    yield h


def shapes_up_to(k):
    return itertools.product(range(1, k + 1), range(1, k + 1))

"""numpy restatement of the warping-path contract of sylber_amd.SyllableIndex.align_phrases / csrc/dtw_align.hip, on top of
tests/dtw_ref.py (whose local costs, recurrence and predecessor order these are).

For one pair (phrase of m rows, window ``[a, b)`` of row ids, ``W = b - a``), with ``d [m, W]`` the local costs of ``search_phrases``:

* the window is **one** sequence whose first column is ``a``: a free start (``A[0][j] = d[0][j]`` for every column) and a forced end:
  the path ends in cell ``(m-1, W-1)``; the recurrence and the order of the predecessors on ties are ``dtw_ref.dtw_loop``'s:
  diagonal, then ``(i-1, j)``, then ``(i, j-1)``;
* the path is the chain of predecessors taken from ``(m-1, W-1)`` back to the row-0 cell it reaches; ``cost = A[m-1][W-1]``, ``steps``
  = the number of cells on it; ``rows[i] = (lo_i, hi_i + 1)`` = the run of columns the path visits in phrase row i.  A monotone path
  visits one contiguous run per row and ``lo[i+1]`` is ``hi[i]`` or ``hi[i] + 1``, so the runs *are* the path;
* if ``A[m-1][W-1]`` is not below ``+inf`` the pair is padding: rows ``(-1, -1)``, steps 0, cost ``+inf``.

The theorem (tests/test_align_ref.py): if ``[a, b)`` is the span the full subsequence DTW reports, the window's path starts in column
``a``, its cost has the bits of the reported cost and it is the full DP's own path."""
import numpy as np

import dtw_ref as R


def predecessor(A, i, j):
    """the cell that ``A[i][j]`` (i > 0) was formed from: the first smallest of (i-1, j-1), (i-1, j), (i, j-1) in that order, exactly
    as ``dtw_ref.dtw_loop`` compares them (terms outside the matrix are +inf)"""
    inf = A.dtype.type(np.inf)
    best, cell = (A[i - 1, j - 1], (i - 1, j - 1)) if j > 0 else (inf, (i - 1, j - 1))
    if A[i - 1, j] < best:
        best, cell = A[i - 1, j], (i - 1, j)
    if j > 0 and A[i, j - 1] < best:
        best, cell = A[i, j - 1], (i, j - 1)
    return cell


def path_to(A, i, j):
    """the chain of predecessors from the finite cell (i, j) back to row 0 -> its cells in ascending order [(0, j0), ..., (i, j)]"""
    assert A[i, j] < np.inf
    cells = [(i, j)]
    while i > 0:
        i, j = predecessor(A, i, j)
        assert j >= 0 and A[i, j] < np.inf               # a finite cell was formed from a finite one
        cells.append((i, j))
    return cells[::-1]


def runs_of(cells, m):
    """the cell list of a path -> int64 [m, 2]: (first column, one past the last column) visited in each phrase row"""
    runs = np.full((m, 2), -1, np.int64)
    for i, j in cells:
        if runs[i, 0] < 0:
            runs[i] = (j, j + 1)
        else:
            assert j == runs[i, 1]                           # one contiguous run per row, visited left to right
            runs[i, 1] = j + 1
    return runs


def cells_of(runs):
    """the inverse of ``runs_of``"""
    return [(i, j) for i, (lo, hi) in enumerate(np.asarray(runs).tolist()) for j in range(lo, hi)]


def fold(d, cells, dtype=np.float32):
    """the left fold of d along a path: the additions the recurrence made for its last cell, in its order"""
    d = R._clean(d, dtype)
    acc = d[cells[0]]
    for c in cells[1:]:
        acc = dtype(d[c] + acc)
    return acc


def align(d, dtype=np.float32):
    """the window DP on d [m, W] -> (cost, steps, runs int64 [m, 2] in window columns, cells), or None for a pair that is padding"""
    A = R.dtw_loop(d, dtype)[3]
    m, W = A.shape
    if not A[m - 1, W - 1] < np.inf:
        return None
    cells = path_to(A, m - 1, W - 1)
    return A[m - 1, W - 1], len(cells), runs_of(cells, m), cells


def full_scan(d, dtype=np.float32):
    """the subsequence DTW of ``dtw_ref.dtw_loop`` on a whole sequence d [m, L] with the path it took ->
    (cost, start column, end column, cells), or None when the cost is +inf"""
    cost, start, end, A = R.dtw_loop(d, dtype)
    if not cost < np.inf:
        return None
    return cost, start, end, path_to(A, A.shape[0] - 1, end)


def align_phrases(d_of, lens, spans, dtype=np.float32):
    """the whole contract from a function ``d_of(p, a, b) -> d [m_p, b - a]`` and spans int64 [P, k, 2] ->
    (rows int64 [P, k, Mx, 2] as row ids, steps int32 [P, k], costs [P, k])"""
    spans = np.asarray(spans)
    P, k = spans.shape[:2]
    Mx = int(max(lens)) if P else 0
    rows = np.full((P, k, Mx, 2), -1, np.int64)
    steps = np.zeros((P, k), np.int32)
    costs = np.full((P, k), np.inf, dtype)
    for p in range(P):
        for r in range(k):
            a, b = (int(v) for v in spans[p, r])
            if a < 0:
                continue
            got = align(d_of(p, a, b), dtype)
            if got is None:
                continue
            costs[p, r], steps[p, r] = got[0], got[1]
            rows[p, r, :lens[p]] = got[2] + a
    return rows, steps, costs

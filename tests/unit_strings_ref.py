"""numpy restatement of "Unit strings" (include/sylber_hip.h; sylber_amd.align_unit_strings / unit_error_rate,
csrc/unit_strings.hip) on top of tests/unit_align_ref.py: the global alignment of a reference string ``r`` of ``m`` units and a
hypothesis string ``h`` of ``L`` units, ``0 <= m, L``, int32::

    E[i][-1] = (i + 1) W        E[-1][j] = (j + 1) W  (predecessor "left")        E[-1][-1] = 0
    E[i][j]  = min(E[i-1][j-1] + sub(i, j), E[i-1][j] + W, E[i][j-1] + W)   the first smallest in that order

``align`` is the DEFINITION: ``unit_align_ref.window_scan(r, h, False)`` -- the table, the predecessor of every cell and the walk
back from ``(m-1, L-1)`` -- plus the rules for an empty side.  ``counters`` is the form the kernel computes its counts in: every
cell carries ``(cost, d, sb)``, ``d`` the diagonal steps on the path its chosen predecessor tracked and ``sb`` those of them with
``sub > 0``, both 0 on row -1 and column -1, so that the last cell gives the counts without a path.  ``strips`` is ``counters`` a
strip of reference rows at a time with the strip's last row handed on as the next one's upper row, as the kernel hands it on."""
import numpy as np

from unit_align_ref import window_scan
from unit_search_ref import as_units


def _pair(r, h):
    """-> (r [m, W], h [L, W], W); an empty side takes the other's width (1 if both are empty)"""
    r, h = as_units(r), as_units(h)
    if r.shape[0] == 0 or h.shape[0] == 0:
        W = r.shape[1] if r.shape[0] else h.shape[1] if h.shape[0] else 1
        r = r if r.shape[0] else np.zeros((0, W), np.int64)
        h = h if h.shape[0] else np.zeros((0, W), np.int64)
    assert r.shape[1] == h.shape[1]
    return r, h, r.shape[1]


def align(r, h):
    """the definition -> (cols int64 [m], subs int32 [m], ops int32 [4], cost)"""
    r, h, W = _pair(r, h)
    m, L = r.shape[0], h.shape[0]
    if m == 0 or L == 0:
        return np.full(m, -1, np.int64), np.full(m, W, np.int32), np.array([0, 0, m, L], np.int32), (m + L) * W
    cols, subs, ops, cost, first = window_scan(r, h, False)
    assert first == 0
    return cols, subs, ops, cost


def _row(above, corner, left, ri, h, W):
    """one row of carried counters, cell by cell: ``above`` = the cells (cost, d, sb) of the row above, ``corner`` = its cell at
    column -1, ``left`` = this row's cell at column -1 -> this row's cells"""
    row, diag = [], corner
    sub = (ri[None, :] != h).sum(1).tolist()
    for j in range(h.shape[0]):
        up = above[j]
        best = (diag[0] + sub[j], diag[1] + 1, diag[2] + (1 if sub[j] else 0))
        if up[0] + W < best[0]:
            best = (up[0] + W, up[1], up[2])
        if left[0] + W < best[0]:
            best = (left[0] + W, left[1], left[2])
        row.append(best)
        diag, left = up, best
    return row


def _counts(cell, m, L):
    cost, d, sb = cell
    return np.array([d - sb, sb, m - d, L - d], np.int32), cost


def counters(r, h):
    """the carried-counter form over the whole table -> (ops int32 [4], cost)"""
    return strips(r, h, rows=None)


def strips(r, h, rows=64):
    """the carried-counter form ``rows`` reference rows at a time (``None``: all at once): between strips nothing but the last
    row's cells is kept -> (ops int32 [4], cost)"""
    r, h, W = _pair(r, h)
    m, L = r.shape[0], h.shape[0]
    if m == 0 or L == 0:
        return np.array([0, 0, m, L], np.int32), (m + L) * W
    boundary = [((j + 1) * W, 0, 0) for j in range(L)]     # row -1
    for s0 in range(0, m, rows or m):
        above = boundary
        for i in range(s0, min(m, s0 + (rows or m))):
            above = _row(above, (i * W, 0, 0), ((i + 1) * W, 0, 0), r[i], h, W)
        boundary = list(above)                             # what the next strip sees of this one
    return _counts(boundary[L - 1], m, L)


def align_batch(refs, hyps):
    """``align`` of every pair, shaped as ``align_unit_strings(..., pairing=True)`` returns it -> (cols int64 [sum m], subs int32
    [sum m], ops int32 [S, 4], costs int32 [S], ref_offsets int64 [S + 1])"""
    out = [align(r, h) for r, h in zip(refs, hyps)]
    lens = [len(o[0]) for o in out]
    cols = np.concatenate([o[0] for o in out]) if out else np.zeros(0, np.int64)
    subs = np.concatenate([o[1] for o in out]) if out else np.zeros(0, np.int32)
    ops = np.array([o[2] for o in out], np.int32).reshape(len(out), 4)
    costs = np.array([o[3] for o in out], np.int32)
    return cols.astype(np.int64), subs.astype(np.int32), ops, costs, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def lev(a, b, W):
    """textbook global edit distance of unit strings a [m, W], b [n, W], a row at a time: substitution = differing columns, indel = W"""
    prev = np.arange(len(b) + 1, dtype=np.int64) * W
    for i in range(1, len(a) + 1):
        c = np.minimum(prev[:-1] + (a[i - 1][None, :] != b).sum(1), prev[1:] + W) if len(b) else np.zeros(0, np.int64)
        key = np.concatenate([[i * W], c]) - np.arange(len(b) + 1) * W
        prev = np.minimum.accumulate(key) + np.arange(len(b) + 1) * W
    return int(prev[-1])

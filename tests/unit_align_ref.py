"""numpy restatement of "Edit scripts" (include/sylber_hip.h; sylber_amd.UnitIndex.align_phrases, csrc/unit_align.hip) on top of
tests/unit_search_ref.py: the window DP of one (phrase, window of rows) pair, the predecessor each cell took and the walk back.

For a phrase of ``m`` units and a window ``[a, b)`` taken as ONE sequence of ``L = b - a`` columns, int32::

    E[i][-1] = (i + 1) W
    E[-1][j] = 0                 (free_start: the searches' DP)        or (j + 1) W with predecessor "left" (global)
    E[i][j]  = min(E[i-1][j-1] + sub(i, j), E[i-1][j] + W, E[i][j-1] + W), the first smallest in that order

The path is the chain of predecessors from ``(m-1, L-1)`` back to row -1 (global: on to the corner) or to column -1.  Per pair:
``cols [m]`` (the column that unit i is paired with by a diagonal step, -1: deleted), ``subs [m]``, ``ops = (equal, substituted,
deleted, inserted)``, ``cost = E[m-1][L-1]`` and the first column of the path.

``window_loop`` is the contract cell by cell; ``window_scan`` one phrase row at a time for one long window, in the manner of
``unit_search_ref.last_row_scan``; ``scan_path`` walks the FULL free-start DP of a sequence back from a cell of the last row: the
scan's own path."""
import numpy as np

from unit_search_ref import PAD, as_units

DIAG, UP, LEFT = 0, 1, 2


def walk_back(pred, sub, W, i, j, free_start):
    """the predecessors ``pred[i][j]`` followed from cell (i, j) to the boundary -> (cols [i + 1], subs [i + 1], ops [4], first
    column of the path); ``sub(i, j)`` is the local cost"""
    m = i + 1
    cols, subs = np.full(m, -1, np.int64), np.full(m, W, np.int32)
    eq = sb = de = ins = 0
    first = j + 1
    while i >= 0 and j >= 0:
        c = pred[i][j]
        if c == LEFT:
            ins += 1
            first = j
            j -= 1
        elif c == UP:
            de += 1
            i -= 1
        else:
            s = sub(i, j)
            cols[i], subs[i] = j, s
            if s:
                sb += 1
            else:
                eq += 1
            first = j
            i -= 1
            j -= 1
    de += i + 1                                            # column -1: units 0 .. i are deletions
    if not free_start and j >= 0:                          # row -1, global: leading insertions to the corner
        ins += j + 1
        first = 0
    return cols, subs, np.array([eq, sb, de, ins], np.int32), first


def window_table(p, t, free_start=True):
    """cell by cell -> (E [m][L] as lists, pred [m][L] as lists)"""
    p, t = as_units(p), as_units(t)
    m, L, W = p.shape[0], t.shape[0], p.shape[1]
    sub = (p[:, None, :] != t[None, :, :]).sum(-1).tolist()
    top = [0] * (L + 1) if free_start else [j * W for j in range(L + 1)]          # index j + 1: row -1
    E, pred = [], []
    for i in range(m):
        above = top if i == 0 else [i * W] + E[i - 1]      # index j + 1: row i - 1 with its boundary column
        row, prow, left = [], [], (i + 1) * W
        si = sub[i]
        for j in range(L):
            best, c = above[j] + si[j], DIAG
            if above[j + 1] + W < best:
                best, c = above[j + 1] + W, UP
            if left + W < best:
                best, c = left + W, LEFT
            row.append(best)
            prow.append(c)
            left = best
        E.append(row)
        pred.append(prow)
    return E, pred


def window_loop(p, t, free_start=True):
    """the contract cell by cell -> (cols, subs, ops, cost, first column)"""
    p, t = as_units(p), as_units(t)
    E, pred = window_table(p, t, free_start)
    m, L, W = p.shape[0], t.shape[0], p.shape[1]
    out = walk_back(pred, lambda i, j: int((p[i] != t[j]).sum()), W, m - 1, L - 1, free_start)
    return out[0], out[1], out[2], int(E[m - 1][L - 1]), out[3]


def window_scan(p, t, free_start=True):
    """``window_loop`` one phrase row at a time: along a row ``E[j] = min(c[j], E[j-1] + W)`` with ``c[j]`` the better of the diagonal
    and the upper term (the diagonal on ties), a running minimum of ``c[j'] + (j - j') W`` whose origin is the LATEST ``j'`` that
    attains it (the left term loses ties); a cell whose origin is an earlier column took "left", else what ``c[j]`` took"""
    p, t = as_units(p), as_units(t)
    m, L, W = p.shape[0], t.shape[0], p.shape[1]
    E = np.zeros(L + 1, np.int64) if free_start else np.arange(L + 1, dtype=np.int64) * W     # index j + 1: row -1
    jj, pos = np.arange(-1, L), np.arange(L + 1)
    pred = np.zeros((m, L), np.uint8)
    for i in range(m):
        cd, cu = E[:-1] + (p[i][None, :] != t).sum(1), E[1:] + W
        up = cu < cd
        key = np.concatenate([[(i + 1) * W], np.where(up, cu, cd)]) - jj * W         # column -1 is (i + 1) W
        cm = np.minimum.accumulate(key)
        org = np.maximum.accumulate(np.where(key == cm, pos, -1))
        pred[i] = np.where(org[1:] != pos[1:], LEFT, np.where(up, UP, DIAG))
        E = cm + jj * W
    out = walk_back(pred, lambda i, j: int((p[i] != t[j]).sum()), W, m - 1, L - 1, free_start)
    return out[0], out[1], out[2], int(E[L]), out[3]


def scan_path(p, t, end):
    """the scan's own path: the FULL free-start DP of phrase p against the whole sequence t, walked back from (m-1, end) ->
    (cols, subs, ops, cost, first column), columns counted in t"""
    p, t = as_units(p), as_units(t)
    E, pred = window_table(p, t, True)
    m, W = p.shape[0], p.shape[1]
    out = walk_back(pred, lambda i, j: int((p[i] != t[j]).sum()), W, m - 1, end, True)
    return out[0], out[1], out[2], int(E[m - 1][end]), out[3]


def align_phrases(corpus, phrases, spans, free_start=True, scan_over=4096):
    """``UnitIndex.align_phrases`` -> (cols int64 [P, k, Mx], subs int32 [P, k, Mx], ops int32 [P, k, 4], costs int32 [P, k],
    first int64 [P, k]: the first ROW of each path, -1 for padding); windows of more than ``scan_over`` cells go through
    ``window_scan``"""
    corpus = as_units(corpus)
    spans = np.asarray(spans, np.int64)
    P, k = spans.shape[:2]
    phrases = [as_units(p) for p in phrases]
    Mx = max([p.shape[0] for p in phrases], default=0)
    cols, subs = np.full((P, k, Mx), -1, np.int64), np.full((P, k, Mx), -1, np.int32)
    ops, costs = np.zeros((P, k, 4), np.int32), np.full((P, k), PAD, np.int32)
    first = np.full((P, k), -1, np.int64)
    for a in range(P):
        m = phrases[a].shape[0]
        for r in range(k):
            lo, hi = spans[a, r]
            if lo < 0:
                continue
            fn = window_scan if m * (hi - lo) > scan_over else window_loop
            c, s, o, cost, f = fn(phrases[a], corpus[lo:hi], free_start)
            cols[a, r, :m] = np.where(c >= 0, c + lo, -1)
            subs[a, r, :m], ops[a, r], costs[a, r], first[a, r] = s, o, cost, lo + f
    return cols, subs, ops, costs, first

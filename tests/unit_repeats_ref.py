"""numpy restatement of "Unit repeats" (include/sylber_hip.h; sylber_amd.local_align_unit_strings / UnitIndex.find_repeats,
csrc/unit_repeats.hip): the local alignment (Smith-Waterman) of a string ``x`` of ``m`` units and a string ``y`` of ``L`` units,
``0 <= m, L``, all int32 in the contract (int64 here: scores stay below ``64 * 8 * 65 536``)::

    s(i, j)  = match * (W - sub(i, j)) - mismatch * sub(i, j)
    H[i][-1] = H[-1][j] = 0
    c_diag   = H[i-1][j-1] + s(i, j)     start: start[i-1][j-1] if H[i-1][j-1] > 0, else (i, j)
    c_up     = H[i-1][j]   - gap * W     start: start[i-1][j]
    c_left   = H[i][j-1]   - gap * W     start: start[i][j-1]
    v        = the first largest of (c_diag, c_up, c_left), in that order
    H[i][j]  = v if v > 0 else 0         start[i][j] = that candidate's start (unused where H = 0)

The result is the best cell: the largest ``H[i][j]``, then the smallest ``i``, then the smallest ``j`` -> ``score = H[i][j]`` and
``(a0, a1, b0, b1) = (si, i + 1, sj, j + 1)``; score 0 and spans -1 without a positive cell.

``local_align`` walks the table an anti-diagonal at a time -- the cells of one anti-diagonal depend on the two before it only, so
each is a handful of numpy calls on at most ``min(m, L)`` cells and 65 536 x 70 takes seconds.  The cell-by-cell form it is held
against is in tests/test_unit_repeats_ref.py."""
import numpy as np

from unit_search_ref import as_units

DEFAULTS = (2, 3, 4)                                       # match, mismatch, gap


def _pair(x, y):
    """-> (x [m, W], y [L, W], W); an empty side takes the other's width (1 if both are empty)"""
    x, y = as_units(x), as_units(y)
    if x.shape[0] == 0 or y.shape[0] == 0:
        W = x.shape[1] if x.shape[0] else y.shape[1] if y.shape[0] else 1
        x = x if x.shape[0] else np.zeros((0, W), np.int64)
        y = y if y.shape[0] else np.zeros((0, W), np.int64)
    assert x.shape[1] == y.shape[1]
    return x, y, x.shape[1]


def _take(cells, lo, a, b):
    """rows a .. b of an anti-diagonal kept as the cells (H, si, sj) of its rows lo .. lo + len - 1; what lies outside it -- row -1,
    column -1 -- is H = 0"""
    out = np.zeros((b - a + 1, 3), np.int64)
    s, e = max(a, lo), min(b, lo + cells.shape[0] - 1)
    if s <= e:
        out[s - a:e - a + 1] = cells[s - lo:e - lo + 1]
    return out


def local_align(x, y, match=2, mismatch=3, gap=4):
    """-> (score, (a0, a1, b0, b1)) of one pair"""
    x, y, W = _pair(x, y)
    m, L = x.shape[0], y.shape[0]
    if m == 0 or L == 0:
        return 0, (-1, -1, -1, -1)
    best = (0, -1, -1, -1, -1)                             # H, i, j, si, sj
    d1 = d2 = np.zeros((0, 3), np.int64)                   # the anti-diagonals d - 1 and d - 2
    lo1 = lo2 = 0
    for d in range(m + L - 1):
        lo, hi = max(0, d - L + 1), min(m - 1, d)
        i = np.arange(lo, hi + 1)
        j = d - i
        sub = (x[lo:hi + 1] != y[d - hi:d - lo + 1][::-1]).sum(1)
        diag, up, left = _take(d2, lo2, lo - 1, hi - 1), _take(d1, lo1, lo - 1, hi - 1), _take(d1, lo1, lo, hi)
        fresh = diag[:, 0] <= 0
        v = diag[:, 0] + match * (W - sub) - mismatch * sub
        si, sj = np.where(fresh, i, diag[:, 1]), np.where(fresh, j, diag[:, 2])
        for cand in (up, left):
            c = cand[:, 0] - gap * W
            take = c > v
            v, si, sj = np.where(take, c, v), np.where(take, cand[:, 1], si), np.where(take, cand[:, 2], sj)
        v = np.maximum(v, 0)
        top = int(v.max())
        if top > 0 and top >= best[0]:
            e = int(np.argmax(v))                          # the first largest: the smallest i of this anti-diagonal
            cell = (top, lo + e, d - lo - e, int(si[e]), int(sj[e]))
            if top > best[0] or cell[1:3] < best[1:3]:
                best = cell
        d2, lo2, d1, lo1 = d1, lo1, np.stack([v, si, sj], 1), lo
    if best[0] == 0:
        return 0, (-1, -1, -1, -1)
    H, i, j, si, sj = best
    return H, (si, i + 1, sj, j + 1)


def local_align_batch(xs, ys, match=2, mismatch=3, gap=4):
    """every pair, shaped as ``local_align_unit_strings`` returns it -> (scores int32 [S], spans int64 [S, 2, 2])"""
    out = [local_align(x, y, match, mismatch, gap) for x, y in zip(xs, ys)]
    scores = np.array([o[0] for o in out], np.int32)
    spans = np.array([o[1] for o in out], np.int64).reshape(len(out), 2, 2)
    return scores, spans


def find_repeats(seqs, k, min_score=None, match=2, mismatch=3, gap=4, groups=None, offsets=None):
    """``UnitIndex.find_repeats`` over the sequences ``seqs``: every pair s < t, x = sequence s, y = sequence t; ``groups``: one group
    per sequence, pairs inside one group are skipped; kept when ``score >= min_score`` (``None``: ``3 * match * W``); the k best by
    (score descending, s, t), padded with score 0, pairs -1, spans -1; spans as row ids with ``offsets`` (default: the sequences one
    after another) -> (scores int32 [k], pairs int64 [k, 2], spans int64 [k, 2, 2])"""
    seqs = [as_units(s) for s in seqs]
    W = seqs[0].shape[1]
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    if min_score is None:
        min_score = 3 * match * W
    found = []
    for s in range(len(seqs)):
        for t in range(s + 1, len(seqs)):
            if groups is not None and groups[s] == groups[t]:
                continue
            score, (a0, a1, b0, b1) = local_align(seqs[s], seqs[t], match, mismatch, gap)
            if score >= min_score:
                found.append((-score, s, t, a0 + offsets[s], a1 + offsets[s], b0 + offsets[t], b1 + offsets[t]))
    found = sorted(found)[:k]
    scores, pairs, spans = np.zeros(k, np.int32), np.full((k, 2), -1, np.int64), np.full((k, 2, 2), -1, np.int64)
    for e, f in enumerate(found):
        scores[e], pairs[e], spans[e] = -f[0], f[1:3], np.array(f[3:]).reshape(2, 2)
    return scores, pairs, spans

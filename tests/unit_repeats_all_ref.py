"""numpy restatement of "Unit repeats, every one" (include/sylber_hip.h; sylber_amd.local_align_unit_strings_all /
UnitIndex.find_repeats with ``per_pair`` or ``within``, csrc/unit_repeats_all.hip): up to ``n_best`` repeats of a string ``x`` of
``m`` units and a string ``y`` of ``L`` units, round by round.  Round r is the recurrence of tests/unit_repeats_ref.py with one
change: a BLOCKED cell has ``H = 0``, carries no start and is never the best cell.  Cell ``(i, j)`` is blocked when

* ``sep > 0`` and ``j - i < sep`` (the band on and below the diagonal, for a string against itself), or
* ``a0 <= i < a1`` and ``b0 <= j < b1`` for the span ``(a0, a1, b0, b1)`` of an earlier round.

The result of a round is the best unblocked cell -- the largest ``H``, then the smallest ``i``, then the smallest ``j`` --
``score = H[i][j]`` and ``(a0, a1, b0, b1) = (si, i + 1, sj, j + 1)``.  A round whose score is below ``min_score`` ends the pair:
it and every later round are score 0 and spans -1.

``local_align_all`` walks the table an anti-diagonal at a time, as ``unit_repeats_ref.local_align`` does: 300 x 300 x 8 rounds take
well under a second.  The cell-by-cell form it is held against is in tests/test_unit_repeats_all_ref.py."""
import numpy as np

from unit_repeats_ref import _pair, _take
from unit_search_ref import as_units

NONE = (-1, -1, -1, -1)


def _round(x, y, W, match, mismatch, gap, sep, rects):
    """one round -> (H, i, j, si, sj) of the best unblocked cell, H = 0 without a positive one"""
    m, L = x.shape[0], y.shape[0]
    best = (0, -1, -1, -1, -1)
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
        blocked = (j - i < sep) if sep > 0 else np.zeros(i.shape, bool)
        for a0, a1, b0, b1 in rects:
            blocked = blocked | ((i >= a0) & (i < a1) & (j >= b0) & (j < b1))
        v = np.where(blocked, 0, np.maximum(v, 0))
        top = int(v.max())
        if top > 0 and top >= best[0]:
            e = int(np.argmax(v))                          # the first largest: the smallest i of this anti-diagonal
            cell = (top, lo + e, d - lo - e, int(si[e]), int(sj[e]))
            if top > best[0] or cell[1:3] < best[1:3]:
                best = cell
        d2, lo2, d1, lo1 = d1, lo1, np.stack([v, si, sj], 1), lo
    return best


def local_align_all(x, y, n_best, min_score=1, sep=0, match=2, mismatch=3, gap=4):
    """-> (scores [n_best], spans [n_best] of (a0, a1, b0, b1)) of one pair, as lists"""
    x, y, W = _pair(x, y)
    scores, spans = [0] * n_best, [NONE] * n_best
    if x.shape[0] == 0 or y.shape[0] == 0:
        return scores, spans
    rects = []
    for r in range(n_best):
        H, i, j, si, sj = _round(x, y, W, match, mismatch, gap, sep, rects)
        if H < min_score:
            break
        scores[r], spans[r] = H, (si, i + 1, sj, j + 1)
        rects.append(spans[r])
    return scores, spans


def _widths(xs, ys):
    for s in list(xs) + list(ys):
        s = as_units(s)
        if s.shape[0]:
            return s.shape[1]
    return 1


def local_align_all_batch(xs, ys=None, n_best=1, min_score=None, min_sep=1, match=2, mismatch=3, gap=4):
    """every pair, shaped as ``local_align_unit_strings_all`` returns it -> (scores int32 [S, n_best], spans int64 [S, n_best, 2,
    2]); ``ys=None``: every string against itself with ``sep = min_sep``; ``min_score=None``: ``3 * match * W``"""
    sep = min_sep if ys is None else 0
    ys = xs if ys is None else ys
    if min_score is None:
        min_score = 3 * match * _widths(xs, ys)
    out = [local_align_all(x, y, n_best, min_score, sep, match, mismatch, gap) for x, y in zip(xs, ys)]
    scores = np.array([o[0] for o in out], np.int32).reshape(len(out), n_best)
    spans = np.array([o[1] for o in out], np.int64).reshape(len(out), n_best, 2, 2)
    return scores, spans


def find_repeats(seqs, k, min_score=None, match=2, mismatch=3, gap=4, groups=None, offsets=None, per_pair=1, within=False, min_sep=1):
    """``UnitIndex.find_repeats(k, per_pair=, within=, min_sep=)`` over the sequences ``seqs``: every pair s < t, and with ``within``
    every (s, s) with ``sep = min_sep``; ``groups``: one per sequence, pairs s < t inside one group are skipped, (s, s) never is;
    every round with ``score >= min_score`` (``None``: ``3 * match * W``) is a candidate; the k best by (score descending, s, t,
    round), padded with score 0, pairs -1, spans -1; spans as row ids with ``offsets`` (default: the sequences one after another)
    -> (scores int32 [k], pairs int64 [k, 2], spans int64 [k, 2, 2])"""
    seqs = [as_units(s) for s in seqs]
    W = seqs[0].shape[1]
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    if min_score is None:
        min_score = 3 * match * W
    found = []
    for s in range(len(seqs)):
        for t in range(s if within else s + 1, len(seqs)):
            if s != t and groups is not None and groups[s] == groups[t]:
                continue
            scores, spans = local_align_all(seqs[s], seqs[t], per_pair, min_score, min_sep if s == t else 0, match, mismatch, gap)
            for r, (score, (a0, a1, b0, b1)) in enumerate(zip(scores, spans)):
                if score >= min_score:
                    found.append((-score, s, t, r, a0 + offsets[s], a1 + offsets[s], b0 + offsets[t], b1 + offsets[t]))
    found = sorted(found)[:k]
    scores, pairs, spans = np.zeros(k, np.int32), np.full((k, 2), -1, np.int64), np.full((k, 2, 2), -1, np.int64)
    for e, f in enumerate(found):
        scores[e], pairs[e], spans[e] = -f[0], f[1:3], np.array(f[4:]).reshape(2, 2)
    return scores, pairs, spans

"""numpy restatement of the "Embedding strings, local" contract of sylber_amd.local_align_sequences /
SyllableIndex.local_align_sequences (include/sylber_hip.h, csrc/dtw_strings_local.hip), on top of tests/repeats_ref.py's recurrence
and tests/dtw_ref.py's local costs.

A pair is ``x`` of m rows and ``y`` of L rows, ``0 <= m, L <= 65 536``; ``d[i][j]`` is ``search_phrases``'s local cost, a NaN counts
as ``+inf``.  Rounds ``r = 0 .. n_best - 1`` run in order; round r is ``repeats_ref.local_loop``'s recurrence unchanged, in fp32 with
one rounding per operation::

    s  = radius - d[i][j];  sg = s - gap;  H[i][-1] = H[-1][j] = 0
    c_diag = H[i-1][j-1] + s     start: start[i-1][j-1] if H[i-1][j-1] > 0 else (i, j)
    c_up   = H[i-1][j]   + sg    start: start[i-1][j]
    c_left = H[i][j-1]   + sg    start: start[i][j-1]
    v = the first largest of (c_diag, c_up, c_left) in that order; H[i][j] = v if v > 0 else 0

with one addition: a BLOCKED cell has ``H = 0``, carries no start and is never the best cell.  ``(i, j)`` is blocked when ``sep > 0``
and ``j - i < sep``, or when ``a0 <= i < a1`` and ``b0 <= j < b1`` for the spans of an earlier round.  The round's result is the best
cell -- the largest ``H``, then the smallest ``i``, then the smallest ``j`` -- with ``score = H[i][j]`` and the spans ``[si, i + 1)``,
``[sj, j + 1)``.  A round without a positive cell or with ``score < min_score`` ends the pair: it and every later round are score 0
and spans -1.  An empty side gives padding only.

``rounds_loop`` is the contract cell by cell, with the path of every round; ``rounds`` is the same additions one anti-diagonal at a
time in the kernel's shape: super-strips of two 64-row strips, tiles of 128 columns, the row between strips and super-strips handed
on, a best cell per lane under a strict ``>`` reduced by (H descending, i ascending), and the tiles that lie wholly in the band
skipped.  ``strip=None`` walks the whole matrix as one strip and one tile: the same cells, fewer python steps.
tests/test_dtw_strings_local_ref.py holds the two against each other and the contract's consequences.

The DP runs in the dtype it is given: float32 restates the device's arithmetic bit for bit, float64 is the yardstick of the bound."""
import numpy as np

import repeats_ref

STRIP, TILE, PER_SUPER = 64, 128, 2
MAX_BEST = 32

# |score32 - score64| of round 0: ``repeats_ref.score_error_bound`` is derived for a path of at most n = m + L - 1 cells with n taken
# from the shapes it is given, a per-cell error from ``dtw_ref.cost_error_bound``'s terms and one rounding per DP addition; nothing in
# it uses m <= 64, and the band only removes candidates from both runs alike (H = 0 exactly in both).  It holds here as it stands.
score_error_bound = repeats_ref.score_error_bound


def blocked(m, L, sep, rects):
    """bool [m, L]: the cells of the band and of the rectangles ``rects`` = [(a0, a1, b0, b1)]"""
    i, j = np.arange(m)[:, None], np.arange(L)[None, :]
    b = (j - i < sep) if sep > 0 else np.zeros((m, L), bool)
    for a0, a1, b0, b1 in rects:
        b = b | ((i >= a0) & (i < a1) & (j >= b0) & (j < b1))
    return b


def _padding(n_best):
    return np.zeros(n_best, np.float32), np.full((n_best, 2, 2), -1, np.int64)


def rounds_loop(d, radius, gap, min_score, n_best=1, sep=0, dtype=np.float32, _defect=None):
    """the contract cell by cell -> (scores fp32 [n_best], spans int64 [n_best, 2, 2], info): ``info[r]`` of every round that
    returned a result = dict(path = the cells [(i, j)] from the start to the best cell, up / left = the number of such steps on it,
    ties = the cells with v > 0 where c_diag equals c_up or c_left exactly).
    ``_defect`` (tests only) plants one wrong reading of the contract: "rect" (rectangles one row and column short), "band" (<=
    instead of <), "zero_start" (a start inherited from a zero cell), "tie" (the last largest instead of the first)."""
    s, sg = repeats_ref._terms(d, radius, gap, dtype)
    scores, spans = _padding(n_best)
    m, L = (s.shape if s.size else (0, 0))
    info = []
    if m == 0 or L == 0:
        return scores, spans, info
    zero = dtype(0)
    rects = []
    for r in range(n_best):
        shown = [(a0, a1 - 1, b0, b1 - 1) for a0, a1, b0, b1 in rects] if _defect == "rect" else rects
        blk = blocked(m, L, sep + 1 if (_defect == "band" and sep > 0) else sep, shown)
        H = np.zeros((m, L), dtype)
        St = np.zeros((m, L, 2), np.int64)
        pred = np.zeros((m, L), np.int8)                           # 0: the path begins here, 1 diagonal, 2 up, 3 left
        ties = 0
        with np.errstate(invalid="ignore"):
            for i in range(m):
                for j in range(L):
                    if blk[i, j]:
                        continue
                    hd = H[i - 1, j - 1] if i > 0 and j > 0 else zero
                    hu = H[i - 1, j] if i > 0 else zero
                    hl = H[i, j - 1] if j > 0 else zero
                    inherit = hd > 0 or (_defect == "zero_start" and i > 0 and j > 0)
                    v, st, pc = dtype(hd + s[i, j]), (St[i - 1, j - 1] if inherit else (i, j)), (1 if hd > 0 else 0)
                    cu, cl = dtype(hu + sg[i, j]), dtype(hl + sg[i, j])
                    ties += int(v > 0 and (cu == v or cl == v))
                    if cu > v or (_defect == "tie" and cu == v and i > 0):
                        v, st, pc = cu, St[i - 1, j], 2
                    if cl > v or (_defect == "tie" and cl == v and j > 0):
                        v, st, pc = cl, St[i, j - 1], 3
                    if v > 0:
                        H[i, j], St[i, j], pred[i, j] = v, st, pc
        i, j = repeats_ref._best_cell(H)
        if not (H[i, j] > 0 and H[i, j] >= dtype(min_score)):
            break
        scores[r] = H[i, j]
        spans[r] = ((St[i, j, 0], i + 1), (St[i, j, 1], j + 1))
        rects.append((int(St[i, j, 0]), i + 1, int(St[i, j, 1]), j + 1))
        info.append(_walk_back(pred, i, j, ties))
    return scores, spans, info


def _walk_back(pred, i, j, ties):
    """the path that ends in (i, j), from the predecessor codes"""
    path, up, left = [(i, j)], 0, 0
    while pred[i, j] != 0:
        pc = pred[i, j]
        up, left = up + (pc == 2), left + (pc == 3)
        i, j = (i - 1, j - 1) if pc == 1 else ((i - 1, j) if pc == 2 else (i, j - 1))
        path.append((i, j))
    return dict(path=path[::-1], up=int(up), left=int(left), ties=ties)


def _round(s, sg, sep, rects, strip, tile, per_super, dtype, pred=None):
    """one round in the kernel's shape -> (H, i, j, start) of the best cell (H = 0: none) and the number of exact ties; ``pred``
    int8 [m, L], where given, takes the predecessor of every cell walked (0: the path begins here, 1 diagonal, 2 up, 3 left)"""
    m, L = s.shape
    ties = 0
    SR, tiles = strip * per_super, -(-L // tile)
    zero = dtype(0)
    lb_h, lb_i = np.zeros(SR, dtype), np.full(SR, np.iinfo(np.int64).max, np.int64)      # a lane's best: (H, i, j, start)
    lb_j, lb_t = np.zeros(SR, np.int64), np.zeros(SR, np.int64)
    car_h, car_t = np.zeros(L, dtype), np.zeros(L, np.int64)       # the row above the super-strip: the row above the matrix is H = 0
    with np.errstate(invalid="ignore"):
        for i0 in range(0, m, SR):
            ms = min(SR, m - i0)
            band = sep + i0 - (tile - 1)
            ft = min(-(-band // tile), tiles) if sep > 0 and band > 0 else 0   # the tiles wholly inside the band: n0 + tile - 1 - i0 < sep
            up_h, up_t = car_h, car_t
            for w in range(per_super):
                rw = min(max(ms - w * strip, 0), strip)
                if rw == 0:
                    break
                lanes = w * strip + np.arange(rw)
                ii = i0 + lanes
                in_rows = [q for q, (a0, a1, _, _) in enumerate(rects) if ii[0] < a1 and ii[-1] >= a0]
                h1, h2, t1, t2 = np.zeros(rw, dtype), np.zeros(rw, dtype), np.zeros(rw, np.int64), np.zeros(rw, np.int64)
                pa, pt = zero, 0                                   # lane 0: the previous cell of the row above; column -1 is 0
                if 0 < ft < tiles and w == 0 and i0 > 0:
                    pa, pt = up_h[ft * tile - 1], up_t[ft * tile - 1]
                out_h, out_t = np.zeros(L, dtype), np.zeros(L, np.int64)    # the strip's last row; zeros where a tile is skipped
                for tl in range(ft, tiles):
                    n0 = tl * tile
                    ncol = min(tile, L - n0)
                    for st in range(ncol + rw - 1):
                        j = st - np.arange(rw)
                        ok = (j >= 0) & (j < ncol)
                        gj = n0 + np.clip(j, 0, ncol - 1)
                        uh, uhp = np.concatenate([[zero], h1[:-1]]).astype(dtype), np.concatenate([[zero], h2[:-1]]).astype(dtype)
                        ut, utp = np.concatenate([[0], t1[:-1]]), np.concatenate([[0], t2[:-1]])
                        if ok[0]:
                            uh[0], ut[0], uhp[0], utp[0] = up_h[gj[0]], up_t[gj[0]], pa, pt
                            pa, pt = uh[0], ut[0]
                        sv, sgv = s[ii, gj], sg[ii, gj]
                        cd = (uhp + sv).astype(dtype)
                        v, code = cd.copy(), (uhp > 0).astype(np.int8)
                        tt = np.where(uhp > 0, utp, (ii << 32) | gj)
                        cu = (uh + sgv).astype(dtype)
                        mk = cu > v
                        v[mk], tt[mk], code[mk] = cu[mk], ut[mk], 2
                        cl = (h1 + sgv).astype(dtype)
                        mk = cl > v
                        v[mk], tt[mk], code[mk] = cl[mk], t1[mk], 3
                        H = np.where(v > 0, v, zero).astype(dtype)
                        blk = (gj - ii < sep) if sep > 0 else np.zeros(rw, bool)
                        for q in in_rows:
                            a0, a1, b0, b1 = rects[q]
                            blk = blk | ((ii >= a0) & (ii < a1) & (gj >= b0) & (gj < b1))
                        H[blk] = zero
                        ties += int((ok & ~blk & (cd > 0) & ((cu == cd) | (cl == cd))).sum())
                        if pred is not None:
                            pred[ii[ok], gj[ok]] = np.where(H[ok] > 0, code[ok], 0)
                        h2[ok], t2[ok] = h1[ok], t1[ok]
                        h1[ok], t1[ok] = H[ok], tt[ok]
                        bt = ok & (H > lb_h[lanes])                # strict: rows ascend, columns ascend inside a row
                        lb_h[lanes[bt]], lb_i[lanes[bt]], lb_j[lanes[bt]], lb_t[lanes[bt]] = H[bt], ii[bt], gj[bt], tt[bt]
                        if rw == strip and ok[-1]:                 # a blocked cell still writes its H = 0
                            out_h[gj[-1]], out_t[gj[-1]] = H[-1], tt[-1]
                up_h, up_t = out_h, out_t
            car_h, car_t = up_h, up_t
    o = np.lexsort((lb_i, -lb_h.astype(np.float64)))[0]            # H descending, i ascending: two lanes never hold the same row
    return lb_h[o], int(lb_i[o]), int(lb_j[o]), int(lb_t[o]), ties


def rounds(d, radius, gap, min_score, n_best=1, sep=0, dtype=np.float32, strip=STRIP, tile=TILE, per_super=PER_SUPER, info=False):
    """the contract in the kernel's shape (see the module docstring) -> (scores fp32 [n_best], spans int64 [n_best, 2, 2]), with
    ``info`` also ``rounds_loop``'s third result; ``strip=None``: the whole matrix as one strip and one tile"""
    s, sg = repeats_ref._terms(d, radius, gap, dtype)
    scores, spans = _padding(n_best)
    m, L = (s.shape if s.size else (0, 0))
    infos = []
    if m == 0 or L == 0:
        return (scores, spans, infos) if info else (scores, spans)
    if strip is None:
        strip, tile, per_super = m, L, 1
    rects = []
    for r in range(n_best):
        pred = np.zeros((m, L), np.int8) if info else None
        h, i, j, t, ties = _round(s, sg, int(sep), rects, strip, tile, per_super, dtype, pred)
        if not (h > 0 and h >= dtype(min_score)):
            break
        si, sj = t >> 32, t & 0xffffffff
        scores[r], spans[r] = h, ((si, i + 1), (sj, j + 1))
        rects.append((si, i + 1, sj, j + 1))
        if info:
            infos.append(_walk_back(pred, i, j, ties))
    return (scores, spans, infos) if info else (scores, spans)


def planted(rng, m, L, D, copies, integer, noise=0.05):
    """a pair with planted repeats -> (x [m, D], y [L, D] fp32): ``copies`` = [(a, n, b, how)]: rows ``x[a : a + n]`` are written
    into y from row b on; how = "same", "drop" (one row of the copy left out: the path takes an up step) or "double" (the middle
    row said twice: a left step; and rows 0 and 1 said twice, n + 3 rows in all: where d is exact, the second x[a] ties c_left with
    c_diag at gap = radius and the second x[a + 1] at gap = 2 radius).  Integer rows are in -2 .. 2 and copied exactly, gaussian
    copies get a little noise."""
    if integer:
        x, y = (rng.integers(-2, 3, (n, D)).astype(np.float32) for n in (m, L))
    else:
        x, y = (rng.standard_normal((n, D)).astype(np.float32) for n in (m, L))
    for a, n, b, how in copies:
        c = x[a:a + n].copy()
        if how == "drop":
            c = np.delete(c, n // 2, 0)
        elif how == "double":
            for q in sorted({n // 2, 1, 0} & set(range(n)), reverse=True):
                c = np.insert(c, q, c[q], 0)
        if not integer:
            c = (c + noise * rng.standard_normal(c.shape)).astype(np.float32)
        assert b + len(c) <= L and a + n <= m
        y[b:b + len(c)] = c
    return x, y


def assert_not_vacuous(d, radius, gap, min_score, n_best, copies, sep=0, need_ties=True):
    """what the reference alone must give on a planted case, so that a kernel returning round 0 only, or diagonal paths only, cannot
    pass: round 0 positive, as many rounds at or above ``min_score`` as copies planted, a path with an up step and one with a left
    step where a copy was planted by dropping / doubling a row, and an exact tie between c_diag and c_up or c_left
    -> (scores, spans, info) of ``rounds`` on the whole matrix, which is ``rounds_loop``'s"""
    scores, spans, info = rounds(d, radius, gap, min_score, n_best, sep, strip=None, info=True)
    assert scores[0] > 0
    assert len(info) >= min(len(copies), n_best), (len(info), len(copies))
    hows = {c[3] for c in copies}
    if n_best >= len(copies):
        assert "drop" not in hows or any(p["up"] for p in info)
        assert "double" not in hows or any(p["left"] for p in info)
    assert not need_ties or any(p["ties"] for p in info)
    return scores, spans, info

"""numpy restatement of the phrase-search contract of sylber_amd.SyllableIndex.search_phrases / csrc/dtw.hip.

Local cost of phrase row i against database row j, in fp32, from the score ``s = fmaf(-2, q_i . x_j, c_j)`` of ``search`` (same
contraction, same bits):

* ``"l2"``: ``d = max(0, ||q_i||^2 + s)``, i.e. exactly the score ``search`` reports;
* ``"cosine"``: phrase rows are made unit rows as ``search`` does; ``d = max(0, 1 - (-s / 2))`` (the halving is exact, the
  subtraction rounds once);
* a NaN ``d`` (a NaN row on either side) counts as ``+inf``.

Subsequence DTW of a phrase of m rows against a sequence with columns j = 0 .. L - 1 (the phrase is consumed whole, its span in the
sequence is free), all additions in fp32, one per cell::

    A[0][j] = d[0][j]                                   start[0][j] = j
    A[i][j] = d[i][j] + min(A[i-1][j-1], A[i-1][j], A[i][j-1])      (terms outside the sequence are +inf)
              on equal values the predecessor is taken in that order: diagonal, then (i-1, j), then (i, j-1);
              start[i][j] = start of the predecessor taken
    cost = min_j A[m-1][j], the smallest such j on ties = end;   span = (row of start[m-1][end], row of end + 1)

A sequence whose cost is ``+inf`` is never returned.  Each phrase's list is ordered by (cost, sequence number) ascending, the strict
order ``search`` uses; lists with fewer than k admissible sequences end in cost ``+inf``, sequence -1, span (-1, -1).  Because fp32
``+`` and ``min`` in a fixed cell order are deterministic, the result is unique.  ``m > L`` is legal (vertical steps).  No
normalisation by path length.

The DP here runs in the dtype it is given: float32 restates the device's arithmetic bit for bit (numpy's fp32 ``+`` is IEEE, one
rounding), float64 is the yardstick of the error bound."""
import numpy as np

import knn_ref


def sequences_from_groups(g):
    """default sequence offsets [S + 1]: the maximal runs of consecutive rows with equal group, in row order"""
    g = np.asarray(g)
    if g.size == 0:
        return np.zeros(1, np.int64)
    return np.concatenate([[0], np.nonzero(g[1:] != g[:-1])[0] + 1, [g.size]]).astype(np.int64)


def local_costs(q, x, metric="l2"):
    """float64 d [m, L] from the rows as the index holds them (for "cosine": unit rows on both sides, not normalised again)"""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        if metric == "cosine":
            v = 1.0 - q @ x.T
        else:
            v = (q * q).sum(1)[:, None] + knn_ref.scores(q, x, "l2")
        return np.where(np.isnan(v), np.inf, np.maximum(0.0, v))


def _clean(d, dtype):
    d = np.array(d, dtype=dtype, ndmin=2)
    d[np.isnan(d)] = np.inf
    return d


def dtw_loop(d, dtype=np.float32):
    """the recurrence cell by cell, as the contract writes it -> (cost, start column, end column, A [m, L])"""
    d = _clean(d, dtype)
    m, L = d.shape
    inf = dtype(np.inf)
    A = np.full((m, L), inf, dtype)
    S = np.zeros((m, L), np.int64)
    for i in range(m):
        for j in range(L):
            if i == 0:
                A[i, j], S[i, j] = d[i, j], j
                continue
            best, bs = (A[i - 1, j - 1], S[i - 1, j - 1]) if j > 0 else (inf, 0)
            if A[i - 1, j] < best:
                best, bs = A[i - 1, j], S[i - 1, j]
            if j > 0 and A[i, j - 1] < best:
                best, bs = A[i, j - 1], S[i, j - 1]
            A[i, j], S[i, j] = dtype(d[i, j] + best), bs
    end = int(np.argmin(A[m - 1]))                       # the first smallest
    return A[m - 1, end], int(S[m - 1, end]), end, A


def dtw(d, dtype=np.float32):
    """the same recurrence, the same additions, evaluated one anti-diagonal at a time (cells of one anti-diagonal do not depend on each
    other) -> (cost, start column, end column)"""
    d = _clean(d, dtype)
    m, L = d.shape
    inf = dtype(np.inf)
    ii = np.arange(m)
    p1, p2 = np.full(m, inf, dtype), np.full(m, inf, dtype)        # A[i][t - 1 - i], A[i][t - 2 - i]
    s1, s2 = np.zeros(m, np.int64), np.zeros(m, np.int64)
    last, lstart = np.full(L, inf, dtype), np.zeros(L, np.int64)
    for t in range(m + L - 1):
        j = t - ii
        ok = (j >= 0) & (j < L)
        dv = d[ii, np.clip(j, 0, L - 1)]
        best = np.concatenate([[inf], p2[:-1]]).astype(dtype)      # diagonal
        bs = np.concatenate([[0], s2[:-1]])
        up, su = np.concatenate([[inf], p1[:-1]]).astype(dtype), np.concatenate([[0], s1[:-1]])
        mk = up < best
        best[mk], bs[mk] = up[mk], su[mk]
        mk = p1 < best                                             # left
        best[mk], bs[mk] = p1[mk], s1[mk]
        cur = (dv + best).astype(dtype)
        cur[0], bs[0] = dv[0], j[0]
        cur[~ok] = inf
        if ok[m - 1]:
            last[j[m - 1]], lstart[j[m - 1]] = cur[m - 1], bs[m - 1]
        p2, s2, p1, s1 = p1, s1, cur, bs
    end = int(np.argmin(last))
    return last[end], int(lstart[end]), end


def brute_force(d, dtype=np.float64):
    """the minimum over every warping path (steps (1,1), (1,0), (0,1), free start and end column) of the sum of its cells, accumulated
    cell by cell from the path's first cell in ``dtype``.  Tiny cases only."""
    d = _clean(d, dtype)
    m, L = d.shape
    best = [dtype(np.inf)]

    def walk(i, j, acc):
        if i == m - 1:
            best[0] = min(best[0], acc)
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            a, b = i + di, j + dj
            if a < m and b < L:
                walk(a, b, dtype(acc + d[a, b]))

    for j0 in range(L):
        walk(0, j0, d[0, j0])
    return best[0]


def rank(costs, starts, ends, offsets, k, admissible=None):
    """one phrase's list from its per-sequence results (columns relative to each sequence) -> (costs [k], seqs [k], spans [k, 2])"""
    costs = np.asarray(costs)
    S = costs.size
    adm = np.ones(S, bool) if admissible is None else np.asarray(admissible, bool)
    s = np.nonzero(adm & (costs < np.inf))[0]
    s = s[np.lexsort((s, costs[s]))][:k]
    oc = np.full(k, np.inf, costs.dtype)
    os_ = np.full(k, -1, np.int64)
    sp = np.full((k, 2), -1, np.int64)
    oc[:s.size], os_[:s.size] = costs[s], s
    sp[:s.size, 0] = np.asarray(offsets)[s] + np.asarray(starts)[s]
    sp[:s.size, 1] = np.asarray(offsets)[s] + np.asarray(ends)[s] + 1
    return oc, os_, sp


def search_phrases(d_of, phrase_count, offsets, k, dtype=np.float32, phrase_groups=None, seq_groups=None):
    """the whole contract from a function ``d_of(p, s) -> d [m_p, L_s]`` -> (costs [P, k], seqs [P, k], spans [P, k, 2])"""
    S = len(offsets) - 1
    C, Q, SP = [], [], []
    for p in range(phrase_count):
        r = [dtw(d_of(p, s), dtype) for s in range(S)]
        adm = None if phrase_groups is None else np.asarray(seq_groups) != phrase_groups[p]
        c, q, sp = rank(np.array([x[0] for x in r], dtype), [x[1] for x in r], [x[2] for x in r], offsets, k, adm)
        C.append(c); Q.append(q); SP.append(sp)
    return np.stack(C), np.stack(Q), np.stack(SP)


def cost_error_bound(q, x, cost64, metric="l2"):
    """an upper bound on |cost32 - cost64| of one phrase (rows q [m, D]) against one sequence (rows x [L, D]), both as the index holds
    them.  A path has at most n = m + L - 1 cells.  Each cell's d is off by at most e_d = knn_ref.dot_error_bound (the score s) plus
    gamma_D ||q||^2 (the fp32 row norm; L2 only) plus one rounding of the add to ||q||^2 / of 1 - sim (u d); max(0, .) is 1-Lipschitz.
    Each DP addition rounds once, so along a path |f32 - f64| <= E + gamma_n (f64 + E) with E = n e_d.  min over paths is 1-Lipschitz
    in those errors: cost32 - cost64 <= that at the float64-optimal path (f64 = cost64), and cost64 - cost32 <= that at the
    fp32-optimal path, whose f64 <= (cost64 + E (1 + gamma_n)) / (1 - gamma_n) when cost32 < cost64.  The second is the larger."""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    m, D = q.shape
    n = m + x.shape[0] - 1
    u = 2.0 ** -24
    gD, gn = D * u / (1 - D * u), n * u / (1 - n * u)
    e0 = float(np.nanmax(knn_ref.dot_error_bound(q, x))) + (gD * float((q * q).sum(1).max()) if metric == "l2" else 0.0)
    d = local_costs(q, x, metric)
    dmax = float(d[np.isfinite(d)].max()) if np.isfinite(d).any() else 0.0
    e_d = e0 + u * (dmax + e0)
    E = n * e_d
    return E + gn * ((cost64 + E * (1 + gn)) / (1 - gn) + E)

"""numpy restatement of the "Embedding repeats" contract of sylber_amd.SyllableIndex.search_repeats / find_repeats
(include/sylber_hip.h, csrc/dtw_local.hip), on top of tests/dtw_ref.py's local costs.

A probe is m rows (1 <= m <= 64), a sequence a run of rows of the index.  The local cost ``d[i][j]`` is ``search_phrases``'s, word
for word; a NaN ``d`` counts as ``+inf``.  ``radius > 0`` and ``gap >= 0`` are finite fp32.  Everything is in fp32 with one rounding
per operation, exactly as written::

    s  = radius - d[i][j]            (-inf where d = +inf)
    sg = s - gap
    H[i][-1] = H[-1][j] = 0
    c_diag = H[i-1][j-1] + s     start: start[i-1][j-1] if H[i-1][j-1] > 0 else (i, j)
    c_up   = H[i-1][j]   + sg    start: start[i-1][j]
    c_left = H[i][j-1]   + sg    start: start[i][j-1]
    v = the first largest of (c_diag, c_up, c_left) in that order; H[i][j] = v if v > 0 else 0

Result of (probe, sequence): the best cell -- the largest ``H``, then the smallest ``i``, then the smallest ``j``; ``score =
H[i][j]``; the probe span is ``[si, i + 1)``, the sequence span ``[sj, j + 1)``, ``(si, sj) = start[i][j]``.  No positive cell: no
result.  Per probe an admissible result has ``score >= min_score``; the k best admissible sequences are ordered strictly by (score
descending, sequence ascending); padding is score 0, sequence -1, spans -1.

Two facts (tests/test_repeats_ref.py holds them):

* a predecessor with ``H = 0`` is never strictly better through ``c_up`` / ``c_left`` than ``c_diag`` (``gap >= 0``), so ``start``
  is only ever read from a positive cell, both spans are non-empty and the first cell of a path has ``s > 0``;
* fp32 addition is monotone, so ``H[i][j]`` is the maximum over paths of the path's left-to-right fp32 sum: restricting the probe
  to a sub-range of its rows never raises a score, and a path that lies inside the sub-range keeps its bits.

``find_repeats`` takes windows of the index's own sequences as probes (``windows``), aligns a window of sequence ``s`` against the
sequences ``t > s``, keeps per pair the best window (score descending, then the smallest window) and returns the k best pairs by
(score descending, s, t).  Window theorem: if the best path of the whole sequence ``s`` against ``t`` covers at most ``window - hop
+ 1`` rows of ``s``, that is what ``find_repeats`` returns, bit for bit; otherwise its score is never larger.

The DP runs in the dtype it is given: float32 restates the device's arithmetic bit for bit, float64 is the yardstick of the bound."""
import numpy as np

import dtw_ref
import knn_ref


def _terms(d, radius, gap, dtype):
    d = np.array(d, dtype=dtype, ndmin=2)
    d[np.isnan(d)] = np.inf
    s = (dtype(radius) - d).astype(dtype)
    return s, (s - dtype(gap)).astype(dtype)


def _best_cell(H):
    """the largest H, then the smallest i, then the smallest j: the first largest in row-major order"""
    i, j = np.unravel_index(int(np.argmax(H)), H.shape)
    return int(i), int(j)


def local_loop(d, radius, gap, dtype=np.float32):
    """the recurrence cell by cell, as the contract writes it -> (score, (si, i + 1), (sj, j + 1), H [m, L], read [m, L]); score 0
    and spans None without a positive cell.  ``read[i][j]``: the H of the predecessor whose start the cell took (1 where it began)."""
    s, sg = _terms(d, radius, gap, dtype)
    m, L = s.shape
    zero = dtype(0)
    H = np.zeros((m, L), dtype)
    St = np.zeros((m, L, 2), np.int64)
    read = np.ones((m, L), dtype)
    for i in range(m):
        for j in range(L):
            hd = H[i - 1, j - 1] if i > 0 and j > 0 else zero
            hu = H[i - 1, j] if i > 0 else zero
            hl = H[i, j - 1] if j > 0 else zero
            v, st, rd = dtype(hd + s[i, j]), ((St[i - 1, j - 1]) if hd > 0 else (i, j)), (hd if hd > 0 else dtype(1))
            c = dtype(hu + sg[i, j])
            if c > v:
                v, st, rd = c, St[i - 1, j], hu
            c = dtype(hl + sg[i, j])
            if c > v:
                v, st, rd = c, St[i, j - 1], hl
            H[i, j] = v if v > 0 else zero
            St[i, j] = st
            read[i, j] = rd
    i, j = _best_cell(H)
    if not H[i, j] > 0:
        return zero, None, None, H, read
    return H[i, j], (int(St[i, j, 0]), i + 1), (int(St[i, j, 1]), j + 1), H, read


def local(d, radius, gap, dtype=np.float32):
    """the same recurrence, the same additions, one anti-diagonal at a time, with the per-row best and the gather over rows that the
    kernel uses (a row keeps its best cell under a strict >, rows are combined with the upper row winning ties)
    -> (score, (si, i + 1), (sj, j + 1)); score 0 and spans None without a positive cell"""
    s, sg = _terms(d, radius, gap, dtype)
    m, L = s.shape
    ii = np.arange(m)
    h1, h2 = np.zeros(m, dtype), np.zeros(m, dtype)                # H[i][t - 1 - i], H[i][t - 2 - i]
    t1, t2 = np.zeros(m, np.int64), np.zeros(m, np.int64)          # their starts: si << 32 | sj
    bh, bt, bj = np.zeros(m, dtype), np.zeros(m, np.int64), np.zeros(m, np.int64)
    z = np.zeros(1, dtype)
    zi = np.zeros(1, np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(m + L - 1):
            j = t - ii
            ok = (j >= 0) & (j < L)
            jc = np.clip(j, 0, L - 1)
            sv, sgv = s[ii, jc], sg[ii, jc]
            hd, td = np.concatenate([z, h2[:-1]]), np.concatenate([zi, t2[:-1]])
            hu, tu = np.concatenate([z, h1[:-1]]), np.concatenate([zi, t1[:-1]])
            v = (hd + sv).astype(dtype)
            tt = np.where(hd > 0, td, (ii << 32) | jc)
            c = (hu + sgv).astype(dtype)
            mk = c > v
            v[mk], tt[mk] = c[mk], tu[mk]
            c = (h1 + sgv).astype(dtype)
            mk = c > v
            v[mk], tt[mk] = c[mk], t1[mk]
            H = np.where(ok & (v > 0), v, dtype(0)).astype(dtype)
            up = H > bh
            bh[up], bt[up], bj[up] = H[up], tt[up], j[up]
            h2, t2, h1, t1 = h1, t1, H, tt
    i = int(np.argmax(bh))                                         # the first largest: the upper row on ties
    if not bh[i] > 0:
        return dtype(0), None, None
    return bh[i], (int(bt[i] >> 32), i + 1), (int(bt[i] & 0xffffffff), int(bj[i]) + 1)


def brute_force(d, radius, gap, dtype=np.float64):
    """the maximum over every path (steps (1,1), (1,0), (0,1); any first cell, any last cell) of the path's left-to-right sum in
    ``dtype``: the first cell's s, then s for a diagonal step and sg for another; 0 if no path is positive.  Tiny cases only."""
    s, sg = _terms(d, radius, gap, dtype)
    m, L = s.shape
    best = [dtype(0)]

    def walk(i, j, acc):
        if acc > best[0]:
            best[0] = acc
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            a, b = i + di, j + dj
            if a < m and b < L:
                walk(a, b, dtype(acc + (s[a, b] if di and dj else sg[a, b])))

    with np.errstate(invalid="ignore"):
        for i0 in range(m):
            for j0 in range(L):
                walk(i0, j0, dtype(dtype(0) + s[i0, j0]))
    return best[0]


def rank(results, offsets, k, min_score, admissible=None):
    """one probe's list from its per-sequence ``local`` results -> (scores fp32 [k], seqs [k], spans [k, 2, 2])"""
    sc = np.array([r[0] for r in results], np.float32)
    adm = np.ones(sc.size, bool) if admissible is None else np.asarray(admissible, bool)
    s = np.nonzero(adm & (sc > 0) & (sc >= np.float32(min_score)))[0]
    s = s[np.lexsort((s, -sc[s].astype(np.float64)))][:k]
    o_sc, o_sq, o_sp = np.zeros(k, np.float32), np.full(k, -1, np.int64), np.full((k, 2, 2), -1, np.int64)
    for r, q in enumerate(s):
        o_sc[r], o_sq[r] = sc[q], q
        o_sp[r, 0] = results[q][1]
        o_sp[r, 1] = np.asarray(results[q][2]) + int(offsets[q])
    return o_sc, o_sq, o_sp


def search_repeats(d_of, probe_count, offsets, k, radius, gap, min_score, dtype=np.float32, probe_groups=None, seq_groups=None,
                   after=None):
    """the whole contract from ``d_of(p, s) -> d [m_p, L_s]`` -> (scores [P, k], seqs [P, k], spans [P, k, 2, 2], positive [P, S]);
    ``after[p]``: sequences numbered <= after[p] are not admissible; ``positive``: which pairs have a positive cell at all"""
    S = len(offsets) - 1
    out, pos = [], np.zeros((probe_count, S), bool)
    for p in range(probe_count):
        first = 0 if after is None else int(after[p]) + 1
        res = [local(d_of(p, s), radius, gap, dtype) if s >= first else (dtype(0), None, None) for s in range(S)]
        pos[p] = [r[0] > 0 for r in res]
        adm = np.arange(S) >= first
        if probe_groups is not None:
            adm &= np.asarray(seq_groups) != probe_groups[p]
        out.append(rank(res, offsets, k, min_score, adm))
    return tuple(np.stack([o[a] for o in out]) for a in range(3)) + (pos,)


def windows(L, window, hop):
    """the first rows (relative to the sequence) of the windows of a sequence of L rows, each min(window, L) rows long"""
    n = 1 if L <= window else -(-(L - window) // hop) + 1
    return [min(r * hop, max(L - window, 0)) for r in range(n)]


def find_repeats(d, offsets, k, radius, gap, min_score, window=64, hop=32, groups=None, dtype=np.float32):
    """the contract of ``find_repeats`` from ``d [N, N]``, the local cost of every row (as a probe row) against every row
    -> (scores [k], pairs [k, 2], spans [k, 2, 2])"""
    S = len(offsets) - 1
    best = {}
    for s in range(S - 1):
        L = int(offsets[s + 1] - offsets[s])
        for w in windows(L, window, hop):
            a = int(offsets[s]) + w
            rows = slice(a, a + min(window, L))
            for t in range(s + 1, S):
                if groups is not None and groups[offsets[s]] == groups[offsets[t]]:
                    continue
                sc, pa, pb = local(d[rows, offsets[t]:offsets[t + 1]], radius, gap, dtype)
                if sc > 0 and sc >= np.float32(min_score) and ((s, t) not in best or sc > best[(s, t)][0]):   # strict: the smallest window
                    best[(s, t)] = (sc, (pa[0] + a, pa[1] + a), (pb[0] + int(offsets[t]), pb[1] + int(offsets[t])))
    order = sorted(best, key=lambda st: (-float(best[st][0]), st))[:k]
    scores, pairs, spans = np.zeros(k, np.float32), np.full((k, 2), -1, np.int64), np.full((k, 2, 2), -1, np.int64)
    for r, st in enumerate(order):
        scores[r], pairs[r], spans[r] = best[st][0], st, best[st][1:]
    return scores, pairs, spans


def local_costs32(q, x, metric="l2"):
    """fp32 ``d [m, L]`` from the rows as the index holds them, with the roundings of the device's formula (a dot product in fp32,
    -2 dot + c_j, then the L2 / cosine forms); the summation order is numpy's, which ``knn_ref.dot_error_bound`` covers like any"""
    q, x = np.asarray(q, np.float32), np.asarray(x, np.float32)
    one, two, half, zero = (np.float32(v) for v in (1, 2, 0.5, 0))
    with np.errstate(invalid="ignore"):
        dot = (q @ x.T).astype(np.float32)
        if metric == "cosine":
            v = one - (zero - half * (-two * dot))
        else:
            v = (q * q).sum(1, dtype=np.float32)[:, None] + (-two * dot + (x * x).sum(1, dtype=np.float32)[None, :])
        return np.where(np.isnan(v), np.float32(np.inf), np.maximum(zero, v)).astype(np.float32)


def score_error_bound(q, x, score64, radius, gap, metric="l2"):
    """an upper bound on |score32 - score64| of one probe (rows q [m, D]) against one sequence (rows x [L, D]), both as the index
    holds them, derived like ``dtw_ref.cost_error_bound``.  A path has at most n = m + L - 1 cells.

    Per cell: d is off by at most e_d (``dtw_ref.cost_error_bound``'s: the score's dot-product error, the fp32 row norm under L2,
    one rounding of the add to ||q||^2 / of 1 - sim; max(0, .) is 1-Lipschitz).  ``radius - d`` rounds once, at most u a with a =
    radius + dmax + e_d, and ``s - gap`` once more, at most u (a (1 + u) + gap): a term is off by at most e_c = e_d + those two.

    Per DP addition: H = max(0, max_k (pred_k + term_k)), and for a maximum only the candidate that wins in one of the two runs
    matters.  Where it wins in fp32 with a value <= 0 there is nothing to show; else its rounded value is at most the table's best,
    so the rounding is at most u' Hmax (u' = u (1 + u)).  Where it wins in float64 (value v64 > 0) the fp32 sum of the same
    candidate is at most v64 + delta + e_c in size.  With delta_t the largest |H32 - H64| over cells t steps deep,
    delta_{t+1} <= delta_t + e_c + u' (Hmax + delta_t + e_c), Hmax <= score64 + delta_n, so over n steps
    delta_n <= n (e_c (1 + u') + u' score64) / (1 - 2 n u').  The score is a maximum over cells: 1-Lipschitz again."""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    m, D = q.shape
    n = m + x.shape[0] - 1
    u = 2.0 ** -24
    u1 = u * (1 + u)
    gD = D * u / (1 - D * u)
    e0 = float(np.nanmax(knn_ref.dot_error_bound(q, x))) + (gD * float((q * q).sum(1).max()) if metric == "l2" else 0.0)
    d = dtw_ref.local_costs(q, x, metric)
    dmax = float(d[np.isfinite(d)].max()) if np.isfinite(d).any() else 0.0
    e_d = e0 + u * (dmax + e0)
    a = float(radius) + dmax + e_d
    e_c = e_d + u * a + u * (a * (1 + u) + float(gap))
    return n * (e_c * (1 + u1) + u1 * float(score64)) / (1 - 2 * n * u1)


def float64_case(metric_seed=11):
    """the inputs of the float64 check, shared by the CPU and the GPU test: (x [N, 768], offsets, probes, the radius of each metric)"""
    rng = np.random.default_rng(metric_seed)
    D = 768
    lens = rng.integers(5, 200, 24)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(offsets[-1])
    x = rng.standard_normal((N, D)).astype(np.float32)
    probes = []
    for m in (3, 8, 20, 64):
        a = int(rng.integers(0, N - m))
        probes.append((x[a:a + m] + 0.5 * rng.standard_normal((m, D))).astype(np.float32))
    # d of a noisy copy is about 0.25 D (L2) / 0.1 (cosine), of unrelated rows about 2 D / 1
    return x, offsets, probes, {"l2": np.float32(600.0), "cosine": np.float32(0.4)}

"""numpy restatement of the two-stage phrase-search contract of sylber_amd.SyllableIndex.search_phrases_refined / csrc/dtw16.hip,
built on dtw_ref (the recurrence, the ranking), knn16_ref (the 16-bit rounding, the coarse score) and knn_ref.

    stage 1:  q~ = round16(q), x~ = round16(x)      (phrase rows prepared as search_phrases prepares them: unit rows under "cosine")
              t(i, j) = c_j - 2 q~_i . x~_j           (knn16_ref.coarse_scores: c_j = ||x_j||^2 of the UNROUNDED row, 0 under cosine)
              d~ = max(0, ||q_i||^2 + t)  (l2, ||q_i||^2 of the UNROUNDED phrase row)   |   max(0, 1 - (-t / 2))  (cosine);  NaN -> +inf
              coarse cost of (phrase, sequence) = dtw_ref's recurrence over d~, min_j A[m-1][j]
              candidates of a phrase = the m = k * refine best admissible sequences under (coarse cost, sequence number);
              a cost of +inf and (with groups) the phrase's own group are not admissible
    stage 2:  dtw_ref's exact (cost, start, end) for each candidate, ordered by (cost, sequence), the best k reported and padded as
              dtw_ref.search_phrases reports them

Everything here is float64: the GPU's coarse cost differs from it by the fp32 accumulation of dot16, the fp32 ||q_i||^2, the rounding
of d~ and one rounding per DP addition, which ``coarse_cost_error_bound`` bounds.  Functions take the rows *as the index holds
them* (``stored``: unit rows on both sides under "cosine") unless they say otherwise."""
import functools

import numpy as np

import dtw_ref as DR
import knn16_ref as K16
import knn_ref as KR  # noqa: F401  (the exact score of stage 2 comes through dtw_ref.local_costs -> knn_ref.scores)

STORAGES = K16.STORAGES


def stored(phrases, x, metric):
    """raw phrases (a list of [m_p, D]) and raw rows -> the fp32 rows the index scores and holds (unit rows for cosine)"""
    if metric == "cosine":
        return [KR.unit_rows(p).astype(np.float32) for p in phrases], KR.unit_rows(x).astype(np.float32)
    return [np.asarray(p, np.float32) for p in phrases], np.asarray(x, np.float32)


def coarse_local_costs(q, x, storage, metric="l2"):
    """float64 d~ [m, L] on the round16 operands, from stored rows q [m, D] and x [L, D]"""
    t = K16.coarse_scores(q, x, storage, metric)
    q64 = np.asarray(q, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (q64 * q64).sum(1)[:, None] + t if metric == "l2" else 1.0 - (-0.5 * t)
        return np.where(np.isnan(v), np.inf, np.maximum(0.0, v))


def coarse_cost_error_bound(q, x, cost64, storage, metric="l2"):
    """an upper bound on |coarse cost in fp32 - coarse cost in float64| of one phrase (stored rows q [m, D]) against one sequence
    (stored rows x [L, D]): dtw_ref.cost_error_bound's derivation with knn16_ref.coarse_error_bound per cell in place of
    knn_ref.dot_error_bound.  A path has at most n = m + L - 1 cells.  Each cell's d~ is off by at most e_d = the bound of t, plus
    gamma_D ||q||^2 (the fp32 norm of the unrounded phrase row; l2 only), plus one rounding of the add to ||q||^2 / of 1 - sim
    (u d~); max(0, .) is 1-Lipschitz.  Each DP addition rounds once, so along a path |f32 - f64| <= E + gamma_n (f64 + E) with
    E = n e_d; min over paths is 1-Lipschitz in those errors, and the larger of the two directions is the one through the
    fp32-optimal path, whose f64 <= (cost64 + E (1 + gamma_n)) / (1 - gamma_n)."""
    q, x = np.asarray(q, np.float32), np.asarray(x, np.float32)
    m, D = q.shape
    n = m + x.shape[0] - 1
    u = 2.0 ** -24
    gD, gn = D * u / (1 - D * u), n * u / (1 - n * u)
    q64 = q.astype(np.float64)
    e0 = float(np.nanmax(K16.coarse_error_bound(q, x, storage, metric))) + (gD * float((q64 * q64).sum(1).max()) if metric == "l2" else 0.0)
    d = coarse_local_costs(q, x, storage, metric)
    dmax = float(d[np.isfinite(d)].max()) if np.isfinite(d).any() else 0.0
    e_d = e0 + u * (dmax + e0)
    E = n * e_d
    return E + gn * ((cost64 + E * (1 + gn)) / (1 - gn) + E)


def coarse_costs(qs, xs, offsets, storage, metric="l2", bounds=False):
    """float64 coarse costs [P, S] of stored phrases ``qs`` against the sequences of stored rows ``xs`` (and their bounds [P, S])"""
    S = len(offsets) - 1
    c = np.empty((len(qs), S))
    b = np.zeros((len(qs), S))
    for p, q in enumerate(qs):
        for s in range(S):
            xr = xs[offsets[s]:offsets[s + 1]]
            c[p, s] = DR.dtw(coarse_local_costs(q, xr, storage, metric), np.float64)[0]
            if bounds:
                b[p, s] = coarse_cost_error_bound(q, xr, c[p, s], storage, metric) if np.isfinite(c[p, s]) else 0.0
    return (c, b) if bounds else c


def exact_results(qs, xs, offsets, metric="l2", dtype=np.float64):
    """dtw_ref's (cost [P, S], start column [P, S], end column [P, S]) of every (phrase, sequence) pair"""
    S = len(offsets) - 1
    c = np.empty((len(qs), S), dtype)
    a, e = np.zeros((len(qs), S), np.int64), np.zeros((len(qs), S), np.int64)
    for p, q in enumerate(qs):
        for s in range(S):
            c[p, s], a[p, s], e[p, s] = DR.dtw(DR.local_costs(q, xs[offsets[s]:offsets[s + 1]], metric), dtype)
    return c, a, e


def candidates(coarse_row, admissible, m):
    """one phrase's (cand [m] int64 padded with -1, coarse [m] padded with +inf) from its coarse costs [S]"""
    s = np.nonzero(np.asarray(admissible, bool) & (coarse_row < np.inf))[0]
    s = s[np.lexsort((s, coarse_row[s]))][:m]
    cand = np.full(m, -1, np.int64)
    co = np.full(m, np.inf)
    cand[:s.size], co[:s.size] = s, coarse_row[s]
    return cand, co


def two_stage(phrases, x, offsets, k, refine, storage="fp16", metric="l2", phrase_groups=None, seq_groups=None, coarse=None, exact=None):
    """(costs [P, k], seqs [P, k], spans [P, k, 2], cand [P, m], coarse [P, m]) of the contract in float64, from raw phrases and
    rows; ``coarse`` / ``exact`` may pass precomputed ``coarse_costs`` / ``exact_results``"""
    qs, xs = stored(phrases, x, metric)
    S, m = len(offsets) - 1, k * refine
    cc = coarse_costs(qs, xs, offsets, storage, metric) if coarse is None else coarse
    ec, ea, ee = exact_results(qs, xs, offsets, metric) if exact is None else exact
    C, Q, SP, CA, CO = [], [], [], [], []
    for p in range(len(qs)):
        adm = np.ones(S, bool) if phrase_groups is None else np.asarray(seq_groups) != phrase_groups[p]
        cand, co = candidates(cc[p], adm, m)
        inside = np.zeros(S, bool)
        inside[cand[cand >= 0]] = True
        c, q, sp = DR.rank(ec[p], ea[p], ee[p], offsets, k, inside)
        C.append(c); Q.append(q); SP.append(sp); CA.append(cand); CO.append(co)
    return np.stack(C), np.stack(Q), np.stack(SP), np.stack(CA), np.stack(CO)


def checkable(qs, xs, offsets, k, refine, storage, metric="l2", coarse=None, exact=None):
    """(decided bool [P], inside bool [P], top [P, m]) from stored rows.  A phrase is *decided* when every sequence outside its float64
    coarse top-m is worse than every one inside by more than the two pairs' bounds (each pair with its own
    ``coarse_cost_error_bound``): no fp32 error can then move a sequence across, so the GPU's candidate set is that top m.
    ``inside``: the float64 exact top-k lies inside the float64 coarse top-m (``top``, padded with -1).  Where both hold,
    search_phrases_refined must equal search_phrases."""
    S, m = len(offsets) - 1, k * refine
    cc, cb = coarse_costs(qs, xs, offsets, storage, metric, bounds=True) if coarse is None else coarse
    ec = (exact_results(qs, xs, offsets, metric) if exact is None else exact)[0]
    P = len(qs)
    decided, inside, top = np.zeros(P, bool), np.zeros(P, bool), np.full((P, m), -1, np.int64)
    for p in range(P):
        cand, _ = candidates(cc[p], np.ones(S, bool), m)
        top[p] = cand
        ins = cand[cand >= 0]
        out = np.setdiff1d(np.nonzero(cc[p] < np.inf)[0], ins)
        decided[p] = out.size == 0 or (cc[p, out] - cb[p, out]).min() > (cc[p, ins] + cb[p, ins]).max()
        best = np.nonzero(ec[p] < np.inf)[0]
        best = best[np.lexsort((best, ec[p, best]))][:k]
        inside[p] = np.isin(best, ins).all()
    return decided, inside, top


@functools.lru_cache(maxsize=None)
def checkable_inputs():
    """the fixed input set of the 'equality where the bound decides it' tests -> (x [N, D], offsets [S + 1], phrases, k, refine):
    clustered rows in 60 sequences of 5 .. 40 rows, 24 phrases of 1, 2, 3, 5, 8 and 13 rows cut from them with noise.  Treat the
    arrays as read-only: they are shared."""
    rng = np.random.default_rng(16)
    D, S = 64, 60
    centres = 3.0 * rng.standard_normal((200, D))
    lens = rng.integers(5, 41, S)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(offsets[-1])
    x = (centres[rng.integers(0, 200, N)] + 0.3 * rng.standard_normal((N, D))).astype(np.float32)
    phrases = []
    for m in (1, 2, 3, 5, 8, 13) * 4:
        s = int(rng.choice(np.nonzero(lens >= m)[0]))
        a = int(offsets[s]) + int(rng.integers(0, lens[s] - m + 1))
        phrases.append((x[a:a + m] + 0.3 * rng.standard_normal((m, D))).astype(np.float32))
    return x, offsets, tuple(phrases), 3, 4


@functools.lru_cache(maxsize=None)
def checkable_reference(storage, metric):
    """float64 (coarse costs, their bounds, exact (cost, start, end)) of ``checkable_inputs`` from numpy-stored rows, computed once"""
    x, offsets, phrases, k, refine = checkable_inputs()
    qs, xs = stored(phrases, x, metric)
    cc, cb = coarse_costs(qs, xs, offsets, storage, metric, bounds=True)
    return cc, cb, _exact_reference(metric)


@functools.lru_cache(maxsize=None)
def _exact_reference(metric):
    x, offsets, phrases, k, refine = checkable_inputs()
    qs, xs = stored(phrases, x, metric)
    return exact_results(qs, xs, offsets, metric)

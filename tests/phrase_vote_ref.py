"""numpy restatement of the vote of sylber_amd.SyllableIndex.search_phrases_seeded / csrc/phrase_vote.hip (``sylber_phrase_vote``), with
explicit ``np.float32`` arithmetic, and the planted case that tests/test_phrase_vote_ref.py and tests/test_gpu_ivf_phrase.py share.

Inputs: ``seed_score`` fp32 and ``seed_id`` int64, ``[R, seeds]`` each: what ``search`` reports for each of the R phrase rows
(concatenated in phrase order) under the metric; ``phrase_row[p]`` / ``phrase_len[p]``: first row and length of phrase p; sequence
offsets ``[S + 1]``.

* local cost of a seed: ``"l2"``: ``d = score``; ``"cosine"``: ``d = max(0, 1 - score)`` -- the ``d`` of ``search_phrases``;
* a seed is ignored when its id is -1, its score is NaN or its ``d`` is ``+inf``;
* ``seq(j)``: the sequence holding row j; ``floor_i``: the largest ``d`` among row i's valid seeds (0 without one);
  ``best_i(s)``: the smallest ``d`` among row i's valid seeds in sequence s (``floor_i`` without one);
* s is *seen* when some row has a valid seed in it, *admissible* unless ``seq_group[s] == phrase_group[p]``;
* ``bound(p, s) = (((0 + best_0) + best_1) + ... + best_{m_p - 1})``, fp32 additions in ascending i;
* ``cand[p]``: the m smallest admissible seen sequences of finite bound under (bound, sequence number), padded with -1;
  ``bound[p]``: their bounds, padded with ``+inf``.

Why ``bound(p, s) <= cost(p, s)`` when the seeds of every row are its ``seeds`` nearest rows: a warping path visits every phrase row
at least once; a visited cell (i, j) with j a seed of row i costs at least ``best_i(s)``, one that is no seed at least ``floor_i``
(every seed is at least as near); dropping the path's other cells only removes non-negative terms, and fp32 addition is monotone in
both arguments, so the inequality survives every rounding.

``dtw_cost`` is a small fp32 subsequence DTW (the recurrence of tests/dtw_ref.py), used only to state that lower bound."""
import numpy as np

F = np.float32


def local_cost(score, metric="l2"):
    score = np.asarray(score, F)
    with np.errstate(invalid="ignore"):
        return np.maximum(F(0), (F(1) - score).astype(F)).astype(F) if metric == "cosine" else score


def vote(seed_score, seed_id, phrase_row, phrase_len, seq_offsets, metric, m, phrase_group=None, seq_group=None, return_seen=False):
    """-> (cand int32 [P, m], bound fp32 [P, m]) (and the number of seen sequences of each phrase)"""
    sc, ids = np.asarray(seed_score, F), np.asarray(seed_id, np.int64)
    off = np.asarray(seq_offsets, np.int64)
    P = len(phrase_len)
    cand = np.full((P, m), -1, np.int32)
    bound = np.full((P, m), np.inf, F)
    seen_count = np.zeros(P, np.int64)
    for p in range(P):
        r0, mp = int(phrase_row[p]), int(phrase_len[p])
        s_p, i_p = sc[r0:r0 + mp], ids[r0:r0 + mp]
        d = local_cost(s_p, metric)
        valid = (i_p != -1) & ~np.isnan(s_p) & (d != np.inf)
        seq = np.searchsorted(off, i_p, side="right") - 1
        floor = np.zeros(mp, F)
        for i in range(mp):
            if valid[i].any():
                floor[i] = d[i][valid[i]].max()
        seen = np.unique(seq[valid])
        seen_count[p] = seen.size
        if seen.size == 0:
            continue
        best = np.repeat(floor[:, None], seen.size, 1)                      # [mp, seen]
        has = np.zeros((mp, seen.size), bool)
        rows = np.nonzero(valid)[0]
        cols = np.searchsorted(seen, seq[valid])
        tmp = np.full((mp, seen.size), np.inf, F)
        np.minimum.at(tmp, (rows, cols), d[valid])
        has[rows, cols] = True
        best[has] = tmp[has]
        acc = np.zeros(seen.size, F)
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(mp):
                acc = (acc + best[i]).astype(F)                             # one fp32 addition per row, ascending i
        ok = acc < np.inf
        if phrase_group is not None:
            ok &= np.asarray(seq_group)[seen] != phrase_group[p]
        s_ok, a_ok = seen[ok], acc[ok]
        order = np.lexsort((s_ok, a_ok))[:m]
        cand[p, :order.size] = s_ok[order]
        bound[p, :order.size] = a_ok[order]
    return (cand, bound, seen_count) if return_seen else (cand, bound)


def dtw_cost(d):
    """fp32 subsequence-DTW cost of local costs d [m, L]: A[0][j] = d[0][j]; A[i][j] = d[i][j] + min(A[i-1][j-1], A[i-1][j],
    A[i][j-1]); cost = min_j A[m-1][j]"""
    d = np.array(d, F, ndmin=2)
    d[np.isnan(d)] = np.inf
    m, L = d.shape
    A = np.full((m, L), np.inf, F)
    A[0] = d[0]
    for i in range(1, m):
        for j in range(L):
            b = A[i - 1, j]
            if j > 0:
                b = min(b, A[i - 1, j - 1], A[i, j - 1])
            A[i, j] = F(d[i, j] + b)
    return A[m - 1].min()


def l2_matrix(q, x):
    """fp32 squared distances [n, N], clamped at 0 as ``search`` reports them"""
    q, x = np.asarray(q, F), np.asarray(x, F)
    return np.maximum(F(0), ((q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - F(2) * (q @ x.T)).astype(F))


def nearest_seeds(dmat, seeds, allowed=None):
    """each row's ``seeds`` nearest columns of a distance matrix under (distance, id) -> (scores fp32 [n, seeds], ids int64
    [n, seeds]) padded with (+inf, -1); ``allowed [n, N]`` masks the columns a row may take"""
    n, N = dmat.shape
    sc = np.full((n, seeds), np.inf, F)
    ids = np.full((n, seeds), -1, np.int64)
    for i in range(n):
        j = np.arange(N) if allowed is None else np.nonzero(allowed[i])[0]
        j = j[~np.isnan(dmat[i, j])]
        j = j[np.lexsort((j, dmat[i, j]))][:seeds]
        sc[i, :j.size], ids[i, :j.size] = dmat[i, j], j
    return sc, ids


# ---- the planted case -------------------------------------------------------------------------------------------------------------------
PLANTED = dict(D=32, n_seq=60, nlist=8, n_phrases=12, k=2, nprobe=3, seeds=32, refine=4)


def planted_case(seed=7):
    """about 1 300 clustered rows in 60 sequences of 8 .. 35 rows (group = sequence number), 8 centroids, and 12 phrases cut from
    distinct sequences (4 .. 9 consecutive rows) with noise added -> dict(x, groups, offsets, centroids, phrases, truth)"""
    rng = np.random.default_rng(seed)
    c = PLANTED
    D = c["D"]
    centroids = (rng.standard_normal((c["nlist"], D)) * 4.0).astype(F)
    lens = rng.integers(8, 36, c["n_seq"])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(off[-1])
    x = (centroids[rng.integers(0, c["nlist"], N)] + rng.standard_normal((N, D))).astype(F)
    groups = np.repeat(np.arange(c["n_seq"]), lens).astype(np.int32)
    truth = rng.choice(c["n_seq"], c["n_phrases"], replace=False)
    phrases = []
    for s in truth:
        L = int(lens[s])
        m = int(rng.integers(4, min(9, L) + 1))
        a = int(rng.integers(0, L - m + 1))
        phrases.append((x[off[s] + a:off[s] + a + m] + 0.15 * rng.standard_normal((m, D))).astype(F))
    return dict(x=x, groups=groups, offsets=off, centroids=centroids, phrases=phrases, truth=truth.astype(np.int64))


def ivf_seeds(q, x, centroids, nprobe, seeds):
    """numpy inverted-file search in fp32: rows in their nearest centroid's list, each query scanning its ``nprobe`` nearest lists"""
    labels = l2_matrix(x, centroids).argmin(1)
    probe = np.argsort(l2_matrix(q, centroids), axis=1, kind="stable")[:, :nprobe]
    allowed = (labels[None, :, None] == probe[:, None, :]).any(2)
    return nearest_seeds(l2_matrix(q, x), seeds, allowed)


def seeded_search(phrases, x, offsets, sc, ids, k, m):
    """vote, then the exact fp32 DTW of the candidates, ordered by (cost, sequence) -> (costs [P, k], seqs [P, k], cand, bound)"""
    lens = np.array([len(p) for p in phrases])
    rows = np.cumsum(lens) - lens
    cand, bound = vote(sc, ids, rows, lens, offsets, "l2", m)
    costs = np.full((len(phrases), k), np.inf, F)
    seqs = np.full((len(phrases), k), -1, np.int64)
    for p, ph in enumerate(phrases):
        s = cand[p][cand[p] >= 0].astype(np.int64)
        c = np.array([dtw_cost(l2_matrix(ph, x[offsets[j]:offsets[j + 1]])) for j in s], F)
        keep = c < np.inf
        s, c = s[keep], c[keep]
        o = np.lexsort((s, c))[:k]
        costs[p, :o.size], seqs[p, :o.size] = c[o], s[o]
    return costs, seqs, cand, bound

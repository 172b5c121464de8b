"""numpy restatement of the product-quantization contract of sylber_amd.pq.PQSyllableIndex / csrc/pq.hip.

    codebooks C [M, 256, dsub], dsub = D / M; sub-row m of a row = its columns [m dsub, (m + 1) dsub)
    code[j, m]   = argmin_c (||C[m, c]||^2 - 2 x_j[sub-row m] . C[m, c]), ties to the smaller c; a sub-row that holds a NaN gets code 0
                   and masks its row
    lut[i, m, c] = cm - 2 q_i[sub-row m] . C[m, c],  cm = ||C[m, c]||^2 (l2) or 0 (cosine, q and x unit rows)
    t(i, j)      = ((lut[i, 0, code[j, 0]] + lut[i, 1, code[j, 1]]) + ...) + lut[i, M - 1, code[j, M - 1]]
    candidates   = the m_c best admissible rows under (t, j); NaN t, masked rows and same-group rows are not admissible
    rerank       : knn_ref's exact score on the candidates only (m_c = k refine), ordered by (s, j), the best k as knn_ref.search reports
    no rerank    : the candidates (m_c = k) in (t, j) order, reported max(0, ||q||^2 + t) (l2) or -t / 2 (cosine)

``encode``, ``lut`` and ``search`` are float64; the GPU's fp32 chains differ from them by at most ``chain_bound``.  ``scan_t`` is the
one place that is fp32 on purpose: given a table, t is a fixed sequence of fp32 additions, so it can be restated bit for bit."""
import numpy as np

import knn_ref as R

KSUB = 256


def stored(x, metric):
    """the fp32 rows an index holds / the queries it scores (unit rows for cosine)"""
    return R.unit_rows(x).astype(np.float32) if metric == "cosine" else np.asarray(x, np.float32)


def _sub(x, M):
    n, D = x.shape
    return np.asarray(x, np.float64).reshape(n, M, D // M)


def sub_scores(x, C, with_norms=True):
    """[n, M, 256] float64: ||c||^2 - 2 x . c per sub-space (without the norm term if ``with_norms`` is false)"""
    C = np.asarray(C, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = -2.0 * np.einsum("nmd,mcd->nmc", _sub(x, C.shape[0]), C)
        if with_norms:
            d = d + (C * C).sum(2)[None]
    return d


def chain_bound(x, C, with_norms=True):
    """[n, M, 256]: an upper bound on |fl32(d) - d| for d = fmaf(-2, x . c, ||c||^2) computed as an fp32 fmaf chain of dsub steps:
    dsub roundings of the dot product, one of the final fmaf and the rounding of the fp32 norm itself, each at most 2^-24 relative to
    a partial result that 2 |x| . |c| + ||c||^2 bounds: (dsub + 2) 2^-24 (2 |x| . |c| + ||c||^2)"""
    C = np.asarray(C, np.float64)
    dsub = C.shape[2]
    mag = 2.0 * np.einsum("nmd,mcd->nmc", np.abs(_sub(x, C.shape[0])), np.abs(C))
    if with_norms:
        mag = mag + (C * C).sum(2)[None]
    return (dsub + 2) * 2.0 ** -24 * mag


def encode(x, C):
    """(codes uint8 [n, M], bad bool [n]) of the contract, in float64"""
    d = sub_scores(x, C)
    nan = np.isnan(_sub(x, np.asarray(C).shape[0])).any(2)              # [n, M]
    codes = np.where(nan, 0, np.argmin(np.where(np.isnan(d), np.inf, d), 2)).astype(np.uint8)      # argmin: the first minimum
    return codes, nan.any(1)


def decided(x, C):
    """bool [n, M]: the decisions the bound alone settles: the float64 gap between the best and the second best centroid exceeds
    twice the largest chain bound of that (row, sub-space)"""
    d = np.sort(sub_scores(x, C), 2)
    return d[:, :, 1] - d[:, :, 0] > 2.0 * chain_bound(x, C).max(2)


def decode(codes, C):
    C = np.asarray(C)
    M = C.shape[0]
    return np.concatenate([C[m][np.asarray(codes)[:, m]] for m in range(M)], 1)


def lut(q, C, metric="l2"):
    """[n, M, 256] float64 tables from the queries as scored (pass unit rows for cosine)"""
    return sub_scores(q, C, with_norms=metric == "l2")


def scan_t(table, codes):
    """[n, N] t(i, j) from a table [n, M, 256] and codes [N, M], additions in ascending m in the table's dtype (float32 for the GPU's
    own table: then the result is the GPU's, bit for bit)"""
    codes = np.asarray(codes)
    with np.errstate(invalid="ignore", over="ignore"):
        t = table[:, 0, codes[:, 0]]
        for m in range(1, codes.shape[1]):
            t = t + table[:, m, codes[:, m]]
    return t


def candidates(t, mc, bad=None, q_group=None, x_group=None):
    """(t [n, mc] padded with +inf, cand int64 [n, mc] padded with -1)"""
    n, N = t.shape
    out_t = np.full((n, mc), np.inf, t.dtype)
    cand = np.full((n, mc), -1, np.int64)
    ok = np.ones(N, bool) if bad is None else ~np.asarray(bad, bool)
    for i in range(n):
        adm = ok if q_group is None else ok & (np.asarray(x_group) != q_group[i])
        c = R.order(t[i], adm)[:mc]
        cand[i, :len(c)] = c
        out_t[i, :len(c)] = t[i, c]
    return out_t, cand


def report(t, cand, qsq, metric):
    """the reported values of the scan's own scores: knn_finish_kernel's formulas with t in place of s, in t's dtype"""
    one = t.dtype.type
    with np.errstate(invalid="ignore"):
        v = np.maximum(one(0), qsq[:, None].astype(t.dtype) + t) if metric == "l2" else one(0) - one(0.5) * t
    return np.where(cand < 0, one(np.inf), v)


def search(q, x, C, k, refine=4, metric="l2", rerank=True, q_group=None, x_group=None):
    """(reported scores [n, k] float64, ids [n, k] int64, cand [n, m_c] int64) of the contract, from raw queries and rows"""
    qs, xs = stored(q, metric), stored(x, metric)
    codes, bad = encode(xs, C)
    t = scan_t(lut(qs, C, metric), codes)
    mc = k * refine if rerank else k
    tc, cand = candidates(t, mc, bad, q_group, x_group)
    if not rerank:
        q64 = qs.astype(np.float64)
        return report(tc, cand, (q64 * q64).sum(1), metric), cand, cand
    s = R.scores(q, x, metric)
    s_cand = np.full(s.shape, np.nan)
    for i in range(s.shape[0]):
        c = cand[i][cand[i] >= 0]
        s_cand[i, c] = s[i, c]                              # everything else NaN: never returned
    out_s, out_i = R.search(q, x, k, metric, q_group, x_group, s=s_cand)
    return out_s, out_i, cand


def clustered(seed, N, D, M, n, noise=0.1):
    """(q, x, C): random codebooks, rows built from centroids plus noise, queries near rows: data that product quantization fits"""
    rng = np.random.default_rng(seed)
    dsub = D // M
    C = rng.standard_normal((M, KSUB, dsub)).astype(np.float32)
    pick = rng.integers(0, KSUB, (N, M))
    x = (decode(pick, C) + noise * rng.standard_normal((N, D))).astype(np.float32)
    q = (x[rng.integers(0, N, n)] + noise * rng.standard_normal((n, D))).astype(np.float32)
    return q, x, C

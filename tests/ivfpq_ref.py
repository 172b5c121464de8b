"""numpy restatement of the compressed inverted-file search of sylber_amd.pq.IVFPQSyllableIndex / csrc/pq.hip (sylber_ivfpq_scan), on
top of tests/pq_ref.py and tests/ivf_ref.py: the product-quantized search with "the row is in a list the query probes" added to
admissibility.

    code[j, :], bad, lut[i], t(i, j)   as pq_ref: codes of the stored rows themselves, one table per query, fp32 sum in ascending m
    candidates of query i              = the m_c best rows under (t, original id) among the rows j with labels[j] in probe[i] that
                                         pq_ref admits (probe entries < 0 name no list; rows with label < 0 are in no list)
    rerank / no rerank                 as pq_ref.search

The list assignment ``labels [N]`` and the probe table ``probe [n, nprobe]`` are inputs, as in ivf_ref, so an fp32 near-tie of the
coarse step never has to be reproduced here; ``assign`` and ``probe_lists`` restate them in float64 for data without near-ties."""
import numpy as np

import ivf_ref as I
import knn_ref as R
import pq_ref as P


def assign(x, centroids):
    """labels [N] of the stored rows: the nearest centroid in squared L2 (ties to the smaller list), -1 for a row with a NaN"""
    s = R.scores(x, centroids, "l2")
    return np.where(np.isnan(np.asarray(x, np.float64)).any(1), -1, np.argmin(np.where(np.isnan(s), np.inf, s), 1))


def probe_lists(q, centroids, nprobe):
    """probe [n, nprobe] of the queries as scored: the exact L2 search of the centroids (-1 for a NaN query)"""
    return R.search(q, centroids, nprobe, "l2")[1]


def member(labels, probe):
    """bool [n, N]: row j is in a list that query i probes"""
    out = np.zeros((len(probe), len(labels)), bool)
    for i, row in enumerate(np.asarray(probe)):
        out[i, I.candidates(labels, row)] = True
    return out


def candidates(t, mc, labels, probe, bad=None, q_group=None, x_group=None):
    """(t [n, mc] padded with +inf, cand int64 [n, mc] padded with -1): pq_ref.candidates over the probed lists (a NaN t is never
    admissible, which is how the other rows leave)"""
    return P.candidates(np.where(member(labels, probe), t, t.dtype.type(np.nan)), mc, bad, q_group, x_group)


def search(q, x, C, k, labels, probe, refine=4, metric="l2", rerank=True, q_group=None, x_group=None):
    """(reported scores [n, k] float64, ids [n, k] int64, cand [n, m_c] int64) of the contract, from raw queries and rows"""
    qs, xs = P.stored(q, metric), P.stored(x, metric)
    codes, bad = P.encode(xs, C)
    t = P.scan_t(P.lut(qs, C, metric), codes)
    mc = k * refine if rerank else k
    tc, cand = candidates(t, mc, labels, probe, bad, q_group, x_group)
    if not rerank:
        q64 = qs.astype(np.float64)
        return P.report(tc, cand, (q64 * q64).sum(1), metric), cand, cand
    s = R.scores(q, x, metric)
    s_cand = np.full(s.shape, np.nan)
    for i in range(s.shape[0]):
        c = cand[i][cand[i] >= 0]
        s_cand[i, c] = s[i, c]                              # everything else NaN: never returned
    out_s, out_i = R.search(q, x, k, metric, q_group, x_group, s=s_cand)
    return out_s, out_i, cand

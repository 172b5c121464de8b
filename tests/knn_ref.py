"""numpy restatement of the k-NN search contract of sylber_amd.search / csrc/knn.hip, in float64.

    l2:      s(i, j) = ||x_j||^2 - 2 q_i . x_j,   reported max(0, ||q_i||^2 + s)   (the squared distance)
    cosine:  rows and queries divided by their norm (a zero row stays zero), s(i, j) = -2 q_i . x_j, reported -s / 2
    each list ordered by (s, j) ascending; NaN scores and (with groups) candidates of the query's own group are not admissible;
    fewer than k admissible candidates -> padded with id -1 and score +inf."""
import numpy as np


def unit_rows(x):
    x = np.asarray(x, np.float64)
    nrm = np.sqrt((x * x).sum(1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(nrm > 0, x / np.where(nrm > 0, nrm, 1.0), 0.0)


def scores(q, x, metric="l2"):
    """[n, N] float64 ranking scores s(i, j)"""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    if metric == "cosine":
        q, x = unit_rows(q), unit_rows(x)
        return -2.0 * (q @ x.T)
    return (x * x).sum(1)[None, :] - 2.0 * (q @ x.T)


def order(s_row, admissible):
    """ids of the admissible candidates of one row in (s, j) order"""
    j = np.nonzero(admissible & ~np.isnan(s_row))[0]
    return j[np.lexsort((j, s_row[j]))]


def search(q, x, k, metric="l2", q_group=None, x_group=None, s=None):
    """(reported scores [n, k] float64, ids [n, k] int64) of the contract; ``s`` may pass precomputed ranking scores"""
    q = np.asarray(q, np.float64)
    s = scores(q, x, metric) if s is None else s
    n, N = s.shape
    out_s = np.full((n, k), np.inf)
    out_i = np.full((n, k), -1, np.int64)
    qn = (q * q).sum(1)
    for i in range(n):
        adm = np.ones(N, bool) if q_group is None else (np.asarray(x_group) != q_group[i])
        j = order(s[i], adm)[:k]
        out_i[i, :len(j)] = j
        v = s[i, j]
        out_s[i, :len(j)] = np.maximum(0.0, qn[i] + v) if metric == "l2" else -v / 2.0
    return out_s, out_i


def dot_error_bound(q, x, D=None):
    """an upper bound on |fl32(s) - s| for every (i, j): the fp32 contraction is an fmaf chain of D steps with one rounding per
    step, so |error of q.x| <= gamma_D sum_k |q_k x_k| with gamma_D = D u / (1 - D u), u = 2^-24; the score doubles it (exact) and
    adds c_j with one more rounding (|s| u) and the rounding of c_j itself (gamma_D ||x_j||^2).  The inputs are fp32 already."""
    q, x = np.abs(np.asarray(q, np.float64)), np.abs(np.asarray(x, np.float64))
    D = q.shape[1] if D is None else D
    u = 2.0 ** -24
    g = D * u / (1 - D * u)
    return 2.0 * g * (q @ x.T) + g * (x * x).sum(1)[None, :] + u * (2.0 * (q @ x.T) + (x * x).sum(1)[None, :])

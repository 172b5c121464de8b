"""numpy restatement of the two-stage search contract of sylber_amd.search.SyllableIndex.search_refined / csrc/knn16.hip.

    stage 1:  q~ = round16(q), x~ = round16(x)   (round to nearest even, NaN stays NaN, fp16 saturates at +-65504)
              t(i, j) = c_j - 2 q~_i . x~_j,  c_j = ||x_j||^2 of the UNROUNDED row (l2) or 0 (cosine, q and x unit rows)
              candidates of query i = the m = k * refine best admissible rows under (t, j); NaN t and same-group rows are not admissible
    stage 2:  knn_ref's exact score s on the candidates only, ordered by (s, j), the best k reported as knn_ref.search reports them

Everything here is float64 on the rounded operands: the GPU's t differs from it by the fp32 accumulation only, which
``coarse_error_bound`` bounds."""
import numpy as np

import knn_ref as R

STORAGES = ("fp16", "bf16")


def round16(a, storage):
    """float32 array -> the float32 values of its 16-bit rounding"""
    a = np.ascontiguousarray(a, np.float32)
    if storage == "fp16":
        with np.errstate(invalid="ignore", over="ignore"):
            sat = np.where(np.isnan(a), a, np.clip(a, -65504.0, 65504.0)).astype(np.float32)
            return sat.astype(np.float16).astype(np.float32)
    if storage == "bf16":
        u = a.view(np.uint32).astype(np.uint64)
        r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
        r = np.where(np.isnan(a), np.uint32(0x7FC00000), r).astype(np.uint32)
        return r.view(np.float32).reshape(a.shape)
    raise ValueError(storage)


def _stored(q, x, metric):
    """the fp32 rows the index holds and the fp32 queries it scores (unit rows for cosine)"""
    if metric == "cosine":
        return R.unit_rows(q).astype(np.float32), R.unit_rows(x).astype(np.float32)
    return np.asarray(q, np.float32), np.asarray(x, np.float32)


def coarse_scores(q, x, storage, metric="l2"):
    """[n, N] float64 coarse scores t(i, j) from stored fp32 rows / queries (pass unit rows for cosine)"""
    qr, xr = round16(q, storage).astype(np.float64), round16(x, storage).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = -2.0 * (qr @ xr.T)
        if metric == "l2":
            x64 = np.asarray(x, np.float64)
            t = (x64 * x64).sum(1)[None, :] + t
    return t


def coarse_error_bound(q, x, storage, metric="l2"):
    """an upper bound on |fl32(t) - t| for every (i, j), knn_ref.dot_error_bound's derivation on the rounded operands: a product of
    two 16-bit values is exact in fp32 (22 / 16 significand bits), so the only errors of dot16 are the D - 1 fp32 additions, in
    whatever fixed order: |error| <= gamma_D sum_k |q~_k x~_k| with gamma_D = D u / (1 - D u), u = 2^-24 (valid for any summation
    order).  The score doubles it (exact) and adds c_j with one more rounding (|t| u); c_j itself is the fp32 chain over the
    unrounded row (gamma_D ||x_j||^2).  No term for the 16-bit rounding: t is defined on the rounded operands."""
    qa, xa = np.abs(round16(q, storage).astype(np.float64)), np.abs(round16(x, storage).astype(np.float64))
    D = qa.shape[1]
    u = 2.0 ** -24
    g = D * u / (1 - D * u)
    dot = qa @ xa.T
    if metric == "l2":
        x64 = np.asarray(x, np.float64)
        c = (x64 * x64).sum(1)[None, :]
    else:
        c = 0.0
    return 2.0 * g * dot + g * c + u * (2.0 * dot + c)


def candidates(t_row, admissible, m):
    return R.order(t_row, admissible)[:m]


def two_stage(q, x, k, refine, storage="fp16", metric="l2", q_group=None, x_group=None):
    """(reported scores [n, k] float64, ids [n, k] int64, cand [n, m] int64) of the contract, from raw queries and rows"""
    qs, xs = _stored(q, x, metric)
    t = coarse_scores(qs, xs, storage, metric)
    s = R.scores(q, x, metric)
    n, N = s.shape
    m = k * refine
    cand = np.full((n, m), -1, np.int64)
    s_cand = np.full((n, N), np.nan)
    for i in range(n):
        adm = np.ones(N, bool) if q_group is None else (np.asarray(x_group) != q_group[i])
        c = candidates(t[i], adm, m)
        cand[i, :len(c)] = c
        s_cand[i, c] = s[i, c]                              # everything else NaN: never returned
    out_s, out_i = R.search(q, x, k, metric, q_group, x_group, s=s_cand)
    return out_s, out_i, cand


def checkable(q, x, k, refine, storage, metric="l2"):
    """bool [n]: the queries for which the bound alone decides that search_refined must equal search: the exact top-k lies inside the
    float64 coarse top-m, and every row outside that top m is worse than every one of those k by more than the two pairs' bounds
    (``2 * coarse_error_bound``, each pair with its own value) -- so no fp32 accumulation error can move one of the k out of the
    GPU's top-m"""
    qs, xs = _stored(q, x, metric)
    t = coarse_scores(qs, xs, storage, metric)
    b = coarse_error_bound(qs, xs, storage, metric)
    s = R.scores(q, x, metric)
    n, N = s.shape
    m = k * refine
    ok = np.zeros(n, bool)
    adm = np.ones(N, bool)
    for i in range(n):
        top = R.order(s[i], adm)[:k]
        ct = R.order(t[i], adm)
        if not np.isin(top, ct[:m]).all():
            continue
        out = ct[m:]                                        # each pair (a in top, j outside the top m) with its own two bounds
        ok[i] = len(out) == 0 or (t[i, out] - b[i, out]).min() > (t[i, top] + b[i, top]).max()
    return ok


def checkable_inputs():
    """the inputs of the 'equality where the bound decides it' test: clustered rows, queries near rows"""
    rng = np.random.default_rng(16)
    N, D, n = 20000, 64, 256
    centres = 3.0 * rng.standard_normal((200, D))
    x = (centres[rng.integers(0, 200, N)] + 0.3 * rng.standard_normal((N, D))).astype(np.float32)
    q = (x[rng.integers(0, N, n)] + 0.3 * rng.standard_normal((n, D))).astype(np.float32)
    return q, x, 10, 4

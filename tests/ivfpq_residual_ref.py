"""numpy restatement of the residual codes of sylber_amd.pq.IVFPQSyllableIndex (``build(..., residual=True)``) / csrc/pq.hip
(sylber_ivfpq_scan_residual, sylber_ivfpq_list_terms, sylber_ivfpq_recon_norms), on top of tests/pq_ref.py, tests/ivf_ref.py and
tests/ivfpq_ref.py.  Lists, probing, candidates, re-rank and reported values are ivfpq_ref's; what changes:

    r_j          = x_j - centroids[l_j]                       (l_j the list of the stored row; one fp32 subtraction per element)
    code[j, :]   = pq_ref.encode(r)[j]; a row in no list (l_j < 0) gets code 0 and is masked
    xhat_j       = centroids[l_j] + pq_ref.decode(code_j)     (one fp32 addition per element; a row in no list: the decode alone)
    nrm_j        = ||xhat_j||^2                               ("l2" only)
    lut[i, m, c] = -2 q_i[sub-row m] . C[m, c]                (both metrics: pq_ref.lut without norms, one table per query)
    a[i, s]      = -2 q_i . centroids[probe[i, s]]            (0 for a slot < 0)
    u(i, j)      = pq_ref.scan_t(lut, code): the sum of the M table entries in ascending m
    t(i, j)      = (u + a[i, s]) + nrm_j ("l2"), u + a[i, s] ("cosine"), s the slot with probe[i, s] == l_j; a row whose list the query
                   does not probe has no t (NaN: never admissible)

so in exact arithmetic t = ||q - xhat||^2 - ||q||^2 ("l2") and -2 q . xhat ("cosine").  ``scan_t`` adds in its inputs' dtype: with
the GPU's own fp32 table, a and nrm it is the GPU's t bit for bit; with float64 inputs it is the contract's value."""
import numpy as np

import ivfpq_ref as F
import knn_ref as R
import pq_ref as P


def clustered_lists(seed, N, D, M, nlist, n, spread=4.0, noise=0.5):
    """(q [n, D], x [N, D], centres [nlist, D], lists [N]) fp32: centres ~ spread N(0, 1), a row = the centre of a random list plus
    noise N(0, 1), a query = a random row plus noise / 2: lists that lie far apart compared with their spread.  M only fixes the
    geometry the data are meant for."""
    assert D % M == 0
    rng = np.random.default_rng(seed)
    cent = (spread * rng.standard_normal((nlist, D))).astype(np.float32)
    lists = rng.integers(0, nlist, N)
    x = (cent[lists] + noise * rng.standard_normal((N, D))).astype(np.float32)
    q = (x[rng.integers(0, N, n)] + 0.5 * noise * rng.standard_normal((n, D))).astype(np.float32)
    return q, x, cent, lists


def coarse_gap(xs, cent):
    """[N] float64: by how much the second nearest centroid is farther (squared L2) than the nearest"""
    d = np.sort(R.scores(xs, cent, "l2"), 1)
    return d[:, 1] - d[:, 0] if cent.shape[0] > 1 else np.full(len(xs), np.inf)


def residuals(xs, cent, labels):
    """fp32 [N, D]: the stored rows minus their lists' centroids, rounded once; NaN rows for the rows in no list"""
    labels = np.asarray(labels)
    r = np.asarray(xs, np.float32) - np.asarray(cent, np.float32)[np.maximum(labels, 0)]
    r[labels < 0] = np.nan
    return r


def sampled_codebooks(r, M, seed):
    """[M, 256, dsub] fp32: 256 rows of r (no NaN rows among them), cut into sub-rows"""
    ok = np.nonzero(~np.isnan(r).any(1))[0]
    pick = np.random.default_rng(seed).choice(ok, P.KSUB, replace=False)
    return np.ascontiguousarray(r[pick].reshape(P.KSUB, M, -1).transpose(1, 0, 2), dtype=np.float32)


def encode(xs, cent, labels, C):
    """(codes uint8 [N, M], bad bool [N]) of the contract, in float64 from the fp32 residuals"""
    return P.encode(residuals(xs, cent, labels), C)


def reconstruct(codes, labels, cent, C, dtype=np.float32):
    """xhat [N, D]: one addition per element in ``dtype`` (fp32: ix.decode's bits)"""
    labels = np.asarray(labels)
    d = P.decode(codes, C).astype(dtype)
    return np.where((labels >= 0)[:, None], np.asarray(cent, dtype)[np.maximum(labels, 0)] + d, d)


def recon_norms(xhat):
    """float64 ||xhat||^2 of the fp32 reconstruction"""
    v = np.asarray(xhat, np.float64)
    return (v * v).sum(1)


def lut(q, C):
    """[n, M, 256] float64: the inner-product table, for both metrics"""
    return P.lut(q, C, "cosine")


def list_terms(q, cent, probe):
    """a [n, nprobe] float64"""
    probe = np.asarray(probe)
    dots = np.einsum("nd,nsd->ns", np.asarray(q, np.float64), np.asarray(cent, np.float64)[np.maximum(probe, 0)])
    return np.where(probe >= 0, -2.0 * dots, 0.0)


def list_term_bound(q, cent, probe):
    """the fp32 chain's error bound on a: D roundings of the dot product and none of the doubling, each at most 2^-24 relative to a
    partial result that |q| . |c| bounds; stated as (D + 1) 2^-24 2 |q| . |c|"""
    probe = np.asarray(probe)
    D = np.asarray(q).shape[1]
    mag = np.einsum("nd,nsd->ns", np.abs(np.asarray(q, np.float64)), np.abs(np.asarray(cent, np.float64))[np.maximum(probe, 0)])
    return (D + 1) * 2.0 ** -24 * 2.0 * mag


def scan_t(table, codes, a, nrm, labels, probe):
    """t [n, N] in the inputs' dtype: (u + a[i, slot of the row's list]) + nrm_j (``nrm`` None: u + a); NaN where the query does not
    probe the row's list.  The additions are done in that order, one rounding each."""
    labels, probe = np.asarray(labels), np.asarray(probe)
    u = P.scan_t(table, codes)
    t = np.full(u.shape, np.nan, u.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(probe.shape[1]):
            hit = (probe[:, s, None] == labels[None]) & (probe[:, s, None] >= 0)               # [n, N]
            v = u + np.asarray(a, u.dtype)[:, s, None]
            if nrm is not None:
                v = v + np.asarray(nrm, u.dtype)[None]
            t = np.where(hit, v, t)
    return t


def candidates(t, mc, bad=None, q_group=None, x_group=None):
    """pq_ref.candidates: ``scan_t`` has already left the rows of the other lists without a t"""
    return P.candidates(t, mc, bad, q_group, x_group)


def search(q, x, cent, C, k, labels, probe, refine=4, metric="l2", rerank=True, q_group=None, x_group=None):
    """(reported scores [n, k] float64, ids [n, k] int64, cand [n, m_c] int64) of the contract, from raw queries and rows"""
    qs, xs = P.stored(q, metric), P.stored(x, metric)
    codes, bad = encode(xs, cent, labels, C)
    xhat = reconstruct(codes, labels, cent, C)
    t = scan_t(lut(qs, C), codes, list_terms(qs, cent, probe), recon_norms(xhat) if metric == "l2" else None, labels, probe)
    mc = k * refine if rerank else k
    tc, cand = candidates(t, mc, bad, q_group, x_group)
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


def recon_error(xs, xhat):
    """mean squared reconstruction error over the rows without a NaN"""
    d = np.asarray(xs, np.float64) - np.asarray(xhat, np.float64)
    ok = ~np.isnan(d).any(1)
    return float((d[ok] ** 2).sum(1).mean())

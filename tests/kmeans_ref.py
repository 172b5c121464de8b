"""Test-only numpy restatement of ``sylber_amd.fit_kmeans`` (never imported by the product).  Inner products and distances are
float64; the centroid update follows the device's summation order (fp64 sums of each cluster's rows in ascending row order, in
pieces of 512 rows added left to right, one division, one rounding to fp32), so that a given labelling gives the device's centroids
bit for bit.  k-means++ takes the same uniforms as the device: ``np.random.default_rng(seed).random(K)``."""
import numpy as np

PIECE = 512


def normalize(x):
    """``x / sqrt(sum x^2 + 1e-8) * 6`` (KMQuantizer(normalize=True)), in float64 then rounded to fp32"""
    x64 = np.asarray(x, np.float64)
    return (x64 / np.sqrt((x64 ** 2).sum(1, keepdims=True) + 1e-8) * 6).astype(np.float32)


def assign(x, c):
    """-> labels (first index on ties), d_min = ||c||^2 - 2 x.c of the chosen centroid, inertia sum_r max(0, ||x||^2 + d_min)"""
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    score = (c64 ** 2).sum(1)[None, :] - 2 * x64 @ c64.T
    lab = score.argmin(1)
    dmin = score[np.arange(len(x64)), lab]
    inertia = float(np.maximum(0.0, (x64 ** 2).sum(1) + dmin).sum())
    return lab, dmin, inertia


def update(x, labels, c):
    """new centroids (fp32) and counts; an empty cluster keeps its previous centroid"""
    x = np.asarray(x, np.float32)
    out = np.array(c, np.float32, copy=True)
    K = len(out)
    counts = np.bincount(labels, minlength=K)
    for k in np.nonzero(counts)[0]:
        rows = np.nonzero(labels == k)[0]                        # ascending
        s = np.zeros(x.shape[1], np.float64)
        for p0 in range(0, len(rows), PIECE):
            piece = np.cumsum(x[rows[p0:p0 + PIECE]].astype(np.float64), axis=0)[-1]     # sequential fp64, ascending rows
            s = s + piece
        out[k] = (s / np.float64(len(rows))).astype(np.float32)
    return out, counts


def kmeans_plusplus(x, K, u):
    """plain k-means++ (one candidate per step): the first center is row floor(u[0] n); the next is the smallest r whose inclusive
    prefix sum of dist exceeds u[j] * total.  Raises ValueError when total == 0 (fewer than K distinct rows)."""
    x64 = np.asarray(x, np.float64)
    n = len(x64)
    chosen = [min(int(np.floor(u[0] * n)), n - 1)]
    dist = np.full(n, np.inf)
    for j in range(1, K):
        dist = np.minimum(dist, ((x64 - x64[chosen[-1]]) ** 2).sum(1))
        cum = np.cumsum(dist)
        total = cum[-1]
        if not total > 0:
            raise ValueError("fewer than K distinct rows")
        hit = np.nonzero(cum > u[j] * total)[0]
        chosen.append(int(hit[0]) if len(hit) else int(np.nonzero(dist > 0)[0][-1]))
    return np.array(chosen, np.int64)


def init_centroids(x, K, init="k-means++", seed=0, init_rows=None):
    x = np.asarray(x, np.float32)
    n = len(x)
    if isinstance(init, str):
        if init == "random":
            return x[np.random.default_rng(seed).choice(n, K, replace=False)].copy()
        if init_rows is not None and init_rows < n:
            rng = np.random.default_rng(seed)
            rows = np.sort(rng.choice(n, init_rows, replace=False))
            return x[rows[kmeans_plusplus(x[rows], K, rng.random(K))]].copy()
        return x[kmeans_plusplus(x, K, np.random.default_rng(seed).random(K))].copy()
    return np.array(init, np.float32, copy=True)


def fit(x, K, max_iter=100, tol=1e-4, init="k-means++", seed=0, init_rows=None, normalize_rows=False):
    """-> dict(centroids, labels, inertia, n_iter, converged, history, labels_per_iter)"""
    x = np.asarray(x, np.float32)
    if K < 1 or K > len(x):
        raise ValueError("need 1 <= K <= n")
    if not np.isfinite(x).all():
        raise ValueError("non-finite features")
    if normalize_rows:
        x = normalize(x)
    C = init_centroids(x, K, init, seed, init_rows)
    history, per_iter = [], []
    prev, prev_inertia = None, None
    converged, n_iter = False, 0
    lab = inertia = None
    for it in range(max_iter):
        lab, _, inertia = assign(x, C)
        per_iter.append(lab)
        changed = len(x) if prev is None else int((lab != prev).sum())
        if it > 0 and (changed == 0 or prev_inertia - inertia <= tol * prev_inertia):
            history.append((inertia, changed, int((np.bincount(lab, minlength=K) == 0).sum())))
            converged = True
            break
        C, counts = update(x, lab, C)
        n_iter += 1
        history.append((inertia, changed, int((counts == 0).sum())))
        prev, prev_inertia = lab, inertia
    if not converged:
        lab, _, inertia = assign(x, C)
    return dict(centroids=C, labels=lab, inertia=inertia, n_iter=n_iter, converged=converged, history=history, labels_per_iter=per_iter)

"""Fitting k-means unit codebooks on the device: ``fit_kmeans`` (k-means++ or given seeds, then Lloyd iterations) and the two
quantizers built from its centroids, ``fit_km_quantizer`` and ``fit_residual_km_quantizer``.  The three hot steps are HIP
(csrc/kmeans.hip): the fused assign (the arg-min of ``sylber_km_assign`` without its ``[n, K]`` dot matrix), the centroid update
(fp64 sums in fixed pieces) and k-means++ seeding (no host round trip per center).  Host code here only converts inputs, groups
rows by label with a stable sort, and runs the stop rule.

Semantics (tests/kmeans_ref.py restates them in numpy)::

    C = init
    for it in range(max_iter):
        labels, inertia = assign(X, C)
        if it > 0 and labels == prev_labels: converged; break
        if it > 0 and prev_inertia - inertia <= tol * prev_inertia: converged; break
        C = update(X, labels, C); prev_labels, prev_inertia = labels, inertia
    labels, inertia = assign(X, C)          # what is returned
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .downstream import KMQuantizer, ResidualKMQuantizer


def _vp(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _stream(dev) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _device(device) -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.SylberHipError("no MI355X visible to PyTorch-ROCm; the HIP path has no CPU fallback")
    d = torch.device(device)
    if d.type != "cuda":
        raise _lib.SylberHipError("k-means fitting runs on the MI355X only (device=%r)" % (device,))
    return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())


def _features(features, dev: torch.device) -> torch.Tensor:
    """a [n, D] tensor / array or a list of per-clip [m, D] arrays (empty clips skipped) -> contiguous fp32 [n, D] on dev"""
    if isinstance(features, (list, tuple)):
        parts = [f if torch.is_tensor(f) else torch.from_numpy(np.asarray(f)) for f in features]
        parts = [p for p in parts if p.numel() > 0]
        if not parts:
            raise ValueError("no feature rows: every clip is empty")
        if any(p.dim() != 2 for p in parts) or len({p.shape[1] for p in parts}) != 1:
            raise ValueError("per-clip features must all be [m, D] with one D, got %s" % [tuple(p.shape) for p in parts])
        x = torch.cat([p.to(dev, torch.float32) for p in parts])
    else:
        x = features if torch.is_tensor(features) else torch.from_numpy(np.asarray(features))
        if x.dim() != 2:
            raise ValueError("features must be [n, D], got %s" % (tuple(x.shape),))
        x = x.to(dev, torch.float32)
    x = x.contiguous()
    if x.shape[0] < 1:
        raise ValueError("no feature rows")
    if x.shape[1] < 16 or x.shape[1] % 16:
        raise ValueError("the feature width D must be a multiple of 16 (as sylber_km_assign requires), got %d" % x.shape[1])
    if not bool(torch.isfinite(x).all()):
        raise ValueError("features hold non-finite values")
    return x


def _normalize(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(lib.sylber_km_normalize(_vp(x), x.shape[0], x.shape[1], _vp(y), _stream(x.device)), "sylber_km_normalize")
    return y


def assign(x: torch.Tensor, centroids: torch.Tensor, prev: Optional[torch.Tensor] = None, row_chunk: Optional[int] = None):
    """the fused assign (``sylber_kmeans_assign``) of contiguous fp32 rows ``x [n, D]`` against ``centroids [K, D]`` on one device ->
    ``(labels int32 [n], d_min fp32 [n], inertia float, changed int or None)``; ``d_min[r] = ||c||^2 - 2 x.c`` of the chosen centroid.
    ``row_chunk`` runs the rows in chunks of that many (labels and d_min do not depend on it; the inertia is summed per chunk, then
    over the chunks in order).  A row without a comparable score (it holds a NaN, or its dot products are inf - inf) has no nearest
    centroid: its label is 2147483647, never one in ``[0, K)``, and its ``d_min`` is +inf.  The fits refuse non-finite features before
    they get here; the inverted-file indexes put such a row in no list.  (``KMQuantizer.get_indices`` gives such a token id 0.)"""
    lib = _lib.load()
    dev = x.device
    n, D = x.shape
    K = centroids.shape[0]
    step = n if not row_chunk else max(1, int(row_chunk))
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    dmin = torch.empty(n, dtype=torch.float32, device=dev)
    nch = (n + step - 1) // step
    inertia = torch.empty(nch, dtype=torch.float64, device=dev)
    changed = torch.empty(nch, dtype=torch.int64, device=dev) if prev is not None else None
    ws = torch.empty(int(lib.sylber_kmeans_assign_workspace_floats(min(step, n), K, D)), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for i, r0 in enumerate(range(0, n, step)):
            m = min(step, n - r0)
            _lib.check(lib.sylber_kmeans_assign(_vp(x[r0:r0 + m]), m, _vp(centroids), K, D, _vp(labels[r0:r0 + m]), _vp(dmin[r0:r0 + m]),
                                                _vp(inertia[i:i + 1]), _vp(prev[r0:r0 + m] if prev is not None else None),
                                                _vp(changed[i:i + 1] if changed is not None else None), _vp(ws), _stream(dev)),
                       "sylber_kmeans_assign")
    tot = float(sum(inertia.tolist()))
    ch = int(changed.sum()) if changed is not None else None
    return labels, dmin, tot, ch


def update(x: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
    """``sylber_kmeans_update`` in place on ``centroids``: the mean of each cluster's rows (fp64 sums), empty clusters untouched;
    returns ``counts`` int32 [K] on the device"""
    lib = _lib.load()
    dev = x.device
    n, D = x.shape
    K = centroids.shape[0]
    order = torch.sort(labels, stable=True).indices          # rows grouped by label, ascending within a label (plumbing)
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.sylber_kmeans_update_workspace_bytes(n, K, D)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.sylber_kmeans_update(_vp(x), n, D, _vp(labels), _vp(order), K, _vp(centroids), _vp(counts), _vp(ws), _stream(dev)),
                   "sylber_kmeans_update")
    return counts


def kmeans_plusplus(x: torch.Tensor, K: int, u: np.ndarray) -> torch.Tensor:
    """``sylber_kmeans_seed``: the rows k-means++ picks (int64 [K] on the device), given the K uniforms ``u`` (float64)"""
    lib = _lib.load()
    dev = x.device
    n, D = x.shape
    ud = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64)).to(dev)
    chosen = torch.empty(K, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.sylber_kmeans_seed_workspace_floats(n)), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.sylber_kmeans_seed(_vp(x), n, D, K, _vp(ud), _vp(chosen), _vp(status), _vp(ws), _stream(dev)), "sylber_kmeans_seed")
    if int(status.item()):
        raise ValueError("k-means++ found fewer than K = %d distinct rows" % K)
    return chosen.to(torch.int64)


@dataclass
class KMeansFit:
    """the result of ``fit_kmeans``: ``centroids [K, D]`` fp32 and ``labels [n]`` int64 on the device (labels against the returned
    centroids), ``inertia`` of those labels, ``n_iter`` centroid updates, ``converged`` (a stop rule fired before ``max_iter``) and
    ``history``: one ``(inertia, rows that changed label, empty clusters)`` per assign of the loop."""
    centroids: torch.Tensor
    labels: torch.Tensor
    inertia: float
    n_iter: int
    converged: bool
    history: List[Tuple[float, int, int]] = field(default_factory=list)
    normalize: bool = False

    def save(self, path: str) -> None:
        """``[K, D]`` float32 ``.npy``: the layout ``KMQuantizer(path)`` (upstream's and ours) loads"""
        np.save(path, self.centroids.detach().cpu().numpy().astype(np.float32))


def _init_centroids(x: torch.Tensor, K: int, init, init_rows, seed: int) -> torch.Tensor:
    n, D = x.shape
    if isinstance(init, str):
        if init == "random":
            rows = np.random.default_rng(seed).choice(n, K, replace=False)
            return x.index_select(0, torch.from_numpy(rows.astype(np.int64)).to(x.device)).contiguous()
        if init != "k-means++":
            raise ValueError("init must be 'k-means++', 'random' or a [K, D] array, got %r" % (init,))
        if init_rows is not None and int(init_rows) < n:
            m = int(init_rows)
            if m < K:
                raise ValueError("init_rows = %d < K = %d" % (m, K))
            rng = np.random.default_rng(seed)
            rows = torch.from_numpy(np.sort(rng.choice(n, m, replace=False)).astype(np.int64)).to(x.device)
            sub = x.index_select(0, rows).contiguous()
            picks = rows.index_select(0, kmeans_plusplus(sub, K, rng.random(K)))
        else:
            picks = kmeans_plusplus(x, K, np.random.default_rng(seed).random(K))
        return x.index_select(0, picks).contiguous()
    c = init if torch.is_tensor(init) else torch.from_numpy(np.asarray(init))
    if tuple(c.shape) != (K, D):
        raise ValueError("an explicit init must be [K, D] = [%d, %d], got %s" % (K, D, tuple(c.shape)))
    c = c.to(x.device, torch.float32).contiguous().clone()
    if not bool(torch.isfinite(c).all()):
        raise ValueError("init holds non-finite values")
    return c


def _fit(x: torch.Tensor, K: int, max_iter: int, tol: float, init, init_rows, seed: int, normalize: bool) -> KMeansFit:
    n = x.shape[0]
    if int(K) != K or K < 1:
        raise ValueError("n_clusters must be an integer >= 1, got %r" % (K,))
    K = int(K)
    if K > n:
        raise ValueError("n_clusters = %d > %d rows" % (K, n))
    if max_iter < 0 or tol < 0:
        raise ValueError("max_iter and tol must be >= 0")
    C = _init_centroids(x, K, init, init_rows, seed)
    history: List[Tuple[float, int, int]] = []
    prev, prev_inertia, labels, inertia = None, None, None, None
    converged, n_iter = False, 0
    for it in range(max_iter):
        labels, _, inertia, changed = assign(x, C, prev)
        changed = n if changed is None else changed
        if it > 0 and (changed == 0 or prev_inertia - inertia <= tol * prev_inertia):
            empty = int((torch.bincount(labels, minlength=K) == 0).sum())
            history.append((inertia, changed, empty))
            converged = True
            break
        counts = update(x, labels, C)
        n_iter += 1
        history.append((inertia, changed, int((counts == 0).sum())))
        prev, prev_inertia = labels, inertia
    if not converged:
        labels, _, inertia, _ = assign(x, C)
    return KMeansFit(centroids=C, labels=labels.to(torch.int64), inertia=float(inertia), n_iter=n_iter, converged=converged,
                     history=history, normalize=bool(normalize))


def fit_kmeans(features, n_clusters: int, *, max_iter: int = 100, tol: float = 1e-4, init="k-means++", init_rows: Optional[int] = None,
               seed: int = 0, normalize: bool = False, device="cuda") -> KMeansFit:
    """k-means on the device.  ``features``: a ``[n, D]`` tensor (host or device; fp32, bf16 or fp16) or numpy array, or a list of
    per-clip ``[m, D]`` arrays (concatenated, empty clips skipped); ``D % 16 == 0``.  ``init``: ``"k-means++"`` (plain, one candidate
    per step, uniforms ``np.random.default_rng(seed).random(K)``), ``"random"`` (``default_rng(seed).choice(n, K, replace=False)``)
    or a ``[K, D]`` array; ``init_rows`` seeds k-means++ on a random subset of that many rows.  ``normalize`` fits on
    ``x / sqrt(sum x^2 + 1e-8) * 6`` (``KMQuantizer(normalize=True)``'s arithmetic).  ``ValueError`` for K < 1, K > n, non-finite
    features, or (k-means++) fewer than K distinct rows."""
    dev = _device(device)
    x = _features(features, dev)
    if normalize:
        x = _normalize(x)
    return _fit(x, n_clusters, max_iter, tol, init, init_rows, seed, normalize)


def fit_km_quantizer(features, n_clusters: int, **kw) -> KMQuantizer:
    """``KMQuantizer(fit.centroids, normalize=kw["normalize"])`` of ``fit_kmeans(features, n_clusters, **kw)``; the fit is ``.fit``"""
    fit = fit_kmeans(features, n_clusters, **kw)
    q = KMQuantizer(fit.centroids, normalize=fit.normalize, device=fit.centroids.device)
    q.fit = fit
    return q


def fit_residual_km_quantizer(features, n_clusters: int, n_clusters2: int, **kw) -> ResidualKMQuantizer:
    """two-stage k-means: stage 1 ``fit_kmeans(x, K1)``, stage 2 ``fit_kmeans(x - c1[labels1], K2)`` (the residual as one fp32 subtract,
    the arithmetic of ``sylber_km_assign_residual``, so that ``get_indices(x)`` reproduces both label columns).  ``init`` may be a pair
    (stage 1, stage 2).  ``normalize`` is refused: upstream's ResidualKMQuantizer ignores it.  The two fits are ``.fits``."""
    if kw.get("normalize"):
        raise ValueError("normalize is not supported for the residual fit: upstream's ResidualKMQuantizer ignores it")
    kw.pop("normalize", None)
    init = kw.pop("init", "k-means++")
    init1, init2 = init if isinstance(init, (tuple, list)) and len(init) == 2 and not isinstance(init[0], (int, float)) else (init, init)
    dev = _device(kw.pop("device", "cuda"))
    x = _features(features, dev)
    max_iter, tol = kw.pop("max_iter", 100), kw.pop("tol", 1e-4)
    init_rows, seed = kw.pop("init_rows", None), kw.pop("seed", 0)
    if kw:
        raise TypeError("unexpected arguments %s" % sorted(kw))
    fit1 = _fit(x, n_clusters, max_iter, tol, init1, init_rows, seed, False)
    r = x - fit1.centroids.index_select(0, fit1.labels)        # token - z_q: one fp32 subtract per element
    fit2 = _fit(r.contiguous(), n_clusters2, max_iter, tol, init2, init_rows, seed, False)
    del r
    q = ResidualKMQuantizer(fit1.centroids, fit2.centroids, device=fit1.centroids.device)
    q.fits = (fit1, fit2)
    return q

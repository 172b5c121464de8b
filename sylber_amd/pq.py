"""Compressed syllable search: ``PQSyllableIndex`` stores every row as ``M`` bytes (product quantization) and scans the codes with
per-query look-up tables held in LDS (csrc/pq.hip).  A row of ``D`` floats is cut into ``M`` sub-rows of ``dsub = D / M`` columns;
sub-space ``m`` has 256 centroids and byte ``m`` of a row's code names the nearest one.  ``4 D / M`` times smaller than the fp32 rows
(D = 768, M = 48: 48 bytes per syllable, 64 times smaller); a query's table is ``M`` KiB.

Contract (tests/pq_ref.py restates it in numpy)::

    codebooks [M, 256, dsub]     given, or codebook m = fit_kmeans(rows[:, m dsub : (m + 1) dsub], 256, seed=seed + m, ...).centroids
    code[j, m]                   = the label sylber_kmeans_assign gives sub-row m of x_j against codebook m, bit for bit; a sub-row that
                                   holds a NaN gets code 0 and its row is masked: never returned
    lut[i, m, c]                 = fmaf(-2, q_i[sub-row m] . C[m, c], cm),  cm = ||C[m, c]||^2 ("l2") or 0 ("cosine", q the unit row)
    t(i, j)                      = ((lut[i, 0, code[j, 0]] + lut[i, 1, code[j, 1]]) + ...) + lut[i, M - 1, code[j, M - 1]]    (fp32)
    candidates of query i        = the m_c best admissible rows under the strict order (t, j); NaN t, masked rows and (with
                                   exclude_same_group) rows of the query's group are not admissible; padded with -1
    rerank=True  (m_c = k refine): the candidates through sylber_knn_rerank: SyllableIndex.search restricted to the candidate set, with
                                   search's score bits, order, reported values and padding; with k refine >= N it is search
    rerank=False (m_c = k):        the candidates in (t, j) order, reported as search reports s: "l2" max(0, ||q||^2 + t),
                                   "cosine" -t / 2, padding (+inf, -1)

Codes, candidates, scores and ids do not depend on ``splits``, ``query_chunk``, how many queries share a workgroup, whether the rows
came in one ``build`` or through later ``add`` calls, or what the workspace held.

``IVFPQSyllableIndex`` puts the same codes behind ``IVFSyllableIndex``'s lists: a search scans the codes of the ``nprobe`` nearest
lists only (``sylber_ivfpq_scan``).  tests/ivfpq_ref.py restates that composition."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .kmeans import _device, _stream, _vp
from .search import (DEFAULT_QUERY_CHUNK, MAX_CANDIDATES, MAX_K, MAX_NPROBE, METRICS, IVFSyllableIndex, SyllableIndex,
                     _chunked_workspace_bytes, _groups, _rows)

KSUB = 256                      # centroids per sub-space: one uint8 per code
MAX_M = 64                      # PQ_MAX_M of csrc/pq.hip: at least two queries' tables (M KiB each) fit beside the top lists in LDS
ENCODE_CHUNK = 1 << 20          # rows per encode launch


def _check_geometry(D: int, M) -> int:
    if isinstance(M, bool) or int(M) != M or not 1 <= int(M) <= MAX_M:
        raise ValueError("M must be an integer in [1, %d], got %r" % (MAX_M, M))
    M = int(M)
    if D % M or (D // M) % 16:
        raise ValueError("D = %d must split into M = %d sub-rows whose width is a multiple of 16" % (D, M))
    return M


def _train_codebooks(index: SyllableIndex, M: int, codebooks, seed: int, max_iter: int, tol: float, train_rows) -> torch.Tensor:
    """``[M, 256, D / M]`` fp32 on the index's device: ``codebooks`` as given (finite), or one ``fit_kmeans`` per sub-space of the
    stored rows with ``seed + m``"""
    from .kmeans import fit_kmeans
    N, dsub = len(index), index.dim // M
    if codebooks is None:
        if N < KSUB:
            raise ValueError("training %d centroids per sub-space needs at least %d rows, the index holds %d" % (KSUB, KSUB, N))
        return torch.stack([fit_kmeans(index._x[:, m * dsub:(m + 1) * dsub].contiguous(), KSUB, seed=seed + m, max_iter=max_iter, tol=tol,
                                       init_rows=train_rows, device=index.device).centroids for m in range(M)]).contiguous()
    c = codebooks if torch.is_tensor(codebooks) else torch.from_numpy(np.asarray(codebooks))
    if tuple(c.shape) != (M, KSUB, dsub):
        raise ValueError("codebooks must be [M, 256, D / M] = [%d, %d, %d], got %s" % (M, KSUB, dsub, tuple(c.shape)))
    if not c.dtype.is_floating_point:
        raise ValueError("codebooks: dtype %s is not floating point" % c.dtype)
    C = c.to(index.device, torch.float32).contiguous().clone()
    if not bool(torch.isfinite(C).all()):
        raise ValueError("codebooks hold non-finite values")
    return C


def _centroid_norms(codebooks: torch.Tensor) -> torch.Tensor:
    """``[M, 256]``: ``sylber_knn_row_norms`` of the codebooks' centroids"""
    M, _, dsub = codebooks.shape
    dev = codebooks.device
    cnorm = torch.empty((M, KSUB), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().sylber_knn_row_norms(_vp(codebooks), M * KSUB, dsub, _vp(cnorm), _stream(dev)), "sylber_knn_row_norms")
    return cnorm


def _encode(x: torch.Tensor, codebooks: torch.Tensor, cnorm: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """stored rows ``[n, D]`` on the device -> ``(codes uint8 [n, M], bad uint8 [n])`` (csrc/pq.hip, ``sylber_pq_encode``)"""
    n, D = x.shape
    M, dev = int(codebooks.shape[0]), codebooks.device
    codes = torch.empty((n, M), dtype=torch.uint8, device=dev)
    bad = torch.empty(n, dtype=torch.uint8, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        for r0 in range(0, n, ENCODE_CHUNK):
            r1 = min(n, r0 + ENCODE_CHUNK)
            _lib.check(lib.sylber_pq_encode(_vp(x[r0:r1]), r1 - r0, D, _vp(codebooks), _vp(cnorm), M, _vp(codes[r0:r1]), _vp(bad[r0:r1]),
                                            _stream(dev)), "sylber_pq_encode")
    return codes, bad


def _prep(x: torch.Tensor, metric: str, device: torch.device) -> torch.Tensor:
    """rows or queries as they are stored / scored: fp32 on the device, unit rows under "cosine" (SyllableIndex._prep)"""
    lib = _lib.load()
    x = x.to(device, torch.float32).contiguous()
    if metric == "cosine" and x.shape[0]:
        y = torch.empty_like(x)
        with torch.cuda.device(device):
            _lib.check(lib.sylber_knn_unit_rows(_vp(x), x.shape[0], x.shape[1], _vp(y), _stream(device)), "sylber_knn_unit_rows")
        x = y
    return x


def _report_scan(metric: str, qd: torch.Tensor, t: torch.Tensor, cand: torch.Tensor, scores: torch.Tensor, ids: torch.Tensor, st) -> None:
    """the reported values of knn_finish_kernel with the scan's t in place of s (plumbing on [n, k]): each is one fp32 operation"""
    n, D = qd.shape
    pad = cand < 0
    if metric == "l2":
        qsq = torch.empty(n, dtype=torch.float32, device=qd.device)
        _lib.check(_lib.load().sylber_knn_row_norms(_vp(qd), n, D, _vp(qsq), st), "sylber_knn_row_norms")
        val = torch.fmax(qsq[:, None] + t, torch.zeros_like(t))
    else:
        val = 0.0 - 0.5 * t
    scores.copy_(torch.where(pad, torch.full_like(t, float("inf")), val))
    ids.copy_(cand)


def _check_k_refine(k, refine, rerank: bool, rows_held: bool) -> Tuple[int, int]:
    """``(k, m_c)`` of a search, or ``ValueError``"""
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError("k must be an integer in [1, %d], got %r" % (MAX_K, k))
    k = int(k)
    if not rerank:
        return k, k
    if not rows_held:
        raise ValueError("rerank=True needs the fp32 rows, which were dropped: search with rerank=False")
    if isinstance(refine, bool) or int(refine) != refine or int(refine) < 1:
        raise ValueError("refine must be an integer >= 1, got %r" % (refine,))
    mc = k * int(refine)
    if mc > MAX_CANDIDATES:
        raise ValueError("k * refine = %d candidates per query, more than %d" % (mc, MAX_CANDIDATES))
    return k, mc


class PQSyllableIndex:
    """A product-quantized syllable index.  Build one with ``PQSyllableIndex.build``.  While the fp32 rows are held (``pq.index`` is
    their ``SyllableIndex``, shared and not copied when the index was built from one) ``search`` re-ranks the scan's candidates with
    the exact score; ``drop_rows()`` frees them and leaves the ``M``-byte codes as the only storage."""

    def __init__(self, index: Optional[SyllableIndex], codebooks: torch.Tensor, codes: torch.Tensor, bad: torch.Tensor, *, metric: str,
                 device: torch.device, groups: Optional[torch.Tensor] = None, prov=None, span_int: bool = False):
        self.index = index
        self.metric = metric
        self.device = device
        self.codebooks = codebooks              # [M, 256, dsub] fp32 on the device
        self._codes = codes                     # [N, M] uint8
        self._bad = bad                         # [N] uint8: 1 = a sub-row had no code, the row is never returned
        self._g = groups                        # groups / provenance of the rows once the fp32 rows are dropped
        self._prov = prov
        self._span_dtype = np.int64 if span_int else np.float64
        self._cnorm = _centroid_norms(codebooks)

    # ---- building -------------------------------------------------------------------------------------------------------------------
    @classmethod
    def build(cls, source, M: int = 48, *, codebooks=None, seed: int = 0, max_iter: int = 25, tol: float = 1e-4,
              train_rows: Optional[int] = None, groups=None, metric: str = "l2", device="cuda") -> "PQSyllableIndex":
        """``source``: a ``SyllableIndex`` (kept as ``pq.index``, not copied) or ``[N, D]`` features (then ``groups``, ``metric`` and
        ``device`` make the index).  ``D % M == 0``, ``(D / M) % 16 == 0``, ``1 <= M <= 64``.  The codebooks are ``codebooks
        [M, 256, D / M]`` as given (finite), or one ``fit_kmeans`` per sub-space on the stored rows (unit rows under ``"cosine"``):
        ``fit_kmeans(rows[:, m-th slice], 256, seed=seed + m, max_iter=, tol=, init_rows=train_rows)``, which needs at least 256
        rows.  ``ValueError`` for an empty index, a bad geometry or whatever ``fit_kmeans`` refuses."""
        index = source if isinstance(source, SyllableIndex) else SyllableIndex(source, metric=metric, groups=groups, device=device)
        if len(index) == 0:
            raise ValueError("the index is empty")
        M = _check_geometry(index.dim, M)
        C = _train_codebooks(index, M, codebooks, seed, max_iter, tol, train_rows)
        pq = cls(index, C, torch.empty((0, M), dtype=torch.uint8, device=index.device),
                 torch.empty(0, dtype=torch.uint8, device=index.device), metric=index.metric, device=index.device)
        pq._codes, pq._bad = pq.encode(index._x, _stored=True)
        return pq

    def encode(self, features, *, _stored: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """``[n, D]`` rows -> ``(codes uint8 [n, M], bad uint8 [n])`` on the device (csrc/pq.hip, ``sylber_pq_encode``: all ``M``
        sub-spaces in one launch per block of rows).  Under ``"cosine"`` the rows are made unit rows first, as ``add`` stores them."""
        x = features if _stored else self._prep(_rows(features, "features"))
        n, D = x.shape
        if D != self.dim:
            raise ValueError("features: expected D = %d, got %d" % (self.dim, D))
        return _encode(x, self.codebooks, self._cnorm)

    def _prep(self, x: torch.Tensor) -> torch.Tensor:
        """rows or queries as they are stored / scored"""
        return _prep(x, self.metric, self.device)

    def add(self, features, groups=None) -> range:
        """append ``[n, D]`` rows, encoded against the existing codebooks (no retraining); while the fp32 rows are held they go to
        ``pq.index`` as well.  The result equals ``build`` from all the rows with ``codebooks=`` these.  A refused ``add`` leaves
        everything unchanged.  Returns the new ids."""
        start = len(self)
        if self.index is not None:
            ids = self.index.add(features, groups=groups)            # validates before it appends
            if len(ids):
                c, b = self.encode(self.index._x[ids.start:ids.stop], _stored=True)
                self._codes, self._bad = torch.cat([self._codes, c]), torch.cat([self._bad, b])
            return ids
        x = _rows(features, "features")
        n, D = x.shape
        if D != self.dim:
            raise ValueError("features: expected D = %d, got %d" % (self.dim, D))
        g = _groups(groups, n, "groups") if groups is not None else np.full(n, -1, np.int32)
        if start + n >= 2 ** 31:
            raise ValueError("a PQSyllableIndex holds fewer than 2^31 rows")
        if n == 0:
            return range(start, start)
        c, b = self.encode(self._prep(x), _stored=True)
        self._codes, self._bad = torch.cat([self._codes, c]), torch.cat([self._bad, b])
        self._g = torch.cat([self._g, torch.from_numpy(g).to(self.device)])
        self._prov = np.concatenate([self._prov, np.full((n, 4), -1.0)])
        return range(start, start + n)

    def drop_rows(self) -> None:
        """free the fp32 rows: the reference to ``pq.index`` goes (the rows live on if somebody else holds that index), the groups
        and the provenance are kept.  From then on only ``rerank=False`` searches work."""
        if self.index is None:
            return
        i = self.index
        self._g, self._prov, self._span_dtype = i._g, i._prov, i._span_dtype
        self.index = None

    # ---- views ----------------------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return int(self._codes.shape[0])

    @property
    def M(self) -> int:
        return int(self.codebooks.shape[0])

    @property
    def dim(self) -> int:
        return int(self.codebooks.shape[0] * self.codebooks.shape[2])

    @property
    def codes(self) -> torch.Tensor:
        """``[N, M]`` uint8 on the device"""
        return self._codes

    @property
    def nbytes(self) -> int:
        """bytes this index holds on the device: codes, row mask, groups, codebooks with their norms, and ``4 N D`` for the fp32 rows
        while they are held (the ``4 N`` bytes of an ``"l2"`` source index's row norms are not counted)"""
        n = self._codes.numel() + self._bad.numel() + 4 * len(self) + 4 * self.codebooks.numel() + 4 * self._cnorm.numel()
        return int(n + (4 * len(self) * self.dim if self.index is not None else 0))

    def _db_groups(self) -> torch.Tensor:
        return self.index._g if self.index is not None else self._g

    def decode(self, ids) -> torch.Tensor:
        """``[len(ids), D]`` fp32 on the device: the rows' reconstruction from their codes (for ``"cosine"``, of the unit rows)"""
        a = ids if torch.is_tensor(ids) else torch.from_numpy(np.asarray(ids))
        if a.dim() != 1 or (a.numel() and (a.dtype.is_floating_point or a.dtype == torch.bool)):
            raise ValueError("ids must be a flat sequence of integers")
        a = a.to(self.device, torch.int64)
        if a.numel() and (int(a.min()) < 0 or int(a.max()) >= len(self)):
            raise ValueError("ids must lie in [0, %d)" % len(self))
        out = torch.empty((a.numel(), self.dim), dtype=torch.float32, device=self.device)
        if a.numel() == 0:
            return out
        c = self._codes.index_select(0, a)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            _lib.check(lib.sylber_pq_decode(_vp(c), c.shape[0], _vp(self.codebooks), self.M, self.dim, _vp(out), _stream(self.device)),
                       "sylber_pq_decode")
        return out

    def provenance(self, ids) -> List[Optional[Tuple[int, int, object, object]]]:
        """as ``SyllableIndex.provenance``"""
        if self.index is not None:
            return self.index.provenance(ids)
        a = np.asarray(ids.detach().cpu().numpy() if torch.is_tensor(ids) else ids, np.int64).reshape(-1)
        out = []
        for i in a.tolist():
            if i < 0 or i >= len(self) or self._prov[i, 0] < 0:
                out.append(None)
                continue
            r, st = self._prov[i], self._span_dtype
            out.append((int(r[0]), int(r[1]), st(r[2]).item(), st(r[3]).item()))
        return out

    # ---- search ---------------------------------------------------------------------------------------------------------------------
    def search(self, queries, k: int, refine: int = 4, *, rerank: Optional[bool] = None, groups=None, exclude_same_group: bool = False,
               return_candidates: bool = False, splits: int = 0, query_chunk: Optional[int] = None, _workspace_fill=None):
        """the k best rows for each query row -> ``(scores fp32 [n, k], ids int64 [n, k])`` on the device, shaped, typed, ordered
        and padded as ``SyllableIndex.search``'s (plus ``cand`` int64 ``[n, m_c]`` with ``return_candidates=True``: the scan's ids in
        scan order, padded with -1).

        ``rerank=True`` (the default while the fp32 rows are held; ``ValueError`` once they are dropped): the scan picks
        ``m_c = k * refine <= 128`` candidates and the exact fp32 score re-ranks them, so every returned score is a real ``search``
        score and with ``k * refine >= N`` the result is ``search``'s, bit for bit.  ``rerank=False``: ``m_c = k``, the scan's own
        order and scores (``refine`` is not used).  ``query_chunk`` bounds the tables (``M`` KiB per query) and the workspace;
        ``splits`` (0 = automatic) is a test hook.  Neither changes the result."""
        if rerank is None:
            rerank = self.index is not None
        k, mc = _check_k_refine(k, refine, rerank, self.index is not None)
        N = len(self)
        if N == 0:
            raise ValueError("the index is empty")
        if self.index is not None and len(self.index) != N:
            raise ValueError("pq.index holds %d rows, the codes %d: add rows through pq.add" % (len(self.index), N))
        q = _rows(queries, "queries")
        n, D = q.shape
        if D != self.dim:
            raise ValueError("queries: expected D = %d, got %d" % (self.dim, D))
        qg = None
        if exclude_same_group:
            if groups is None:
                raise ValueError("exclude_same_group needs the queries' groups")
            qg = torch.from_numpy(_groups(groups, n, "groups")).to(self.device)
        elif groups is not None:
            _groups(groups, n, "groups")
        query_chunk = DEFAULT_QUERY_CHUNK if query_chunk is None else query_chunk
        if int(splits) < 0 or int(query_chunk) < 1:
            raise ValueError("splits must be >= 0 and query_chunk >= 1")
        dev = self.device
        scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        ids = torch.empty((n, k), dtype=torch.int64, device=dev)
        cand = torch.empty((n, mc), dtype=torch.int32, device=dev)
        if n == 0:
            return (scores, ids, cand.to(torch.int64)) if return_candidates else (scores, ids)
        lib = _lib.load()
        qd = self._prep(q)
        M = self.M
        step = min(n, int(query_chunk))
        ws = torch.empty(_chunked_workspace_bytes(lib.sylber_pq_workspace_bytes, n, step, N, M, mc, int(splits)), dtype=torch.uint8, device=dev)
        if _workspace_fill is not None:
            ws.fill_(_workspace_fill)
        lut = torch.empty((step, M, KSUB), dtype=torch.float32, device=dev)
        t = torch.empty((n, mc), dtype=torch.float32, device=dev)
        metric = METRICS[self.metric]
        xg = self._db_groups() if qg is not None else None
        with torch.cuda.device(dev):
            st = _stream(dev)
            for r0 in range(0, n, step):
                r1 = min(n, r0 + step)
                _lib.check(lib.sylber_pq_lut(_vp(qd[r0:r1]), r1 - r0, D, _vp(self.codebooks), _vp(self._cnorm), M, metric, _vp(lut), st),
                           "sylber_pq_lut")
                _lib.check(lib.sylber_pq_scan(_vp(lut), r1 - r0, _vp(self._codes), _vp(self._bad), N, M, mc,
                                              _vp(qg[r0:r1] if qg is not None else None), _vp(xg), int(splits), _vp(t[r0:r1]), _vp(cand[r0:r1]),
                                              _vp(ws), st), "sylber_pq_scan")
                if rerank:
                    i = self.index
                    _lib.check(lib.sylber_knn_rerank(_vp(qd[r0:r1]), r1 - r0, _vp(i._x), N, D, _vp(i._c), metric, _vp(cand[r0:r1]), mc, k,
                                                     _vp(scores[r0:r1]), _vp(ids[r0:r1]), st), "sylber_knn_rerank")
            if not rerank:
                _report_scan(self.metric, qd, t, cand, scores, ids, st)
        return (scores, ids, cand.to(torch.int64)) if return_candidates else (scores, ids)

    # ---- persistence ----------------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """``.npz`` with the codebooks, codes, row mask, groups, provenance and metric, and the fp32 rows if they are still held.
        Loading neither trains nor encodes, so a round trip searches bit for bit the same."""
        held = self.index is not None
        i = self.index
        np.savez(path, metric=np.array(self.metric), codebooks=self.codebooks.cpu().numpy(), codes=self._codes.cpu().numpy(),
                 bad=self._bad.cpu().numpy(), groups=self._db_groups().cpu().numpy(), provenance=(i._prov if held else self._prov),
                 span_int=np.array((i._span_dtype if held else self._span_dtype) is np.int64), rows_held=np.array(held),
                 features=(i._x.cpu().numpy() if held else np.zeros((0, self.dim), np.float32)))

    @classmethod
    def load(cls, path: str, device="cuda") -> "PQSyllableIndex":
        z = np.load(path, allow_pickle=False)
        if "codebooks" not in z.files or "codes" not in z.files:
            raise ValueError("%s is not a saved PQSyllableIndex" % path)
        dev = _device(device)
        metric = str(z["metric"])
        C = torch.from_numpy(np.ascontiguousarray(z["codebooks"], np.float32)).to(dev)
        codes = torch.from_numpy(np.ascontiguousarray(z["codes"], np.uint8)).to(dev)
        bad = torch.from_numpy(np.ascontiguousarray(z["bad"], np.uint8)).to(dev)
        N = codes.shape[0]
        if C.dim() != 3 or C.shape[1] != KSUB or codes.dim() != 2 or codes.shape[1] != C.shape[0] or bad.shape != (N,) \
                or z["groups"].shape != (N,):
            raise ValueError("%s: codebooks / codes / mask / groups do not match" % path)
        _check_geometry(int(C.shape[0] * C.shape[2]), int(C.shape[0]))
        span_int = bool(z["span_int"])
        if bool(z["rows_held"]):
            idx = SyllableIndex(metric=metric, device=dev)
            idx._load_rows(z["features"], z["groups"], z["provenance"])
            if span_int:
                idx._span_dtype = np.int64
            if len(idx) != N or idx.dim != C.shape[0] * C.shape[2]:
                raise ValueError("%s: the rows do not match the codes" % path)
            return cls(idx, C, codes, bad, metric=metric, device=idx.device)
        g = torch.from_numpy(np.ascontiguousarray(z["groups"], np.int32)).to(dev)
        return cls(None, C, codes, bad, metric=metric, device=dev, groups=g, prov=np.asarray(z["provenance"], np.float64).reshape(N, 4),
                   span_int=span_int)


class IVFPQSyllableIndex:
    """An inverted file of product-quantized rows: ``IVFSyllableIndex``'s lists hold ``PQSyllableIndex``'s ``M``-byte codes, and a
    search scans, per query, the codes of the ``nprobe`` nearest lists only (csrc/pq.hip, ``sylber_ivfpq_scan``).  The contract is the
    composition of the two (tests/ivfpq_ref.py restates it in numpy)::

        list of row j      = IVFSyllableIndex's: sylber_kmeans_assign(stored rows, centroids)[j]; a row with a NaN is in no list
        code[j, :], bad    = PQSyllableIndex's, of the stored row itself (not of its residual to the list's centroid)
        lists of query i   = IVFSyllableIndex.probe: SyllableIndex(centroids, "l2").search(q_i, nprobe) (-1 for a NaN query)
        lut[i], t(i, j)    = PQSyllableIndex's table (one per query, shared by all its lists) and fp32 sum in ascending m
        candidates of i    = the m_c best rows under the strict order (t, ORIGINAL id) among the rows of the probed lists that
                             PQSyllableIndex admits; padded with (+inf, -1)
        rerank=True / False: as PQSyllableIndex.search (m_c = k refine <= 128 through sylber_knn_rerank / m_c = k, the scan's t reported)

    so with ``nprobe == nlist`` a search is ``PQSyllableIndex.search`` with the same codebooks, bit for bit, and otherwise that search
    with "the row is in a probed list" added to admissibility.  Nothing depends on ``splits``, ``query_chunk``, the workspace's
    contents or whether the rows came in one ``build`` or through ``add``.

    Build one with ``IVFPQSyllableIndex.build``.  The device holds ``M + 9`` bytes per row (code, original id, group, mask) in list
    order plus the centroids and codebooks; ``ix.index`` is the source ``SyllableIndex`` with the fp32 rows (shared, not copied)
    until ``drop_rows()``."""

    def __init__(self, index: Optional[SyllableIndex], centroids: torch.Tensor, codebooks: torch.Tensor, labels: torch.Tensor,
                 codes: torch.Tensor, bad: torch.Tensor, groups: torch.Tensor, *, metric: str, device: torch.device, prov=None,
                 span_int: bool = False):
        """``labels`` / ``codes`` / ``bad`` / ``groups``: per row in id order; they are kept in list order only"""
        self.index = index
        self.metric = metric
        self.device = device
        self.centroids = centroids              # [nlist, D] fp32 on the device
        self.codebooks = codebooks              # [M, 256, dsub] fp32 on the device
        self._coarse = SyllableIndex(centroids, metric="l2", device=device)
        self._cnorm = _centroid_norms(codebooks)
        self._prov = prov                       # provenance of the rows once the fp32 rows are dropped
        self._span_dtype = np.int64 if span_int else np.float64
        self._last = None
        self._layout(labels, codes, bad, groups)

    # ---- building -------------------------------------------------------------------------------------------------------------------
    @classmethod
    def build(cls, source, nlist: Optional[int] = None, M: int = 48, *, centroids=None, codebooks=None, seed: int = 0, max_iter: int = 25,
              tol: float = 1e-4, train_rows: Optional[int] = None, groups=None, metric: str = "l2", device="cuda") -> "IVFPQSyllableIndex":
        """``source``: a ``SyllableIndex`` (kept as ``ix.index``, not copied) or ``[N, D]`` features (then ``groups``, ``metric`` and
        ``device`` make the index).  The centroids are trained or given as for ``IVFSyllableIndex.build`` (``fit_kmeans`` on the stored
        rows with ``seed``), the codebooks as for ``PQSyllableIndex.build`` (sub-space ``m`` with ``seed + m``; at least 256 rows).
        ``ValueError`` for whatever either of them refuses."""
        index = source if isinstance(source, SyllableIndex) else SyllableIndex(source, metric=metric, groups=groups, device=device)
        if len(index) == 0:
            raise ValueError("the index is empty")
        M = _check_geometry(index.dim, M)
        Cl = IVFSyllableIndex._train_centroids(index, nlist, centroids, seed, max_iter, tol, train_rows)
        Cb = _train_codebooks(index, M, codebooks, seed, max_iter, tol, train_rows)
        codes, bad = _encode(index._x, Cb, _centroid_norms(Cb))
        return cls(index, Cl, Cb, IVFSyllableIndex._assign(index._x, Cl), codes, bad, index._g, metric=index.metric, device=index.device)

    def _layout(self, labels: torch.Tensor, codes: torch.Tensor, bad: torch.Tensor, groups: torch.Tensor) -> None:
        """IVFSyllableIndex._layout's counting sort (plumbing): list by list, ascending id within a list; the rows in no list come
        last, so that every row keeps its code"""
        nlist = self.nlist
        key = torch.where(labels < 0, torch.full_like(labels, nlist), labels).to(torch.int64)
        order = torch.sort(key, stable=True).indices
        sizes = torch.bincount(key, minlength=nlist + 1)[:nlist]
        off = torch.zeros(nlist + 1, dtype=torch.int64, device=self.device)
        off[1:] = torch.cumsum(sizes, 0)
        self.list_sizes = sizes                                         # [nlist] int64 on the device
        self._off = off.to(torch.int32)                                 # [nlist + 1] positions
        self._listed = int(off[nlist])                                  # rows in a list: the positions [0, _listed) are scanned
        self._rid = order.to(torch.int32)                               # [N] position -> original id
        self._codes = codes.index_select(0, order)                      # [N, M] uint8 in position order
        self._rbad = bad.index_select(0, order)
        self._rg = groups.index_select(0, order)

    def _by_id(self, t: torch.Tensor) -> torch.Tensor:
        """a per-position tensor in id order"""
        out = torch.empty_like(t)
        out[self._rid.to(torch.int64)] = t
        return out

    def add(self, features, groups=None) -> range:
        """append ``[n, D]`` rows: they are assigned to the existing centroids and encoded with the existing codebooks (no
        retraining), and the lists are laid out again; while the fp32 rows are held they go to ``ix.index`` as well.  The result equals
        ``build`` from all the rows with ``centroids=`` and ``codebooks=`` these.  A refused ``add`` leaves everything unchanged.
        Returns the new ids."""
        start = len(self)
        if self.index is not None:
            ids = self.index.add(features, groups=groups)                # validates before it appends
            if len(ids) == 0:
                return ids
            xd, gd = self.index._x[ids.start:ids.stop], self.index._g[ids.start:ids.stop]
        else:
            x = _rows(features, "features")
            n, D = x.shape
            if D != self.dim:
                raise ValueError("features: expected D = %d, got %d" % (self.dim, D))
            g = _groups(groups, n, "groups") if groups is not None else np.full(n, -1, np.int32)
            if start + n >= 2 ** 31:
                raise ValueError("an IVFPQSyllableIndex holds fewer than 2^31 rows")
            if n == 0:
                return range(start, start)
            xd, gd = _prep(x, self.metric, self.device), torch.from_numpy(g).to(self.device)
            self._prov = np.concatenate([self._prov, np.full((n, 4), -1.0)])
            ids = range(start, start + n)
        c, b = _encode(xd, self.codebooks, self._cnorm)
        lab = IVFSyllableIndex._assign(xd, self.centroids)
        self._layout(torch.cat([self._labels32(), lab]), torch.cat([self.codes, c]), torch.cat([self._by_id(self._rbad), b]),
                     torch.cat([self._by_id(self._rg), gd]))
        return ids

    def drop_rows(self) -> None:
        """free the fp32 rows: the reference to ``ix.index`` goes (the rows live on if somebody else holds that index), the
        provenance is kept.  From then on only ``rerank=False`` searches work."""
        if self.index is None:
            return
        self._prov, self._span_dtype = self.index._prov, self.index._span_dtype
        self.index = None

    # ---- views ----------------------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return int(self._codes.shape[0])

    @property
    def nlist(self) -> int:
        return int(self.centroids.shape[0])

    @property
    def M(self) -> int:
        return int(self.codebooks.shape[0])

    @property
    def dim(self) -> int:
        return int(self.codebooks.shape[0] * self.codebooks.shape[2])

    @property
    def codes(self) -> torch.Tensor:
        """``[N, M]`` uint8 on the device, in id order (a copy: the index holds them list by list)"""
        return self._by_id(self._codes)

    def _labels32(self) -> torch.Tensor:
        lab = torch.full((len(self),), -1, dtype=torch.int32, device=self.device)
        lab[:self._listed] = torch.repeat_interleave(torch.arange(self.nlist, dtype=torch.int32, device=self.device), self.list_sizes)
        return self._by_id(lab)

    @property
    def labels(self) -> torch.Tensor:
        """``[N]`` int64: the list of every row (-1 for a row in no list)"""
        return self._labels32().to(torch.int64)

    def list_ids(self, l: int) -> torch.Tensor:
        """the row ids of list ``l``, ascending"""
        lo, hi = (int(v) for v in self._off[int(l):int(l) + 2])
        return self._rid[lo:hi].to(torch.int64)

    @property
    def nbytes(self) -> int:
        """bytes this index holds on the device: ``M + 9`` per row (code, id, group, mask), the list offsets, the centroids and the
        codebooks with their norms, and ``4 N D`` for the fp32 rows while they are held (the ``4 N`` bytes of an ``"l2"`` source
        index's row norms are not counted)"""
        n = self._codes.numel() + 9 * len(self) + 4 * self._off.numel() + 4 * self.centroids.numel() + 4 * self.nlist \
            + 4 * self.codebooks.numel() + 4 * self._cnorm.numel()
        return int(n + (4 * len(self) * self.dim if self.index is not None else 0))

    @property
    def last_search(self) -> Optional[dict]:
        """``{"pairs", "fraction", "workspace_bytes"}`` of the last ``search``: the (query, row) pairs it scanned, their share of
        ``n N`` and the workspace it took.  Reading it waits for the device; ``search`` does not."""
        if self._last is None:
            return None
        pairs, n, N, ws = self._last
        pairs = int(pairs)
        return {"pairs": pairs, "fraction": pairs / (float(n) * N) if n else 0.0, "workspace_bytes": ws}

    def decode(self, ids) -> torch.Tensor:
        """``[len(ids), D]`` fp32 on the device: the rows' reconstruction from their codes (for ``"cosine"``, of the unit rows)"""
        a = ids if torch.is_tensor(ids) else torch.from_numpy(np.asarray(ids))
        if a.dim() != 1 or (a.numel() and (a.dtype.is_floating_point or a.dtype == torch.bool)):
            raise ValueError("ids must be a flat sequence of integers")
        a = a.to(self.device, torch.int64)
        if a.numel() and (int(a.min()) < 0 or int(a.max()) >= len(self)):
            raise ValueError("ids must lie in [0, %d)" % len(self))
        out = torch.empty((a.numel(), self.dim), dtype=torch.float32, device=self.device)
        if a.numel() == 0:
            return out
        pos = self._by_id(torch.arange(len(self), dtype=torch.int64, device=self.device))      # original id -> position
        c = self._codes.index_select(0, pos.index_select(0, a))
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().sylber_pq_decode(_vp(c), c.shape[0], _vp(self.codebooks), self.M, self.dim, _vp(out), _stream(self.device)),
                       "sylber_pq_decode")
        return out

    def provenance(self, ids) -> List[Optional[Tuple[int, int, object, object]]]:
        """as ``SyllableIndex.provenance``"""
        if self.index is not None:
            return self.index.provenance(ids)
        a = np.asarray(ids.detach().cpu().numpy() if torch.is_tensor(ids) else ids, np.int64).reshape(-1)
        out = []
        for i in a.tolist():
            if i < 0 or i >= len(self) or self._prov[i, 0] < 0:
                out.append(None)
                continue
            r, st = self._prov[i], self._span_dtype
            out.append((int(r[0]), int(r[1]), st(r[2]).item(), st(r[3]).item()))
        return out

    # ---- search ---------------------------------------------------------------------------------------------------------------------
    def _check_nprobe(self, nprobe) -> int:
        hi = min(self.nlist, MAX_NPROBE)
        if isinstance(nprobe, bool) or int(nprobe) != nprobe or not 1 <= int(nprobe) <= hi:
            raise ValueError("nprobe must be an integer in [1, min(nlist, %d) = %d], got %r" % (MAX_NPROBE, hi, nprobe))
        return int(nprobe)

    def probe(self, queries, nprobe: int) -> torch.Tensor:
        """``[n, nprobe]`` int64: the lists a search of these queries scans, nearest centroid first (-1 where a query is NaN)"""
        nprobe = self._check_nprobe(nprobe)
        q = _rows(queries, "queries")
        if q.shape[1] != self.dim:
            raise ValueError("queries: expected D = %d, got %d" % (self.dim, q.shape[1]))
        return self._coarse.search(_prep(q, self.metric, self.device), nprobe)[1]

    def search(self, queries, k: int, nprobe: int, refine: int = 4, *, rerank: Optional[bool] = None, groups=None,
               exclude_same_group: bool = False, return_candidates: bool = False, query_chunk: int = DEFAULT_QUERY_CHUNK, splits: int = 0,
               _workspace_fill=None):
        """as ``PQSyllableIndex.search`` over the rows of each query's ``nprobe`` nearest lists -> ``(scores fp32 [n, k], ids int64
        [n, k])`` on the device, ids those of the rows as they were added (plus ``cand`` int64 ``[n, m_c]`` with
        ``return_candidates=True``).  ``rerank`` defaults to whether the fp32 rows are held.  ``query_chunk`` bounds the tables
        (``M`` KiB per query) and the workspace; ``splits`` (0 = automatic) is a test hook.  Neither changes the result.  The call
        only queues work on the device's stream: it never waits for the device."""
        if rerank is None:
            rerank = self.index is not None
        k, mc = _check_k_refine(k, refine, rerank, self.index is not None)
        nprobe = self._check_nprobe(nprobe)
        N = len(self)
        if N == 0:
            raise ValueError("the index is empty")
        if self.index is not None and len(self.index) != N:
            raise ValueError("ix.index holds %d rows, the codes %d: add rows through ix.add" % (len(self.index), N))
        q = _rows(queries, "queries")
        n, D = q.shape
        if D != self.dim:
            raise ValueError("queries: expected D = %d, got %d" % (self.dim, D))
        qg = None
        if exclude_same_group:
            if groups is None:
                raise ValueError("exclude_same_group needs the queries' groups")
            qg = torch.from_numpy(_groups(groups, n, "groups")).to(self.device)
        elif groups is not None:
            _groups(groups, n, "groups")
        if int(splits) < 0 or int(query_chunk) < 1:
            raise ValueError("splits must be >= 0 and query_chunk >= 1")
        dev = self.device
        scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        ids = torch.empty((n, k), dtype=torch.int64, device=dev)
        cand = torch.empty((n, mc), dtype=torch.int32, device=dev)
        self._last = (0, 0, N, 0)
        if n == 0:
            return (scores, ids, cand.to(torch.int64)) if return_candidates else (scores, ids)
        lib = _lib.load()
        qd = _prep(q, self.metric, dev)
        M, nlist = self.M, self.nlist
        step = min(n, int(query_chunk))
        nbytes = _chunked_workspace_bytes(lib.sylber_ivfpq_workspace_bytes, n, step, nprobe, mc, int(splits))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        if _workspace_fill is not None:
            ws.fill_(_workspace_fill)
        lut = torch.empty((step, M, KSUB), dtype=torch.float32, device=dev)
        t = torch.empty((n, mc), dtype=torch.float32, device=dev)
        metric = METRICS[self.metric]
        sizes = torch.cat([self.list_sizes, torch.zeros(1, dtype=torch.int64, device=dev)])      # [-1]: a probe slot without a list
        pairs = torch.zeros((), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            st = _stream(dev)
            for r0 in range(0, n, step):
                r1 = min(n, r0 + step)
                probe = self._coarse.search(qd[r0:r1], nprobe)[1]                               # the coarse step, on the device
                pairs += sizes[probe].sum()
                probe = probe.to(torch.int32)
                _lib.check(lib.sylber_pq_lut(_vp(qd[r0:r1]), r1 - r0, D, _vp(self.codebooks), _vp(self._cnorm), M, metric, _vp(lut), st),
                           "sylber_pq_lut")
                _lib.check(lib.sylber_ivfpq_scan(_vp(lut), r1 - r0, _vp(probe), nprobe, _vp(self._off), nlist, _vp(self._codes), _vp(self._rbad),
                                                 _vp(self._rid), self._listed, M, mc, _vp(qg[r0:r1] if qg is not None else None),
                                                 _vp(self._rg if qg is not None else None), int(splits), _vp(t[r0:r1]), _vp(cand[r0:r1]),
                                                 _vp(ws), st), "sylber_ivfpq_scan")
                if rerank:
                    i = self.index
                    _lib.check(lib.sylber_knn_rerank(_vp(qd[r0:r1]), r1 - r0, _vp(i._x), N, D, _vp(i._c), metric, _vp(cand[r0:r1]), mc, k,
                                                     _vp(scores[r0:r1]), _vp(ids[r0:r1]), st), "sylber_knn_rerank")
            if not rerank:
                _report_scan(self.metric, qd, t, cand, scores, ids, st)
        self._last = (pairs, n, N, nbytes + lut.numel() * 4)
        return (scores, ids, cand.to(torch.int64)) if return_candidates else (scores, ids)

    # ---- persistence ----------------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """``.npz`` with the centroids, codebooks, every row's list, code, mask and group (in id order), the provenance and metric,
        and the fp32 rows if they are still held.  Loading neither trains, assigns nor encodes, so a round trip searches bit for bit
        the same."""
        held = self.index is not None
        i = self.index
        np.savez(path, metric=np.array(self.metric), centroids=self.centroids.cpu().numpy(), codebooks=self.codebooks.cpu().numpy(),
                 labels=self._labels32().cpu().numpy(), codes=self.codes.cpu().numpy(), bad=self._by_id(self._rbad).cpu().numpy(),
                 groups=self._by_id(self._rg).cpu().numpy(), provenance=(i._prov if held else self._prov),
                 span_int=np.array((i._span_dtype if held else self._span_dtype) is np.int64), rows_held=np.array(held),
                 features=(i._x.cpu().numpy() if held else np.zeros((0, self.dim), np.float32)))

    @classmethod
    def load(cls, path: str, device="cuda") -> "IVFPQSyllableIndex":
        z = np.load(path, allow_pickle=False)
        if "codebooks" not in z.files or "codes" not in z.files or "centroids" not in z.files or "labels" not in z.files:
            raise ValueError("%s is not a saved IVFPQSyllableIndex" % path)
        dev = _device(device)
        metric = str(z["metric"])
        Cl = torch.from_numpy(np.ascontiguousarray(z["centroids"], np.float32)).to(dev)
        Cb = torch.from_numpy(np.ascontiguousarray(z["codebooks"], np.float32)).to(dev)
        codes = torch.from_numpy(np.ascontiguousarray(z["codes"], np.uint8)).to(dev)
        bad = torch.from_numpy(np.ascontiguousarray(z["bad"], np.uint8)).to(dev)
        labels = torch.from_numpy(np.ascontiguousarray(z["labels"], np.int32)).to(dev)
        g = torch.from_numpy(np.ascontiguousarray(z["groups"], np.int32)).to(dev)
        N = codes.shape[0]
        if Cb.dim() != 3 or Cb.shape[1] != KSUB or codes.dim() != 2 or codes.shape[1] != Cb.shape[0] or bad.shape != (N,) \
                or g.shape != (N,) or labels.shape != (N,) or Cl.dim() != 2 or Cl.shape[1] != Cb.shape[0] * Cb.shape[2]:
            raise ValueError("%s: centroids / codebooks / labels / codes / mask / groups do not match" % path)
        _check_geometry(int(Cb.shape[0] * Cb.shape[2]), int(Cb.shape[0]))
        if N and (int(labels.min()) < -1 or int(labels.max()) >= Cl.shape[0]):
            raise ValueError("%s: labels outside the lists" % path)
        span_int = bool(z["span_int"])
        if bool(z["rows_held"]):
            idx = SyllableIndex(metric=metric, device=dev)
            idx._load_rows(z["features"], z["groups"], z["provenance"])
            if span_int:
                idx._span_dtype = np.int64
            if len(idx) != N or idx.dim != Cl.shape[1]:
                raise ValueError("%s: the rows do not match the codes" % path)
            return cls(idx, Cl, Cb, labels, codes, bad, idx._g, metric=metric, device=idx.device)
        return cls(None, Cl, Cb, labels, codes, bad, g, metric=metric, device=dev, prov=np.asarray(z["provenance"], np.float64).reshape(N, 4),
                   span_int=span_int)

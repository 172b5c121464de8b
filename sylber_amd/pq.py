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
lists only (``sylber_ivfpq_scan``).  tests/ivfpq_ref.py restates that composition.  With ``residual=True`` the codes are those of
each row's residual to its list's centroid (``sylber_ivfpq_scan_residual``; tests/ivfpq_residual_ref.py).  Its ``search_phrases`` is
``IVFSyllableIndex``'s seed, vote and exact re-rank on those lists; once the fp32 rows are dropped the exact DTW and ``align_phrases``
run on the codes themselves (csrc/dtw_codes.hip; tests/ivfpq_phrase_ref.py).

The two classes differ in where the codes lie and which scan reads them; what they share is written once: the rules of every index in
_index.py, and here ``_pq_search`` (the search body), ``_decode`` / ``_check_ids``, ``_saved_codes`` / ``_saved_rows`` (the file) and
the ``rerank=False`` phrase paths (``_check_rerank``, ``_rerank_codes_launch``, ``_align_codes``): with ``rerank=False`` both classes run
the exact DTW of ``search_phrases``, ``search_occurrences`` and ``align_phrases`` on the codes themselves (csrc/dtw_codes.hip) and
differ there by their ``_coded_db()`` alone."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._index import (DEFAULT_PHRASE_CHUNK, DEFAULT_QUERY_CHUNK, MAX_SEEDS, METRICS, STORAGES, _added_rows, _base_arrays, _check_k_refine,
                     _check_nprobe, _check_splits_chunk, _chunked_workspace_bytes, _group_runs, _list_layout, _on_device, _outputs, _pack16,
                     _phrase_args, _prep, _provenance, _query_groups, _result, _row_norms, _rows, _rows_of_width, _scan_phrases)
from .kmeans import _device, _stream, _vp
from .search import IVFSyllableIndex, SyllableIndex, _align_phrases, _occ_rerank_launch, _rerank_launch, _seeded_phrases

KSUB = 256                      # centroids per sub-space: one uint8 per code
MAX_M = 64                      # PQ_MAX_M of csrc/pq.hip: at least two queries' tables (M KiB each) fit beside the top lists in LDS
ENCODE_CHUNK = 1 << 20          # rows per encode launch
RESIDUAL_CHUNK = 1 << 18        # rows whose fp32 residuals exist at a time while residual codes are made
NORM_CHUNK = 1 << 16            # rows decoded at a time while the ||decode(code)||^2 of search_phrases are made


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


def _report_scan(metric: str, qd: torch.Tensor, t: torch.Tensor, cand: torch.Tensor, scores: torch.Tensor, ids: torch.Tensor) -> None:
    """the reported values of knn_finish_kernel with the scan's t in place of s (plumbing on [n, k]): each is one fp32 operation"""
    pad = cand < 0
    if metric == "l2":
        val = torch.fmax(_row_norms(qd)[:, None] + t, torch.zeros_like(t))
    else:
        val = 0.0 - 0.5 * t
    scores.copy_(torch.where(pad, torch.full_like(t, float("inf")), val))
    ids.copy_(cand)


def _pq_search(ix, name: str, queries, k: int, mc: int, rerank: bool, groups, exclude_same_group: bool, return_candidates: bool, splits,
               query_chunk, fill, size_fn, scan, ip_table: bool = False):
    """the search of both classes once ``k`` and ``m_c`` are settled -> ``(result, n, scratch bytes)``.  The class supplies
    ``size_fn(m, splits)``, the workspace of a chunk of ``m`` queries, and ``scan(lib, qc, lut, qg, splits, t, cand, ws, st)``, which
    scans for one chunk: prepared queries ``qc``, their tables, their groups or ``None``.  ``ip_table``: the inner-product table
    whatever the metric (residual codes).  Queues work only: no wait for the device."""
    N = len(ix)
    if N == 0:
        raise ValueError("the index is empty")
    if ix.index is not None and len(ix.index) != N:
        raise ValueError("%s.index holds %d rows, the codes %d: add rows through %s.add" % (name, len(ix.index), N, name))
    q = _rows_of_width(queries, ix.dim, "queries")
    n, D = q.shape
    dev = ix.device
    qg = _query_groups(groups, n, exclude_same_group, dev)
    splits, query_chunk = _check_splits_chunk(splits, query_chunk)
    scores, ids, cand = _outputs(n, k, dev, mc)
    if n == 0:
        return _result(scores, ids, cand, return_candidates), 0, 0
    lib = _lib.load()
    qd = _prep(q, ix.metric, dev)
    M = ix.M
    step = min(n, query_chunk)
    nbytes = _chunked_workspace_bytes(size_fn, n, step, splits)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    lut = torch.empty((step, M, KSUB), dtype=torch.float32, device=dev)
    t = torch.empty((n, mc), dtype=torch.float32, device=dev)
    metric = METRICS[ix.metric]
    with torch.cuda.device(dev):
        st = _stream(dev)
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            _lib.check(lib.sylber_pq_lut(_vp(qd[r0:r1]), r1 - r0, D, _vp(ix.codebooks), _vp(ix._cnorm), M, METRICS["cosine"] if ip_table else metric,
                                         _vp(lut), st), "sylber_pq_lut")
            scan(lib, qd[r0:r1], lut, qg[r0:r1] if qg is not None else None, splits, t[r0:r1], cand[r0:r1], ws, st)
            if rerank:
                i = ix.index
                _lib.check(lib.sylber_knn_rerank(_vp(qd[r0:r1]), r1 - r0, _vp(i._x), N, D, _vp(i._c), metric, _vp(cand[r0:r1]), mc, k,
                                                 _vp(scores[r0:r1]), _vp(ids[r0:r1]), st), "sylber_knn_rerank")
        if not rerank:
            _report_scan(ix.metric, qd, t, cand, scores, ids)
    return _result(scores, ids, cand, return_candidates), n, nbytes + lut.numel() * 4


def _check_ids(ids, N: int, device) -> torch.Tensor:
    """a flat sequence of ids in ``[0, N)`` -> int64 on the device"""
    a = ids if torch.is_tensor(ids) else torch.from_numpy(np.asarray(ids))
    if a.dim() != 1 or (a.numel() and (a.dtype.is_floating_point or a.dtype == torch.bool)):
        raise ValueError("ids must be a flat sequence of integers")
    a = a.to(device, torch.int64)
    if a.numel() and (int(a.min()) < 0 or int(a.max()) >= N):
        raise ValueError("ids must lie in [0, %d)" % N)
    return a


def _decode(codes: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    """code rows ``[n, M]`` -> their fp32 rows ``[n, D]`` (csrc/pq.hip, ``sylber_pq_decode``)"""
    M, _, dsub = codebooks.shape
    out = torch.empty((codes.shape[0], M * dsub), dtype=torch.float32, device=codes.device)
    if codes.shape[0]:
        with torch.cuda.device(codes.device):
            _lib.check(_lib.load().sylber_pq_decode(_vp(codes), codes.shape[0], _vp(codebooks), M, M * dsub, _vp(out), _stream(codes.device)),
                       "sylber_pq_decode")
    return out


# ---- the exact DTW on the codes: what the rerank=False phrase paths of both classes share -------------------------------------------
def _check_rerank(index: Optional[SyllableIndex], n_codes: int, rerank: Optional[bool], verb: str, name: str) -> bool:
    """``rerank`` settled (``None``: whether the fp32 rows ``index`` are held), or ``ValueError``; ``name`` is ``"pq"`` or ``"ix"``"""
    if rerank is None:
        rerank = index is not None
    if rerank and index is None:
        raise ValueError("rerank=True needs the fp32 rows, which were dropped: %s with rerank=False" % verb)
    if index is not None and len(index) != n_codes:
        raise ValueError("%s.index holds %d rows, the codes %d: add rows through %s.add" % (name, len(index), n_codes, name))
    return bool(rerank)


def _rerank_codes_launch(c, db: tuple, cn) -> None:
    """``_rerank_launch`` on a coded database, ``sylber_dtw_rerank_codes``: ``db, cn`` are what the index's ``_coded_db()`` returns"""
    b = c.b
    _lib.check(c.lib.sylber_dtw_rerank_codes(_vp(b.qp), b.nb, _vp(c.qn), _vp(c.place_d), _vp(c.len_d), int(c.cand.shape[0]), *db, c.N, c.dim,
                                             _vp(cn), c.metric, _vp(c.cand), c.m, _vp(c.off_d), c.S, c.k, _vp(c.costs), _vp(c.seqs),
                                             _vp(c.spans), _vp(c.ws), c.st), "sylber_dtw_rerank_codes")


def _align_codes(N: int, dim: int, dev, metric: str, coded_db, phrases, spans, lengths, pair_chunk, tracked: bool):
    """``align_phrases(rerank=False)`` of both classes: ``_align_phrases`` with ``sylber_dtw_align_codes`` on the real windows, so the
    row ids are the real ones.  ``coded_db()`` is called once, behind the checks: it may build the index's lazy state."""
    state = []

    def run(lib, b, qn, place_d, len_d, pair_phrase, win, max_cols, rows, steps, costs, start, ws, st):
        if not state:
            state.extend(coded_db())
        db, cn = state
        _lib.check(lib.sylber_dtw_align_codes(_vp(b.qp), b.nb, _vp(qn), _vp(place_d), _vp(len_d), b.Pc, *db, N, dim, _vp(cn), METRICS[metric],
                                              _vp(pair_phrase), _vp(win), int(pair_phrase.shape[0]), max_cols, int(rows.shape[1]),
                                              _vp(rows), _vp(steps), _vp(costs), _vp(start), _vp(ws), st), "sylber_dtw_align_codes")

    return _align_phrases(N, dim, dev, metric, phrases, spans, lengths, pair_chunk, run, tracked)


def _check_residual(residual) -> bool:
    if not isinstance(residual, (bool, np.bool_)):
        raise ValueError("residual must be a bool, got %r" % (residual,))
    return bool(residual)


def _residuals(x: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
    """``x_j - centroids[l_j]``, one fp32 subtraction per element (plumbing); a row in no list becomes a NaN row, which
    ``sylber_pq_encode`` gives code 0 and masks"""
    lab = labels.to(torch.int64)
    r = x - centroids.index_select(0, lab.clamp(min=0))
    return torch.where((lab < 0)[:, None], torch.full_like(r, float("nan")), r).contiguous()


def _encode_residual(x: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor, codebooks: torch.Tensor,
                     cnorm: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``_encode`` of the rows' residuals to their lists' centroids, ``RESIDUAL_CHUNK`` rows at a time"""
    parts = [_encode(_residuals(x[r0:r0 + RESIDUAL_CHUNK], labels[r0:r0 + RESIDUAL_CHUNK], centroids), codebooks, cnorm)
             for r0 in range(0, x.shape[0], RESIDUAL_CHUNK)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def _train_residual_codebooks(index: SyllableIndex, labels: torch.Tensor, centroids: torch.Tensor, M: int, seed: int, max_iter: int,
                              tol: float, train_rows) -> torch.Tensor:
    """``[M, 256, D / M]``: one ``fit_kmeans`` per sub-space, with ``seed + m``, on the residuals of the rows that are in a list"""
    from .kmeans import fit_kmeans
    dsub = index.dim // M
    keep = torch.nonzero(labels >= 0).flatten()
    if keep.numel() < KSUB:
        raise ValueError("training %d centroids per sub-space needs at least %d rows in a list, %d are" % (KSUB, KSUB, keep.numel()))
    lab = labels.index_select(0, keep).to(torch.int64)
    out = []
    for m in range(M):
        sl = slice(m * dsub, (m + 1) * dsub)
        r = index._x[:, sl].index_select(0, keep) - centroids[:, sl].index_select(0, lab)      # the slice of _residuals: the same bits
        out.append(fit_kmeans(r.contiguous(), KSUB, seed=seed + m, max_iter=max_iter, tol=tol, init_rows=train_rows,
                              device=index.device).centroids)
    return torch.stack(out).contiguous()


def _recon_norms(codes: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    """``||centroids[l_j] + decode(code_j)||^2`` fp32 ``[n]`` (csrc/pq.hip, ``sylber_ivfpq_recon_norms``); ``labels`` int32"""
    n, (M, _, dsub) = codes.shape[0], codebooks.shape
    out = torch.empty(n, dtype=torch.float32, device=codes.device)
    if n:
        with torch.cuda.device(codes.device):
            _lib.check(_lib.load().sylber_ivfpq_recon_norms(_vp(codes), n, _vp(labels), _vp(centroids), centroids.shape[0], _vp(codebooks), M,
                                                            M * dsub, _vp(out), _stream(codes.device)), "sylber_ivfpq_recon_norms")
    return out


def _decode_residual(codes: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    """``centroids[l_j] + decode(code_j)`` ``[n, D]`` (csrc/pq.hip, ``sylber_ivfpq_decode``); ``labels`` int32"""
    n, (M, _, dsub) = codes.shape[0], codebooks.shape
    out = torch.empty((n, M * dsub), dtype=torch.float32, device=codes.device)
    if n:
        with torch.cuda.device(codes.device):
            _lib.check(_lib.load().sylber_ivfpq_decode(_vp(codes), n, _vp(labels), _vp(centroids), centroids.shape[0], _vp(codebooks), M,
                                                       M * dsub, _vp(out), _stream(codes.device)), "sylber_ivfpq_decode")
    return out


def _saved_codes(z, path: str, dev):
    """``(codebooks, codes, bad, groups)`` of a saved file on the device, or ``ValueError`` if they do not fit each other"""
    C, codes, bad, g = (_on_device(z[key], dt, dev) for key, dt in (("codebooks", np.float32), ("codes", np.uint8), ("bad", np.uint8),
                                                                   ("groups", np.int32)))
    N = codes.shape[0]
    if C.dim() != 3 or C.shape[1] != KSUB or codes.dim() != 2 or codes.shape[1] != C.shape[0] or bad.shape != (N,) or g.shape != (N,):
        raise ValueError("%s: codebooks / codes / mask / groups do not match" % path)
    _check_geometry(int(C.shape[0] * C.shape[2]), int(C.shape[0]))
    return C, codes, bad, g


def _saved_rows(z, path: str, dev, N: int, D: int):
    """``(index, {})`` if the file holds the fp32 rows, else ``(None, the constructor's keywords for the state after drop_rows)``"""
    if not bool(z["rows_held"]):
        return None, dict(prov=np.asarray(z["provenance"], np.float64).reshape(N, 4), span_int=bool(z["span_int"]))
    idx = SyllableIndex._from_saved(z, dev)
    if len(idx) != N or idx.dim != D:
        raise ValueError("%s: the rows do not match the codes" % path)
    return idx, {}


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
        self._cnorm = _row_norms(codebooks)              # [M, 256] ||centroid||^2
        self._seq_cache = None                  # (N, default sequence offsets)
        self._cb16 = {}                         # storage -> [M, 256, dsub] 16-bit codebooks for search_phrases, built on first use
        self._rnorm = None                      # [N] ||decode(code)||^2, NaN for a masked row ("l2"), built on first use

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
        return _encode(_rows_of_width(x, self.dim, "features"), self.codebooks, self._cnorm)

    def _prep(self, x: torch.Tensor) -> torch.Tensor:
        """rows or queries as they are stored / scored"""
        return _prep(x, self.metric, self.device)

    def add(self, features, groups=None) -> range:
        """append ``[n, D]`` rows, encoded against the existing codebooks (no retraining); while the fp32 rows are held they go to
        ``pq.index`` as well.  The result equals ``build`` from all the rows with ``codebooks=`` these.  A refused ``add`` leaves
        everything unchanged.  Returns the new ids."""
        if self.index is not None:
            ids = self.index.add(features, groups=groups)            # validates before it appends
            xd = self.index._x[ids.start:ids.stop]
        else:
            xd, gd, ids, prov = _added_rows(features, groups, self.dim, len(self), "a PQSyllableIndex", self.metric, self.device)
        if not len(ids):
            return ids
        c, b = _encode(xd, self.codebooks, self._cnorm)
        self._codes, self._bad = torch.cat([self._codes, c]), torch.cat([self._bad, b])
        if self._rnorm is not None:
            self._rnorm = torch.cat([self._rnorm, self._norms_of(c, b)])
        if self.index is None:
            self._g, self._prov = torch.cat([self._g, gd]), np.concatenate([self._prov, prov])
        return ids

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
        """bytes this index holds on the device: codes, row mask, groups, codebooks with their norms, what ``search_phrases`` has
        built so far (a 16-bit copy of the codebooks per storage used, ``4 N`` of reconstruction norms under ``"l2"``), and ``4 N D``
        for the fp32 rows while they are held (the ``4 N`` bytes of an ``"l2"`` source index's row norms are not counted)"""
        n = self._codes.numel() + self._bad.numel() + 4 * len(self) + 4 * self.codebooks.numel() + 4 * self._cnorm.numel()
        n += sum(2 * c.numel() for c in self._cb16.values()) + (4 * self._rnorm.numel() if self._rnorm is not None else 0)
        return int(n + (4 * len(self) * self.dim if self.index is not None else 0))

    def _db_groups(self) -> torch.Tensor:
        return self.index._g if self.index is not None else self._g

    def decode(self, ids) -> torch.Tensor:
        """``[len(ids), D]`` fp32 on the device: the rows' reconstruction from their codes (for ``"cosine"``, of the unit rows)"""
        return _decode(self._codes.index_select(0, _check_ids(ids, len(self), self.device)), self.codebooks)

    def provenance(self, ids) -> List[Optional[Tuple[int, int, object, object]]]:
        """as ``SyllableIndex.provenance``"""
        if self.index is not None:
            return self.index.provenance(ids)
        return _provenance(self._prov, self._span_dtype, len(self), ids)

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
        N, M = len(self), self.M

        def scan(lib, qc, lut, qg, splits, t, cand, ws, st):
            _lib.check(lib.sylber_pq_scan(_vp(lut), qc.shape[0], _vp(self._codes), _vp(self._bad), N, M, mc, _vp(qg),
                                          _vp(self._db_groups() if qg is not None else None), splits, _vp(t), _vp(cand), _vp(ws), st),
                       "sylber_pq_scan")

        return _pq_search(self, "pq", queries, k, mc, rerank, groups, exclude_same_group, return_candidates, splits,
                          DEFAULT_QUERY_CHUNK if query_chunk is None else query_chunk, _workspace_fill,
                          lambda m, splits: _lib.load().sylber_pq_workspace_bytes(m, N, M, mc, splits), scan)[0]

    # ---- phrase search --------------------------------------------------------------------------------------------------------------
    def sequence_offsets(self) -> np.ndarray:
        """as ``SyllableIndex.sequence_offsets``, from the index's groups: it works after ``drop_rows()``"""
        N = len(self)
        if self._seq_cache is None or self._seq_cache[0] != N:
            self._seq_cache = (N, _group_runs(self._db_groups(), N))
        return self._seq_cache[1].copy()

    def _codebooks16(self, storage: str) -> torch.Tensor:
        """``[M, 256, dsub]``: the codebooks as ``sylber_knn16_pack`` rounds them, built on first use.  Rounding is element-wise, so a
        gather from it is the rounded reconstruction.  ``"fp16"`` raises ``ValueError`` for a finite value beyond +-65504."""
        if storage not in self._cb16:
            M, _, dsub = self.codebooks.shape
            self._cb16[storage] = _pack16(self.codebooks.reshape(M * KSUB, dsub), storage, refuse=True).reshape(M, KSUB, dsub)
        return self._cb16[storage]

    def _norms_of(self, codes: torch.Tensor, bad: torch.Tensor) -> torch.Tensor:
        """``||decode(code)||^2`` of these rows as ``_row_norms`` computes it from the decoded row, NaN for a masked row"""
        parts = [_row_norms(_decode(codes[r0:r0 + NORM_CHUNK], self.codebooks)) for r0 in range(0, codes.shape[0], NORM_CHUNK)]
        c = torch.cat(parts)
        return torch.where(bad != 0, torch.full_like(c, float("nan")), c)

    def _recon_norms(self) -> Optional[torch.Tensor]:
        """the ``c_j`` of ``search_phrases`` under ``"l2"`` (``None`` under ``"cosine"``), built on first use, ``NORM_CHUNK`` rows at a
        time: the corpus is never materialised"""
        if self.metric != "l2":
            return None
        if self._rnorm is None:
            self._rnorm = self._norms_of(self._codes, self._bad)
        return self._rnorm

    def search_phrases(self, phrases, k: int, refine: int = 4, storage: str = "fp16", *, rerank: Optional[bool] = None, lengths=None,
                       groups=None, exclude_same_group: bool = False, sequences=None, splits: int = 0,
                       phrase_chunk: int = DEFAULT_PHRASE_CHUNK, block_phrases: int = 0, return_candidates: bool = False,
                       _workspace_fill=None):
        """``SyllableIndex.search_phrases_refined`` on the codes: the same arguments, and ``(costs, seqs, spans)`` (plus ``cand`` and
        ``coarse`` with ``return_candidates=True``) shaped, typed, ordered, padded and placed exactly as there.  ``m = k * refine <=
        128`` candidate sequences per phrase in both modes.

        Stage 1 reads the codes alone (csrc/dtwpq.hip, ``sylber_dtwpq_scan``).  With ``x^_j = decode(code_j)`` (under ``"cosine"`` the
        reconstruction of the unit row, not renormalised) and ``c_j`` the fp32 ``||x^_j||^2`` (``"l2"``) or 0 (``"cosine"``), the coarse
        score is ``t(i, j) = fmaf(-2, dot16(q~_i, round16(x^_j)), c_j)``; local cost, recurrence, coarse cost and candidates are
        ``search_phrases_refined``'s word for word.  A masked row behaves as a NaN row: its local cost is ``+inf`` against every
        phrase row.  So ``cand`` and ``coarse`` are those of ``sylber_dtw16_scan`` on the plane ``pack16(decode(all codes))`` with
        ``c`` for the norms, bit for bit, and that plane is never built: the kernel gathers ``round16(x^_j)`` from a 16-bit copy of
        the codebooks.

        Stage 2, ``rerank=True`` (the default while the fp32 rows are held; ``ValueError`` once they are dropped): the exact DTW of
        ``pq.index.search_phrases`` on the fp32 rows for each candidate, so every returned cost and span is a real
        ``search_phrases`` cost and span, and with ``m`` at least the number of admissible sequences the result is
        ``pq.index.search_phrases``'s, bit for bit.  ``rerank=False`` (the only mode after ``drop_rows()``): the same exact DTW on the
        rows that ``pq.decode`` returns, a masked row being a NaN row, rebuilt from the code bytes inside the kernel's dot products
        (csrc/dtw_codes.hip, ``sylber_dtw_rerank_codes``): no decoded scratch and no copy to the host.  Under ``"l2"`` with no
        masked row the whole call equals ``SyllableIndex(pq.decode(arange(N)), metric="l2", groups=g).search_phrases_refined(...)``,
        bit for bit.  Once ``sequence_offsets()`` and the lazy state (the 16-bit codebooks, the reconstruction norms) exist, a
        ``rerank=False`` call only queues work: it never waits for the device.

        Nothing returned depends on ``splits``, ``phrase_chunk``, ``block_phrases``, stale workspace contents, how the index was
        built, whether it was saved and loaded or, with ``rerank=False``, whether the rows are still held.  ``storage="fp16"``
        refuses a finite codebook value beyond +-65504."""
        if _check_rerank(self.index, len(self), rerank, "search", "pq"):
            def stage2(c):
                _rerank_launch(c, self.index._x, self.index._c)
        else:
            def stage2(c):
                _rerank_codes_launch(c, *self._coded_db())
        return self._scan_codes(stage2, phrases, k, refine, storage, lengths, groups, exclude_same_group, sequences, splits, phrase_chunk,
                                block_phrases, return_candidates, _workspace_fill)

    def search_occurrences(self, phrases, k: int, refine: int = 4, storage: str = "fp16", *, rerank: Optional[bool] = None, lengths=None,
                           groups=None, exclude_same_group: bool = False, sequences=None, splits: int = 0,
                           phrase_chunk: int = DEFAULT_PHRASE_CHUNK, block_phrases: int = 0, return_candidates: bool = False,
                           _workspace_fill=None):
        """``SyllableIndex.search_occurrences_refined`` on the codes: every non-overlapping occurrence of each phrase in ``m = k *
        refine <= 128`` candidate sequences -> ``(costs, seqs, spans)`` as ``SyllableIndex.search_occurrences`` returns them (plus
        ``cand`` and ``coarse`` with ``return_candidates=True``).  The arguments are ``search_phrases``'s.

        Stage 1 is ``search_phrases``'s, unchanged (``sylber_dtwpq_scan``): ``cand`` and ``coarse`` are its, bit for bit.  Stage 2,
        ``rerank=True`` (the default while the fp32 rows are held; ``ValueError`` once they are dropped):
        ``sylber_dtw_rerank_occurrences`` on the fp32 rows, so the result is ``pq.index.search_occurrences`` restricted to ``cand``.
        ``rerank=False`` (the only mode after ``drop_rows()``): the same occurrences on the rows that ``pq.decode`` returns, a masked
        row being a NaN row, rebuilt from the code bytes inside the kernel's dot products (csrc/dtw_codes.hip,
        ``sylber_dtw_rerank_occurrences_codes``): no decoded scratch, no wait for the device.  Under ``"l2"`` with no masked row the
        whole call equals ``SyllableIndex(pq.decode(arange(N)), metric="l2", groups=g).search_occurrences_refined(...)``, bit for
        bit.  Stage 1 ranks a sequence by its best match: a sequence whose many occurrences are all mediocre can be left out.

        Nothing returned depends on ``splits``, ``phrase_chunk``, ``block_phrases``, stale workspace contents, how the index was
        built, whether it was saved and loaded or, with ``rerank=False``, whether the rows are still held."""
        if _check_rerank(self.index, len(self), rerank, "search", "pq"):
            def stage2(c):
                _occ_rerank_launch(c, "sylber_dtw_rerank_occurrences", (_vp(self.index._x), c.N, c.dim, _vp(self.index._c)))
        else:
            def stage2(c):
                db, cn = self._coded_db()
                _occ_rerank_launch(c, "sylber_dtw_rerank_occurrences_codes", db + (c.N, c.dim, _vp(cn)))
        return self._scan_codes(stage2, phrases, k, refine, storage, lengths, groups, exclude_same_group, sequences, splits, phrase_chunk,
                                block_phrases, return_candidates, _workspace_fill)

    def _coded_db(self):
        """the coded-database argument group of ``sylber_dtw_rerank_codes`` / ``sylber_dtw_align_codes`` up to ``nlist``, and ``c``:
        the codes lie in id order (no ``pos``) and are codes of the rows themselves (no lists)"""
        return (_vp(self._codes), _vp(self._bad), None, _vp(self.codebooks), self.M, None, None, 0), self._recon_norms()

    def _scan_codes(self, stage2, phrases, k, refine, storage, lengths, groups, exclude_same_group, sequences, splits, phrase_chunk,
                    block_phrases, return_candidates, fill):
        """``_scan_phrases`` with stage 1 = ``sylber_dtwpq_scan`` on the codes and ``stage2(c)`` behind it"""
        N = len(self)

        def stages():
            cb16, cn, code = self._codebooks16(storage), self._recon_norms(), STORAGES[storage][0]

            def scan(c):
                b = c.b
                c.ws = c.workspace(c.lib.sylber_dtw16_workspace_bytes(b.Pc, c.m, b.C))
                _lib.check(c.lib.sylber_dtwpq_scan(_vp(c.q16), b.nb, _vp(c.meta_d), _vp(c.sp_d), _vp(c.br_d), b.Pc, b.slots, _vp(self._codes),
                                                   _vp(self._bad), _vp(cb16), N, c.dim, self.M, _vp(cn), _vp(c.qn), c.metric, code, c.m,
                                                   _vp(c.seq_id), _vp(c.cut_d), b.C, _vp(c.pg_d), _vp(c.seq_grp), _vp(c.cand), _vp(c.coarse),
                                                   _vp(c.ws), c.st), "sylber_dtwpq_scan")

            return scan, stage2

        return _scan_phrases(N, self.dim, self.device, self.metric, self._db_groups(), self.sequence_offsets, stages, phrases, k, refine, storage,
                             lengths, groups, exclude_same_group, sequences, splits, phrase_chunk, block_phrases, return_candidates, fill)

    def align_phrases(self, phrases, spans, lengths=None, pair_chunk: Optional[int] = None, *, rerank: Optional[bool] = None,
                      _tracked_start: bool = False):
        """the warping paths behind the spans of ``search_phrases`` or ``search_occurrences`` -> ``(rows, steps, costs)`` as
        ``SyllableIndex.align_phrases`` returns them; ``rerank`` is what that search was given.  ``rerank=True`` (the default while the
        fp32 rows are held; ``ValueError`` once they are dropped): ``pq.index.align_phrases``, on the rows the exact re-rank ran on.
        ``rerank=False`` (the only mode after ``drop_rows()``): the same alignment on the rows that ``pq.decode`` returns, a masked
        row being a NaN row, rebuilt from the codes inside the kernel (csrc/dtw_codes.hip, ``sylber_dtw_align_codes``; no scratch,
        no wait for the device beyond the one check of the spans) -- as both searches score them with ``rerank=False``, so on their
        spans ``costs`` has the bits of its costs, and the result is ``SyllableIndex(pq.decode(arange(N)), ...).align_phrases``'s.
        Nothing returned depends on ``pair_chunk`` or, with ``rerank=False``, on whether the rows are still held."""
        if _check_rerank(self.index, len(self), rerank, "align", "pq"):
            return self.index.align_phrases(phrases, spans, lengths=lengths, pair_chunk=pair_chunk, _tracked_start=_tracked_start)
        return _align_codes(len(self), self.dim, self.device, self.metric, self._coded_db, phrases, spans, lengths, pair_chunk, _tracked_start)

    # ---- persistence ----------------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """``.npz`` with the codebooks, codes, row mask, groups, provenance and metric, and the fp32 rows if they are still held.
        Loading neither trains nor encodes, so a round trip searches bit for bit the same."""
        i = self.index
        base = i._saved() if i is not None else _base_arrays(self.metric, self.dim, None, self._g, self._prov, self._span_dtype)
        np.savez(path, **base, codebooks=self.codebooks.cpu().numpy(), codes=self._codes.cpu().numpy(), bad=self._bad.cpu().numpy(),
                 rows_held=np.array(i is not None))

    @classmethod
    def load(cls, path: str, device="cuda") -> "PQSyllableIndex":
        z = np.load(path, allow_pickle=False)
        if "codebooks" not in z.files or "codes" not in z.files:
            raise ValueError("%s is not a saved PQSyllableIndex" % path)
        dev = _device(device)
        C, codes, bad, g = _saved_codes(z, path, dev)
        idx, dropped = _saved_rows(z, path, dev, codes.shape[0], int(C.shape[0] * C.shape[2]))
        return cls(idx, C, codes, bad, metric=str(z["metric"]), device=dev, groups=(g if idx is None else None), **dropped)


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

    ``build(..., residual=True)`` codes each row's residual to its list's centroid instead, so that the codebooks do not spend their
    256 entries on where the lists lie (tests/ivfpq_residual_ref.py restates it).  Lists, probing, candidates, re-rank and reported
    values are as above; what changes::

        r_j                = x_j - centroids[l_j] on the stored row, one fp32 subtraction per element (l_j the row's list)
        codebooks          given, or codebook m = fit_kmeans(r[:, slice m] of the rows in a list, 256, seed=seed + m, ...).centroids
        code[j, :], bad    = sylber_pq_encode's of r; a row in no list gets code 0 and is masked
        xhat_j             = centroids[l_j] + decode(code_j), one fp32 addition per element: what ix.decode returns
        nrm_j              = ||xhat_j||^2, the fmaf chain from 0 in ascending column (sylber_ivfpq_recon_norms); "l2" only
        lut[i, m, c]       = fmaf(-2, q_i[slice m] . C[m, c], 0) for both metrics: still one table per query
        a[i, s]            = -2 (q_i . centroids[probe[i, s]]), the ascending fmaf chain from 0 (sylber_ivfpq_list_terms)
        t(i, j)            = (u + a[i, s]) + nrm_j ("l2") or u + a[i, s] ("cosine"), u the fp32 sum of the table entries as above and
                             s the slot of the row's list: ||q - xhat||^2 - ||q||^2, respectively -2 q . xhat

    Build one with ``IVFPQSyllableIndex.build``.  The device holds ``M + 9`` bytes per row (code, original id, group, mask) in list
    order -- ``M + 13`` with residual codes under ``"l2"`` (``nrm``) -- plus the centroids and codebooks, and 4 more (8 under ``"l2"``)
    once ``search_phrases`` or ``align_phrases`` has run with ``rerank=False``; ``ix.index`` is the source ``SyllableIndex`` with the
    fp32 rows (shared, not copied) until ``drop_rows()``."""

    def __init__(self, index: Optional[SyllableIndex], centroids: torch.Tensor, codebooks: torch.Tensor, labels: torch.Tensor,
                 codes: torch.Tensor, bad: torch.Tensor, groups: torch.Tensor, *, metric: str, device: torch.device, prov=None,
                 span_int: bool = False, residual: bool = False):
        """``labels`` / ``codes`` / ``bad`` / ``groups``: per row in id order; they are kept in list order only"""
        self.index = index
        self._residual = residual
        self.metric = metric
        self.device = device
        self.centroids = centroids              # [nlist, D] fp32 on the device
        self.codebooks = codebooks              # [M, 256, dsub] fp32 on the device
        self._coarse = SyllableIndex(centroids, metric="l2", device=device)
        self._cnorm = _row_norms(codebooks)              # [M, 256] ||centroid||^2
        self._prov = prov                       # provenance of the rows once the fp32 rows are dropped
        self._span_dtype = np.int64 if span_int else np.float64
        self._last = None
        self._seeds = None                      # what the last search_phrases keeps for last_search's "seen"
        self._seq_cache = None                  # (N, default sequence offsets)
        self._layout(labels, codes, bad, groups, self._norms_of(codes, labels))

    # ---- building -------------------------------------------------------------------------------------------------------------------
    @classmethod
    def build(cls, source, nlist: Optional[int] = None, M: int = 48, *, centroids=None, codebooks=None, seed: int = 0, max_iter: int = 25,
              tol: float = 1e-4, train_rows: Optional[int] = None, groups=None, metric: str = "l2", device="cuda",
              residual: bool = False) -> "IVFPQSyllableIndex":
        """``source``: a ``SyllableIndex`` (kept as ``ix.index``, not copied) or ``[N, D]`` features (then ``groups``, ``metric`` and
        ``device`` make the index).  The centroids are trained or given as for ``IVFSyllableIndex.build`` (``fit_kmeans`` on the stored
        rows with ``seed``), the codebooks as for ``PQSyllableIndex.build`` (sub-space ``m`` with ``seed + m``; at least 256 rows).
        ``residual=True``: the codes are those of the rows' residuals to their lists' centroids, and codebooks that are not given are
        trained on the residuals of the rows that are in a list (at least 256).  ``ValueError`` for whatever either of them refuses
        and for a ``residual`` that is no ``bool``."""
        residual = _check_residual(residual)
        index = source if isinstance(source, SyllableIndex) else SyllableIndex(source, metric=metric, groups=groups, device=device)
        if len(index) == 0:
            raise ValueError("the index is empty")
        M = _check_geometry(index.dim, M)
        Cl = IVFSyllableIndex._train_centroids(index, nlist, centroids, seed, max_iter, tol, train_rows)
        if not residual:
            Cb = _train_codebooks(index, M, codebooks, seed, max_iter, tol, train_rows)
            codes, bad = _encode(index._x, Cb, _row_norms(Cb))
            return cls(index, Cl, Cb, IVFSyllableIndex._assign(index._x, Cl), codes, bad, index._g, metric=index.metric, device=index.device)
        if codebooks is not None:
            Cb = _train_codebooks(index, M, codebooks, seed, max_iter, tol, train_rows)      # validates them
        labels = IVFSyllableIndex._assign(index._x, Cl)
        if codebooks is None:
            Cb = _train_residual_codebooks(index, labels, Cl, M, seed, max_iter, tol, train_rows)
        codes, bad = _encode_residual(index._x, labels, Cl, Cb, _row_norms(Cb))
        return cls(index, Cl, Cb, labels, codes, bad, index._g, metric=index.metric, device=index.device, residual=True)

    def _norms_of(self, codes: torch.Tensor, labels: torch.Tensor) -> Optional[torch.Tensor]:
        """``nrm`` of these rows (``[n]``, in their order) where the index keeps it: residual codes under ``"l2"``"""
        if not (self._residual and self.metric == "l2"):
            return None
        return _recon_norms(codes.contiguous(), labels.to(torch.int32).contiguous(), self.centroids, self.codebooks)

    def _layout(self, labels: torch.Tensor, codes: torch.Tensor, bad: torch.Tensor, groups: torch.Tensor,
                nrm: Optional[torch.Tensor] = None) -> None:
        """the rows in list order (plumbing): list by list, ascending id within a list; the rows in no list come last, so that
        every row keeps its code"""
        order, self.list_sizes, off = _list_layout(labels, self.nlist)  # list_sizes: [nlist] int64 on the device
        self._off = off.to(torch.int32)                                 # [nlist + 1] positions
        self._listed = int(off[-1])                                     # rows in a list: the positions [0, _listed) are scanned
        self._rid = order.to(torch.int32)                               # [N] position -> original id
        self._codes = codes.index_select(0, order)                      # [N, M] uint8 in position order
        self._rbad = bad.index_select(0, order)
        self._rg = groups.index_select(0, order)
        self._nrm = nrm.index_select(0, order) if nrm is not None else None     # [N] ||xhat||^2 in position order (residual "l2")
        self._probe_sizes = torch.cat([self.list_sizes, self.list_sizes.new_zeros(1)])      # [-1]: a probe slot without a list
        self._pos = self._pc = None             # what the phrase search on the codes adds, built on first use (_phrase_state)

    def _by_id(self, t: torch.Tensor) -> torch.Tensor:
        """a per-position tensor in id order"""
        out = torch.empty_like(t)
        out[self._rid.to(torch.int64)] = t
        return out

    def add(self, features, groups=None) -> range:
        """append ``[n, D]`` rows: they are assigned to the existing centroids and encoded with the existing codebooks (no
        retraining; with residual codes, their residuals are, and ``nrm`` is computed for them), and the lists are laid out again; while
        the fp32 rows are held they go to ``ix.index`` as well.  The result equals ``build`` from all the rows with ``centroids=`` and
        ``codebooks=`` these.  A refused ``add`` leaves everything unchanged.
        Returns the new ids."""
        if self.index is not None:
            ids = self.index.add(features, groups=groups)                # validates before it appends
            xd, gd = self.index._x[ids.start:ids.stop], self.index._g[ids.start:ids.stop]
        else:
            xd, gd, ids, prov = _added_rows(features, groups, self.dim, len(self), "an IVFPQSyllableIndex", self.metric, self.device)
        if not len(ids):
            return ids
        if self.index is None:
            self._prov = np.concatenate([self._prov, prov])
        lab = IVFSyllableIndex._assign(xd, self.centroids)
        if self._residual:
            c, b = _encode_residual(xd, lab, self.centroids, self.codebooks, self._cnorm)
        else:
            c, b = _encode(xd, self.codebooks, self._cnorm)
        nrm = torch.cat([self._by_id(self._nrm), self._norms_of(c, lab)]) if self._nrm is not None else None
        self._layout(torch.cat([self._labels32(), lab]), torch.cat([self.codes, c]), torch.cat([self._by_id(self._rbad), b]),
                     torch.cat([self._by_id(self._rg), gd]), nrm)
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
    def residual(self) -> bool:
        """whether the codes are those of the rows' residuals to their lists' centroids (``build(..., residual=True)``)"""
        return self._residual

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
        """bytes this index holds on the device: ``M + 9`` per row (code, id, group, mask; ``M + 13`` with the ``nrm`` of residual codes
        under ``"l2"``), the list offsets, the centroids and the codebooks with their norms, what ``search_phrases(rerank=False)`` has
        built so far (``4 N`` of positions, and ``4 N`` of reconstruction norms under ``"l2"``), and ``4 N D`` for the fp32 rows while
        they are held (the ``4 N`` bytes of an ``"l2"`` source index's row norms are not counted)"""
        n = self._codes.numel() + 9 * len(self) + 4 * self._off.numel() + 4 * self.centroids.numel() + 4 * self.nlist \
            + 4 * self.codebooks.numel() + 4 * self._cnorm.numel() + (4 * self._nrm.numel() if self._nrm is not None else 0) \
            + sum(4 * t.numel() for t in (self._pos, self._pc) if t is not None)
        return int(n + (4 * len(self) * self.dim if self.index is not None else 0))

    @property
    def last_search(self) -> Optional[dict]:
        """``{"pairs", "fraction", "workspace_bytes"}`` of the last ``search``: the (query, row) pairs it scanned, their share of
        ``n N`` and the workspace it took; after a ``search_phrases`` those of its stage 1a and ``"seen"``, the mean number of seen
        sequences per phrase.  Reading it waits for the device; the searches do not."""
        if self._last is None:
            return None
        pairs, n, N, ws = self._last
        pairs = int(pairs)
        out = {"pairs": pairs, "fraction": pairs / (float(n) * N) if n else 0.0, "workspace_bytes": ws}
        if self._seeds is not None:
            sc, si, off, lens = self._seeds                 # the seen sequences of each phrase, counted as the vote sees them
            P, dev = int(lens.size), self.device
            out["seen"] = 0.0
            if P:
                d = sc if self.metric == "l2" else torch.clamp_min(1.0 - sc, 0.0)
                valid = (si >= 0) & ~torch.isnan(sc) & ~torch.isposinf(d)
                seq = torch.bucketize(si, torch.from_numpy(off[1:]).to(dev), right=True)
                owner = torch.repeat_interleave(torch.arange(P, device=dev), torch.from_numpy(lens).to(dev))
                out["seen"] = float(torch.unique((owner[:, None] * (off.size - 1) + seq)[valid]).numel()) / P
        return out

    def decode(self, ids) -> torch.Tensor:
        """``[len(ids), D]`` fp32 on the device: the rows' reconstruction from their codes (for ``"cosine"``, of the unit rows); with
        residual codes the list's centroid plus the code's centroids (for a row in no list those alone)"""
        a = _check_ids(ids, len(self), self.device)
        pos = self._by_id(torch.arange(len(self), dtype=torch.int64, device=self.device))      # original id -> position
        codes = self._codes.index_select(0, pos.index_select(0, a))
        if not self._residual:
            return _decode(codes, self.codebooks)
        return _decode_residual(codes, self._labels32().index_select(0, a), self.centroids, self.codebooks)

    def provenance(self, ids) -> List[Optional[Tuple[int, int, object, object]]]:
        """as ``SyllableIndex.provenance``"""
        if self.index is not None:
            return self.index.provenance(ids)
        return _provenance(self._prov, self._span_dtype, len(self), ids)

    # ---- search ---------------------------------------------------------------------------------------------------------------------
    def probe(self, queries, nprobe: int) -> torch.Tensor:
        """``[n, nprobe]`` int64: the lists a search of these queries scans, nearest centroid first (-1 where a query is NaN)"""
        nprobe = _check_nprobe(nprobe, self.nlist)
        return self._coarse.search(_prep(_rows_of_width(queries, self.dim, "queries"), self.metric, self.device), nprobe)[1]

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
        nprobe = _check_nprobe(nprobe, self.nlist)
        M, nlist = self.M, self.nlist
        pairs = [0]                      # the rows scanned: a device tensor once a chunk has run, read only by last_search

        def scan(lib, qc, lut, qg, splits, t, cand, ws, st):
            probe = self._coarse.search(qc, nprobe)[1]                                          # the coarse step, on the device
            pairs[0] = pairs[0] + self._probe_sizes[probe].sum()
            probe = probe.to(torch.int32)
            if self._residual:
                a = torch.empty(probe.shape, dtype=torch.float32, device=self.device)
                _lib.check(lib.sylber_ivfpq_list_terms(_vp(qc), qc.shape[0], self.dim, _vp(self.centroids), nlist, _vp(probe), nprobe, _vp(a), st),
                           "sylber_ivfpq_list_terms")
                _lib.check(lib.sylber_ivfpq_scan_residual(_vp(lut), qc.shape[0], _vp(probe), nprobe, _vp(self._off), nlist, _vp(self._codes),
                                                          _vp(self._rbad), _vp(self._rid), self._listed, M, mc, _vp(qg),
                                                          _vp(self._rg if qg is not None else None), splits, _vp(a), _vp(self._nrm), _vp(t),
                                                          _vp(cand), _vp(ws), st), "sylber_ivfpq_scan_residual")
                return
            _lib.check(lib.sylber_ivfpq_scan(_vp(lut), qc.shape[0], _vp(probe), nprobe, _vp(self._off), nlist, _vp(self._codes), _vp(self._rbad),
                                             _vp(self._rid), self._listed, M, mc, _vp(qg), _vp(self._rg if qg is not None else None), splits,
                                             _vp(t), _vp(cand), _vp(ws), st), "sylber_ivfpq_scan")

        out, n, nbytes = _pq_search(self, "ix", queries, k, mc, rerank, groups, exclude_same_group, return_candidates, splits, query_chunk,
                                    _workspace_fill, lambda m, splits: _lib.load().sylber_ivfpq_workspace_bytes(m, nprobe, mc, splits), scan,
                                    ip_table=self._residual)
        self._last, self._seeds = (pairs[0], n, len(self), nbytes), None
        return out

    # ---- phrase search --------------------------------------------------------------------------------------------------------------
    def sequence_offsets(self) -> np.ndarray:
        """as ``SyllableIndex.sequence_offsets``, from the index's groups: it works after ``drop_rows()``"""
        N = len(self)
        if self._seq_cache is None or self._seq_cache[0] != N:
            self._seq_cache = (N, _group_runs(self._by_id(self._rg), N))
        return self._seq_cache[1].copy()

    def _phrase_state(self) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """what the exact DTW on the codes needs beside the lists, built on first use and dropped when ``add`` lays the lists out
        again: ``pos [N]`` int32, row id -> position, and under ``"l2"`` ``c [N]`` fp32 in id order: ``_row_norms`` of the rows that
        ``decode`` returns (``NORM_CHUNK`` at a time), NaN for a masked row -- what a ``SyllableIndex`` built from the decoded rows
        holds, and not ``_nrm``, whose chain is the scan's"""
        if self._pos is None:
            N, dev = len(self), self.device
            pos = torch.empty(N, dtype=torch.int32, device=dev)
            pos[self._rid.to(torch.int64)] = torch.arange(N, dtype=torch.int32, device=dev)
            if self.metric == "l2":
                lab = torch.full((N,), -1, dtype=torch.int32, device=dev)       # by position
                lab[:self._listed] = torch.repeat_interleave(torch.arange(self.nlist, dtype=torch.int32, device=dev), self.list_sizes)
                parts = []
                for r0 in range(0, N, NORM_CHUNK):
                    c = self._codes[r0:r0 + NORM_CHUNK]
                    parts.append(_row_norms(_decode_residual(c, lab[r0:r0 + NORM_CHUNK].contiguous(), self.centroids, self.codebooks)
                                            if self._residual else _decode(c, self.codebooks)))
                c = torch.cat(parts)
                self._pc = self._by_id(torch.where(self._rbad != 0, torch.full_like(c, float("nan")), c))
            self._pos = pos
        return self._pos, self._pc

    def _coded_db(self):
        """the coded-database argument group of ``sylber_dtw_rerank_codes`` / ``sylber_dtw_align_codes`` up to ``nlist``, and ``c``"""
        pos, pc = self._phrase_state()
        lists = (_vp(self._off), _vp(self.centroids), self.nlist) if self._residual else (None, None, 0)
        return (_vp(self._codes), _vp(self._rbad), _vp(pos), _vp(self.codebooks), self.M) + lists, pc

    def search_phrases(self, phrases, k: int, nprobe: int, seeds: int = 32, refine: int = 4, *, rerank: Optional[bool] = None, lengths=None,
                       groups=None, exclude_same_group: bool = False, sequences=None, query_chunk: int = DEFAULT_QUERY_CHUNK,
                       phrase_chunk: int = DEFAULT_PHRASE_CHUNK, splits: int = 0, return_candidates: bool = False, _workspace_fill=None):
        """``IVFSyllableIndex.search_phrases`` on the compressed lists: seed, vote, exact re-rank -> ``(costs, seqs, spans)`` as
        ``SyllableIndex.search_phrases`` returns them (plus ``cand`` int64 ``[P, m]`` and ``bound`` fp32 ``[P, m]`` with
        ``return_candidates=True``).  The arguments are those of ``IVFSyllableIndex.search_phrases`` with ``rerank=`` added and
        ``splits=`` (``search``'s test hook) in place of ``item_tiles=``; ``1 <= seeds <= 128``, ``m = k * refine <= 128``.

        Stage 1a: ``ix.search(all phrase rows, k=seeds, nprobe, refine=1, rerank=rerank)``; with ``exclude_same_group`` and the
        default sequences every row carries its phrase's group, with explicit ``sequences=`` stage 1a excludes nothing and the vote
        drops the excluded sequences.  Stage 1b: ``sylber_phrase_vote`` on what stage 1a reported (the contract of
        ``SyllableIndex.search_phrases_seeded``).

        Stage 2, ``rerank=True`` (the default while the fp32 rows are held; ``ValueError`` once they are dropped):
        ``ix.index.search_phrases_seeded``, so every returned cost and span is a real ``search_phrases`` cost and span, bit for bit.
        ``rerank=False`` (the only mode after ``drop_rows()``): the same exact DTW on the rows that ``ix.decode`` returns, a masked row
        being a NaN row (``+inf`` against every phrase row).  The rows are rebuilt from the code bytes, the codebooks and, for residual
        codes, the list centroids inside the kernel's dot products (csrc/dtw_codes.hip, ``sylber_dtw_rerank_codes``): there is no
        decoded scratch and no copy to the host.  Under ``"l2"`` with no masked row the whole call equals
        ``SyllableIndex(ix.decode(arange(N)), metric="l2", groups=g).search_phrases_seeded(phrases, *ix.search(rows, seeds, nprobe,
        rerank=False), k, refine)``, bit for bit.

        ``bound`` ranks the candidates and certifies nothing, in either mode: with ``rerank=False`` the seeds' scores are sums of
        table entries, not the ``d`` of the DTW's chain; with ``rerank=True`` the seeds are the best of the scan's candidates, not
        each row's nearest rows.  So ``bound <= cost`` does not hold in general.

        ``rerank=False`` needs ``pos`` (4 bytes per row) and under ``"l2"`` the norms of the reconstructions (4 more), built on the
        first call, rebuilt after ``add``, counted in ``nbytes`` and not saved.  Once they and ``sequence_offsets()`` exist, a
        ``rerank=False`` call only queues work: it never waits for the device.  ``ix.last_search`` keeps stage 1a's numbers and adds
        ``"seen"``, both computed when it is read.  Nothing returned depends on ``query_chunk``, ``phrase_chunk``, ``splits``, stale
        workspaces, ``build`` versus ``build`` + ``add``, a ``save`` / ``load`` round trip or, with ``rerank=False``, on whether the
        rows are still held.  ``ValueError`` before any launch: what ``IVFSyllableIndex.search_phrases`` and ``ix.search`` refuse,
        ``rerank=True`` without the rows, an ``ix.index`` of another length."""
        return self._seeded_codes(False, phrases, k, nprobe, seeds, refine, rerank, lengths, groups, exclude_same_group, sequences, query_chunk,
                                  phrase_chunk, splits, return_candidates, _workspace_fill)

    def search_occurrences(self, phrases, k: int, nprobe: int, seeds: int = 32, refine: int = 4, *, rerank: Optional[bool] = None,
                           lengths=None, groups=None, exclude_same_group: bool = False, sequences=None,
                           query_chunk: int = DEFAULT_QUERY_CHUNK, phrase_chunk: int = DEFAULT_PHRASE_CHUNK, splits: int = 0,
                           return_candidates: bool = False, _workspace_fill=None):
        """every non-overlapping occurrence of each phrase on the compressed lists -> ``(costs, seqs, spans)`` as
        ``SyllableIndex.search_occurrences`` returns them (plus ``cand`` and ``bound`` with ``return_candidates=True``).  The
        arguments are ``search_phrases``'s.  Stages 1a and 1b are ``search_phrases``'s, unchanged: ``cand`` and ``bound`` are its, bit
        for bit, for the same ``rerank``.

        Stage 2, ``rerank=True`` (the default while the fp32 rows are held; ``ValueError`` once they are dropped):
        ``ix.index.search_occurrences_seeded`` on ``ix.search``'s seeds, so the result is ``ix.index.search_occurrences`` restricted
        to ``cand``.  ``rerank=False`` (the only mode after ``drop_rows()``): the same occurrences on the rows that ``ix.decode``
        returns, a masked row being a NaN row, rebuilt inside the kernel's dot products (csrc/dtw_codes.hip,
        ``sylber_dtw_rerank_occurrences_codes``): no decoded scratch, and once the lazy state of ``search_phrases(rerank=False)``
        exists the call only queues work.  Stage 1 ranks a sequence by a bound on its best match: a sequence whose many occurrences
        are all mediocre can be left out.

        Nothing returned depends on ``query_chunk``, ``phrase_chunk``, ``splits``, stale workspaces, ``build`` versus ``build`` +
        ``add``, a ``save`` / ``load`` round trip or, with ``rerank=False``, on whether the rows are still held.  Refusals are
        ``search_phrases``'s."""
        return self._seeded_codes(True, phrases, k, nprobe, seeds, refine, rerank, lengths, groups, exclude_same_group, sequences, query_chunk,
                                  phrase_chunk, splits, return_candidates, _workspace_fill)

    def _seeded_codes(self, occurrences: bool, phrases, k, nprobe, seeds, refine, rerank, lengths, groups, exclude_same_group, sequences,
                      query_chunk, phrase_chunk, splits, return_candidates, _workspace_fill):
        """``search_phrases`` (one match per candidate sequence) or ``search_occurrences`` (every occurrence in it): the checks, stage 1a
        and, by ``rerank``, the seeded search of ``ix.index`` or the vote and the DTW on the codes"""
        rerank = _check_rerank(self.index, len(self), rerank, "search", "ix")
        N, dev = len(self), self.device
        k, m = _check_k_refine(k, refine, rerank=True)
        nprobe = _check_nprobe(nprobe, self.nlist)
        if isinstance(seeds, bool) or int(seeds) != seeds or not 1 <= int(seeds) <= MAX_SEEDS:
            raise ValueError("seeds must be an integer in [1, %d], got %r" % (MAX_SEEDS, seeds))
        seeds = int(seeds)
        q, lens, pg, off = _phrase_args(N, self.dim, dev, self.sequence_offsets, phrases, lengths, groups, exclude_same_group, sequences, 0,
                                        phrase_chunk, 0)
        _check_splits_chunk(splits, query_chunk)
        own = pg is not None and sequences is None             # the rows' groups decide the default sequences: exclude in stage 1a
        sc, si = self.search(q, seeds, nprobe, 1, rerank=rerank, groups=np.repeat(pg, lens) if own else None, exclude_same_group=own,
                             query_chunk=query_chunk, splits=splits, _workspace_fill=_workspace_fill)
        self._seeds = (sc, si, off, lens)
        if rerank:
            kw = dict(lengths=lens, groups=groups, exclude_same_group=exclude_same_group, sequences=sequences, phrase_chunk=phrase_chunk,
                      return_candidates=return_candidates, _trusted_ids=True)
            if occurrences:
                return self.index.search_occurrences_seeded(q, sc, si, k, refine, _workspace_fill=_workspace_fill, **kw)
            return self.index.search_phrases_seeded(q, sc, si, k, refine, **kw)
        db, pc = self._coded_db()

        def occ_codes(c):
            _occ_rerank_launch(c, "sylber_dtw_rerank_occurrences_codes", db + (N, c.dim, _vp(pc)))

        return _seeded_phrases(N, self.dim, dev, self.metric, self._by_id(self._rg), q, lens, pg, off, sc, si, k, m, phrase_chunk,
                               return_candidates, occ_codes if occurrences else (lambda c: _rerank_codes_launch(c, db, pc)), _workspace_fill)

    def align_phrases(self, phrases, spans, lengths=None, pair_chunk: Optional[int] = None, *, rerank: Optional[bool] = None,
                      _tracked_start: bool = False):
        """the warping paths behind the spans of ``search_phrases`` or ``search_occurrences`` -> ``(rows, steps, costs)`` as
        ``SyllableIndex.align_phrases`` returns them; ``rerank`` is what that search was given.  ``rerank=True`` (the default while the
        fp32 rows are held; ``ValueError`` once they are dropped): ``ix.index.align_phrases``, on the rows the exact re-rank ran on.
        ``rerank=False``: the same alignment on the rows that ``ix.decode`` returns, rebuilt from the codes inside the kernel
        (csrc/dtw_codes.hip, ``sylber_dtw_align_codes``; no scratch) -- so on spans from ``search_phrases(rerank=False)`` or
        ``search_occurrences(rerank=False)`` ``costs`` has the bits of that search's costs, before and after ``drop_rows()``.  Nothing returned depends on ``pair_chunk``."""
        if _check_rerank(self.index, len(self), rerank, "align", "ix"):
            return self.index.align_phrases(phrases, spans, lengths=lengths, pair_chunk=pair_chunk, _tracked_start=_tracked_start)
        return _align_codes(len(self), self.dim, self.device, self.metric, self._coded_db, phrases, spans, lengths, pair_chunk, _tracked_start)

    # ---- persistence ----------------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """``.npz`` with the centroids, codebooks, every row's list, code, mask and group (in id order), the provenance and metric,
        a ``residual`` entry if the codes are residual codes (without them the file is what it always was), and the fp32 rows if they
        are still held.  Loading neither trains, assigns nor encodes
        (``nrm`` is computed again from the codes, lists, centroids and codebooks: the same bits), so a round trip searches bit for
        bit the same."""
        i = self.index
        base = i._saved() if i is not None else _base_arrays(self.metric, self.dim, None, self._by_id(self._rg), self._prov, self._span_dtype)
        np.savez(path, **base, centroids=self.centroids.cpu().numpy(), codebooks=self.codebooks.cpu().numpy(),
                 labels=self._labels32().cpu().numpy(), codes=self.codes.cpu().numpy(), bad=self._by_id(self._rbad).cpu().numpy(),
                 rows_held=np.array(i is not None), **({"residual": np.array(True)} if self._residual else {}))

    @classmethod
    def load(cls, path: str, device="cuda") -> "IVFPQSyllableIndex":
        z = np.load(path, allow_pickle=False)
        if "codebooks" not in z.files or "codes" not in z.files or "centroids" not in z.files or "labels" not in z.files:
            raise ValueError("%s is not a saved IVFPQSyllableIndex" % path)
        dev = _device(device)
        Cb, codes, bad, g = _saved_codes(z, path, dev)
        Cl, labels = _on_device(z["centroids"], np.float32, dev), _on_device(z["labels"], np.int32, dev)
        N, D = codes.shape[0], int(Cb.shape[0] * Cb.shape[2])
        if labels.shape != (N,) or Cl.dim() != 2 or Cl.shape[1] != D:
            raise ValueError("%s: centroids / labels do not match the codes" % path)
        if N and (int(labels.min()) < -1 or int(labels.max()) >= Cl.shape[0]):
            raise ValueError("%s: labels outside the lists" % path)
        idx, dropped = _saved_rows(z, path, dev, N, D)
        residual = bool(z["residual"]) if "residual" in z.files else False     # a file from before residual codes
        return cls(idx, Cl, Cb, labels, codes, bad, g, metric=str(z["metric"]), device=dev, residual=residual, **dropped)

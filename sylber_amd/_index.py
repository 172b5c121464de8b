"""The host rules that the four syllable indexes share (search.py: ``SyllableIndex``, ``IVFSyllableIndex``; pq.py: ``PQSyllableIndex``,
``IVFPQSyllableIndex``), each written once: what a search accepts (``k`` / ``refine``, ``nprobe``, ``splits`` / ``query_chunk``, query
rows, query groups), how rows are stored (``_prep``, ``_row_norms``), where a search puts its results, what ``provenance`` answers, how
rows are sorted into lists, and how the common arrays reach an ``.npz`` and come back.  Private: the classes are the public surface."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .kmeans import _stream, _vp

METRICS = {"l2": 0, "cosine": 1}        # SYLBER_KNN_L2, SYLBER_KNN_IP (cosine = inner product on unit rows)
MAX_K = 128
DEFAULT_QUERY_CHUNK = 8192
MAX_NPROBE = 128
MAX_CANDIDATES = 128            # k * refine of a two-stage search: the LDS top-list of the scan beside a 128-row query block


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def _rows(a, what: str) -> torch.Tensor:
    """a [n, D] tensor or array -> a 2-D tensor (any device), refusing what cannot become fp32"""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))
    if t.dim() != 2:
        raise ValueError("%s must be [n, D], got %s" % (what, tuple(t.shape)))
    if not (t.dtype.is_floating_point or t.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)):
        raise ValueError("%s: dtype %s cannot be cast to float32" % (what, t.dtype))
    return t


def _rows_of_width(a, dim: Optional[int], what: str) -> torch.Tensor:
    """``_rows`` for an index of width ``dim`` (``None``: an empty index, which takes any multiple of 16)"""
    t = _rows(a, what)
    D = t.shape[1]
    if dim is None:
        if D < 16 or D % 16:
            raise ValueError("%s: the feature width D must be a multiple of 16, got %d" % (what, D))
    elif D != dim:
        raise ValueError("%s: expected D = %d, got %d" % (what, dim, D))
    return t


def _groups(g, n: int, what: str) -> np.ndarray:
    a = np.asarray(g.detach().cpu().numpy() if torch.is_tensor(g) else g)
    if a.ndim == 0:
        a = np.full(n, a)
    if a.shape != (n,):
        raise ValueError("%s must have one entry per row (%d), got shape %s" % (what, n, a.shape))
    if a.dtype.kind not in "iub":
        raise ValueError("%s must be integers, got %s" % (what, a.dtype))
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError("%s must fit in int32" % what)
    return a.astype(np.int32)


def _query_groups(groups, n: int, exclude_same_group: bool, device, whose: str = "queries"):
    """the int32 ``[n]`` groups that the exclusion compares, on ``device`` (``None``: as a host array), or ``None`` without
    ``exclude_same_group``; groups that are given are validated either way"""
    if groups is None:
        if exclude_same_group:
            raise ValueError("exclude_same_group needs the %s' groups" % whose)
        return None
    g = _groups(groups, n, "groups")
    if not exclude_same_group:
        return None
    return g if device is None else torch.from_numpy(g).to(device)


def _check_k_refine(k, refine=1, rerank: bool = False, rows_held: bool = True) -> Tuple[int, int]:
    """``(k, m_c)`` of a search, or ``ValueError``: ``m_c = k refine`` candidates with ``rerank``, else ``m_c = k``"""
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


def _check_nprobe(nprobe, nlist: int) -> int:
    hi = min(nlist, MAX_NPROBE)
    if isinstance(nprobe, bool) or int(nprobe) != nprobe or not 1 <= int(nprobe) <= hi:
        raise ValueError("nprobe must be an integer in [1, min(nlist, %d) = %d], got %r" % (MAX_NPROBE, hi, nprobe))
    return int(nprobe)


def _check_splits_chunk(splits, query_chunk, what: str = "splits") -> Tuple[int, int]:
    if int(splits) < 0 or int(query_chunk) < 1:
        raise ValueError("%s must be >= 0 and query_chunk >= 1" % what)
    return int(splits), int(query_chunk)


def _chunked_workspace_bytes(size_fn, n: int, step: int, *rest) -> int:
    """the workspace that serves every chunk of n queries taken ``step`` at a time: with automatic splits a shorter last chunk gets
    MORE splits than a full one and can need more bytes, so the buffer is the larger of the two sizes"""
    need = int(size_fn(step, *rest))
    if n % step:
        need = max(need, int(size_fn(n % step, *rest)))
    return need


# ---- rows --------------------------------------------------------------------------------------------------------------------------
def _prep(x: torch.Tensor, metric: str, device: torch.device) -> torch.Tensor:
    """rows or queries as they are stored / scored: fp32, contiguous, on the device, unit rows under "cosine" """
    x = x.to(device, torch.float32).contiguous()
    if metric == "cosine" and x.shape[0]:
        y = torch.empty_like(x)
        with torch.cuda.device(device):
            _lib.check(_lib.load().sylber_knn_unit_rows(_vp(x), x.shape[0], x.shape[1], _vp(y), _stream(device)), "sylber_knn_unit_rows")
        x = y
    return x


def _row_norms(x: torch.Tensor) -> torch.Tensor:
    """``||row||^2`` fp32 over the last axis of a contiguous fp32 device tensor with at least one row (``sylber_knn_row_norms``)"""
    out = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().sylber_knn_row_norms(_vp(x), out.numel(), x.shape[-1], _vp(out), _stream(x.device)), "sylber_knn_row_norms")
    return out


def _added_rows(features, groups, dim: Optional[int], start: int, a_class: str, metric: str, device):
    """``[n, D]`` rows for an index that holds ``start`` rows of width ``dim`` -> ``(stored rows, groups on the device, their ids,
    filler provenance)``; with no rows only the (empty) ids are not ``None``.  ``ValueError`` before anything touches the device."""
    x = _rows_of_width(features, dim, "features")
    n = x.shape[0]
    g = _groups(groups, n, "groups") if groups is not None else np.full(n, -1, np.int32)
    if start + n >= 2 ** 31:
        raise ValueError("%s holds fewer than 2^31 rows" % a_class)
    if n == 0:
        return None, None, range(start, start), None
    return _prep(x, metric, device), torch.from_numpy(g).to(device), range(start, start + n), np.full((n, 4), -1.0)


def _list_layout(labels: torch.Tensor, nlist: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """the counting sort of rows into lists: ``labels [N]`` (-1 = in no list) -> ``(order [N] int64, sizes [nlist] int64, offsets
    [nlist + 1] int64)`` on the labels' device.  ``order`` lists the row ids list by list, ascending within a list, the rows in no
    list last; list ``l`` is ``order[offsets[l] : offsets[l + 1]]``."""
    key = torch.where(labels < 0, torch.full_like(labels, nlist), labels).to(torch.int64)
    order = torch.sort(key, stable=True).indices
    sizes = torch.bincount(key, minlength=nlist + 1)[:nlist]
    off = torch.zeros(nlist + 1, dtype=torch.int64, device=labels.device)
    off[1:] = torch.cumsum(sizes, 0)
    return order, sizes, off


# ---- results -----------------------------------------------------------------------------------------------------------------------
def _outputs(n: int, k: int, device, mc: Optional[int] = None):
    """``(scores fp32 [n, k], ids int64 [n, k])`` of a search, and ``cand int32 [n, mc]`` for a two-stage one"""
    scores = torch.empty((n, k), dtype=torch.float32, device=device)
    ids = torch.empty((n, k), dtype=torch.int64, device=device)
    return (scores, ids) if mc is None else (scores, ids, torch.empty((n, mc), dtype=torch.int32, device=device))


def _result(scores, ids, cand, return_candidates: bool):
    return (scores, ids, cand.to(torch.int64)) if return_candidates else (scores, ids)


def _provenance(prov, span_dtype, N: int, ids) -> List[Optional[Tuple[int, int, object, object]]]:
    """``(clip, segment, start, end)`` from ``prov [N, 4]`` for each of ``ids``; ``None`` for ids outside ``[0, N)`` and rows without"""
    a = np.asarray(ids.detach().cpu().numpy() if torch.is_tensor(ids) else ids, np.int64).reshape(-1)
    out = []
    for i in a.tolist():
        if i < 0 or i >= N or prov[i, 0] < 0:
            out.append(None)
            continue
        r = prov[i]
        out.append((int(r[0]), int(r[1]), span_dtype(r[2]).item(), span_dtype(r[3]).item()))
    return out


# ---- persistence -------------------------------------------------------------------------------------------------------------------
def _on_device(a, dtype, device) -> torch.Tensor:
    """a saved array of this numpy dtype onto the device"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(device)


def _base_arrays(metric: str, dim: Optional[int], x, g, prov, span_dtype) -> dict:
    """the arrays every saved index holds; ``x = None``: the fp32 rows were dropped, ``features`` is ``[0, D]``"""
    N = 0 if g is None else int(g.shape[0])
    return dict(metric=np.array(metric), features=(x.cpu().numpy() if N and x is not None else np.zeros((0, dim or 16), np.float32)),
                groups=(g.cpu().numpy() if N else np.zeros(0, np.int32)), provenance=(prov if N else np.zeros((0, 4))),
                span_int=np.array(span_dtype is np.int64))

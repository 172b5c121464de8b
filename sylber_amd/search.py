"""Exact k-nearest-neighbour search over syllable embeddings: ``SyllableIndex``.  The database lives on the device as fp32 rows; the
hot path is HIP (csrc/knn.hip, ``sylber_knn_search``): the exact-fp32 MFMA contraction of the k-means assign with a running top-k in
its epilogue, the database split across the chip, the partial lists merged on the device.  No ``[n, N]`` distance matrix is written.

Contract (tests/knn_ref.py restates it in numpy)::

    s(i, j) = ||x_j||^2 - 2 q_i . x_j      (metric "l2")        reported: max(0, ||q_i||^2 + s)   (squared L2 distance)
    s(i, j) = -2 q_i . x_j                 (metric "cosine",    reported: -s / 2                 (cosine similarity)
                                            q and x unit rows)
    each list ordered by (s, j) ascending: the better score first, then the smaller id; NaN scores never returned;
    with exclude_same_group, candidates whose group equals the query's are skipped;
    rows with fewer than k admissible candidates are padded with id -1 and score +inf.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .kmeans import _device, _stream, _vp

METRICS = {"l2": 0, "cosine": 1}        # SYLBER_KNN_L2, SYLBER_KNN_IP (cosine = inner product on unit rows)
MAX_K = 128
DEFAULT_QUERY_CHUNK = 8192


def _rows(a, what: str) -> torch.Tensor:
    """a [n, D] tensor or array -> a 2-D tensor (any device), refusing what cannot become fp32"""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))
    if t.dim() != 2:
        raise ValueError("%s must be [n, D], got %s" % (what, tuple(t.shape)))
    if not (t.dtype.is_floating_point or t.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)):
        raise ValueError("%s: dtype %s cannot be cast to float32" % (what, t.dtype))
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


class SyllableIndex:
    """A device-resident database of syllable embeddings with exact k-NN search.

    ``SyllableIndex(features=None, *, metric="l2" | "cosine", groups=None, device="cuda")``.  Rows are stored as fp32 ``[N, D]``
    (``D % 16 == 0``); for ``"l2"`` their squared norms, for ``"cosine"`` the rows are stored normalised to unit length (a zero row
    stays zero and so has similarity 0 with every query).  ``groups`` (one integer per row, e.g. the clip id) drives
    ``search(..., exclude_same_group=True)``; rows added without groups get group -1."""

    def __init__(self, features=None, *, metric: str = "l2", groups=None, device="cuda"):
        if metric not in METRICS:
            raise ValueError("metric must be 'l2' or 'cosine', got %r" % (metric,))
        self.metric = metric
        self.device = _device(device)
        self.dim: Optional[int] = None
        self._x = None              # [N, D] fp32 (unit rows for cosine)
        self._c = None              # [N] ||x||^2 (l2)
        self._g = None              # [N] int32 groups on the device
        self._prov = None           # [N, 4] int64/float provenance (clip, segment, start, end), or None
        self._span_dtype = np.float64
        if features is not None:
            self.add(features, groups=groups)

    def __len__(self) -> int:
        return 0 if self._x is None else int(self._x.shape[0])

    @property
    def features(self) -> torch.Tensor:
        """the stored ``[N, D]`` fp32 rows (unit rows for ``"cosine"``)"""
        return self._x

    # ---- building -------------------------------------------------------------------------------------------------------------------
    def _prep(self, x: torch.Tensor) -> torch.Tensor:
        lib = _lib.load()
        x = x.to(self.device, torch.float32).contiguous()
        if self.metric == "cosine" and x.shape[0]:
            y = torch.empty_like(x)
            with torch.cuda.device(self.device):
                _lib.check(lib.sylber_knn_unit_rows(_vp(x), x.shape[0], x.shape[1], _vp(y), _stream(self.device)), "sylber_knn_unit_rows")
            x = y
        return x

    def _check_width(self, D: int, what: str) -> None:
        if self.dim is None:
            if D < 16 or D % 16:
                raise ValueError("%s: the feature width D must be a multiple of 16, got %d" % (what, D))
        elif D != self.dim:
            raise ValueError("%s: expected D = %d, got %d" % (what, self.dim, D))

    def add(self, features, groups=None, *, _prov=None) -> range:
        """append ``[m, D]`` rows (tensor or array, host or device; cast to fp32) with optional ``groups [m]``; returns their ids"""
        x = _rows(features, "features")
        m, D = x.shape
        self._check_width(D, "features")
        g = _groups(groups, m, "groups") if groups is not None else np.full(m, -1, np.int32)
        if len(self) + m >= 2 ** 31:
            raise ValueError("a SyllableIndex holds fewer than 2^31 rows")
        start = len(self)
        if m == 0:
            return range(start, start)
        lib = _lib.load()
        xd = self._prep(x)
        gd = torch.from_numpy(g).to(self.device)
        c = None
        if self.metric == "l2":
            c = torch.empty(m, dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(lib.sylber_knn_row_norms(_vp(xd), m, D, _vp(c), _stream(self.device)), "sylber_knn_row_norms")
        prov = np.full((m, 4), -1.0) if _prov is None else np.asarray(_prov, np.float64).reshape(m, 4)
        if self._x is None:
            self.dim, self._x, self._c, self._g, self._prov = D, xd, c, gd, prov
        else:
            self._x = torch.cat([self._x, xd])
            self._c = torch.cat([self._c, c]) if c is not None else None
            self._g = torch.cat([self._g, gd])
            self._prov = np.concatenate([self._prov, prov])
        return range(start, start + m)

    @classmethod
    def from_outputs(cls, outs: Sequence[dict], *, metric: str = "l2", device="cuda") -> "SyllableIndex":
        """an index over the ``segment_features`` of a list of ``Segmenter`` output dicts, one group per clip (its position in
        ``outs``), with provenance ``(clip, segment, start, end)`` from each clip's ``segments``"""
        idx = cls(metric=metric, device=device)
        for ci, o in enumerate(outs):
            f = np.asarray(o["segment_features"])
            segs = np.asarray(o["segments"])
            if f.size == 0:
                continue
            if f.ndim != 2 or segs.shape != (f.shape[0], 2):
                raise ValueError("clip %d: segment_features %s and segments %s do not match" % (ci, f.shape, segs.shape))
            m = f.shape[0]
            prov = np.column_stack([np.full(m, ci), np.arange(m), segs[:, 0], segs[:, 1]]).astype(np.float64)
            idx.add(f, groups=np.full(m, ci, np.int32), _prov=prov)
            if np.issubdtype(segs.dtype, np.integer):
                idx._span_dtype = np.int64
        return idx

    def provenance(self, ids) -> List[Optional[Tuple[int, int, object, object]]]:
        """``(clip, segment, start, end)`` for each id of a flat sequence or array of ids (``None`` for -1 and for rows added
        without provenance); ``start, end`` in the unit of the outputs' ``segments``"""
        a = np.asarray(ids.detach().cpu().numpy() if torch.is_tensor(ids) else ids, np.int64).reshape(-1)
        out = []
        for i in a.tolist():
            if i < 0 or i >= len(self) or self._prov[i, 0] < 0:
                out.append(None)
                continue
            r = self._prov[i]
            st = self._span_dtype
            out.append((int(r[0]), int(r[1]), st(r[2]).item(), st(r[3]).item()))
        return out

    # ---- search ---------------------------------------------------------------------------------------------------------------------
    def search(self, queries, k: int, *, groups=None, exclude_same_group: bool = False, splits: int = 0,
               query_chunk: int = DEFAULT_QUERY_CHUNK) -> Tuple[torch.Tensor, torch.Tensor]:
        """the k best rows for each query row -> ``(scores fp32 [n, k], ids int64 [n, k])`` on the device.  ``"l2"``: squared
        distances, ascending; ``"cosine"``: similarities (queries normalised like the rows), descending.  Ties go to the smaller id;
        missing entries are (+inf, -1).  ``exclude_same_group`` skips rows whose group equals the query's (``groups [n]``).
        ``query_chunk`` bounds the workspace; ``splits`` (0 = automatic) is a test hook.  Neither changes the result."""
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_K:
            raise ValueError("k must be an integer in [1, %d], got %r" % (MAX_K, k))
        k = int(k)
        if len(self) == 0:
            raise ValueError("the index is empty")
        q = _rows(queries, "queries")
        n, D = q.shape
        if D != self.dim:
            raise ValueError("queries: expected D = %d, got %d" % (self.dim, D))
        if exclude_same_group:
            if groups is None:
                raise ValueError("exclude_same_group needs the queries' groups")
            qg = torch.from_numpy(_groups(groups, n, "groups")).to(self.device)
        elif groups is not None:
            _groups(groups, n, "groups")
            qg = None
        else:
            qg = None
        if int(splits) < 0 or int(query_chunk) < 1:
            raise ValueError("splits must be >= 0 and query_chunk >= 1")
        scores = torch.empty((n, k), dtype=torch.float32, device=self.device)
        ids = torch.empty((n, k), dtype=torch.int64, device=self.device)
        if n == 0:
            return scores, ids
        lib = _lib.load()
        qd = self._prep(q)
        N = len(self)
        step = min(n, int(query_chunk))
        ws = torch.empty(int(lib.sylber_knn_workspace_bytes(step, N, D, k, int(splits))), dtype=torch.uint8, device=self.device)
        metric = METRICS[self.metric]
        with torch.cuda.device(self.device):
            for r0 in range(0, n, step):
                m = min(step, n - r0)
                _lib.check(lib.sylber_knn_search(_vp(qd[r0:r0 + m]), m, _vp(self._x), N, D, _vp(self._c), metric, k,
                                                 _vp(qg[r0:r0 + m] if qg is not None else None), _vp(self._g if qg is not None else None),
                                                 int(splits), _vp(scores[r0:r0 + m]), _vp(ids[r0:r0 + m]), _vp(ws), _stream(self.device)),
                           "sylber_knn_search")
        return scores, ids

    # ---- persistence ----------------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """``.npz`` with the stored rows, groups, provenance and metric (cosine rows are saved normalised; loading does not
        normalise them again, so a round trip gives the same results bit for bit)"""
        N = len(self)
        np.savez(path, metric=np.array(self.metric), features=(self._x.cpu().numpy() if N else np.zeros((0, self.dim or 16), np.float32)),
                 groups=(self._g.cpu().numpy() if N else np.zeros(0, np.int32)),
                 provenance=(self._prov if N else np.zeros((0, 4))), span_int=np.array(self._span_dtype is np.int64))

    @classmethod
    def load(cls, path: str, device="cuda") -> "SyllableIndex":
        z = np.load(path, allow_pickle=False)
        idx = cls(metric=str(z["metric"]), device=device)
        x = z["features"]
        if x.shape[0]:
            idx._load_rows(x, z["groups"], z["provenance"])      # rows as saved: cosine rows are not normalised a second time
        if bool(z["span_int"]):
            idx._span_dtype = np.int64
        return idx

    def _load_rows(self, x, g, prov) -> None:
        lib = _lib.load()
        xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(self.device)
        m, D = xd.shape
        self._check_width(D, "features")
        c = None
        if self.metric == "l2":
            c = torch.empty(m, dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(lib.sylber_knn_row_norms(_vp(xd), m, D, _vp(c), _stream(self.device)), "sylber_knn_row_norms")
        self.dim, self._x, self._c = D, xd, c
        self._g = torch.from_numpy(np.ascontiguousarray(g, np.int32)).to(self.device)
        self._prov = np.asarray(prov, np.float64).reshape(m, 4)

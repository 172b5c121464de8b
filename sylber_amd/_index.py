"""The host rules that the four syllable indexes share (search.py: ``SyllableIndex``, ``IVFSyllableIndex``; pq.py: ``PQSyllableIndex``,
``IVFPQSyllableIndex``), each written once: what a search accepts (``k`` / ``refine``, ``nprobe``, ``splits`` / ``query_chunk``, query
rows, query groups; the arguments, sequences and packed blocks of a phrase search and the host loop of the ones that scan the corpus,
``_scan_phrases``), how rows are stored (``_prep``, ``_row_norms``, ``_pack16``), where a search puts its results, what ``provenance`` answers, how
rows are sorted into lists, and how the common arrays reach an ``.npz`` and come back.  Private: the classes are the public surface."""
from __future__ import annotations

import ctypes
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
MAX_PHRASE_ROWS = 64            # DT_MAX_M of csrc/dtw.hip: one wave holds a phrase
MAX_SEEDS = 128                 # PV_MAX_SEEDS of csrc/phrase_vote.hip: the seeds per phrase row of a seeded phrase search
MAX_SEQUENCE_ROWS = 65536       # DT_MAX_SEQ: the DP along one sequence is serial
DEFAULT_PHRASE_CHUNK = 4096
STORAGES = {"fp16": (0, torch.float16), "bf16": (1, torch.bfloat16)}     # SYLBER_KNN16_FP16 / _BF16: the 16-bit planes of the two-stage searches


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


def _pack16(x: torch.Tensor, storage: str, refuse: bool) -> torch.Tensor:
    """contiguous fp32 rows on the device -> their 16-bit rows (csrc/knn16.hip, ``sylber_knn16_pack``: round to nearest even, fp16
    saturates); ``refuse``: a finite value that fp16 cannot hold is a ``ValueError``"""
    code, dtype = STORAGES[storage]
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    if x.shape[0] == 0:
        return out
    sat = torch.zeros(1, dtype=torch.int32, device=x.device) if refuse and storage == "fp16" else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().sylber_knn16_pack(_vp(x), x.shape[0], x.shape[1], code, _vp(out), _vp(sat), _stream(x.device)),
                   "sylber_knn16_pack")
    if sat is not None and int(sat.item()):
        raise ValueError('%d stored values lie beyond +-65504, the range of storage="fp16": use storage="bf16"' % int(sat.item()))
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


# ---- phrase searches ----------------------------------------------------------------------------------------------------------------
# What the phrase searches share: SyllableIndex.search_phrases, search_phrases_refined, search_occurrences,
# search_occurrences_refined and PQSyllableIndex.search_phrases (all five through _scan_phrases below), search_phrases_seeded and the
# two align_phrases.  An index enters only as (N rows, width dim, device, metric, the rows' groups on the device).
def _phrase_outputs(P: int, k: int, device, span=(2,)):
    """``(costs fp32 [P, k], seqs int64 [P, k], spans int64 [P, k, 2])`` of a phrase search; ``span=(2, 2)``: the two spans of
    ``search_repeats``"""
    return (torch.empty((P, k), dtype=torch.float32, device=device), torch.empty((P, k), dtype=torch.int64, device=device),
            torch.empty((P, k) + tuple(span), dtype=torch.int64, device=device))


def _group_runs(g: Optional[torch.Tensor], N: int) -> np.ndarray:
    """int64 ``[S + 1]``: the maximal runs of consecutive rows with equal group, the default sequences of a phrase search"""
    if N == 0:
        return np.zeros(1, np.int64)
    g = g.cpu().numpy()
    return np.concatenate([[0], np.nonzero(g[1:] != g[:-1])[0] + 1, [N]]).astype(np.int64)


def _sequences(sequences, N: int, default) -> np.ndarray:
    """the sequence offsets int64 ``[S + 1]`` of a phrase search: ``sequences`` validated, or ``default()``"""
    if sequences is None:
        off = default()
    else:
        a = np.asarray(sequences.detach().cpu().numpy() if torch.is_tensor(sequences) else sequences)
        if a.ndim != 1 or a.size < 2 or a.dtype.kind not in "iu":
            raise ValueError("sequences must be integer offsets [S + 1]")
        off = a.astype(np.int64)
        if off[0] != 0 or off[-1] != N or np.any(np.diff(off) < 1):
            raise ValueError("sequences must ascend from 0 to %d rows without an empty sequence" % N)
    longest = int(np.diff(off).max())
    if longest > MAX_SEQUENCE_ROWS:
        raise ValueError("a sequence has %d rows, more than %d: cut it with sequences=" % (longest, MAX_SEQUENCE_ROWS))
    return off


def _phrase_args(N: int, dim: int, device, default_sequences, phrases, lengths, groups, exclude_same_group, sequences, splits,
                 phrase_chunk, block_phrases):
    """the checks of a phrase search -> ``(phrase rows [sum m, D] as given, lengths int64 [P], the phrases' groups on the host or
    None, sequence offsets int64 [S + 1])``, or ``ValueError``"""
    if N == 0:
        raise ValueError("the index is empty")
    if lengths is None:
        if torch.is_tensor(phrases) or isinstance(phrases, np.ndarray):
            raise ValueError("phrases given as one [sum m, D] array need lengths=")
        parts = [_rows(p, "phrases[%d]" % i) for i, p in enumerate(phrases)]
        lens = np.array([p.shape[0] for p in parts], np.int64)
        for p in parts:
            _rows_of_width(p, dim, "phrases")
        q = torch.cat([p.to(device, torch.float32) for p in parts]) if parts else torch.zeros((0, dim), device=device)
    else:
        q = _rows_of_width(phrases, dim, "phrases")
        lens = np.asarray(lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else lengths)
        if lens.ndim != 1 or (lens.size and lens.dtype.kind not in "iu"):
            raise ValueError("lengths must be a 1-D sequence of integers")
        lens = lens.astype(np.int64)
        if int(lens.sum()) != q.shape[0]:
            raise ValueError("lengths sum to %d, phrases has %d rows" % (int(lens.sum()), q.shape[0]))
    P = int(lens.size)
    if P and (lens.min() < 1 or lens.max() > MAX_PHRASE_ROWS):
        raise ValueError("a phrase has between 1 and %d rows, got lengths from %d to %d" % (MAX_PHRASE_ROWS, lens.min(), lens.max()))
    pg = _query_groups(groups, P, exclude_same_group, None, "phrases")         # on the host: a chunk's groups go to the device with it
    if int(splits) < 0 or int(phrase_chunk) < 1 or int(block_phrases) < 0:
        raise ValueError("splits and block_phrases must be >= 0 and phrase_chunk >= 1")
    return q, lens, pg, _sequences(sequences, N, default_sequences)


def _sequence_tables(off: np.ndarray, g: Optional[torch.Tensor], device):
    """plumbing: the sequence of every row and (with the rows' groups ``g``, for the exclusion) the group of every sequence, on the
    device"""
    off_d = torch.from_numpy(off).to(device)
    seq_id = torch.repeat_interleave(torch.arange(off.size - 1, dtype=torch.int32, device=device), off_d[1:] - off_d[:-1])
    return seq_id, (g.index_select(0, off_d[:-1]) if g is not None else None)


class _PhraseBlocks:
    """one chunk of phrases as ``sylber_dtw_plan`` packs it: ``Pc`` phrases in ``nb`` blocks of 128 rows (``qp``, padding rows zero)
    against ``C`` cuts; ``slots`` = the most phrases in any block; ``place`` / ``ln``: first packed row and length of each phrase"""

    def __init__(self, dev, Pc, nb, C, slots, place, ln, qp, meta, slot_phrase, block_rows, cut_rows, pg):
        self.dev, self.Pc, self.nb, self.C, self.slots, self.place, self.ln, self.qp = dev, Pc, nb, C, slots, place, ln, qp
        self._host = (meta, slot_phrase, block_rows, cut_rows)
        self._pg = pg

    def tables(self):
        """``(row meta, slot -> phrase, rows per block, cut rows, the phrases' groups or None)`` on the device"""
        meta_d, sp_d, br_d, cut_d = (torch.from_numpy(a).to(self.dev) for a in self._host)
        return meta_d, sp_d, br_d, cut_d, (_on_device(self._pg, np.int32, self.dev) if self._pg is not None else None)


def _phrase_blocks(lib, dev, qd, lens, p0: int, p1: int, off, list_size: int, splits, block_phrases, pg) -> _PhraseBlocks:
    """phrases ``p0 : p1`` of the prepared rows ``qd`` packed by ``sylber_dtw_plan`` for lists of ``list_size`` entries: the
    packed layout of the chunk's rows (where each row goes, what it is, which phrase owns each slot), the rows scattered into
    zeroed 128-row blocks, and the cut table"""
    S = off.size - 1
    off32 = np.ascontiguousarray(off, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    Pc = p1 - p0
    ln = np.ascontiguousarray(lens[p0:p1], np.int32)
    nb, ph = ctypes.c_int32(0), ctypes.c_int32(0)
    place = np.empty(Pc, np.int32)
    args = (off32.ctypes.data_as(i32p), S, ln.ctypes.data_as(i32p), Pc, list_size, int(splits), int(block_phrases))
    C = int(lib.sylber_dtw_plan(*args, None, 0, place.ctypes.data_as(i32p), ctypes.byref(nb), ctypes.byref(ph)))
    cut_rows = np.empty(max(C, 1) + 1, np.int32)
    if C < 1 or int(lib.sylber_dtw_plan(*args, cut_rows.ctypes.data_as(i32p), C + 1, None, None, None)) != C:
        raise _lib.SylberHipError("sylber_dtw_plan failed (%d)" % C)
    nb = nb.value
    R = int(ln.sum())
    first = np.repeat(place.astype(np.int64), ln)
    local = np.arange(R) - np.repeat(np.cumsum(ln) - ln, ln)
    blk = place // 128
    slot = np.arange(Pc) - np.searchsorted(blk, blk, side="left")
    meta = np.full(nb * 128, -1, np.int32)
    meta[first + local] = local | ((local == np.repeat(ln, ln) - 1).astype(np.int64) << 7) | (np.repeat(slot, ln) << 8)
    slot_phrase = np.full(nb * 128, -1, np.int32)
    slot_phrase[blk.astype(np.int64) * 128 + slot] = np.arange(Pc)
    block_rows = np.zeros(nb, np.int32)
    np.maximum.at(block_rows, blk, place % 128 + ln)
    r0 = int(lens[:p0].sum())
    qp = torch.zeros((nb * 128, qd.shape[1]), dtype=torch.float32, device=dev)
    qp[torch.from_numpy(first + local).to(dev)] = qd[r0:r0 + R]
    return _PhraseBlocks(dev, Pc, nb, C, int(slot.max()) + 1, place, ln, qp, meta, slot_phrase, block_rows, cut_rows,
                         pg[p0:p1] if pg is not None else None)


class _PhraseChunk:
    """what ``_scan_phrases`` hands to the stages of a search.  For the whole call: ``lib, dev, st`` (the stream), ``N, dim, metric``
    (its code), ``k``, ``m`` (entries per list in stage 1: ``k``, or ``k * refine``), ``off_d`` (two-stage only),
    ``S, seq_id, seq_grp``.  For the chunk: ``b`` (its ``_PhraseBlocks``), ``meta_d, sp_d, br_d, cut_d, pg_d`` (``b.tables()``) and
    the chunk's slices ``costs, seqs, spans``; two-stage searches also get ``place_d, len_d, qn`` (the ``||q||^2`` that
    ``sylber_dtw_search`` adds, same kernel; ``None`` under "cosine"), ``q16`` (the packed rows in 16 bits), ``cand, coarse`` and
    ``ws``: stage 1 leaves its workspace there for stage 2."""

    def __init__(self, fill, **whole_call):
        self._fill = fill
        self.__dict__.update(whole_call)

    def workspace(self, nbytes) -> torch.Tensor:
        """``nbytes`` of workspace; a test's ``_workspace_fill`` reaches every workspace of the call through here"""
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.dev)
        if self._fill is not None:
            ws.fill_(self._fill)
        return ws


def _scan_phrases(N: int, dim: int, dev, metric: str, db_groups, default_sequences, stages, phrases, k, refine, storage, lengths, groups,
                  exclude_same_group, sequences, splits, phrase_chunk, block_phrases, return_candidates, workspace_fill, local=None):
    """the host loop of every phrase search that scans the corpus: the checks in their order (``k`` / ``refine`` / ``storage``, then
    ``_phrase_args``), the outputs, the return for no phrase, the prepared rows, the sequence tables and, ``phrase_chunk`` phrases
    at a time, the packed blocks with their tables -> ``(costs, seqs, spans)``, and ``cand`` int64, ``coarse`` with
    ``return_candidates``.  ``refine=None``: one stage with lists of ``k`` (``storage`` and ``return_candidates`` unused); else two
    with ``m = k * refine`` candidates.  ``stages()`` is called once, behind every check and before anything is launched (it may
    still refuse, e.g. values that fp16 cannot hold) -> ``(scan, rerank)``: ``scan(c)`` launches stage 1 of the chunk ``c`` (a
    ``_PhraseChunk``) -- into ``c.costs, c.seqs, c.spans`` when it is the only stage, else into ``c.cand, c.coarse`` -- and
    ``rerank(c)`` (``None`` with one stage) stage 2, inside the loop.  ``local`` (``search_repeats``): ``(radius, gap, min_score)`` as
    fp32 and ``after`` (int32 ``[P]`` on the host, or ``None``); the spans are then ``[P, k, 2, 2]``, the chunk carries ``c.local``
    (the three scalars) and ``c.after_d`` (its slice of ``after`` on the device, or ``None``)."""
    two = refine is not None
    k, m = _check_k_refine(k, refine, rerank=True) if two else _check_k_refine(k)
    if two and storage not in STORAGES:
        raise ValueError("storage must be 'fp16' or 'bf16', got %r" % (storage,))
    q, lens, pg, off = _phrase_args(N, dim, dev, default_sequences, phrases, lengths, groups, exclude_same_group, sequences, splits,
                                    phrase_chunk, block_phrases)
    P = int(lens.size)
    if local is not None and local[3] is not None and len(local[3]) != P:
        raise ValueError("after_seq must have one entry per probe (%d), got %d" % (P, len(local[3])))
    costs, seqs, spans = _phrase_outputs(P, k, dev, (2,) if local is None else (2, 2))
    cand = torch.empty((P, m), dtype=torch.int32, device=dev) if two else None
    coarse = torch.empty((P, m), dtype=torch.float32, device=dev) if two else None
    if P:
        scan, rerank = stages()
        lib = _lib.load()
        qd = _prep(q, metric, dev)
        seq_id, seq_grp = _sequence_tables(off, db_groups if pg is not None else None, dev)
        c = _PhraseChunk(workspace_fill, lib=lib, dev=dev, N=N, dim=dim, metric=METRICS[metric], k=k, m=m, S=off.size - 1,
                         off_d=_on_device(off, np.int32, dev) if two else None, seq_id=seq_id, seq_grp=seq_grp)
        with torch.cuda.device(dev):
            c.st = _stream(dev)
            for p0 in range(0, P, int(phrase_chunk)):
                p1 = min(P, p0 + int(phrase_chunk))
                c.b = b = _phrase_blocks(lib, dev, qd, lens, p0, p1, off, m, splits, block_phrases, pg)
                c.meta_d, c.sp_d, c.br_d, c.cut_d, c.pg_d = b.tables()
                c.costs, c.seqs, c.spans = costs[p0:p1], seqs[p0:p1], spans[p0:p1]
                if local is not None:
                    c.local, c.after_d = local[:3], (_on_device(local[3][p0:p1], np.int32, dev) if local[3] is not None else None)
                if two:
                    c.place_d, c.len_d = _on_device(b.place, np.int32, dev), _on_device(b.ln, np.int32, dev)
                    c.qn = _row_norms(b.qp) if metric == "l2" else None
                    c.q16 = _pack16(b.qp, storage, refuse=False)
                    c.cand, c.coarse = cand[p0:p1], coarse[p0:p1]
                scan(c)
                if two:
                    rerank(c)
    return (costs, seqs, spans, cand.to(torch.int64), coarse) if two and return_candidates else (costs, seqs, spans)


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

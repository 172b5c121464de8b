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

``SyllableIndex.search_phrases`` searches for a *sequence* of syllables: subsequence DTW of each phrase against every sequence (by
default: clip) of the index, in the epilogue of the same contraction (csrc/dtw.hip, ``sylber_dtw_search``); its contract is in the
method's docstring, restated in numpy in tests/dtw_ref.py.  ``SyllableIndex.search_phrases_refined`` is its two-stage form (csrc/dtw16.hip:
a 16-bit MFMA scan picks candidate sequences, the exact DTW re-ranks them; tests/dtw16_ref.py).  ``IVFSyllableIndex.search_phrases`` finds the
candidate sequences without a scan of the corpus: each phrase row's neighbours from the lists vote for them (csrc/phrase_vote.hip;
``SyllableIndex.search_phrases_seeded`` is the vote and the re-rank on seeds from anywhere; tests/phrase_vote_ref.py).
``SyllableIndex.search_occurrences`` / ``search_occurrences_refined`` return every non-overlapping occurrence of a phrase instead of one
match per sequence (``sylber_dtw_occurrences``, ``sylber_dtw_rerank_occurrences``; tests/occ_ref.py);
``SyllableIndex.search_occurrences_seeded`` and ``IVFSyllableIndex.search_occurrences`` do so among the candidate sequences of the vote.
``align_phrases`` takes the spans of any of them and returns the warping path of each match: the stored rows every phrase row was
aligned to (csrc/dtw_align.hip, ``sylber_dtw_align``; tests/align_ref.py).
``SyllableIndex.search_repeats`` / ``find_repeats`` need no whole-phrase match and no query: the LOCAL alignment of probes -- or of
windows of the index's own sequences -- against every sequence, in the same epilogue (csrc/dtw_local.hip, ``sylber_dtw_local``;
tests/repeats_ref.py).
``align_sequences`` / ``SyllableIndex.align_sequences`` align two WHOLE sequences of any length, the global DTW with its path
(csrc/dtw_strings.hip, ``sylber_dtw_strings_align``; tests/dtw_strings_ref.py); a call of few long pairs spreads each pair over the
chip in blocks, with the same bits (``split=``; csrc/dtw_strings_split.hip, ``sylber_dtw_strings_align_split``).
``local_align_sequences`` / ``SyllableIndex.local_align_sequences`` are its LOCAL form: every repeat between two whole sequences,
or inside one (csrc/dtw_strings_local.hip, ``sylber_dtw_strings_local``; tests/dtw_strings_local_ref.py).

The rules that every index shares -- argument checks, row preparation, result buffers, provenance, the list layout, the arrays of a
saved file -- are in _index.py, each once; this file and pq.py hold what differs between the indexes.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._index import MAX_CANDIDATES, MAX_K, MAX_NPROBE  # noqa: F401  (limits of this module's searches, kept importable from here)
from ._index import DEFAULT_PHRASE_CHUNK, MAX_PHRASE_ROWS, MAX_SEEDS, MAX_SEQUENCE_ROWS, STORAGES  # noqa: F401  (likewise, for the phrase searches)
from ._index import (DEFAULT_QUERY_CHUNK, METRICS, _added_rows, _base_arrays, _check_k_refine, _check_nprobe, _check_splits_chunk,
                     _chunked_workspace_bytes, _group_runs, _list_layout, _on_device, _outputs, _pack16, _phrase_args, _phrase_blocks,
                     _phrase_outputs, _PhraseChunk, _prep, _provenance, _query_groups, _result, _row_norms, _rows, _rows_of_width,
                     _scan_phrases, _sequences)
from .kmeans import _device, _stream, _vp

RERANK_CHUNK = 32               # DP_CH of csrc/dtw_pair.h: the columns of a sequence that search_phrases_refined re-ranks at a time
OCC_RERANK_ENTRIES = 1 << 24    # list entries (24 B each with the merge rounds' half) of one sylber_dtw_rerank_occurrences launch
MAX_WINDOW_ROWS = 65536         # DA_MAX_COLS of csrc/dtw_align.hip: the rows of a window that align_phrases walks (= MAX_SEQUENCE_ROWS)
ALIGN_WORKSPACE_BYTES = 256 << 20       # the default pair_chunk of align_phrases keeps its workspace below this
SEQUENCE_SUPER_ROWS = 128       # KN_BM of csrc/dtw_strings.hip: the rows of x that align_sequences takes between two carried rows
SPLIT_BLOCK = (128, 128)        # DSS_BLOCK_ROWS, DSS_BLOCK_COLS of csrc/dtw_strings_split.hip: the blocks of a split pair by default
SPLIT_MIN_CELLS = 256 * 256     # split=None: the smallest m L that is split (profiles/dtw_strings_split_bench.md, "The automatic threshold")


# ---- repeated phrases: the three fp32 scalars of search_repeats / find_repeats ---------------------------------------------------
def _local_scalars(radius, gap, min_score) -> Tuple[np.float32, np.float32, np.float32]:
    """``(radius, gap, min_score)`` as fp32 with the defaults ``gap = 2 radius``, ``min_score = 3 radius``, or ``ValueError``"""
    def f32(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("%s must be a number, got %r" % (what, v))
        with np.errstate(over="ignore"):
            return np.float32(v)
    radius = f32(radius, "radius")
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError("radius must be finite and > 0 as float32, got %r" % (radius,))
    with np.errstate(over="ignore"):
        gap = np.float32(2) * radius if gap is None else f32(gap, "gap")
        min_score = np.float32(3) * radius if min_score is None else f32(min_score, "min_score")
    if not (np.isfinite(gap) and gap >= 0):
        raise ValueError("gap must be finite and >= 0 as float32, got %r" % (gap,))
    if not (np.isfinite(min_score) and min_score > 0):
        raise ValueError("min_score must be finite and > 0 as float32, got %r" % (min_score,))
    return radius, gap, min_score


# ---- warping paths: what the align_phrases of SyllableIndex and of the compressed indexes share -------------------------------
def _align_spans(spans, P: int, N: int, device) -> Tuple[torch.Tensor, int]:
    """the checks of ``align_phrases`` on ``spans`` -> ``(spans int64 [P, k, 2] on the device, the widest window)``, or ``ValueError``;
    one reduction on the device and one copy of two numbers to the host"""
    sp = spans if torch.is_tensor(spans) else torch.from_numpy(np.asarray(spans))
    if sp.dtype != torch.int64 or sp.dim() != 3 or sp.shape[0] != P or sp.shape[2] != 2:
        raise ValueError("spans must be int64 [%d phrases, k, 2], got %s %s" % (P, sp.dtype, tuple(sp.shape)))
    sp = sp.to(device).contiguous()
    if sp.numel() == 0:
        return sp, 0
    a, b = sp[..., 0], sp[..., 1]
    pad = (a == -1) & (b == -1)
    ok = pad | ((a >= 0) & (a < b) & (b <= N))
    width = torch.where(ok & ~pad, b - a, torch.zeros_like(a))
    bad, widest = torch.stack([(~ok).sum(), width.max()]).cpu().tolist()
    if bad:
        raise ValueError("%d spans are neither (-1, -1) nor 0 <= first < one past the last <= %d rows" % (bad, N))
    if widest > MAX_WINDOW_ROWS:
        raise ValueError("a window has %d rows, more than %d" % (widest, MAX_WINDOW_ROWS))
    return sp, int(widest)


def _rerank_launch(c: "_PhraseChunk", x, cn) -> None:
    """the exact re-rank, ``sylber_dtw_rerank``, of the chunk's phrases on their candidates ``c.cand`` among the ``c.S`` sequences
    ``c.off_d`` of the ``c.N`` rows ``x`` with norms ``cn`` -> ``c.costs, c.seqs, c.spans``; ``c.ws`` is its workspace"""
    b = c.b
    _lib.check(c.lib.sylber_dtw_rerank(_vp(b.qp), b.nb, _vp(c.qn), _vp(c.place_d), _vp(c.len_d), int(c.cand.shape[0]), _vp(x), c.N, c.dim,
                                       _vp(cn), c.metric, _vp(c.cand), c.m, _vp(c.off_d), c.S, c.k, _vp(c.costs), _vp(c.seqs), _vp(c.spans),
                                       _vp(c.ws), c.st), "sylber_dtw_rerank")


def _occ_rerank_launch(c: "_PhraseChunk", entry: str, db: tuple) -> None:
    """every occurrence of the chunk's phrases in their candidate sequences ``c.cand`` -> ``c.costs, c.seqs, c.spans``: ``entry`` is
    ``sylber_dtw_rerank_occurrences`` with ``db = (rows, N, D, norms)`` or ``sylber_dtw_rerank_occurrences_codes`` with ``db`` = the
    coded-database group, ``N, D`` and the norms.  At most ``OCC_RERANK_ENTRIES`` list entries per launch: that bounds the workspace
    (m lists of k per phrase and their merge rounds), and the phrases of a launch do not meet, so nothing depends on it."""
    step = max(1, OCC_RERANK_ENTRIES // (c.m * c.k))
    Pc = int(c.cand.shape[0])
    wo = c.workspace(c.lib.sylber_dtw_occ_workspace_bytes(min(step, Pc), c.m, c.k))
    fn = getattr(c.lib, entry)
    for r0 in range(0, Pc, step):
        r1 = min(Pc, r0 + step)
        _lib.check(fn(_vp(c.b.qp), c.b.nb, _vp(c.qn), _vp(c.place_d[r0:r1]), _vp(c.len_d[r0:r1]), r1 - r0, *db, c.metric,
                      _vp(c.cand[r0:r1]), c.m, _vp(c.off_d), c.S, c.k, _vp(c.costs[r0:r1]), _vp(c.seqs[r0:r1]), _vp(c.spans[r0:r1]), _vp(wo),
                      c.st), entry)


def _seeded_phrases(N: int, dim: int, dev, metric: str, db_groups, q, lens, pg, off, sc, si, k: int, m: int, phrase_chunk,
                    return_candidates: bool, rerank, fill=None):
    """``search_phrases_seeded`` behind its checks, for an index of N rows of width ``dim`` with the rows' groups ``db_groups`` (in id
    order, on the device): ``phrase_chunk`` phrases at a time, ``sylber_phrase_vote`` on the seeds ``sc, si`` (on the device), the
    phrases packed as ``search_phrases`` packs them and ``rerank(c)``, which scores the chunk's candidates ``c.cand`` exactly into
    ``c.costs, c.seqs, c.spans`` on the index's rows, however it holds them.  ``fill``: a test's workspace fill.  Queues work only."""
    P, seeds, S = int(lens.size), int(sc.shape[1]), off.size - 1
    costs, seqs, spans = _phrase_outputs(P, k, dev)
    cand = torch.empty((P, m), dtype=torch.int32, device=dev)
    bound = torch.empty((P, m), dtype=torch.float32, device=dev)
    if P == 0:
        return (costs, seqs, spans, cand.to(torch.int64), bound) if return_candidates else (costs, seqs, spans)
    lib = _lib.load()
    qd = _prep(q, metric, dev)
    off_d = _on_device(off, np.int32, dev)
    seq_grp = db_groups.index_select(0, off_d[:-1].to(torch.int64)) if pg is not None else None
    row_d, len_d = _on_device(np.cumsum(lens) - lens, np.int32, dev), _on_device(lens, np.int32, dev)
    pg_d = _on_device(pg, np.int32, dev) if pg is not None else None
    code = METRICS[metric]
    with torch.cuda.device(dev):
        st = _stream(dev)
        for p0 in range(0, P, int(phrase_chunk)):
            p1 = min(P, p0 + int(phrase_chunk))
            _lib.check(lib.sylber_phrase_vote(_vp(sc), _vp(si), seeds, _vp(row_d[p0:p1]), _vp(len_d[p0:p1]), p1 - p0, _vp(off_d), S,
                                              code, _vp(pg_d[p0:p1] if pg_d is not None else None), _vp(seq_grp), m,
                                              _vp(cand[p0:p1]), _vp(bound[p0:p1]), st), "sylber_phrase_vote")
            b = _phrase_blocks(lib, dev, qd, lens, p0, p1, off, m, 0, 0, None)
            c = _PhraseChunk(fill, lib=lib, dev=dev, st=st, N=N, dim=dim, metric=code, k=k, m=m, S=S, off_d=off_d, b=b,
                             qn=_row_norms(b.qp) if metric == "l2" else None, place_d=_on_device(b.place, np.int32, dev),
                             len_d=len_d[p0:p1], cand=cand[p0:p1], costs=costs[p0:p1], seqs=seqs[p0:p1], spans=spans[p0:p1])
            c.ws = c.workspace(lib.sylber_dtw16_workspace_bytes(b.Pc, m, 1))
            rerank(c)
    return (costs, seqs, spans, cand.to(torch.int64), bound) if return_candidates else (costs, seqs, spans)


def _align_phrases(N: int, dim: int, dev, metric: str, phrases, spans, lengths, pair_chunk, run, tracked: bool = False):
    """``align_phrases`` of an index of N rows of width ``dim``: the checks, the phrase rows prepared and packed as ``search_phrases``
    packs them, the pairs taken ``pair_chunk`` at a time.  ``run(lib, b, qn, place_d, len_d, pair_phrase, win, max_cols, rows,
    steps, costs, start, ws, st)`` aligns one chunk against the index's rows, however it holds them.  ``tracked`` (a test hook):
    also return ``start`` int64 ``[P, k]``, the start row that the kernel's walk tracked as the re-rank tracks it (-1 for padding),
    which must equal ``rows[:, :, 0, 0]``."""
    # a window is its own sequence: the sequences of the search do not enter, so neither do their checks (one dummy sequence)
    q, lens, _, _ = _phrase_args(N, dim, dev, lambda: np.zeros(2, np.int64), phrases, lengths, None, False, None, 0, 1, 0)
    if pair_chunk is not None and (isinstance(pair_chunk, bool) or int(pair_chunk) != pair_chunk or int(pair_chunk) < 1):
        raise ValueError("pair_chunk must be an integer >= 1, got %r" % (pair_chunk,))
    P = int(lens.size)
    sp, widest = _align_spans(spans, P, N, dev)
    k, Mx = int(sp.shape[1]), (int(lens.max()) if P else 0)
    n = P * k
    rows = torch.full((n, Mx, 2), -1, dtype=torch.int32, device=dev)
    steps = torch.zeros(n, dtype=torch.int32, device=dev)
    costs = torch.full((n,), float("inf"), dtype=torch.float32, device=dev)
    start = torch.full((n,), -1, dtype=torch.int32, device=dev) if tracked else None
    if n and widest:                                        # else: nothing but padding, and no launch
        lib = _lib.load()
        qd = _prep(q, metric, dev)
        b = _phrase_blocks(lib, dev, qd, lens, 0, P, np.array([0, 1], np.int64), 1, 0, 0, None)      # the packing alone: no cut is used
        qn = _row_norms(b.qp) if metric == "l2" else None   # the ||q||^2 that sylber_dtw_search adds, same kernel
        place_d, len_d = _on_device(b.place, np.int32, dev), _on_device(b.ln, np.int32, dev)
        pair_phrase = torch.arange(P, dtype=torch.int32, device=dev).repeat_interleave(k)
        win = sp.reshape(n, 2).to(torch.int32)
        step = int(pair_chunk) if pair_chunk is not None else max(1, ALIGN_WORKSPACE_BYTES // (16 * (widest + 63)))
        step = min(step, n)
        with torch.cuda.device(dev):
            st = _stream(dev)
            ws = torch.empty(int(lib.sylber_dtw_align_workspace_bytes(step, widest)), dtype=torch.uint8, device=dev)
            for r0 in range(0, n, step):
                r1 = min(n, r0 + step)
                run(lib, b, qn, place_d, len_d, pair_phrase[r0:r1], win[r0:r1], widest, rows[r0:r1], steps[r0:r1], costs[r0:r1],
                    start[r0:r1] if tracked else None, ws, st)
    out = (rows.to(torch.int64).reshape(P, k, Mx, 2), steps.reshape(P, k), costs.reshape(P, k))
    return out + (start.to(torch.int64).reshape(P, k),) if tracked else out


# ---- whole sequences: what align_sequences and SyllableIndex.align_sequences share --------------------------------------------------
_i32p, _i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)


def dtw_strings_workspace_bytes(m, L, path: bool) -> np.ndarray:
    """int64: the bytes of workspace that each pair (``m`` rows of x, ``L`` rows of y; arrays) adds to a launch of
    ``sylber_dtw_strings_align`` beyond its 64 B of table: two rows of (A, n), 8 B per column, between super-strips of 128 rows where
    ``m > 128``, and with ``path`` 2 bits per cell of ``ceil(m / 64)`` strips of ``ceil(L / 128)`` tiles, 2048 B each"""
    m, L = np.asarray(m, np.int64), np.asarray(L, np.int64)
    rows = np.where((m > SEQUENCE_SUPER_ROWS) & (L > 0), (16 * L + 255) // 256 * 256, 0)
    if not path:
        return rows
    return rows + np.where((m > 0) & (L > 0), ((m + 63) // 64) * ((L + 127) // 128) * 2048, 0)


def _check_pair_chunk(pair_chunk) -> None:
    if pair_chunk is not None and (isinstance(pair_chunk, bool) or int(pair_chunk) != pair_chunk or int(pair_chunk) < 1):
        raise ValueError("pair_chunk must be an integer >= 1, got %r" % (pair_chunk,))


def dtw_strings_split_workspace_bytes(m, L, path: bool, block_rows: int = 0, block_cols: int = 0) -> np.ndarray:
    """int64: the bytes of workspace that each pair adds to a call of ``sylber_dtw_strings_align_split`` with these block sizes (0:
    ``SPLIT_BLOCK``) beyond its 64 B of table, every term rounded up to 256 B: for a pair with two non-empty sides 256 B for its last
    cell, two boundary rows of (A, n), ``16 L``, where it has more than one band of ``block_rows`` rows, two rows between a block's
    own super-strips, ``16 L``, where ``block_rows > 128`` and ``m > 128``, two boundary columns with one corner per band,
    ``16 (m + bands)``, where it has more than one chunk of ``block_cols`` columns, and with ``path`` the codes of
    ``dtw_strings_workspace_bytes``"""
    m, L = np.asarray(m, np.int64), np.asarray(L, np.int64)
    BR, BC = int(block_rows) or SPLIT_BLOCK[0], int(block_cols) or SPLIT_BLOCK[1]
    al = lambda b: (b + 255) // 256 * 256
    nbr, nbc = (m + BR - 1) // BR, (L + BC - 1) // BC
    some = (m > 0) & (L > 0)
    state = 256 + np.where(nbr > 1, al(16 * L), 0) + np.where((m > SEQUENCE_SUPER_ROWS) & (BR > SEQUENCE_SUPER_ROWS), al(16 * L), 0) \
        + np.where(nbc > 1, al(16 * (m + nbr)), 0)
    out = np.where(some, state, 0)
    if path:
        out = out + np.where(some, ((m + 63) // 64) * ((L + 127) // 128) * 2048, 0)
    return out


def split_schedule(nbr: int, nbc: int) -> List[List[Tuple[int, int]]]:
    """the launches of one split pair of ``nbr`` bands by ``nbc`` chunks, by the arithmetic of ``sylber_dtw_strings_align_split``
    (dss_run and dtw_strings_split_kernel, restated for the tests and for whoever schedules blocks next): launch d has
    ``min(d + 1, nbr, nbc, launches - d)`` workgroups, workgroup k takes block ``b = max(0, d - nbc + 1) + k``, ``c = d - b`` and
    returns at once unless ``b < nbr`` and ``c >= 0``.  A block's inputs -- blocks ``(b-1, c)`` and ``(b, c-1)`` -- are then always of
    the launch before.  Nothing in it knows the recurrence."""
    launches = nbr + nbc - 1 if nbr > 0 and nbc > 0 else 0
    out = []
    for d in range(launches):
        blocks = []
        for k in range(min(d + 1, nbr, nbc, launches - d)):
            b = max(0, d - nbc + 1) + k
            if b < nbr and d - b >= 0:
                blocks.append((b, d - b))
        out.append(blocks)
    return out


def _split_plan(ml: np.ndarray, Ll: np.ndarray, split, pair_chunk, dev=None):
    """what ``split`` asks for -> ``None`` (no pair is split) or ``(mask bool [S], block_rows, block_cols)``, or ``ValueError``.
    ``None``: automatic, ``False``: never, ``True``: every pair larger than one block of ``SPLIT_BLOCK``, ``(block_rows, block_cols)``
    (a test hook): every pair with two non-empty sides, in blocks of that size."""
    if split is False:
        return None
    some = (ml > 0) & (Ll > 0)
    if split is None or split is True:
        BR, BC = SPLIT_BLOCK
        mask = some & ((ml > BR) | (Ll > BC))
        if split is None:
            # the workgroups of a launch of today's entry are its pairs: split only where they would leave CUs idle
            launch = int(ml.size) if pair_chunk is None else min(int(ml.size), int(pair_chunk))
            if not mask.any() or launch >= torch.cuda.get_device_properties(dev).multi_processor_count:
                return None
            # at least two bands AND two chunks: a pair of one band or one chunk has one block per anti-diagonal, so its blocks
            # would run one after the other, with a launch between them
            mask = mask & (ml > BR) & (Ll > BC) & (ml * Ll >= SPLIT_MIN_CELLS)
    else:
        try:
            BR, BC = split
        except (TypeError, ValueError):
            raise ValueError("split must be None, a bool or (block_rows, block_cols), got %r" % (split,)) from None
        for v in (BR, BC):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 128 or v % 128 or v > MAX_SEQUENCE_ROWS:
                raise ValueError("split = (block_rows, block_cols) must be multiples of 128 from 128 to %d, got %r" % (MAX_SEQUENCE_ROWS, split))
        BR, BC, mask = int(BR), int(BC), some
    return (mask, BR, BC) if mask.any() else None


def _check_sequence_pairs(ml: np.ndarray, Ll: np.ndarray, path: bool, pair_chunk, plan=None) -> np.ndarray:
    """the checks of ``align_sequences`` on the lengths of its pairs -> the workspace bytes of each pair (``plan``: ``_split_plan``'s,
    the split pairs with the hand-over state of their blocks), or ``ValueError``"""
    _check_pair_chunk(pair_chunk)
    for what, ln in (("xs", ml), ("ys", Ll)):
        if ln.size and int(ln.max()) > MAX_SEQUENCE_ROWS:
            raise ValueError("%s[%d] has %d rows, more than %d" % (what, int(ln.argmax()), int(ln.max()), MAX_SEQUENCE_ROWS))
        if int(ln.sum()) >= 2 ** 31:
            raise ValueError("one call takes fewer than 2^31 rows on each side")
    need = dtw_strings_workspace_bytes(ml, Ll, path) + 64
    if plan is not None:
        need = np.where(plan[0], dtw_strings_split_workspace_bytes(ml, Ll, path, plan[1], plan[2]) + 64, need)
    if need.size and int(need.max()) + 256 > ALIGN_WORKSPACE_BYTES:
        s = int(need.argmax())
        raise ValueError("pair %d (%d x %d rows) needs %d bytes of predecessor codes for its path, more than %d; path=False never "
                         "needs more than 1 MiB per pair" % (s, ml[s], Ll[s], need[s], ALIGN_WORKSPACE_BYTES))
    return need


def _launch_cuts(S: int, need: np.ndarray, pair_chunk) -> List[Tuple[int, int]]:
    """the launches of S > 0 pairs as ``(first pair, one past the last)``: ``pair_chunk`` pairs each, or as many as keep the workspace
    (``need`` bytes per pair) below ``ALIGN_WORKSPACE_BYTES``"""
    if pair_chunk is not None:
        cuts = list(range(0, S, int(pair_chunk))) + [S]
    else:
        cuts, acc = [0], np.concatenate([[0], np.cumsum(need)])
        while cuts[-1] < S:
            cuts.append(max(cuts[-1] + 1, int(np.searchsorted(acc, acc[cuts[-1]] + ALIGN_WORKSPACE_BYTES - 256, side="right")) - 1))
    return list(zip(cuts[:-1], cuts[1:]))


def _align_windows(xd, xn, yd, yn, D: int, metric: str, xw: np.ndarray, yw: np.ndarray, need: np.ndarray, path: bool, pair_chunk, fill,
                   dev, _steps_walk: bool = False, plan=None):
    """``sylber_dtw_strings_align`` on the pairs of windows ``xw, yw`` int32 ``[S, 2]`` = (first row, rows) into the prepared rows
    ``xd, yd`` with norms ``xn, yn`` (``None`` under cosine), behind every check -> ``(rows int32 [sum m, 2] or None, costs, steps,
    x offsets int64 on the host)``; the launches are grouped as ``_align_strings`` groups them.  ``plan``: ``_split_plan``'s; its
    pairs go to ``sylber_dtw_strings_align_split`` in calls of their own, grouped the same way, and every output lands in the caller's
    order."""
    S = int(xw.shape[0])
    xo = np.concatenate([[0], np.cumsum(xw[:, 1], dtype=np.int64)]).astype(np.int64)
    costs = torch.empty((S,), dtype=torch.float32, device=dev)
    steps = torch.empty((S,), dtype=torch.int32, device=dev)
    walk = torch.empty((S,), dtype=torch.int32, device=dev) if _steps_walk and path else None
    rows = torch.empty((max(int(xo[-1]), 1), 2), dtype=torch.int32, device=dev) if path else None
    if S:
        lib = _lib.load()
        parts = [(None, None)] if plan is None else [(np.flatnonzero(~plan[0]), None), (np.flatnonzero(plan[0]), (plan[1], plan[2]))]
        with torch.cuda.device(dev):
            st = _stream(dev)
            for sel, blocks in parts:
                if sel is None or sel.size == S:           # the whole call: straight into the outputs
                    _align_launches(lib, xd, xn, yd, yn, D, metric, xw, yw, need, xo[:-1], path, pair_chunk, fill, dev, st, blocks,
                                    rows, costs, steps, walk)
                elif sel.size:                             # a part: its pairs side by side, then to their places
                    n = int(sel.size)
                    c, s = torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
                    w = torch.empty((n,), dtype=torch.int32, device=dev) if walk is not None else None
                    _align_launches(lib, xd, xn, yd, yn, D, metric, xw[sel], yw[sel], need[sel], xo[:-1][sel], path, pair_chunk, fill, dev,
                                    st, blocks, rows, c, s, w)
                    at = torch.from_numpy(sel).to(dev)
                    costs[at], steps[at] = c, s
                    if walk is not None:
                        walk[at] = w
    if path:
        rows = rows[:int(xo[-1])]
    return (rows, costs, steps, xo) + ((walk,) if _steps_walk else ())


def _align_launches(lib, xd, xn, yd, yn, D: int, metric: str, xw, yw, need, ro_all, path: bool, pair_chunk, fill, dev, st, blocks,
                    rows, costs, steps, walk) -> None:
    """the calls of ``sylber_dtw_strings_align`` (``blocks`` None) or ``sylber_dtw_strings_align_split`` (``blocks`` = its block sizes)
    on these pairs, ``_launch_cuts`` pairs each: pair p writes ``costs[p]``, ``steps[p]`` and its runs at ``rows[ro_all[p]:]``"""
    name = "sylber_dtw_strings_align" if blocks is None else "sylber_dtw_strings_align_split"
    size_of = lib.sylber_dtw_strings_workspace_bytes if blocks is None else lib.sylber_dtw_strings_split_workspace_bytes
    more = () if blocks is None else (int(blocks[0]), int(blocks[1]))
    groups = []
    for g0, g1 in _launch_cuts(int(xw.shape[0]), need, pair_chunk):
        x32, y32 = np.ascontiguousarray(xw[g0:g1], np.int32), np.ascontiguousarray(yw[g0:g1], np.int32)
        size = int(size_of(x32.ctypes.data_as(_i32p), y32.ctypes.data_as(_i32p), g1 - g0, int(path), *more))
        if size < 0:
            raise _lib.SylberHipError("sylber_dtw_strings_%sworkspace_bytes refused the call" % ("" if blocks is None else "split_"))
        groups.append((g0, g1, x32, y32, np.ascontiguousarray(ro_all[g0:g1], np.int64), size))

    def at(t, row):                                        # the address of element `row` of a non-empty 4-byte tensor
        return ctypes.c_void_p(t.data_ptr() + int(row) * 4)

    ws = None
    for g0, g1, x32, y32, ro, size in groups:
        if ws is None or ws.numel() != size:               # every launch gets exactly what its size function asked for
            ws = torch.empty(size, dtype=torch.uint8, device=dev)
            if fill is not None:
                ws.fill_(fill)
        _lib.check(getattr(lib, name)(_vp(xd), int(xd.shape[0]), _vp(xn), _vp(yd), int(yd.shape[0]), _vp(yn), D, METRICS[metric],
                                      x32.ctypes.data_as(_i32p), y32.ctypes.data_as(_i32p), g1 - g0, int(path),
                                      ro.ctypes.data_as(_i64p) if path else None, _vp(rows), at(steps, g0), at(costs, g0),
                                      at(walk, g0) if walk is not None else None, *more, _vp(ws), st), name)


def _sequence_rows(seqs, what: str):
    """a list of ``[m, D]`` float arrays / tensors -> ``(the parts as tensors, their lengths int64, D or None)``, or ``ValueError``"""
    if torch.is_tensor(seqs) or isinstance(seqs, np.ndarray):
        raise ValueError("%s must be a list of [m, D] arrays, got one array" % what)
    parts = [_rows(p, "%s[%d]" % (what, i)) for i, p in enumerate(seqs)]
    D = None
    for i, p in enumerate(parts):
        if not p.dtype.is_floating_point:
            raise ValueError("%s[%d]: embeddings are floating point, got %s" % (what, i, p.dtype))
        if D is not None and p.shape[1] != D:
            raise ValueError("%s[%d]: expected D = %d, got %d" % (what, i, D, p.shape[1]))
        D = int(p.shape[1])
    return parts, np.array([p.shape[0] for p in parts], np.int64), D


def _flat_rows(parts, D: int, metric: str, dev):
    """the parts as one prepared ``[max(sum m, 1), D]`` buffer on the device with its norms (``None`` under cosine): a buffer without
    a row gets one zero row, which no window reaches"""
    if sum(int(p.shape[0]) for p in parts) == 0:
        flat = torch.zeros((1, D), dtype=torch.float32, device=dev)
    else:
        flat = _prep(torch.cat([p.to(dev, torch.float32) for p in parts]), metric, dev)
    return flat, (_row_norms(flat) if metric == "l2" else None)


def align_sequences(xs, ys, *, metric: str = "l2", path: bool = False, device="cuda", pair_chunk: Optional[int] = None,
                    split=None, _workspace_fill=None, _steps_walk: bool = False):
    """how two whole recordings line up, syllable by syllable or frame by frame: the global DTW of whole embedding sequences of any
    length up to 65 536 rows, pair by pair (csrc/dtw_strings.hip, ``sylber_dtw_strings_align``; contract in include/sylber_hip.h
    "Embedding strings", restated in tests/dtw_strings_ref.py).  ``xs`` and ``ys``: equally long lists of ``[m, D]`` float arrays or
    tensors (host or device, empty ones allowed) -- the ``segment_features`` or ``hidden_states`` of two ``Segmenter`` calls;
    ``D`` a multiple of 16.

    Without ``path``: ``(costs fp32 [S], steps int32 [S])`` on the device.  With it: ``(rows int64 [sum m, 2], costs, steps,
    x_offsets int64 [S + 1])``, sequence ``xs[s]`` in rows ``x_offsets[s] : x_offsets[s + 1]``.

    The local cost ``d[i][j]`` of row i of x against row j of y is ``search_phrases``'s, word for word, with x in the role of the
    phrase (``"cosine"``: both sides made unit rows).  Global DTW, all additions in fp32, one per cell::

        A[0][0] = d[0][0]                                     n[0][0] = 1
        A[i][j] = d[i][j] + min(A[i-1][j-1], A[i-1][j], A[i][j-1])      (terms outside the matrix are +inf)
                  the first smallest in that order: diagonal, then (i-1, j), then (i, j-1)
        n[i][j] = n[the predecessor taken] + 1

    ``costs = A[m-1][L-1]``; ``steps = n[m-1][L-1]``, the cells on the path, so ``costs / steps`` is the length-normalised DTW
    distance; ``rows[i] = (lo, hi)``: the run of positions inside y (0-based, ``hi`` exclusive) that the path visits in row i of x:
    ``lo[0] = 0``, ``hi[m-1] = L`` and ``lo[i+1]`` is ``hi[i] - 1`` or ``hi[i]``, so the runs are the path.  A pair whose cost is
    not below ``+inf`` (a NaN row on either side) and a pair with an empty side are padding: cost ``+inf``, steps 0, rows
    ``(-1, -1)``.  (Under ``"cosine"`` the rows are made unit rows first, exactly as the index makes them: that keeps a row with a
    NaN in it as the zero row, as it keeps a zero row, and turns a row of ``inf`` into a NaN row.)  For a phrase of at most 64 rows and a span ``[a, b)`` that a phrase search returned,
    ``align_sequences([phrase], [rows[a:b]], path=True)`` is ``align_phrases`` on that span: costs bit for bit, the same steps, the
    runs shifted by ``a``; for any other window the global cost is at least ``align_phrases``'s.

    Nothing depends on ``pair_chunk`` (the pairs per launch; by default as many as keep a launch's workspace below
    ``ALIGN_WORKSPACE_BYTES``), on which pairs share a call, on their order or on stale workspace contents.  It costs ``m L D``
    multiply-adds per pair, on the fp32 MFMA; without ``path`` a pair needs at most 1 MiB of workspace, the path keeps 2 bits per
    cell, about ``m L / 4`` bytes.  ``ValueError`` before any allocation or launch: lists of different length, differing widths or
    a width that is no multiple of 16, a non-float input, a side of more than 65 536 rows, 2^31 or more rows in total on a side,
    ``pair_chunk < 1``, and with ``path`` a single pair whose codes exceed ``ALIGN_WORKSPACE_BYTES``.  ``S = 0`` returns empty
    tensors without a launch.

    ``split``: one pair in one workgroup takes ``m L`` time on one CU of 256 (0.64 s for 8192 x 8192 at D = 768).  A split pair is
    cut into blocks of ``SPLIT_BLOCK`` rows by columns; the blocks of one anti-diagonal run side by side, one launch per
    anti-diagonal (csrc/dtw_strings_split.hip, ``sylber_dtw_strings_align_split``), and every cell is computed by the same code in
    the same order, so the results are the unsplit ones bit for bit.  ``None`` (default): a pair is split when the call's launch
    has fewer pairs than the chip has CUs, the pair has at least two blocks each way (with one band or one chunk no two blocks
    ever run side by side) and ``m L >= SPLIT_MIN_CELLS`` (profiles/dtw_strings_split_bench.md); ``False``: never; ``True``: every pair larger than one block; ``(block_rows,
    block_cols)``, multiples of 128: a test hook, every pair with two non-empty sides in blocks of that size.  The split pairs of a
    call share one workspace and one loop over anti-diagonals per ``pair_chunk`` of them, the others go through the one-workgroup
    kernel as before, and the outputs come back in the caller's order.  A split pair adds to its workspace what
    ``dtw_strings_split_workspace_bytes`` says: about ``32 L + 16 m`` bytes of boundary rows and columns in place of ``16 L``."""
    if metric not in METRICS:
        raise ValueError("metric must be 'l2' or 'cosine', got %r" % (metric,))
    xp, ml, Dx = _sequence_rows(xs, "xs")
    yp, Ll, Dy = _sequence_rows(ys, "ys")
    S, path = int(ml.size), bool(path)
    if S != int(Ll.size):
        raise ValueError("xs and ys must be equally long, got %d and %d sequences" % (S, int(Ll.size)))
    if Dx is not None and Dy is not None and Dx != Dy:
        raise ValueError("xs have D = %d, ys have D = %d" % (Dx, Dy))
    D = Dx or Dy
    if D is not None and (D < 16 or D % 16):
        raise ValueError("the feature width D must be a multiple of 16, got %d" % D)
    _split_plan(ml, Ll, False if split is None else split, None)       # what is wrong with `split` itself
    need = _check_sequence_pairs(ml, Ll, path, pair_chunk)
    dev = _device(device)
    plan = _split_plan(ml, Ll, split, pair_chunk, dev)
    if plan is not None:
        need = _check_sequence_pairs(ml, Ll, path, pair_chunk, plan)
    xw = np.stack([np.cumsum(ml) - ml, ml], 1).astype(np.int32).reshape(S, 2)
    yw = np.stack([np.cumsum(Ll) - Ll, Ll], 1).astype(np.int32).reshape(S, 2)
    if S == 0:
        xd = xn = yd = yn = None
    else:
        (xd, xn), (yd, yn) = _flat_rows(xp, D, metric, dev), _flat_rows(yp, D, metric, dev)
    out = _align_windows(xd, xn, yd, yn, D or 16, metric, xw, yw, need, path, pair_chunk, _workspace_fill, dev, _steps_walk, plan)
    rows, costs, steps, xo = out[:4]
    res = (rows.to(torch.int64), costs, steps, torch.from_numpy(xo).to(dev)) if path else (costs, steps)
    return res + tuple(out[4:])


# ---- whole sequences, local: what local_align_sequences and SyllableIndex.local_align_sequences share -----------------------------
MAX_LOCAL_BEST = 32             # DSL_MAX_BEST of csrc/dtw_strings_local.hip: the rounds of a pair


def _local_rounds(n_best, min_sep) -> Tuple[int, int]:
    """``(n_best, min_sep)`` as ints, or ``ValueError``"""
    for name, v in (("n_best", n_best), ("min_sep", min_sep)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    if not 1 <= int(n_best) <= MAX_LOCAL_BEST:
        raise ValueError("need 1 <= n_best <= %d, got %d" % (MAX_LOCAL_BEST, int(n_best)))
    if not 1 <= int(min_sep) < 2 ** 31:
        raise ValueError("need min_sep >= 1, got %d" % int(min_sep))
    return int(n_best), int(min_sep)


def _local_align_windows(xd, xn, yd, yn, D: int, metric: str, xw: np.ndarray, yw: np.ndarray, sep: np.ndarray, need: np.ndarray, local,
                         n_best: int, pair_chunk, fill, dev):
    """``sylber_dtw_strings_local`` on the pairs of windows ``xw, yw`` int32 ``[S, 2]`` = (first row, rows) with ``sep`` int32 ``[S]``
    into the prepared rows ``xd, yd`` with norms ``xn, yn`` (``None`` under cosine), behind every check -> ``(scores fp32 [S, n_best],
    spans int32 [S, n_best, 4])``; the launches are grouped as ``_align_windows`` groups them"""
    S = int(xw.shape[0])
    scores = torch.empty((S, n_best), dtype=torch.float32, device=dev)
    spans = torch.empty((S, n_best, 4), dtype=torch.int32, device=dev)
    if S:
        lib = _lib.load()
        groups = []
        for g0, g1 in _launch_cuts(S, need, pair_chunk):
            x32, y32 = np.ascontiguousarray(xw[g0:g1], np.int32), np.ascontiguousarray(yw[g0:g1], np.int32)
            size = int(lib.sylber_dtw_strings_local_workspace_bytes(x32.ctypes.data_as(_i32p), y32.ctypes.data_as(_i32p), g1 - g0))
            if size < 0:
                raise _lib.SylberHipError("sylber_dtw_strings_local_workspace_bytes refused the call")
            groups.append((g0, g1, x32, y32, np.ascontiguousarray(sep[g0:g1], np.int32), size))
        radius, gap, min_score = (float(v) for v in local)
        with torch.cuda.device(dev):
            st = _stream(dev)
            ws = None
            for g0, g1, x32, y32, s32, size in groups:
                if ws is None or ws.numel() != size:       # every launch gets exactly what its size function asked for
                    ws = torch.empty(size, dtype=torch.uint8, device=dev)
                    if fill is not None:
                        ws.fill_(fill)
                _lib.check(lib.sylber_dtw_strings_local(_vp(xd), int(xd.shape[0]), _vp(xn), _vp(yd), int(yd.shape[0]), _vp(yn), D, METRICS[metric],
                                                        x32.ctypes.data_as(_i32p), y32.ctypes.data_as(_i32p), s32.ctypes.data_as(_i32p), g1 - g0,
                                                        radius, gap, min_score, n_best, _vp(scores[g0:g1]), _vp(spans[g0:g1]), _vp(ws), st),
                           "sylber_dtw_strings_local")
    return scores, spans


def local_align_sequences(xs, ys=None, *, radius, gap=None, min_score=None, n_best: int = 1, min_sep: int = 1, metric: str = "l2",
                          device="cuda", pair_chunk: Optional[int] = None, _workspace_fill=None):
    """what two whole recordings share, and what one recording says more than once: the LOCAL alignment of whole embedding sequences
    of any length up to 65 536 rows, pair by pair, up to ``n_best`` repeats per pair (csrc/dtw_strings_local.hip,
    ``sylber_dtw_strings_local``; contract in include/sylber_hip.h "Embedding strings, local", restated in
    tests/dtw_strings_local_ref.py).  ``xs`` and ``ys`` are ``align_sequences``'s: equally long lists of ``[m, D]`` float arrays or
    tensors, prepared exactly as there.  ``ys=None`` aligns every sequence of ``xs`` against ITSELF: cells with ``j - i < min_sep``
    are blocked, so with ``min_sep >= 1`` a repeat is reported once, above the diagonal, and never as the sequence against itself.

    -> ``(scores fp32 [S, n_best], spans int64 [S, n_best, 2, 2])`` on the device: ``spans[s, r, 0]`` = (first, one past the last)
    position inside ``xs[s]``, ``spans[s, r, 1]`` the same inside ``ys[s]`` (inside ``xs[s]`` with ``ys=None``).

    The local cost ``d[i][j]`` is ``search_phrases``'s, word for word.  Round ``r = 0 .. n_best - 1`` is ``search_repeats``'s
    recurrence (``radius``, ``gap``, ``min_score`` and their defaults ``2 * radius`` and ``3 * radius`` as there) with the cells of
    the band and of the rectangles ``spans[s, :r]`` of the earlier rounds held at ``H = 0``; its result is the best cell left -- the
    largest ``H``, then the smallest ``i``, then the smallest ``j``.  A round without a positive cell or below ``min_score`` ends
    the pair: it and the later rounds are score 0 and spans -1, as is every round of a pair with an empty side.  Scores never
    increase along ``r``; no path cell of a round lies in an earlier rectangle.  Round 0 between two sequences equals
    ``SyllableIndex.search_repeats`` of ``xs[s]`` as a probe against ``ys[s]`` as the one sequence of an index, bit for bit, where
    that applies (at most 64 rows); here a side may have 65 536.  With ``ys=None`` the two spans of a repeat may overlap (tandem
    repetition); ``spans[..., 0, 1] <= spans[..., 1, 0]`` is the caller's filter.

    Nothing depends on ``pair_chunk``, on which pairs share a call, on their order or on stale workspace contents.  A round costs
    ``m L D`` multiply-adds (about half with ``ys=None``), on the fp32 MFMA, and every round repeats them; a pair needs at most
    1 MiB of workspace whatever ``n_best`` is.  ``ValueError`` before any allocation or launch: what ``align_sequences`` refuses,
    what ``search_repeats`` refuses of ``radius``, ``gap`` and ``min_score``, ``n_best`` outside 1 .. 32, ``min_sep < 1``.
    ``S = 0`` returns empty tensors without a launch.

    Not here: blocking the cells of a path rather than its rectangle; one pair split across workgroups; 16-bit and PQ forms; a
    scan of all pairs of whole sequences without a query (``find_repeats`` proposes pairs); what radius suits real speech."""
    if metric not in METRICS:
        raise ValueError("metric must be 'l2' or 'cosine', got %r" % (metric,))
    local = _local_scalars(radius, gap, min_score)
    n_best, min_sep = _local_rounds(n_best, min_sep)
    xp, ml, Dx = _sequence_rows(xs, "xs")
    S = int(ml.size)
    if ys is None:
        yp, Ll, Dy = xp, ml, Dx
    else:
        yp, Ll, Dy = _sequence_rows(ys, "ys")
        if S != int(Ll.size):
            raise ValueError("xs and ys must be equally long, got %d and %d sequences" % (S, int(Ll.size)))
    if Dx is not None and Dy is not None and Dx != Dy:
        raise ValueError("xs have D = %d, ys have D = %d" % (Dx, Dy))
    D = Dx or Dy
    if D is not None and (D < 16 or D % 16):
        raise ValueError("the feature width D must be a multiple of 16, got %d" % D)
    need = _check_sequence_pairs(ml, Ll, False, pair_chunk)
    dev = _device(device)
    xw = np.stack([np.cumsum(ml) - ml, ml], 1).astype(np.int32).reshape(S, 2)
    yw = np.stack([np.cumsum(Ll) - Ll, Ll], 1).astype(np.int32).reshape(S, 2)
    sep = np.full(S, min_sep if ys is None else 0, np.int32)
    if S == 0:
        xd = xn = yd = yn = None
    else:
        xd, xn = _flat_rows(xp, D, metric, dev)
        yd, yn = (xd, xn) if ys is None else _flat_rows(yp, D, metric, dev)        # a sequence against itself: both windows in one buffer
    scores, spans = _local_align_windows(xd, xn, yd, yn, D or 16, metric, xw, yw, sep, need, local, n_best, pair_chunk, _workspace_fill, dev)
    return scores, spans.to(torch.int64).reshape(S, n_best, 2, 2)


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
        self._seq_cache = None      # (N, default sequence offsets)
        self._planes = {}           # storage -> [N, D] 16-bit copy of _x for search_refined, built on first use
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
        return _prep(x, self.metric, self.device)

    def add(self, features, groups=None, *, _prov=None) -> range:
        """append ``[m, D]`` rows (tensor or array, host or device; cast to fp32) with optional ``groups [m]``; returns their ids"""
        xd, gd, ids, prov = _added_rows(features, groups, self.dim, len(self), "a SyllableIndex", self.metric, self.device)
        if not len(ids):
            return ids
        m, D = xd.shape
        c = _row_norms(xd) if self.metric == "l2" else None
        if _prov is not None:
            prov = np.asarray(_prov, np.float64).reshape(m, 4)
        more = {st: _pack16(xd, st, refuse=True) for st in self._planes}      # raises before anything is appended
        for st, h in more.items():
            self._planes[st] = torch.cat([self._planes[st], h])
        if self._x is None:
            self.dim, self._x, self._c, self._g, self._prov = D, xd, c, gd, prov
        else:
            self._x = torch.cat([self._x, xd])
            self._c = torch.cat([self._c, c]) if c is not None else None
            self._g = torch.cat([self._g, gd])
            self._prov = np.concatenate([self._prov, prov])
        return ids

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
        return _provenance(self._prov, self._span_dtype, len(self), ids)

    # ---- search ---------------------------------------------------------------------------------------------------------------------
    def search(self, queries, k: int, *, groups=None, exclude_same_group: bool = False, splits: int = 0,
               query_chunk: int = DEFAULT_QUERY_CHUNK) -> Tuple[torch.Tensor, torch.Tensor]:
        """the k best rows for each query row -> ``(scores fp32 [n, k], ids int64 [n, k])`` on the device.  ``"l2"``: squared
        distances, ascending; ``"cosine"``: similarities (queries normalised like the rows), descending.  Ties go to the smaller id;
        missing entries are (+inf, -1).  ``exclude_same_group`` skips rows whose group equals the query's (``groups [n]``).
        ``query_chunk`` bounds the workspace; ``splits`` (0 = automatic) is a test hook.  Neither changes the result."""
        k = _check_k_refine(k)[0]
        if len(self) == 0:
            raise ValueError("the index is empty")
        q = _rows_of_width(queries, self.dim, "queries")
        n, D = q.shape
        qg = _query_groups(groups, n, exclude_same_group, self.device)
        splits, query_chunk = _check_splits_chunk(splits, query_chunk)
        scores, ids = _outputs(n, k, self.device)
        if n == 0:
            return scores, ids
        lib = _lib.load()
        qd = self._prep(q)
        N = len(self)
        step = min(n, query_chunk)
        ws = torch.empty(_chunked_workspace_bytes(lib.sylber_knn_workspace_bytes, n, step, N, D, k, splits), dtype=torch.uint8, device=self.device)
        metric = METRICS[self.metric]
        with torch.cuda.device(self.device):
            for r0 in range(0, n, step):
                m = min(step, n - r0)
                _lib.check(lib.sylber_knn_search(_vp(qd[r0:r0 + m]), m, _vp(self._x), N, D, _vp(self._c), metric, k,
                                                 _vp(qg[r0:r0 + m] if qg is not None else None), _vp(self._g if qg is not None else None),
                                                 splits, _vp(scores[r0:r0 + m]), _vp(ids[r0:r0 + m]), _vp(ws), _stream(self.device)),
                           "sylber_knn_search")
        return scores, ids

    # ---- two-stage search ------------------------------------------------------------------------------------------------------------
    def half_rows(self, storage: str = "fp16") -> torch.Tensor:
        """the ``[N, D]`` 16-bit plane of the stored rows that ``search_refined(storage=...)`` scans (``torch.float16`` or
        ``torch.bfloat16``, round to nearest even), built on first use and extended by ``add``; ``2 N D`` bytes.  ``"fp16"`` raises
        ``ValueError`` if a finite stored value lies beyond +-65504."""
        if storage not in STORAGES:
            raise ValueError("storage must be 'fp16' or 'bf16', got %r" % (storage,))
        if len(self) == 0:
            raise ValueError("the index is empty")
        if storage not in self._planes:
            self._planes[storage] = _pack16(self._x, storage, refuse=True)
        return self._planes[storage]

    def search_refined(self, queries, k: int, refine: int = 4, storage: str = "fp16", groups=None, exclude_same_group: bool = False,
                       splits: int = 0, query_chunk: int = DEFAULT_QUERY_CHUNK, return_candidates: bool = False):
        """two-stage ``search``: a 16-bit MFMA scan of ``half_rows(storage)`` picks ``m = k * refine`` candidates per query, the exact
        fp32 score re-ranks only those -> ``(scores, ids)`` shaped, typed, ordered, padded and reported exactly as ``search``'s
        (plus ``cand`` int64 ``[n, m]`` with ``return_candidates=True``: the stage-1 ids in stage-1 order, padded with -1).

        Stage 1: ``q~ = round16(q)``, ``x~ = round16(x)`` (round to nearest even, NaN stays NaN, fp16 saturates at +-65504; queries
        are never refused), ``t(i, j) = fmaf(-2, dot16(q~_i, x~_j), c_j)`` with ``c_j`` the index's fp32 ``||x_j||^2`` (``"l2"``) or
        0 (``"cosine"``) and ``dot16`` the fp32-accumulated sum of the exact 16-bit products in the one fixed order of the kernel's
        MFMA chain.  The candidates of query i are the m best admissible rows under ``(t, j)``; NaN ``t`` and same-group rows are
        not admissible.  Stage 2: the exact ``s = fmaf(-2, q_i . x_j, c_j)`` of ``search``, bit for bit, for each candidate; order
        ``(s, id)``, keep k.

        So the result is ``search`` restricted to the candidate set -- every returned score is a real ``search`` score -- and with
        ``m >= N`` it *is* ``search``, bit for bit.  The only approximation is which rows get re-ranked; ``refine`` controls it.
        ``cand``, scores and ids do not depend on ``splits``, ``query_chunk``, how the index was built or stale workspace contents.
        ``1 <= k <= 128``, integer ``refine >= 1``, ``k * refine <= 128``."""
        k, m = _check_k_refine(k, refine, rerank=True)
        if storage not in STORAGES:
            raise ValueError("storage must be 'fp16' or 'bf16', got %r" % (storage,))
        if len(self) == 0:
            raise ValueError("the index is empty")
        q = _rows_of_width(queries, self.dim, "queries")
        n, D = q.shape
        qg = _query_groups(groups, n, exclude_same_group, self.device)
        splits, query_chunk = _check_splits_chunk(splits, query_chunk)
        scores, ids, cand = _outputs(n, k, self.device, m)
        if n == 0:
            return _result(scores, ids, cand, return_candidates)
        x16 = self.half_rows(storage)
        lib = _lib.load()
        qd = self._prep(q)
        q16 = _pack16(qd, storage, refuse=False)
        N = len(self)
        step = min(n, query_chunk)
        ws = torch.empty(_chunked_workspace_bytes(lib.sylber_knn16_workspace_bytes, n, step, N, D, m, splits), dtype=torch.uint8, device=self.device)
        metric, code = METRICS[self.metric], STORAGES[storage][0]
        xg = self._g if qg is not None else None
        with torch.cuda.device(self.device):
            st = _stream(self.device)
            for r0 in range(0, n, step):
                r1 = min(n, r0 + step)
                _lib.check(lib.sylber_knn16_scan(_vp(q16[r0:r1]), r1 - r0, _vp(x16), N, D, _vp(self._c), code, m,
                                                 _vp(qg[r0:r1] if qg is not None else None), _vp(xg), splits, _vp(cand[r0:r1]), _vp(ws),
                                                 st), "sylber_knn16_scan")
                _lib.check(lib.sylber_knn_rerank(_vp(qd[r0:r1]), r1 - r0, _vp(self._x), N, D, _vp(self._c), metric, _vp(cand[r0:r1]), m, k,
                                                 _vp(scores[r0:r1]), _vp(ids[r0:r1]), st), "sylber_knn_rerank")
        return _result(scores, ids, cand, return_candidates)

    # ---- phrase search --------------------------------------------------------------------------------------------------------------
    def sequence_offsets(self) -> np.ndarray:
        """int64 ``[S + 1]``: the default sequences of ``search_phrases``, sequence ``s`` = rows ``offsets[s] : offsets[s + 1]``: the
        maximal runs of consecutive rows with equal group, numbered in row order (``from_outputs``: one per non-empty clip)"""
        N = len(self)
        if self._seq_cache is None or self._seq_cache[0] != N:
            self._seq_cache = (N, _group_runs(self._g, N))
        return self._seq_cache[1].copy()

    def search_phrases(self, phrases, k: int, *, lengths=None, groups=None, exclude_same_group: bool = False, sequences=None,
                       splits: int = 0, phrase_chunk: int = DEFAULT_PHRASE_CHUNK, block_phrases: int = 0,
                       _workspace_fill=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """query-by-example search of syllable *sequences*: the k best sequences of the index for each phrase, by subsequence DTW
        -> ``(costs fp32 [P, k], seqs int64 [P, k], spans int64 [P, k, 2])`` on the device; a span is (first row id, one past the last
        row id) of the match, so ``provenance`` works on it.  At most one match per sequence: its best one.  ``phrases``: a list of
        ``[m_p, D]`` arrays / tensors (host or device), or one ``[sum m_p, D]`` array with ``lengths=[m_0, m_1, ...]``; ``1 <= m_p <= 64``.

        Sequences: by default ``sequence_offsets()``; ``sequences=`` takes explicit offsets ``[S + 1]`` (ascending, first 0, last N, no
        empty sequence; at most 65 536 rows each).  A sequence's group, for ``exclude_same_group`` (``groups [P]``), is the group of
        its first row.

        Local cost of phrase row i against database row j, in fp32, from the score ``s = fmaf(-2, q_i . x_j, c_j)`` of ``search``
        (same contraction, same bits):

        * ``"l2"``: ``d = max(0, ||q_i||^2 + s)``, i.e. exactly the score ``search`` reports;
        * ``"cosine"``: phrase rows are made unit rows as ``search`` does; ``d = max(0, 1 - (-s / 2))`` (the halving is exact, the
          subtraction rounds once);
        * a NaN ``d`` (a NaN row on either side) counts as ``+inf``.

        Subsequence DTW of a phrase of m rows against a sequence with columns j = 0 .. L - 1 (the phrase is consumed whole, its span
        in the sequence is free), all additions in fp32, one per cell::

            A[0][j] = d[0][j]                                   start[0][j] = j
            A[i][j] = d[i][j] + min(A[i-1][j-1], A[i-1][j], A[i][j-1])      (terms outside the sequence are +inf)
                      on equal values the predecessor is taken in that order: diagonal, then (i-1, j), then (i, j-1);
                      start[i][j] = start of the predecessor taken
            cost = min_j A[m-1][j], the smallest such j on ties = end;   span = (row of start[m-1][end], row of end + 1)

        A sequence whose cost is ``+inf`` is never returned.  Each phrase's list is ordered by (cost, sequence number) ascending, the
        strict order ``search`` uses; lists with fewer than k admissible sequences end in cost ``+inf``, sequence -1, span (-1, -1).
        Because fp32 ``+`` and ``min`` in a fixed cell order are deterministic, the result is unique: it does not depend on the split
        of the database, the packing or chunking of phrases, stale workspace contents, or whether the index came from one ``add`` or
        many.  ``m > L`` is legal (vertical steps).  No normalisation by path length: divide by ``m`` if you want it.

        Test hooks, none of which changes the result: ``splits`` (0 = automatic) asks for that many cuts of the database (cuts fall
        on sequence starts only), ``phrase_chunk`` bounds the phrases per launch (and so the workspace), ``block_phrases`` (0 =
        automatic) the phrases packed into one 128-row query block."""
        return self._scan_phrases(lambda: (self._scan32("sylber_dtw_search"), None), phrases, k, None, None, lengths, groups, exclude_same_group,
                                  sequences, splits, phrase_chunk, block_phrases, False, _workspace_fill)

    def search_phrases_refined(self, phrases, k: int, refine: int = 4, storage: str = "fp16", *, lengths=None, groups=None,
                               exclude_same_group: bool = False, sequences=None, splits: int = 0,
                               phrase_chunk: int = DEFAULT_PHRASE_CHUNK, block_phrases: int = 0, return_candidates: bool = False,
                               _workspace_fill=None):
        """two-stage ``search_phrases``: a 16-bit MFMA subsequence-DTW scan of ``half_rows(storage)`` picks ``m = k * refine`` candidate
        sequences per phrase, the exact fp32 subsequence DTW re-ranks only those -> ``(costs, seqs, spans)`` shaped, typed, ordered,
        padded and placed exactly as ``search_phrases``'s; with ``return_candidates=True`` also ``cand`` int64 ``[P, m]`` (the stage-1
        sequence numbers in stage-1 order, padded with -1) and ``coarse`` fp32 ``[P, m]`` (their stage-1 costs, padded with ``+inf``).

        Stage 1: the phrase rows, prepared as ``search_phrases`` prepares them, and the stored rows are rounded to 16 bits as
        ``search_refined`` rounds them (round to nearest even, NaN stays NaN, fp16 saturates at +-65504; phrases are never
        refused); ``t(i, j) = fmaf(-2, dot16(q~_i, x~_j), c_j)`` is ``search_refined``'s coarse score.  Local cost in fp32:
        ``"l2"``: ``d~ = max(0, ||q_i||^2 + t)`` with the fp32 ``||q_i||^2`` of the *unrounded* phrase row; ``"cosine"``:
        ``d~ = max(0, 1 - (0 - t / 2))``; a NaN ``d~`` counts as ``+inf``.  Over ``d~`` the recurrence of ``search_phrases``, one
        fp32 addition per cell; the coarse cost of (phrase, sequence) is ``min_j A[m-1][j]``.  The candidates of a phrase are its m
        best admissible sequences under (coarse cost, sequence number); a cost of ``+inf`` and, with ``exclude_same_group``, the
        phrase's own group are not admissible.  Stage 2: for each candidate the exact ``search_phrases`` cost, start and end of that
        (phrase, sequence) pair, bit for bit; order (cost, sequence), keep k.

        So the result is ``search_phrases`` restricted to the candidate sequences -- every returned cost and span is a real
        ``search_phrases`` cost and span -- and with m at least the number of admissible sequences of finite cost it *is*
        ``search_phrases``, bit for bit.  The only approximation is which sequences get re-ranked; ``refine`` controls it.  ``cand``,
        ``coarse``, costs, seqs and spans do not depend on ``splits``, ``phrase_chunk``, ``block_phrases``, stale workspace contents
        or how the index was built.  All of ``search_phrases``'s limits, integer ``refine >= 1``, ``k * refine <= 128``,
        ``storage`` ``"fp16"`` (refuses stored values beyond +-65504, as ``half_rows`` does) or ``"bf16"``."""
        return self._scan_phrases(lambda: (self._scan16(storage), lambda c: _rerank_launch(c, self._x, self._c)), phrases, k, refine, storage,
                                  lengths, groups, exclude_same_group, sequences, splits, phrase_chunk, block_phrases, return_candidates,
                                  _workspace_fill)

    def search_occurrences(self, phrases, k: int, *, lengths=None, groups=None, exclude_same_group: bool = False, sequences=None,
                           splits: int = 0, phrase_chunk: int = DEFAULT_PHRASE_CHUNK, block_phrases: int = 0,
                           _workspace_fill=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """every non-overlapping occurrence of each phrase, not one match per sequence: the k best occurrences over the whole index
        -> ``(costs fp32 [P, k], seqs int64 [P, k], spans int64 [P, k, 2])`` on the device, as ``search_phrases`` shapes them; a
        keyword said five times in one long recording comes back five times, with one sequence number.  Arguments, sequences,
        local costs ``d``, the recurrence, the predecessor order on ties, ``start[i][j]`` and the NaN -> ``+inf`` rule are
        ``search_phrases``'s, word for word (csrc/dtw.hip, ``sylber_dtw_occurrences``; restated in tests/occ_ref.py).

        For one phrase (m rows) and one sequence (columns ``0 .. L - 1``) let ``E[j] = A[m-1][j]``, ``st[j] = start[m-1][j]``:

        1. Families.  Only columns with ``E[j] < +inf`` count.  Columns with equal ``st[j]`` form a family: ``start = st[j]``,
           ``cost = min E[j]``, ``end`` = the smallest such j.  Over the finite columns ``st[j]`` does not decrease with j, so a
           family is a run of neighbouring finite columns and families arrive in ascending start and ascending end.
        2. One left-to-right pass keeps non-overlapping families.  The first becomes *pending*.  For each later family ``F``: if
           ``F.start <= pending.end`` (the spans share a row) the cheaper of the two stays pending, the pending one on equal cost;
           otherwise the pending family is *emitted* and ``F`` becomes pending.  At the sequence end the pending family is emitted.
           Emitted occurrences of one sequence are pairwise disjoint; each is a real warping path with the cost, start and end the
           recurrence gives it.
        3. Per phrase the k best emitted occurrences over all admissible sequences (``exclude_same_group`` as in
           ``search_phrases``), ordered strictly by (cost, first row id of the span) ascending, which refines ``search_phrases``'s
           (cost, sequence); padding ``(+inf, -1, (-1, -1))``.

        So the best occurrence of a sequence under (cost, start) is bit for bit ``search_phrases``'s (cost, span) of that pair, and
        keeping each sequence's first entry gives ``search_phrases`` when nothing was cut off at k; for one-row phrases every
        finite row is an occurrence, so the call is ``search`` (ids = span starts); nothing depends on ``splits``,
        ``phrase_chunk``, ``block_phrases``, stale workspace contents or one ``add`` against many.

        The pass is **not** global greedy suppression by cost: of a chain A - B - C with A and C disjoint, both overlapping B, and
        costs A > B > C it emits only C, where greedy suppression would also keep A.  The one-pass rule is what runs inside the
        scan with constant state per lane.  No cost threshold, no cap per sequence: filter the result."""
        return self._scan_phrases(lambda: (self._scan32("sylber_dtw_occurrences"), None), phrases, k, None, None, lengths, groups,
                                  exclude_same_group, sequences, splits, phrase_chunk, block_phrases, False, _workspace_fill)

    def search_occurrences_refined(self, phrases, k: int, refine: int = 4, storage: str = "fp16", *, lengths=None, groups=None,
                                   exclude_same_group: bool = False, sequences=None, splits: int = 0,
                                   phrase_chunk: int = DEFAULT_PHRASE_CHUNK, block_phrases: int = 0, return_candidates: bool = False,
                                   _workspace_fill=None):
        """two-stage ``search_occurrences``: stage 1 is ``search_phrases_refined``'s, unchanged -- the 16-bit MFMA scan picks
        ``m = k * refine`` candidate *sequences* per phrase -- and stage 2 finds every occurrence in those sequences with the exact
        fp32 recurrence (csrc/dtw16.hip, ``sylber_dtw_rerank_occurrences``) -> ``(costs, seqs, spans)`` as ``search_occurrences``
        returns them; with ``return_candidates=True`` also ``cand`` int64 ``[P, m]`` and ``coarse`` fp32 ``[P, m]``, which are
        ``search_phrases_refined``'s.

        The result is ``search_occurrences`` restricted to the sequences of ``cand``, bit for bit, and with m at least the number
        of admissible sequences of finite cost it *is* ``search_occurrences``.  The only approximation is which sequences are
        searched: stage 1 ranks a sequence by its best match, so a sequence whose many occurrences are all mediocre can be left
        out.  Nothing returned depends on ``splits``, ``phrase_chunk``, ``block_phrases``, stale workspace contents or how the
        index was built.  Limits and refusals are ``search_phrases_refined``'s."""
        def rerank(c):
            _occ_rerank_launch(c, "sylber_dtw_rerank_occurrences", (_vp(self._x), c.N, c.dim, _vp(self._c)))

        return self._scan_phrases(lambda: (self._scan16(storage), rerank), phrases, k, refine, storage, lengths, groups, exclude_same_group,
                                  sequences, splits, phrase_chunk, block_phrases, return_candidates, _workspace_fill)

    def search_phrases_seeded(self, phrases, seed_scores, seed_ids, k: int, refine: int = 4, *, lengths=None, groups=None,
                              exclude_same_group: bool = False, sequences=None, phrase_chunk: int = DEFAULT_PHRASE_CHUNK,
                              return_candidates: bool = False, _trusted_ids: bool = False):
        """``search_phrases`` over candidate sequences found from per-row neighbours instead of a scan of the corpus: ``seed_scores``
        fp32 and ``seed_ids`` int64, ``[R, seeds]`` each (tensors or arrays; ``1 <= seeds <= 128``), are what a ``search`` *reports*
        for each of the R phrase rows (concatenated in phrase order) under this index's metric -- from ``IVFSyllableIndex.search``,
        ``search`` itself or anywhere else.  Stage 1 (csrc/phrase_vote.hip, ``sylber_phrase_vote``; tests/phrase_vote_ref.py) lets
        the seeds vote for ``m = k * refine <= 128`` candidate sequences per phrase; stage 2 is the exact re-rank of
        ``search_phrases_refined`` -> ``(costs, seqs, spans)`` shaped, typed, ordered, padded and placed exactly as
        ``search_phrases``'s; with ``return_candidates=True`` also ``cand`` int64 ``[P, m]`` (padded with -1) and ``bound`` fp32
        ``[P, m]`` (padded with ``+inf``).

        The vote.  Local cost of a seed: ``"l2"``: ``d = score``; ``"cosine"``: ``d = max(0, 1 - score)`` -- bit for bit the ``d`` of
        ``search_phrases`` for that pair of rows.  A seed is ignored when its id is -1, its score is NaN or its ``d`` is ``+inf``.
        For phrase p with rows i = 0 .. m_p - 1: ``floor_i`` = the largest ``d`` among row i's valid seeds (0 without one);
        ``best_i(s)`` = the smallest ``d`` among row i's valid seeds in sequence s (``floor_i`` without one); s is *seen* when some
        row has a valid seed in it, *admissible* unless, with ``exclude_same_group``, its group is the phrase's;
        ``bound(p, s) = (((0 + best_0) + best_1) + ... + best_{m_p - 1})`` in fp32, ascending i.  The candidates are the m smallest
        admissible seen sequences of finite bound under (bound, sequence number).

        So the result is ``search_phrases`` restricted to the candidates: every returned cost and span is a real ``search_phrases``
        cost and span, bit for bit; the only approximation is which sequences are re-ranked.  When the seeds of every row are its
        ``seeds`` nearest rows of the whole index, ``bound(p, s) <= cost(p, s)`` exactly (a warping path visits every phrase row; a
        row that is no seed costs at least the floor; fp32 addition is monotone); when every admissible row is a seed and m is at
        least the number of admissible sequences, the result *is* ``search_phrases``.  Every operation of the vote is an fp32 min,
        max or add in a fixed order: nothing returned depends on the order of the seeds within a row, on duplicates or on
        ``phrase_chunk``.  ``ValueError`` before any launch: ``search_phrases_refined``'s checks, seed tensors of another shape or
        dtype, an id outside ``[-1, N)``."""
        return self._seeded(lambda c: _rerank_launch(c, self._x, self._c), phrases, seed_scores, seed_ids, k, refine, lengths, groups,
                            exclude_same_group, sequences, phrase_chunk, return_candidates, _trusted_ids)

    def search_occurrences_seeded(self, phrases, seed_scores, seed_ids, k: int, refine: int = 4, *, lengths=None, groups=None,
                                  exclude_same_group: bool = False, sequences=None, phrase_chunk: int = DEFAULT_PHRASE_CHUNK,
                                  return_candidates: bool = False, _trusted_ids: bool = False, _workspace_fill=None):
        """``search_occurrences`` over candidate sequences found from per-row neighbours: stage 1 is ``search_phrases_seeded``'s,
        unchanged -- the seeds vote for ``m = k * refine <= 128`` candidate *sequences* per phrase -- and stage 2 finds every
        occurrence in those sequences with the exact fp32 recurrence (``sylber_dtw_rerank_occurrences``) -> ``(costs, seqs,
        spans)`` as ``search_occurrences`` returns them; with ``return_candidates=True`` also ``cand`` int64 ``[P, m]`` and ``bound``
        fp32 ``[P, m]``, which are ``search_phrases_seeded``'s, bit for bit.

        The result is ``search_occurrences`` restricted to the sequences of ``cand``, bit for bit.  The only approximation is which
        sequences are searched: the vote ranks a sequence by a bound on its best match, so a sequence whose many occurrences are
        all mediocre can be left out.  Nothing returned depends on ``phrase_chunk``, on stale workspace contents or on how the
        index was built.  Arguments, checks and refusals are ``search_phrases_seeded``'s."""
        def rerank(c):
            _occ_rerank_launch(c, "sylber_dtw_rerank_occurrences", (_vp(self._x), c.N, c.dim, _vp(self._c)))

        return self._seeded(rerank, phrases, seed_scores, seed_ids, k, refine, lengths, groups, exclude_same_group, sequences, phrase_chunk,
                            return_candidates, _trusted_ids, _workspace_fill)

    def _seeded(self, rerank, phrases, seed_scores, seed_ids, k, refine, lengths, groups, exclude_same_group, sequences, phrase_chunk,
                return_candidates, trusted_ids, fill=None):
        """the checks of ``search_phrases_seeded`` in their order, then ``_seeded_phrases`` with this stage 2"""
        k, m = _check_k_refine(k, refine, rerank=True)
        q, lens, pg, off = _phrase_args(len(self), self.dim, self.device, self.sequence_offsets, phrases, lengths, groups, exclude_same_group,
                                        sequences, 0, phrase_chunk, 0)
        R, N, dev = int(q.shape[0]), len(self), self.device
        sc = seed_scores if torch.is_tensor(seed_scores) else torch.from_numpy(np.asarray(seed_scores))
        si = seed_ids if torch.is_tensor(seed_ids) else torch.from_numpy(np.asarray(seed_ids))
        if sc.dim() != 2 or si.dim() != 2 or sc.shape != si.shape or sc.shape[0] != R:
            raise ValueError("seed_scores and seed_ids must both be [%d phrase rows, seeds], got %s and %s" % (R, tuple(sc.shape), tuple(si.shape)))
        if sc.dtype != torch.float32 or si.dtype != torch.int64:
            raise ValueError("seed_scores must be float32 and seed_ids int64, got %s and %s" % (sc.dtype, si.dtype))
        seeds = int(sc.shape[1])
        if not 1 <= seeds <= MAX_SEEDS:
            raise ValueError("seeds must be in [1, %d], got %d" % (MAX_SEEDS, seeds))
        sc, si = sc.to(dev).contiguous(), si.to(dev).contiguous()
        if not trusted_ids and R and (int(si.min()) < -1 or int(si.max()) >= N):
            raise ValueError("seed_ids must lie in [-1, %d)" % N)
        return _seeded_phrases(N, self.dim, dev, self.metric, self._g, q, lens, pg, off, sc, si, k, m, phrase_chunk, return_candidates,
                               rerank, fill)

    # ---- warping paths -------------------------------------------------------------------------------------------------------------
    def align_phrases(self, phrases, spans, lengths=None, pair_chunk: Optional[int] = None, *, _tracked_start: bool = False):
        """*how* each phrase matches each of its spans: the stored rows every phrase row was warped onto ->
        ``(rows int64 [P, k, Mx, 2], steps int32 [P, k], costs fp32 [P, k])`` on the device, ``Mx = max_p m_p``.  ``phrases`` and
        ``lengths=`` are exactly what the search that produced ``spans`` was given; ``spans`` int64 ``[P, k, 2]`` (host or device):
        (first row id, one past the last), ``(-1, -1)`` = padding -- the spans of ``search_phrases``, ``search_phrases_refined``,
        ``search_phrases_seeded``, ``search_occurrences``, ``search_occurrences_refined`` or ``search_occurrences_seeded``, or any windows
        of your own.
        ``rows[p, r, i]`` = (first row id, one past the last row id) of the stored rows that phrase row i is aligned to, so
        ``provenance`` works on it; ``(-1, -1)`` for ``i >= m_p``, for padding spans and for pairs of cost ``+inf``.  ``steps``: the
        cells on the path, 0 where ``rows`` is all padding; ``costs``: the DP's cost of that path, ``+inf`` there
        (csrc/dtw_align.hip, ``sylber_dtw_align``; restated in tests/align_ref.py).

        Window DP, for one pair (phrase of m rows, window ``[a, b)``): the local costs ``d[i][j]`` are ``search_phrases``'s, bit for
        bit (phrase rows prepared as there: unit rows under ``"cosine"``); the window is taken as **one** sequence whose first
        column is ``a``, with a free start (``A[0][j] = d[0][j]`` for every column of the window) and a forced end: the path ends in
        cell ``(m-1, b-1)``; recurrence and predecessor order on ties are ``search_phrases``'s: diagonal, then ``(i-1, j)``, then
        ``(i, j-1)``.  The path is the chain of predecessors from ``(m-1, b-1)`` back to the row-0 cell it reaches; ``costs =
        A[m-1][b-1]``; ``rows[i]`` is the run of columns the path visits in phrase row i (a monotone path visits one contiguous run
        per row and ``lo[i+1]`` is ``hi[i]`` or ``hi[i] + 1``, so the runs *are* the path).

        The theorem: if ``[a, b)`` is a span a phrase search of this index returned for that phrase, the path starts in column
        ``a``, ``costs`` has the bits of the reported cost, and the path is the full scan's own path (every window cell's ``A`` is
        at least the full DP's -- fewer paths, monotone fp32 ``+`` -- and equal on the optimal path, so the first smallest
        predecessor is the same one).  Any other window is legal and gets what the definition gives; its path may start inside it.

        ``costs / steps`` is the length-normalised DTW cost: ``steps`` is the divisor that belongs under a DTW sum.  Nothing
        returned depends on ``pair_chunk`` (the pairs per launch; by default the workspace, 16 B per window column and pair, stays
        below 256 MiB), on stale workspace contents, on one ``add`` against many or on a ``save`` / ``load`` round trip.
        ``ValueError`` before any launch: what ``search_phrases`` refuses of the phrases; ``spans`` of another shape or dtype; a
        span that is neither ``(-1, -1)`` nor ``0 <= a < b <= N``; a window of more than 65 536 rows."""
        N = len(self)

        def run(lib, b, qn, place_d, len_d, pair_phrase, win, max_cols, rows, steps, costs, start, ws, st):
            _lib.check(lib.sylber_dtw_align(_vp(b.qp), b.nb, _vp(qn), _vp(place_d), _vp(len_d), b.Pc, _vp(self._x), N, self.dim, _vp(self._c),
                                            METRICS[self.metric], _vp(pair_phrase), _vp(win), int(pair_phrase.shape[0]), max_cols,
                                            int(rows.shape[1]), _vp(rows), _vp(steps), _vp(costs), _vp(start), _vp(ws), st), "sylber_dtw_align")

        return _align_phrases(N, self.dim, self.device, self.metric, phrases, spans, lengths, pair_chunk, run, _tracked_start)

    def align_sequences(self, pairs, *, path: bool = False, pair_chunk: Optional[int] = None, sequences=None, split=None,
                        _workspace_fill=None):
        """``align_sequences`` between stored sequences, with no copy: ``pairs`` int ``[S, 2]`` (host or device) are sequence numbers
        of the index, x then y -- by default of ``sequence_offsets()``, or of ``sequences=`` as ``search_phrases`` takes them.  The
        windows go into the index's own rows with its stored norms (unit rows under ``"cosine"``), so the result is the free
        function's on those rows under the index's metric, bit for bit.  Without ``path``: ``(costs fp32 [S], steps int32 [S])``.
        With it: ``(rows int64 [sum m, 2], costs, steps, x_offsets int64 [S + 1])`` where ``rows`` are row ids of the index (``lo``
        and ``hi`` shifted by y's first row, padding stays ``(-1, -1)``): ``align_phrases`` and ``provenance`` take them.
        ``ValueError`` before any launch: an empty index, ``pairs`` of another shape or dtype, a sequence number outside
        ``[0, number of sequences)``, and what ``align_sequences`` refuses of ``pair_chunk``, of ``split`` and of a pair's codes.
        ``split`` is ``align_sequences``'s: by default a call of few long pairs spreads each over the chip, with the same bits."""
        N = len(self)
        if N == 0:
            raise ValueError("the index is empty")
        pr = np.asarray(pairs.detach().cpu().numpy() if torch.is_tensor(pairs) else pairs)
        if pr.size == 0:
            pr = pr.reshape(0, 2).astype(np.int64)
        if pr.ndim != 2 or pr.shape[1] != 2 or pr.dtype.kind not in "iu":
            raise ValueError("pairs must be integer [S, 2] sequence numbers, got %s %s" % (pr.dtype, pr.shape))
        off = _sequences(sequences, N, self.sequence_offsets)
        nseq = off.size - 1
        pr = pr.astype(np.int64)
        if pr.size and (pr.min() < 0 or pr.max() >= nseq):
            raise ValueError("pairs must name sequences in [0, %d)" % nseq)
        path = bool(path)
        first, length = off[:-1][pr], np.diff(off)[pr]      # [S, 2] each
        _check_pair_chunk(pair_chunk)
        plan = _split_plan(length[:, 0], length[:, 1], split, pair_chunk, self.device)
        need = _check_sequence_pairs(length[:, 0], length[:, 1], path, pair_chunk, plan)
        xw = np.stack([first[:, 0], length[:, 0]], 1).astype(np.int32)
        yw = np.stack([first[:, 1], length[:, 1]], 1).astype(np.int32)
        rows, costs, steps, xo = _align_windows(self._x, self._c, self._x, self._c, self.dim, self.metric, xw, yw, need, path, pair_chunk,
                                                _workspace_fill, self.device, plan=plan)
        if not path:
            return costs, steps
        rows = rows.to(torch.int64)
        shift = torch.from_numpy(np.repeat(first[:, 1], length[:, 0])).to(self.device)
        rows = torch.where(rows >= 0, rows + shift[:, None], rows)
        return rows, costs, steps, torch.from_numpy(xo).to(self.device)

    def local_align_sequences(self, pairs, radius, *, gap=None, min_score=None, n_best: int = 1, min_sep: int = 1,
                              pair_chunk: Optional[int] = None, sequences=None, _workspace_fill=None):
        """``local_align_sequences`` between stored sequences, with no copy: every repeat between two whole sequences of the index,
        or inside one.  ``pairs`` int ``[S, 2]`` are sequence numbers as ``align_sequences`` takes them; a pair ``(s, s)`` is the
        repeats inside ``s``, with the cells ``j - i < min_sep`` blocked, every other pair has no band.  The windows go into the
        index's own rows with its stored norms, so the result is the free function's on those rows under the index's metric, bit
        for bit -> ``(scores fp32 [S, n_best], spans int64 [S, n_best, 2, 2])`` where ``spans`` are ROW IDS of the index (first,
        one past the last; padding stays -1): ``provenance`` and ``align_phrases`` take them.  The pairs that ``find_repeats``
        returns are pairs for this call: it gives the full extent of a repeat whose window ``find_repeats`` found, with a score
        that is never smaller.  ``ValueError`` before any launch: an empty index, what ``align_sequences`` refuses of ``pairs``,
        ``sequences`` and ``pair_chunk``, and what the free function refuses of its scalars."""
        N = len(self)
        if N == 0:
            raise ValueError("the index is empty")
        local = _local_scalars(radius, gap, min_score)
        n_best, min_sep = _local_rounds(n_best, min_sep)
        pr = np.asarray(pairs.detach().cpu().numpy() if torch.is_tensor(pairs) else pairs)
        if pr.size == 0:
            pr = pr.reshape(0, 2).astype(np.int64)
        if pr.ndim != 2 or pr.shape[1] != 2 or pr.dtype.kind not in "iu":
            raise ValueError("pairs must be integer [S, 2] sequence numbers, got %s %s" % (pr.dtype, pr.shape))
        off = _sequences(sequences, N, self.sequence_offsets)
        nseq = off.size - 1
        pr = pr.astype(np.int64)
        if pr.size and (pr.min() < 0 or pr.max() >= nseq):
            raise ValueError("pairs must name sequences in [0, %d)" % nseq)
        first, length = off[:-1][pr], np.diff(off)[pr]      # [S, 2] each
        need = _check_sequence_pairs(length[:, 0], length[:, 1], False, pair_chunk)
        xw = np.stack([first[:, 0], length[:, 0]], 1).astype(np.int32)
        yw = np.stack([first[:, 1], length[:, 1]], 1).astype(np.int32)
        sep = np.where(pr[:, 0] == pr[:, 1], min_sep, 0).astype(np.int32)
        scores, spans = _local_align_windows(self._x, self._c, self._x, self._c, self.dim, self.metric, xw, yw, sep, need, local, n_best,
                                             pair_chunk, _workspace_fill, self.device)
        S = int(pr.shape[0])
        spans = spans.to(torch.int64).reshape(S, n_best, 2, 2)
        shift = torch.from_numpy(np.ascontiguousarray(first)).to(self.device)[:, None, :, None]
        return scores, torch.where(spans >= 0, spans + shift, spans)

    # ---- repeated phrases ---------------------------------------------------------------------------------------------------------------
    def search_repeats(self, probes, k: int, radius, *, gap=None, min_score=None, lengths=None, groups=None,
                       exclude_same_group: bool = False, sequences=None, splits: int = 0, phrase_chunk: int = DEFAULT_PHRASE_CHUNK,
                       block_phrases: int = 0, _workspace_fill=None, _after_seq=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """which part of each probe is said anywhere in the index: LOCAL alignment of each probe against every sequence, the k best
        sequences per probe -> ``(scores fp32 [P, k], seqs int64 [P, k], spans int64 [P, k, 2, 2])`` on the device.
        ``spans[p, r, 0]`` = (first, one past the last) position inside the probe, ``spans[p, r, 1]`` = (first, one past the last)
        row id of the index, so ``provenance`` works on it.  ``probes``, ``lengths``, ``groups``, ``sequences`` and the test hooks
        are ``search_phrases``'s, and so are the limits (``1 <= m <= 64`` rows, sequences of at most 65 536 rows, ``k <= 128``).

        Contract ("Embedding repeats" in include/sylber_hip.h, restated in tests/repeats_ref.py; csrc/dtw_local.hip).  The local
        cost ``d[i][j]`` is ``search_phrases``'s, word for word.  ``radius > 0`` and ``gap >= 0`` are taken as fp32; everything is
        fp32 with one rounding per operation, exactly as written::

            s  = radius - d[i][j]            (-inf where d = +inf)
            sg = s - gap
            H[i][-1] = H[-1][j] = 0
            c_diag = H[i-1][j-1] + s     start: start[i-1][j-1] if H[i-1][j-1] > 0 else (i, j)
            c_up   = H[i-1][j]   + sg    start: start[i-1][j]
            c_left = H[i][j-1]   + sg    start: start[i][j-1]
            v = the first largest of (c_diag, c_up, c_left) in that order; H[i][j] = v if v > 0 else 0

        Every step lands on a cell and earns that cell's ``s``: a pair of syllables closer than ``radius`` earns, a farther one
        costs.  A non-diagonal step (one syllable said as two, a syllable without a partner) also pays ``gap``.  ``gap = 0`` is a
        local DTW with free warping, a large ``gap`` is Smith-Waterman without gaps.  The result of (probe, sequence) is the best
        cell -- the largest ``H``, then the smallest ``i``, then the smallest ``j`` -- with ``score = H[i][j]`` and the spans
        ``[si, i + 1)``, ``[sj, j + 1)`` from ``(si, sj) = start[i][j]``; no positive cell, no result.  Both spans are non-empty.

        Per probe a sequence is admissible with ``score >= min_score`` (and a group other than the probe's under
        ``exclude_same_group``); the k best are ordered strictly by (score descending, sequence ascending); padding is score 0,
        sequence -1, spans -1.  Nothing depends on ``splits``, ``phrase_chunk``, ``block_phrases``, stale workspace contents or one
        ``add`` against many.

        ``radius`` is required: it is in the unit of ``d`` (squared L2 distance, or ``1 - cosine``), and what radius suits real
        speech has not been measured here -- look at the ``search`` scores of syllables you know to be the same.  ``gap=None``
        means ``2 * radius``, ``min_score=None`` means ``3 * radius`` (three perfect matches), both exact products in fp32.
        ``ValueError`` before any launch: whatever ``search_phrases`` refuses, a ``radius`` that is not finite and ``> 0``, a ``gap``
        that is not finite and ``>= 0``, a ``min_score`` that is not finite and ``> 0`` (all three as fp32)."""
        local = _local_scalars(radius, gap, min_score)
        after = None if _after_seq is None else np.ascontiguousarray(_after_seq, np.int32)
        return self._scan_phrases(lambda: (self._scan_local(), None), probes, k, None, None, lengths, groups, exclude_same_group, sequences,
                                  splits, phrase_chunk, block_phrases, False, _workspace_fill, local + (after,))

    def find_repeats(self, k: int, radius, *, gap=None, min_score=None, window: int = 64, hop: int = 32, sequences=None,
                     exclude_same_group: bool = False, splits: int = 0, phrase_chunk: int = DEFAULT_PHRASE_CHUNK,
                     _workspace_fill=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """what is said more than once, found without a query and without a codebook: the k best repeats between two sequences of
        the index -> ``(scores fp32 [k], pairs int64 [k, 2], spans int64 [k, 2, 2])`` on the device, shaped and padded like
        ``UnitIndex.find_repeats``'s: ``pairs[r] = (s, t)`` with ``s < t``, ``spans[r] = ((a0, a1), (b0, b1))`` ROW IDS (first,
        one past the last) in sequence ``s`` and in sequence ``t``; shorter lists end in score 0, pairs ``(-1, -1)``, spans -1.

        The probes are windows of the index's own sequences -- the rows as the index holds them, prepared like any probe (under
        ``"cosine"`` the stored unit rows are normalised once more) -- searched with ``search_repeats`` (same ``radius``, ``gap``,
        ``min_score``, same contract).  A sequence of ``L`` rows gives one window if ``L <= window``, else
        ``ceil((L - window) / hop) + 1``; window ``r`` = rows ``min(r * hop, L - window)`` onwards, ``min(window, L)`` of them
        (``1 <= hop <= window <= 64``).  A window of sequence ``s`` is aligned against the sequences ``t > s`` only (with
        ``exclude_same_group``: of another group than ``s``'s first row) and asks for its k best (``k <= 128``).  Per pair
        ``(s, t)`` the best window counts, by score descending and then the smallest window; the k best pairs are ordered by
        (score descending, ``s``, ``t``).  This is exact: a pair among the k best has fewer than k better sequences in its best
        window's list, so it is in that list.

        Window theorem (held in tests/test_repeats_ref.py).  If the best local alignment of the WHOLE sequence ``s`` against
        ``t`` covers at most ``window - hop + 1`` rows of ``s``, some window contains it and ``find_repeats`` returns it bit for
        bit, score and both spans; otherwise it returns a score that is never larger (fp32 addition is monotone: restricting the
        probe to a sub-range of its rows never raises a score, and a path inside the sub-range keeps its bits).

        Nothing depends on ``splits``, ``phrase_chunk`` (the windows per launch), stale workspace contents, one ``add`` against
        many or a ``save`` / ``load`` round trip.  ``ValueError`` before any launch: an empty index, what ``search_repeats``
        refuses, ``window`` / ``hop`` outside ``1 <= hop <= window <= 64``.  Fewer than two sequences: padding only, no launch.

        Not here: more than one repeat per pair of sequences and repeats inside one sequence (both: ``local_align_sequences`` on
        the pairs this returns), the 16-bit / PQ / IVF forms, scores normalised by length."""
        N, dev = len(self), self.device
        if N == 0:
            raise ValueError("the index is empty")
        k = _check_k_refine(k)[0]
        local = _local_scalars(radius, gap, min_score)
        for name, v in (("window", window), ("hop", hop)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError("%s must be an integer, got %r" % (name, v))
        window, hop = int(window), int(hop)
        if not 1 <= hop <= window <= MAX_PHRASE_ROWS:
            raise ValueError("need 1 <= hop <= window <= %d, got hop = %d, window = %d" % (MAX_PHRASE_ROWS, hop, window))
        if int(splits) < 0 or int(phrase_chunk) < 1:
            raise ValueError("splits must be >= 0 and phrase_chunk >= 1")
        off = _sequences(sequences, N, self.sequence_offsets)
        S = int(off.size - 1)
        scores = torch.zeros((k,), dtype=torch.float32, device=dev)
        pairs = torch.full((k, 2), -1, dtype=torch.int64, device=dev)
        spans = torch.full((k, 2, 2), -1, dtype=torch.int64, device=dev)
        if S < 2:
            return scores, pairs, spans
        # the windows, in (sequence, window) order; the last sequence has no t > s and gives none
        lens = np.diff(off)[:-1]
        n_w = np.where(lens <= window, 1, -(-(lens - window) // hop) + 1)
        ws = np.repeat(np.arange(S - 1, dtype=np.int64), n_w)                      # the sequence of every window
        r = np.arange(ws.size, dtype=np.int64) - np.repeat(np.cumsum(n_w) - n_w, n_w)
        wlen = np.minimum(window, lens)[ws]
        wrow = off[ws] + np.minimum(r * hop, np.maximum(lens[ws] - window, 0))     # the first row of every window
        grp = self._g.index_select(0, torch.from_numpy(off[:-1]).to(dev)).cpu().numpy()[ws] if exclude_same_group else None
        found = []
        step = int(phrase_chunk)
        for w0 in range(0, ws.size, step):
            w1 = min(ws.size, w0 + step)
            wl = wlen[w0:w1]
            rows = np.repeat(wrow[w0:w1], wl) + np.arange(int(wl.sum())) - np.repeat(np.cumsum(wl) - wl, wl)
            probes = self._x.index_select(0, torch.from_numpy(rows).to(dev))
            sc, sq, sp = self.search_repeats(probes, k, local[0], gap=local[1], min_score=local[2], lengths=wl,
                                             groups=None if grp is None else grp[w0:w1], exclude_same_group=exclude_same_group,
                                             sequences=off, splits=splits, phrase_chunk=step, _workspace_fill=_workspace_fill,
                                             _after_seq=ws[w0:w1])
            hit = (sq >= 0).nonzero()                                              # [n, 2]: (window of the chunk, rank), windows ascending
            if hit.shape[0] == 0:
                continue
            wi, ri = hit[:, 0], hit[:, 1]
            s_d = torch.from_numpy(ws[w0:w1]).to(dev).index_select(0, wi)
            sp = sp[wi, ri]
            sp[:, 0] += torch.from_numpy(wrow[w0:w1]).to(dev).index_select(0, wi)[:, None]
            found.append((sc[wi, ri], s_d, sq[wi, ri], sp))
        if not found:
            return scores, pairs, spans
        sc, s_d, t_d, sp = (torch.cat(a) for a in zip(*found))
        # entries are in window order: a stable sort by score, then by pair, leaves each pair's best window (the smallest on ties) first
        o = torch.sort(sc, descending=True, stable=True).indices
        o = o.index_select(0, torch.sort((s_d * S + t_d).index_select(0, o), stable=True).indices)
        key = (s_d * S + t_d).index_select(0, o)
        first = torch.ones_like(key, dtype=torch.bool)
        first[1:] = key[1:] != key[:-1]
        o = o[first]                                                               # one entry per pair, pairs ascending by (s, t)
        o = o.index_select(0, torch.sort(sc.index_select(0, o), descending=True, stable=True).indices[:k])
        n = int(o.shape[0])
        scores[:n], spans[:n] = sc.index_select(0, o), sp.index_select(0, o)
        pairs[:n, 0], pairs[:n, 1] = s_d.index_select(0, o), t_d.index_select(0, o)
        return scores, pairs, spans

    # ---- the stages that the scanning phrase searches hand to _index.py's _scan_phrases ------------------------------------------------
    def _scan_phrases(self, stages, *args):
        return _scan_phrases(len(self), self.dim, self.device, self.metric, self._g, self.sequence_offsets, stages, *args)

    def _scan_local(self):
        """the only stage of ``search_repeats``: ``sylber_dtw_local``, whose lists are laid out as ``sylber_dtw_search``'s"""
        def scan(c):
            b = c.b
            ws = c.workspace(c.lib.sylber_dtw_workspace_bytes(b.nb, b.Pc, c.k, b.C))
            radius, gap, min_score = (float(v) for v in c.local)
            _lib.check(c.lib.sylber_dtw_local(_vp(b.qp), b.nb, _vp(c.meta_d), _vp(c.sp_d), _vp(c.br_d), b.Pc, b.slots, _vp(self._x), c.N, c.dim,
                                              _vp(self._c), c.metric, c.k, radius, gap, min_score, _vp(c.seq_id), _vp(c.cut_d), b.C,
                                              _vp(c.pg_d), _vp(c.seq_grp), _vp(c.after_d), _vp(c.costs), _vp(c.seqs), _vp(c.spans), _vp(ws),
                                              c.st), "sylber_dtw_local")
        return scan

    def _scan32(self, entry: str):
        """stage 1 on the fp32 rows, the only stage: ``sylber_dtw_search`` or ``sylber_dtw_occurrences``, which take the same arguments"""
        def scan(c):
            b = c.b
            ws = c.workspace(c.lib.sylber_dtw_workspace_bytes(b.nb, b.Pc, c.k, b.C))
            _lib.check(getattr(c.lib, entry)(_vp(b.qp), b.nb, _vp(c.meta_d), _vp(c.sp_d), _vp(c.br_d), b.Pc, b.slots, _vp(self._x), c.N, c.dim,
                                             _vp(self._c), c.metric, c.k, _vp(c.seq_id), _vp(c.cut_d), b.C, _vp(c.pg_d), _vp(c.seq_grp),
                                             _vp(c.costs), _vp(c.seqs), _vp(c.spans), _vp(ws), c.st), entry)
        return scan

    def _scan16(self, storage: str):
        """stage 1 of the two-stage searches: ``sylber_dtw16_scan`` on ``half_rows(storage)``, which may refuse"""
        x16, code = self.half_rows(storage), STORAGES[storage][0]

        def scan(c):
            b = c.b
            c.ws = c.workspace(c.lib.sylber_dtw16_workspace_bytes(b.Pc, c.m, b.C))
            _lib.check(c.lib.sylber_dtw16_scan(_vp(c.q16), b.nb, _vp(c.meta_d), _vp(c.sp_d), _vp(c.br_d), b.Pc, b.slots, _vp(x16), c.N, c.dim,
                                               _vp(self._c), _vp(c.qn), c.metric, code, c.m, _vp(c.seq_id), _vp(c.cut_d), b.C, _vp(c.pg_d),
                                               _vp(c.seq_grp), _vp(c.cand), _vp(c.coarse), _vp(c.ws), c.st), "sylber_dtw16_scan")
        return scan

    # ---- persistence ----------------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """``.npz`` with the stored rows, groups, provenance and metric (cosine rows are saved normalised; loading does not
        normalise them again, so a round trip gives the same results bit for bit)"""
        np.savez(path, **self._saved())

    def _saved(self) -> dict:
        return _base_arrays(self.metric, self.dim, self._x, self._g, self._prov, self._span_dtype)

    @classmethod
    def load(cls, path: str, device="cuda") -> "SyllableIndex":
        return cls._from_saved(np.load(path, allow_pickle=False), device)

    @classmethod
    def _from_saved(cls, z, device) -> "SyllableIndex":
        """the index of a saved file's ``_base_arrays``, rows as saved: cosine rows are not normalised a second time"""
        idx = cls(metric=str(z["metric"]), device=device)
        x = z["features"]
        if x.shape[0]:
            xd = _rows_of_width(_on_device(x, np.float32, idx.device), None, "features")
            idx.dim, idx._x, idx._c = xd.shape[1], xd, (_row_norms(xd) if idx.metric == "l2" else None)
            idx._g = _on_device(z["groups"], np.int32, idx.device)
            idx._prov = np.asarray(z["provenance"], np.float64).reshape(len(idx), 4)
        if bool(z["span_int"]):
            idx._span_dtype = np.int64
        return idx


class IVFSyllableIndex:
    """An inverted file over a ``SyllableIndex``: the rows are clustered into ``nlist`` lists once (``fit_kmeans``), and a search scans,
    per query, only the ``nprobe`` lists whose centroids are nearest (csrc/knn.hip, ``sylber_ivf_search``).  The result is the exact
    search's restricted to the rows of the probed lists, bit for bit (tests/ivf_ref.py restates the composition)::

        list of row j      = sylber_kmeans_assign(rows, centroids)[j]      (squared L2 for both metrics; unit rows for "cosine";
                                                                            a row with NaN is in no list)
        lists of query i   = the ids of SyllableIndex(centroids, metric="l2").search(q_i, nprobe)
        result of query i  = SyllableIndex.search's order (s, original id), reported values, exclusion and padding over those rows

    Build one with ``IVFSyllableIndex.build``.  ``ivf.index`` is the source ``SyllableIndex`` (rows in id order; ``add`` appends to
    it); the lists hold a second copy of the rows, laid out list by list."""

    def __init__(self, index: SyllableIndex, centroids: torch.Tensor, labels: torch.Tensor):
        self.index = index
        self.centroids = centroids
        self._coarse = SyllableIndex(centroids, metric="l2", device=index.device)
        self._labels = labels                   # [N] int32 on the device, -1 = in no list
        self.last_search = None
        self._layout()

    # ---- building -------------------------------------------------------------------------------------------------------------------
    @classmethod
    def build(cls, source, nlist: Optional[int] = None, *, centroids=None, seed: int = 0, max_iter: int = 25,
              train_rows: Optional[int] = None, tol: float = 1e-4, groups=None, metric: str = "l2", device="cuda") -> "IVFSyllableIndex":
        """``source``: a ``SyllableIndex`` (kept as ``ivf.index``, not copied) or ``[N, D]`` features (then ``groups``, ``metric`` and
        ``device`` make the index).  The centroids are ``fit_kmeans(rows, nlist, seed=, max_iter=, tol=, init_rows=train_rows)`` on the
        stored rows, or ``centroids [nlist, D]`` as given (finite).  ``ValueError`` for ``nlist < 1``, ``nlist > N`` or an empty index."""
        index = source if isinstance(source, SyllableIndex) else SyllableIndex(source, metric=metric, groups=groups, device=device)
        C = cls._train_centroids(index, nlist, centroids, seed, max_iter, tol, train_rows)
        return cls(index, C, cls._assign(index._x, C))

    @staticmethod
    def _train_centroids(index: SyllableIndex, nlist, centroids, seed: int, max_iter: int, tol: float, train_rows) -> torch.Tensor:
        """``[nlist, D]`` fp32 on the index's device: ``centroids`` as given (finite), or ``fit_kmeans`` on the stored rows"""
        from .kmeans import fit_kmeans
        N = len(index)
        if N == 0:
            raise ValueError("the index is empty")
        if centroids is None:
            if nlist is None or isinstance(nlist, bool) or int(nlist) != nlist or nlist < 1:
                raise ValueError("nlist must be an integer >= 1, got %r" % (nlist,))
            if nlist > N:
                raise ValueError("nlist = %d > %d rows" % (nlist, N))
            C = fit_kmeans(index._x, int(nlist), seed=seed, max_iter=max_iter, tol=tol, init_rows=train_rows, device=index.device).centroids
        else:
            c = _rows(centroids, "centroids")
            if nlist is not None and c.shape[0] != nlist:
                raise ValueError("centroids has %d rows, nlist = %r" % (c.shape[0], nlist))
            if c.shape[0] < 1 or c.shape[0] > N:
                raise ValueError("nlist = %d must be in [1, %d rows]" % (c.shape[0], N))
            if c.shape[1] != index.dim:
                raise ValueError("centroids: expected D = %d, got %d" % (index.dim, c.shape[1]))
            C = c.to(index.device, torch.float32).contiguous().clone()
            if not bool(torch.isfinite(C).all()):
                raise ValueError("centroids hold non-finite values")
        return C

    @staticmethod
    def _assign(x: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
        from .kmeans import assign
        lab = assign(x, C)[0]
        return torch.where((lab >= 0) & (lab < C.shape[0]), lab, torch.full_like(lab, -1))      # a NaN row has no nearest centroid

    def _layout(self) -> None:
        """the counting sort of the rows into lists (plumbing): positions, offsets and the list-ordered copies"""
        idx, nlist = self.index, self.nlist
        order, self.list_sizes, off = _list_layout(self._labels, nlist)
        off = np.append(off.cpu().numpy(), 0)
        off[nlist + 1] = off[nlist]                                      # a virtual empty list for probe slots without a list
        order = order[:int(off[nlist])]                                  # the rows in no list are not laid out
        self._off_host = off.astype(np.int32)
        self._rid = order.to(torch.int32)
        self._rows = idx._x.index_select(0, order)
        self._rc = idx._c.index_select(0, order) if idx._c is not None else None
        self._rg = idx._g.index_select(0, order)
        self._sizes_host = np.diff(off[:nlist + 1])

    def add(self, features, groups=None) -> range:
        """append rows to ``ivf.index``, assign them to the existing centroids (no retraining) and re-lay the lists out; the result
        equals ``build`` from all the rows with ``centroids=`` these"""
        ids = self.index.add(features, groups=groups)
        if len(ids):
            self._labels = torch.cat([self._labels, self._assign(self.index._x[ids.start:ids.stop], self.centroids)])
            self._layout()
        return ids

    # ---- views ----------------------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return len(self.index)

    @property
    def nlist(self) -> int:
        return int(self.centroids.shape[0])

    @property
    def metric(self) -> str:
        return self.index.metric

    @property
    def labels(self) -> torch.Tensor:
        """``[N]`` int64: the list of every row (-1 for a row in no list)"""
        return self._labels.to(torch.int64)

    def list_ids(self, l: int) -> torch.Tensor:
        """the row ids of list ``l``, ascending"""
        return self._rid[int(self._off_host[l]):int(self._off_host[l + 1])].to(torch.int64)

    def provenance(self, ids):
        return self.index.provenance(ids)

    # ---- search ---------------------------------------------------------------------------------------------------------------------
    def probe(self, queries, nprobe: int) -> torch.Tensor:
        """``[n, nprobe]`` int64: the lists a search of these queries scans, nearest centroid first (-1 where a query is NaN)"""
        nprobe = _check_nprobe(nprobe, self.nlist)
        return self._coarse.search(self.index._prep(_rows_of_width(queries, self.index.dim, "queries")), nprobe)[1]

    def search(self, queries, k: int, nprobe: int, *, groups=None, exclude_same_group: bool = False,
               query_chunk: int = DEFAULT_QUERY_CHUNK, item_tiles: int = 0, _workspace_fill=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """as ``SyllableIndex.search`` over the rows of each query's ``nprobe`` nearest lists -> ``(scores fp32 [n, k], ids int64
        [n, k])`` on the device, ids those of ``ivf.index``.  ``query_chunk`` bounds the workspace and the pair tables;
        ``item_tiles`` (0 = automatic) is a test hook that cuts lists into work items of that many 128-row tiles.  Neither changes
        the result.  ``ivf.last_search`` = ``{"pairs", "fraction", "items", "workspace_bytes"}`` of the call."""
        idx = self.index
        k = _check_k_refine(k)[0]
        nprobe = _check_nprobe(nprobe, self.nlist)
        if len(idx) == 0:
            raise ValueError("the index is empty")
        q = _rows_of_width(queries, idx.dim, "queries")
        n, D = q.shape
        qg = _query_groups(groups, n, exclude_same_group, idx.device)
        item_tiles, query_chunk = _check_splits_chunk(item_tiles, query_chunk, "item_tiles")
        dev = idx.device
        scores, ids = _outputs(n, k, dev)
        self.last_search = {"pairs": 0, "fraction": 0.0, "items": 0, "workspace_bytes": 0}
        if n == 0:
            return scores, ids
        lib = _lib.load()
        qd = idx._prep(q)
        nlist = self.nlist
        step = min(n, query_chunk, max(1, 2 ** 25 // nprobe))     # n x nprobe x cuts (<= 16) stays below 2^30
        metric = METRICS[idx.metric]
        i32p = ctypes.POINTER(ctypes.c_int32)
        off_p = self._off_host.ctypes.data_as(i32p)
        pairs_scanned = 0
        with torch.cuda.device(dev):
            for r0 in range(0, n, step):
                m = min(step, n - r0)
                qc = qd[r0:r0 + m]
                # the coarse step and the grouping of the (query, slot) pairs by list: plumbing
                probe = self._coarse.search(qc, nprobe)[1].reshape(-1)
                key = torch.where(probe < 0, torch.full_like(probe, nlist), probe)
                pair = torch.sort(key, stable=True).indices.to(torch.int32)
                counts = np.ascontiguousarray(torch.bincount(key, minlength=nlist + 1).cpu().numpy().astype(np.int32))
                cnt_p = counts.ctypes.data_as(i32p)
                cuts = ctypes.c_int32(0)
                W = int(lib.sylber_ivf_work_items(cnt_p, off_p, nlist + 1, item_tiles, None, 0, ctypes.byref(cuts)))
                items = np.empty((max(W, 1), 8), np.int32)
                if W < 1 or int(lib.sylber_ivf_work_items(cnt_p, off_p, nlist + 1, item_tiles, items.ctypes.data_as(i32p), W,
                                                          ctypes.byref(cuts))) != W:
                    raise _lib.SylberHipError("sylber_ivf_work_items failed")
                items_d = torch.from_numpy(items).to(dev)
                nbytes = int(lib.sylber_ivf_workspace_bytes(m, nprobe, k, cuts.value))
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                if _workspace_fill is not None:
                    ws.fill_(_workspace_fill)
                _lib.check(lib.sylber_ivf_search(_vp(qc), m, D, nprobe, _vp(pair), _vp(items_d), W, cuts.value, _vp(self._rows), _vp(self._rid),
                                                 _vp(self._rc), metric, k, _vp(qg[r0:r0 + m] if qg is not None else None),
                                                 _vp(self._rg if qg is not None else None), _vp(scores[r0:r0 + m]), _vp(ids[r0:r0 + m]),
                                                 _vp(ws), _stream(dev)), "sylber_ivf_search")
                pairs_scanned += int((counts[:nlist].astype(np.int64) * self._sizes_host).sum())
                self.last_search["items"] += W
                self.last_search["workspace_bytes"] = max(self.last_search["workspace_bytes"], nbytes + pair.numel() * 4 + items.nbytes)
        self.last_search["pairs"] = pairs_scanned
        self.last_search["fraction"] = pairs_scanned / (float(n) * len(idx))
        return scores, ids

    # ---- phrase search --------------------------------------------------------------------------------------------------------------
    def sequence_offsets(self) -> np.ndarray:
        """int64 ``[S + 1]``: the default sequences of ``search_phrases``, those of ``ivf.index`` (rows in id order, not list order)"""
        return self.index.sequence_offsets()

    def search_phrases(self, phrases, k: int, nprobe: int, seeds: int = 32, refine: int = 4, *, lengths=None, groups=None,
                       exclude_same_group: bool = False, sequences=None, query_chunk: int = DEFAULT_QUERY_CHUNK,
                       phrase_chunk: int = DEFAULT_PHRASE_CHUNK, item_tiles: int = 0, return_candidates: bool = False,
                       _workspace_fill=None):
        """phrase search without a scan of the corpus: seed, vote, exact re-rank -> ``(costs, seqs, spans)`` as
        ``SyllableIndex.search_phrases`` returns them (plus ``cand`` int64 ``[P, m]`` and ``bound`` fp32 ``[P, m]`` with
        ``return_candidates=True``).  The lists are in list order, which breaks a DTW scan over them; they are used only to find
        candidate sequences, and the DTW runs on ``ivf.index``, whose rows are still in id order.

        Stage 1a: ``ivf.search(all phrase rows, k=seeds, nprobe)``: each row's ``seeds`` nearest rows among its ``nprobe`` nearest
        lists.  With ``exclude_same_group`` and the default sequences every row carries its phrase's group, so that no seed is spent
        on the phrase's own clip; with explicit ``sequences=`` stage 1a excludes nothing and the vote drops the excluded sequences.
        Stages 1b and 2: ``ivf.index.search_phrases_seeded`` on those seeds with ``m = k * refine`` candidates, which has the
        contract of the vote and of the result: ``search_phrases`` restricted to the candidates, every cost and span bit for bit a
        ``search_phrases`` cost and span.

        What the parameters trade: ``nprobe`` the share of the lists each row scans (stage 1a's time; a matching row in a list that
        is not probed cannot be a seed); ``seeds`` how many sequences a row can vote for and how tight its floor is (the vote's LDS
        and sort grow with it); ``refine`` how many candidates the exact DTW scores per returned sequence (stage 2's time).  Under the
        default sequences with ``nprobe == nlist``, ``bound[p, r] <= cost(p, cand[p, r])`` exactly; if also ``seeds`` is at least the
        number of admissible rows and m at least the number of admissible sequences, the result *is* ``search_phrases``, bit for
        bit.  Nothing returned depends on ``query_chunk``, ``phrase_chunk``, ``item_tiles``, stale workspaces, ``build`` versus
        ``build`` + ``add`` or a ``save`` / ``load`` round trip.  ``ivf.last_search`` keeps stage 1a's numbers and ``"seen"``: the
        mean number of seen sequences per phrase.  ``1 <= seeds <= 128``, ``k * refine <= 128``."""
        q, lens, sc, si = self._phrase_seeds(phrases, k, nprobe, seeds, refine, lengths, groups, exclude_same_group, sequences, query_chunk,
                                             phrase_chunk, item_tiles, _workspace_fill)
        return self.index.search_phrases_seeded(q, sc, si, k, refine, lengths=lens, groups=groups, exclude_same_group=exclude_same_group,
                                                sequences=sequences, phrase_chunk=phrase_chunk, return_candidates=return_candidates,
                                                _trusted_ids=True)

    def search_occurrences(self, phrases, k: int, nprobe: int, seeds: int = 32, refine: int = 4, *, lengths=None, groups=None,
                           exclude_same_group: bool = False, sequences=None, query_chunk: int = DEFAULT_QUERY_CHUNK,
                           phrase_chunk: int = DEFAULT_PHRASE_CHUNK, item_tiles: int = 0, return_candidates: bool = False,
                           _workspace_fill=None):
        """every non-overlapping occurrence of each phrase without a scan of the corpus -> ``(costs, seqs, spans)`` as
        ``SyllableIndex.search_occurrences`` returns them (plus ``cand`` and ``bound`` with ``return_candidates=True``).  The
        arguments are ``search_phrases``'s.  Stage 1a is ``search_phrases``'s, unchanged (``ivf.search`` on all phrase rows; it sets
        ``ivf.last_search`` and its ``"seen"`` as there); stages 1b and 2 are ``ivf.index.search_occurrences_seeded``: the vote
        for ``m = k * refine`` candidate sequences, then every occurrence in them by the exact fp32 recurrence.

        So ``cand`` and ``bound`` are ``search_phrases``'s, bit for bit, and the result is ``ivf.index.search_occurrences`` restricted
        to the sequences of ``cand``; with ``nprobe == nlist``, ``seeds`` at least the number of admissible rows and m at least the
        number of admissible sequences it *is* ``ivf.index.search_occurrences``.  Stage 1 ranks a sequence by its best match: a
        sequence whose many occurrences are all mediocre can be left out.  Nothing returned depends on ``query_chunk``,
        ``phrase_chunk``, ``item_tiles``, stale workspaces, ``build`` versus ``build`` + ``add`` or a ``save`` / ``load`` round trip."""
        q, lens, sc, si = self._phrase_seeds(phrases, k, nprobe, seeds, refine, lengths, groups, exclude_same_group, sequences, query_chunk,
                                             phrase_chunk, item_tiles, _workspace_fill)
        return self.index.search_occurrences_seeded(q, sc, si, k, refine, lengths=lens, groups=groups, exclude_same_group=exclude_same_group,
                                                    sequences=sequences, phrase_chunk=phrase_chunk, return_candidates=return_candidates,
                                                    _trusted_ids=True, _workspace_fill=_workspace_fill)

    def _phrase_seeds(self, phrases, k, nprobe, seeds, refine, lengths, groups, exclude_same_group, sequences, query_chunk, phrase_chunk,
                      item_tiles, fill):
        """the checks and stage 1a of ``search_phrases`` / ``search_occurrences`` -> ``(phrase rows, lengths, seed scores, seed ids)``;
        sets ``last_search``"""
        idx = self.index
        k, m = _check_k_refine(k, refine, rerank=True)
        nprobe = _check_nprobe(nprobe, self.nlist)
        if isinstance(seeds, bool) or int(seeds) != seeds or not 1 <= int(seeds) <= MAX_SEEDS:
            raise ValueError("seeds must be an integer in [1, %d], got %r" % (MAX_SEEDS, seeds))
        seeds = int(seeds)
        q, lens, pg, off = _phrase_args(len(idx), idx.dim, idx.device, idx.sequence_offsets, phrases, lengths, groups, exclude_same_group,
                                        sequences, 0, phrase_chunk, 0)
        _check_splits_chunk(item_tiles, query_chunk, "item_tiles")
        dev = idx.device
        P = int(lens.size)
        if P == 0:
            self.last_search = {"pairs": 0, "fraction": 0.0, "items": 0, "workspace_bytes": 0, "seen": 0.0}
            sc = torch.empty((0, seeds), dtype=torch.float32, device=dev)
            si = torch.empty((0, seeds), dtype=torch.int64, device=dev)
        else:
            own = pg is not None and sequences is None         # the rows' groups decide the default sequences: exclude in stage 1a
            sc, si = self.search(q, seeds, nprobe, groups=np.repeat(pg, lens) if own else None, exclude_same_group=own,
                                 query_chunk=query_chunk, item_tiles=item_tiles, _workspace_fill=fill)
            # the seen sequences of each phrase, counted as the vote sees them
            d = sc if idx.metric == "l2" else torch.clamp_min(1.0 - sc, 0.0)
            valid = (si >= 0) & ~torch.isnan(sc) & ~torch.isposinf(d)
            seq = torch.bucketize(si, torch.from_numpy(off[1:]).to(dev), right=True)
            owner = torch.repeat_interleave(torch.arange(P, device=dev), torch.from_numpy(lens).to(dev))
            pairs = (owner[:, None] * (off.size - 1) + seq)[valid]
            self.last_search["seen"] = float(torch.unique(pairs).numel()) / P
        return q, lens, sc, si

    def align_phrases(self, phrases, spans, lengths=None, pair_chunk: Optional[int] = None):
        """the warping paths behind the spans of ``search_phrases`` or ``search_occurrences``: ``ivf.index.align_phrases``, whose rows
        (in id order) are the ones the exact re-rank ran on -> ``(rows, steps, costs)`` as there"""
        return self.index.align_phrases(phrases, spans, lengths=lengths, pair_chunk=pair_chunk)

    def align_sequences(self, pairs, *, path: bool = False, pair_chunk: Optional[int] = None, sequences=None, split=None):
        """the global DTW of whole stored sequences: ``ivf.index.align_sequences`` on the rows in id order"""
        return self.index.align_sequences(pairs, path=path, pair_chunk=pair_chunk, sequences=sequences, split=split)

    def local_align_sequences(self, pairs, radius, *, gap=None, min_score=None, n_best: int = 1, min_sep: int = 1,
                              pair_chunk: Optional[int] = None, sequences=None):
        """every repeat between whole stored sequences: ``ivf.index.local_align_sequences`` on the rows in id order"""
        return self.index.local_align_sequences(pairs, radius, gap=gap, min_score=min_score, n_best=n_best, min_sep=min_sep,
                                                pair_chunk=pair_chunk, sequences=sequences)

    # ---- persistence ----------------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """``.npz``: the source index's rows, groups, provenance and metric, the centroids and every row's list.  Loading neither
        retrains nor reassigns, so a round trip searches bit for bit the same."""
        np.savez(path, **self.index._saved(), centroids=self.centroids.cpu().numpy(), labels=self._labels.cpu().numpy())

    @classmethod
    def load(cls, path: str, device="cuda") -> "IVFSyllableIndex":
        z = np.load(path, allow_pickle=False)
        if "centroids" not in z.files or "labels" not in z.files:
            raise ValueError("%s is not a saved IVFSyllableIndex" % path)
        idx = SyllableIndex._from_saved(z, device)
        C = _on_device(z["centroids"], np.float32, idx.device)
        labels = _on_device(z["labels"], np.int32, idx.device)
        if labels.shape != (len(idx),) or C.dim() != 2 or C.shape[1] != idx.dim:
            raise ValueError("%s: centroids / labels do not match the rows" % path)
        return cls(idx, C, labels)

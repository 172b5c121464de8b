"""``UnitIndex``: a device-resident corpus of syllable *unit ids* -- what ``SegmentSynthesis.tokenize`` returns -- searched by
semi-global edit distance (csrc/unit_search.hip; contract in include/sylber_hip.h "Unit search", restated in
tests/unit_search_ref.py).  The four syllable indexes (search.py, pq.py) need every syllable's embedding; this one needs ``4 W``
bytes per syllable (``W`` codebooks) and answers "where is this word said?" for a corpus kept as tokens, for a unit language
model's output and for a lexicon written as unit strings.  ``align_phrases`` takes the spans of either search, or any windows,
and returns the edit script of each match: the stored row every phrase unit is paired with and the equal / substituted / deleted /
inserted counts (csrc/unit_align.hip, "Edit scripts", tests/unit_align_ref.py); in global mode that is the weighted Levenshtein
distance of two unit strings, for a phrase of at most 64 units.  ``align_unit_strings`` and ``unit_error_rate`` align WHOLE unit
strings of any length up to 65 536 units, pair by pair, without an index (csrc/unit_strings.hip, "Unit strings",
tests/unit_strings_ref.py): how far two tokenisations of the same audio are from each other.  ``local_align_unit_strings`` and
``UnitIndex.find_repeats`` need no query: the local alignment of two unit strings, i.e. the phrase that both recordings hold, pair
by pair or over every pair of sequences of an index (csrc/unit_repeats.hip, "Unit repeats", tests/unit_repeats_ref.py);
``local_align_unit_strings_all`` and ``find_repeats(per_pair=, within=)`` return every repeat of a pair and the repeats inside one
string (csrc/unit_repeats_all.hip, "Unit repeats, every one", tests/unit_repeats_all_ref.py).  The argument rules ``UnitIndex``
shares with the syllable indexes are ``_index.py``'s, the span checks of ``align_phrases`` are search.py's."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._index import (DEFAULT_PHRASE_CHUNK, MAX_PHRASE_ROWS, _check_k_refine, _group_runs, _groups, _provenance, _query_groups,
                     _sequence_tables, _sequences)
from .kmeans import _device, _stream, _vp
from .search import ALIGN_WORKSPACE_BYTES, _align_spans       # the span checks and the workspace bound of every align_phrases

TILE_COLS = 256                 # US_TILE of csrc/unit_search.hip: the columns a workgroup stages at a time
ALIGN_CHUNK_COLS = 32           # UA_CH of csrc/unit_align.hip: the anti-diagonal steps whose 2-bit codes fill one 64-bit word
MAX_WIDTH = 8                   # US_MAX_W: ids per unit
STRING_ROWS = 64                # UST_ROWS of csrc/unit_strip.h: the reference rows of a strip
MAX_STRING_UNITS = 65536        # UST_MAX_LEN: the units of one string of align_unit_strings
MAX_LOCAL_PARAM = 64            # UST_MAX_PARAM: match, mismatch and gap of a local alignment
MAX_BEST = 32                   # ULA_MAX_BEST of csrc/unit_repeats_all.hip: the repeats of one pair
REPEAT_PAIRS = 1 << 16          # the pairs of sequences that find_repeats enumerates on the host at a time
FORMAT = "sylber_amd.UnitIndex/1"
_i32p = ctypes.POINTER(ctypes.c_int32)


def _unit_rows(a, width: Optional[int], what: str) -> torch.Tensor:
    """``[n]`` (one id per unit) or ``[n, W]`` integers, tensor or array on any device -> int64 ``[n, W]`` as given, refusing
    what is not a row of ``width`` ids (``None``: any width in 1 .. 8) in ``0 .. 2**31 - 1``"""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError("%s must be integers, got %s" % (what, t.dtype))
    if t.dim() == 1:
        t = t[:, None]
    if t.dim() != 2:
        raise ValueError("%s must be [n] or [n, W], got %s" % (what, tuple(t.shape)))
    W = t.shape[1]
    if width is None:
        if not 1 <= W <= MAX_WIDTH:
            raise ValueError("%s: the width W must be in [1, %d], got %d" % (what, MAX_WIDTH, W))
    elif W != width:
        raise ValueError("%s: expected W = %d, got %d" % (what, width, W))
    if t.numel():
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi > 2 ** 31 - 1:
            raise ValueError("%s: unit ids lie in [0, 2**31 - 1], got %d .. %d" % (what, lo, hi))
    return t


class UnitIndex:
    """A device-resident corpus of syllable unit strings with exact phrase search by edit distance.

    ``UnitIndex(units=None, *, width=None, groups=None, device="cuda")``.  A *unit* is a row of ``W`` non-negative ids (``W`` =
    ``width``, ``1 <= W <= 8``: 1 for k-means units, 2 for residual units, ``Qa + Qp`` for the learned quantizer), stored int32:
    ``4 W`` bytes per syllable.  ``groups`` (one integer per row, e.g. the clip id) cut the corpus into sequences and drive
    ``exclude_same_group``; rows added without groups get group -1."""

    def __init__(self, units=None, *, width: Optional[int] = None, groups=None, device="cuda"):
        if width is not None and (isinstance(width, bool) or int(width) != width or not 1 <= int(width) <= MAX_WIDTH):
            raise ValueError("width must be an integer in [1, %d], got %r" % (MAX_WIDTH, width))
        self.device = _device(device)
        self.width: Optional[int] = None if width is None else int(width)
        self._u = None              # [N, W] int32 on the device
        self._g = None              # [N] int32 groups on the device
        self._prov = None           # [N, 4] provenance (clip, segment, start, end)
        self._span_dtype = np.float64
        self._seq_cache = None      # (N, default sequence offsets)
        if units is not None:
            self.add(units, groups=groups)

    def __len__(self) -> int:
        return 0 if self._u is None else int(self._u.shape[0])

    @property
    def units(self) -> torch.Tensor:
        """the stored ``[N, W]`` int32 ids"""
        return self._u

    @property
    def nbytes(self) -> int:
        """device bytes of the corpus: ``4 W`` per syllable of ids and 4 of group"""
        return 0 if self._u is None else int(self._u.numel() * 4 + self._g.numel() * 4)

    # ---- building -------------------------------------------------------------------------------------------------------------------
    def add(self, units, groups=None, *, _prov=None) -> range:
        """append ``[n]`` or ``[n, W]`` integer ids (tensor or array, host or device) with optional ``groups [n]``; returns their
        row ids.  ``ValueError`` before anything is stored for an id outside ``0 .. 2**31 - 1`` or another width."""
        t = _unit_rows(units, self.width, "units")
        n, start = t.shape[0], len(self)
        g = _groups(groups, n, "groups") if groups is not None else np.full(n, -1, np.int32)
        if start + n >= 2 ** 31:
            raise ValueError("a UnitIndex holds fewer than 2^31 rows")
        if self.width is None:
            self.width = int(t.shape[1])
        if n == 0:
            return range(start, start)
        ud = t.to(self.device, torch.int32).contiguous()
        gd = torch.from_numpy(g).to(self.device)
        prov = np.full((n, 4), -1.0) if _prov is None else np.asarray(_prov, np.float64).reshape(n, 4)
        if self._u is None:
            self._u, self._g, self._prov = ud, gd, prov
        else:
            self._u, self._g, self._prov = torch.cat([self._u, ud]), torch.cat([self._g, gd]), np.concatenate([self._prov, prov])
        return range(start, start + n)

    @classmethod
    def from_tokens(cls, toks: Sequence[dict], *, device="cuda") -> "UnitIndex":
        """an index over the list ``SegmentSynthesis.tokenize`` returns: each clip's ``units``, one group per clip (its position in
        ``toks``), with provenance ``(clip, segment, start frame, end frame)`` from the clip's ``segments``"""
        idx = cls(device=device)
        for ci, o in enumerate(toks):
            u, segs = np.asarray(o["units"]), np.asarray(o["segments"])
            if u.size == 0:
                continue
            if u.ndim == 1:
                u = u[:, None]
            if u.ndim != 2 or segs.shape != (u.shape[0], 2):
                raise ValueError("clip %d: units %s and segments %s do not match" % (ci, u.shape, segs.shape))
            n = u.shape[0]
            prov = np.column_stack([np.full(n, ci), np.arange(n), segs[:, 0], segs[:, 1]]).astype(np.float64)
            idx.add(u, groups=np.full(n, ci, np.int32), _prov=prov)
            if np.issubdtype(segs.dtype, np.integer):
                idx._span_dtype = np.int64
        return idx

    def provenance(self, ids) -> List[Optional[Tuple[int, int, object, object]]]:
        """``(clip, segment, start, end)`` for each id of a flat sequence or array of row ids (``None`` for -1 and for rows added
        without provenance); a span ``(a, b)`` of a search covers ``provenance(range(a, b))``"""
        return _provenance(self._prov, self._span_dtype, len(self), ids)

    def sequence_offsets(self) -> np.ndarray:
        """int64 ``[S + 1]``: the default sequences of the searches, sequence ``s`` = rows ``offsets[s] : offsets[s + 1]``: the
        maximal runs of consecutive rows with equal group, numbered in row order (``from_tokens``: one per non-empty clip)"""
        N = len(self)
        if self._seq_cache is None or self._seq_cache[0] != N:
            self._seq_cache = (N, _group_runs(self._g, N))
        return self._seq_cache[1].copy()

    # ---- search ---------------------------------------------------------------------------------------------------------------------
    def search_phrases(self, phrases, k: int, *, lengths=None, groups=None, exclude_same_group: bool = False, sequences=None,
                       max_cost=None, splits: int = 0, phrase_chunk: int = DEFAULT_PHRASE_CHUNK,
                       _workspace_fill=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """the k best sequences of the index for each phrase of units, by semi-global edit distance (Sellers' approximate string
        matching) -> ``(costs int32 [P, k], seqs int64 [P, k], spans int64 [P, k, 2])`` on the device; a span is (first row id, one
        past the last row id) of the match, so ``provenance`` works on it.  At most one match per sequence: its best one.
        ``phrases``: a list of ``[m_p]`` / ``[m_p, W]`` integer arrays or tensors, or one packed ``[sum m_p]`` / ``[sum m_p, W]``
        array with ``lengths=[m_0, m_1, ...]``; ``1 <= m_p <= 64``.

        Sequences, ``groups [P]`` / ``exclude_same_group`` (a sequence's group is its first row's) and ``sequences=`` follow
        ``SyllableIndex.search_phrases``; a sequence has at most 65 536 rows.

        For phrase unit ``p_i`` and sequence unit ``t_j`` (columns ``0 .. L - 1``), all in int32::

            sub(i, j) = number of columns c with p_i[c] != t_j[c]  (0 .. W);   an insertion or a deletion costs W
            E[-1][j] = 0,           start[-1][j] = j + 1           (j = -1 .. L - 1: the phrase may begin anywhere)
            E[i][-1] = (i + 1) W,   start[i][-1] = 0
            E[i][j]  = min(E[i-1][j-1] + sub(i, j), E[i-1][j] + W, E[i][j-1] + W)
                       on equal values the predecessor is taken in that order: diagonal, then (i-1, j), then (i, j-1);
                       start[i][j] = start of the predecessor taken

        A column of the last row is *admissible* when ``E[m-1][j] <= thr``, ``thr = min(max_cost, m W - 1)``; ``max_cost`` is
        ``None`` (``m W - 1``: anything cheaper than deleting the whole phrase), an int, or ``[P]``; 0 keeps exact matches only.
        An admissible column has a path with a diagonal step, so its span is never empty.  Per (phrase, sequence):
        ``cost = min_j E[m-1][j]`` over the admissible columns, ``end`` = the smallest such j, ``start = start[m-1][end]``; a
        sequence without an admissible column is not returned.  Each phrase's list is ordered by (cost, sequence number)
        ascending; lists with fewer than k sequences end in cost ``2**31 - 1``, sequence -1, span (-1, -1).

        Costs are small integers, so the result is exact and unique: it does not depend on ``splits`` (0 = automatic: the cuts of
        the corpus, on sequence starts only), ``phrase_chunk`` (the phrases per launch), stale workspace contents or one ``add``
        against many.  ``m > L`` is legal.  The scan evaluates every cell; a bit-parallel (Myers) pre-scan that skips sequences
        without an admissible column is the known next step."""
        return self._search("sylber_unit_search", phrases, k, lengths, groups, exclude_same_group, sequences, max_cost, splits,
                            phrase_chunk, _workspace_fill)

    def search_occurrences(self, phrases, k: int, *, lengths=None, groups=None, exclude_same_group: bool = False, sequences=None,
                           max_cost=None, splits: int = 0, phrase_chunk: int = DEFAULT_PHRASE_CHUNK,
                           _workspace_fill=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """every non-overlapping occurrence of each phrase, not one match per sequence: the k best occurrences over the whole
        index, shaped and padded as ``search_phrases``'s; a keyword said five times in one recording comes back five times with
        one sequence number.  Arguments, the recurrence, the order on ties, ``start`` and "admissible" are ``search_phrases``'s;
        the three steps are ``SyllableIndex.search_occurrences``' word for word, with "admissible" in place of "finite":

        1. Families: admissible columns of the last row with equal ``start``; ``cost`` = their minimum, ``end`` = the smallest
           such j.  Starts do not decrease with j, so families arrive in order.
        2. One left-to-right pass: the first family becomes pending; a later family that shares a row with the pending one
           competes with it (the cheaper stays, the pending one on equal cost), otherwise the pending one is emitted and the
           later one becomes pending; at the sequence end the pending family is emitted.
        3. Per phrase the k best emitted occurrences by (cost, first row id of the span).

        The best occurrence of a sequence under (cost, start) is ``search_phrases``' (cost, span) of that pair.  Not global
        greedy suppression: of a chain A - B - C with A and C disjoint, both overlapping B, and costs A > B > C only C is
        emitted."""
        return self._search("sylber_unit_occurrences", phrases, k, lengths, groups, exclude_same_group, sequences, max_cost, splits,
                            phrase_chunk, _workspace_fill)

    def _phrases(self, phrases, lengths) -> Tuple[torch.Tensor, np.ndarray]:
        """``(the phrases' units int64 [sum m, W] as given, lengths int64 [P])`` or ``ValueError``"""
        W = self.width
        if lengths is None:
            if torch.is_tensor(phrases) or isinstance(phrases, np.ndarray):
                raise ValueError("phrases given as one packed array need lengths=")
            parts = [_unit_rows(p, W, "phrases[%d]" % i) for i, p in enumerate(phrases)]
            lens = np.array([p.shape[0] for p in parts], np.int64)
            q = torch.cat([p.to(self.device, torch.int64) for p in parts]) if parts else torch.zeros((0, W), dtype=torch.int64)
        else:
            q = _unit_rows(phrases, W, "phrases")
            lens = np.asarray(lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else lengths)
            if lens.ndim != 1 or (lens.size and lens.dtype.kind not in "iu"):
                raise ValueError("lengths must be a 1-D sequence of integers")
            lens = lens.astype(np.int64)
            if int(lens.sum()) != q.shape[0]:
                raise ValueError("lengths sum to %d, phrases has %d units" % (int(lens.sum()), q.shape[0]))
        if lens.size and (lens.min() < 1 or lens.max() > MAX_PHRASE_ROWS):
            raise ValueError("a phrase has between 1 and %d units, got lengths from %d to %d" % (MAX_PHRASE_ROWS, lens.min(), lens.max()))
        return q, lens

    def _thresholds(self, max_cost, lens: np.ndarray) -> np.ndarray:
        """int32 ``[P]``: ``min(max_cost, m W - 1)``"""
        cap = lens * self.width - 1
        if max_cost is None:
            return cap.astype(np.int32)
        a = np.asarray(max_cost.detach().cpu().numpy() if torch.is_tensor(max_cost) else max_cost)
        if a.dtype.kind not in "iu" or a.shape not in ((), (lens.size,)):
            raise ValueError("max_cost must be None, an integer or %d integers, got %r" % (lens.size, max_cost))
        a = np.broadcast_to(a.astype(np.int64), (lens.size,))
        if a.size and a.min() < 0:
            raise ValueError("max_cost must be >= 0, got %d" % a.min())
        return np.minimum(a, cap).astype(np.int32)

    def _search(self, entry: str, phrases, k, lengths, groups, exclude_same_group, sequences, max_cost, splits, phrase_chunk, fill):
        k, _ = _check_k_refine(k)
        N, dev = len(self), self.device
        if N == 0:
            raise ValueError("the index is empty")
        q, lens = self._phrases(phrases, lengths)
        P = int(lens.size)
        pg = _query_groups(groups, P, exclude_same_group, None, "phrases")
        if int(splits) < 0 or int(phrase_chunk) < 1:
            raise ValueError("splits must be >= 0 and phrase_chunk >= 1")
        thr = self._thresholds(max_cost, lens)
        off = _sequences(sequences, N, self.sequence_offsets)
        costs = torch.empty((P, k), dtype=torch.int32, device=dev)
        seqs = torch.empty((P, k), dtype=torch.int64, device=dev)
        spans = torch.empty((P, k, 2), dtype=torch.int64, device=dev)
        if P == 0:
            return costs, seqs, spans
        lib = _lib.load()
        qd = q.to(dev, torch.int32).contiguous()
        seq_id, seq_grp = _sequence_tables(off, self._g if pg is not None else None, dev)
        off32, S = np.ascontiguousarray(off, np.int32), off.size - 1
        rows = np.ascontiguousarray(np.cumsum(lens) - lens, np.int32)
        ln = np.ascontiguousarray(lens, np.int32)
        offp = off32.ctypes.data_as(_i32p)
        with torch.cuda.device(dev):
            st = _stream(dev)
            for p0 in range(0, P, int(phrase_chunk)):
                p1 = min(P, p0 + int(phrase_chunk))
                lp, rp, tp = (np.ascontiguousarray(a[p0:p1]) for a in (ln, rows, thr))
                gp = np.ascontiguousarray(pg[p0:p1], np.int32) if pg is not None else None
                need = int(lib.sylber_unit_workspace_bytes(lp.ctypes.data_as(_i32p), p1 - p0, offp, S, k, int(splits)))
                if need < 0:
                    raise _lib.SylberHipError("sylber_unit_workspace_bytes refused the call")
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
                if fill is not None:
                    ws.fill_(fill)
                _lib.check(getattr(lib, entry)(_vp(qd), qd.shape[0], self.width, rp.ctypes.data_as(_i32p), lp.ctypes.data_as(_i32p),
                                               tp.ctypes.data_as(_i32p), p1 - p0, _vp(self._u), N, offp, S, _vp(seq_id),
                                               gp.ctypes.data_as(_i32p) if gp is not None else None, _vp(seq_grp), int(splits), k,
                                               _vp(costs[p0:p1]), _vp(seqs[p0:p1]), _vp(spans[p0:p1]), _vp(ws), st), entry)
        return costs, seqs, spans

    # ---- edit scripts ---------------------------------------------------------------------------------------------------------------
    def align_phrases(self, phrases, spans, *, lengths=None, free_start: bool = True, pair_chunk: Optional[int] = None,
                      _workspace_fill=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """*how* each phrase matches each of its spans: the edit script -> ``(cols int64 [P, k, Mx], subs int32 [P, k, Mx],
        ops int32 [P, k, 4], costs int32 [P, k])`` on the device, ``Mx = max_p m_p`` (csrc/unit_align.hip, ``sylber_unit_align``;
        contract in include/sylber_hip.h "Edit scripts", restated in tests/unit_align_ref.py).  ``phrases`` and ``lengths=`` are
        exactly as the search took them; ``spans`` int64 ``[P, k, 2]`` (host or device): (first row id, one past the last),
        ``(-1, -1)`` = padding -- the spans of ``search_phrases`` or ``search_occurrences``, or any windows of your own.

        ``cols[p, r, i]``: the row id that phrase unit i is paired with by a diagonal step, so ``provenance`` works on it; -1 if
        the unit is deleted or ``i >= m_p``.  ``subs``: ``sub(i, j)`` of that pairing (0 .. W), W for a deleted unit, -1 for
        ``i >= m_p``.  ``ops``: (equal, substituted, deleted, inserted) = diagonal steps with ``sub = 0``, diagonal steps with
        ``sub > 0``, phrase units without a row, rows of the path without a phrase unit.  ``costs``: ``E[m-1][L-1]``.  A padding
        span gives ``cols`` and ``subs`` -1, ``ops`` 0 and cost ``2**31 - 1``; every legal window has a finite cost.

        Window DP, for one pair (phrase of m units, window ``[a, b)``, ``L = b - a``): ``sub``, the recurrence, the predecessor
        order on ties and the int32 arithmetic are ``search_phrases``'s; the window is taken as **one** sequence whose column 0 is
        row ``a``, even across a sequence boundary of the index; ``E[i][-1] = (i + 1) W``; the end is forced: the path ends in
        cell ``(m-1, L-1)``.  ``free_start=True``: ``E[-1][j] = 0``, the searches' DP -- the phrase may begin anywhere in the
        window.  ``free_start=False`` (global): ``E[-1][j] = (j + 1) W`` with predecessor "left", so the whole window is consumed
        and ``costs`` is the weighted Levenshtein distance of phrase and window: with ``ops`` the unit error rate between two
        tokenisations.  The path is the chain of predecessors from ``(m-1, L-1)`` back to the boundary: to row -1 in column j
        (first row ``a + j + 1``; global: on to the corner, leading insertions, first row ``a``) or to column -1 in row i
        (units ``0 .. i`` are deletions, first row ``a``).

        By construction ``equal + substituted + deleted = m``, the path's first row is ``b - (equal + substituted + inserted)``,
        ``costs = subs[:m].sum() + W * inserted``, and ``ops.sum(-1)`` is the number of edit operations: ``costs / ops.sum(-1)``
        is the length-normalised cost.

        The theorem: if ``[a, b)`` is a span a search of this index returned for that phrase, then in either mode the path's
        first row is ``a``, ``costs`` is the reported cost and the path is the scan's own path (a window cell is a minimum over
        fewer paths, so never below the full DP's; the boundary ``(i + 1) W`` is what deletions from row -1 cost there; on the
        scan's path the two are equal, and a predecessor that lost in the full DP was strictly larger and still is).  Any other
        window is legal and gets what the definition gives.

        Nothing returned depends on ``pair_chunk`` (the pairs per launch; by default the workspace, 16 B per window column and
        pair, stays below 256 MiB), on stale workspace contents, on one ``add`` against many or on a ``save`` / ``load`` round
        trip.  ``ValueError`` before any launch: what ``search_phrases`` refuses of the phrases; ``spans`` of another shape or
        dtype; a span that is neither ``(-1, -1)`` nor ``0 <= a < b <= N`` (one reduction on the device); a window of more than
        65 536 rows; ``pair_chunk < 1``; an empty index."""
        N, dev = len(self), self.device
        if N == 0:
            raise ValueError("the index is empty")
        q, lens = self._phrases(phrases, lengths)
        if pair_chunk is not None and (isinstance(pair_chunk, bool) or int(pair_chunk) != pair_chunk or int(pair_chunk) < 1):
            raise ValueError("pair_chunk must be an integer >= 1, got %r" % (pair_chunk,))
        P = int(lens.size)
        sp, widest = _align_spans(spans, P, N, dev)
        k, Mx = int(sp.shape[1]), (int(lens.max()) if P else 0)
        n = P * k
        cols = torch.full((n, Mx), -1, dtype=torch.int32, device=dev)
        subs = torch.full((n, Mx), -1, dtype=torch.int32, device=dev)
        ops = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        costs = torch.full((n,), 2 ** 31 - 1, dtype=torch.int32, device=dev)
        if n and widest:                                    # else: nothing but padding, and no launch
            lib = _lib.load()
            qd = q.to(dev, torch.int32).contiguous()
            row_d = torch.from_numpy(np.ascontiguousarray(np.cumsum(lens) - lens, np.int32)).to(dev)
            len_d = torch.from_numpy(np.ascontiguousarray(lens, np.int32)).to(dev)
            pair_phrase = torch.arange(P, dtype=torch.int32, device=dev).repeat_interleave(k)
            win = sp.reshape(n, 2).to(torch.int32)
            step = int(pair_chunk) if pair_chunk is not None else \
                max(1, ALIGN_WORKSPACE_BYTES // int(lib.sylber_unit_align_workspace_bytes(1, widest)))
            step = min(step, n)
            with torch.cuda.device(dev):
                st = _stream(dev)
                ws = torch.empty(int(lib.sylber_unit_align_workspace_bytes(step, widest)), dtype=torch.uint8, device=dev)
                if _workspace_fill is not None:
                    ws.fill_(_workspace_fill)
                for r0 in range(0, n, step):
                    r1 = min(n, r0 + step)
                    _lib.check(lib.sylber_unit_align(_vp(qd), qd.shape[0], self.width, _vp(row_d), _vp(len_d), P, _vp(self._u), N,
                                                     _vp(pair_phrase[r0:r1]), _vp(win[r0:r1]), r1 - r0, widest, Mx, 1 if free_start else 0,
                                                     _vp(cols[r0:r1]), _vp(subs[r0:r1]), _vp(ops[r0:r1]), _vp(costs[r0:r1]), None,
                                                     _vp(ws), st), "sylber_unit_align")
        return cols.to(torch.int64).reshape(P, k, Mx), subs.reshape(P, k, Mx), ops.reshape(P, k, 4), costs.reshape(P, k)

    # ---- repeats --------------------------------------------------------------------------------------------------------------------
    def find_repeats(self, k: int, *, min_score=None, match: int = 2, mismatch: int = 3, gap: int = 4, sequences=None,
                     exclude_same_group: bool = False, pair_chunk: Optional[int] = None, per_pair: int = 1, within: bool = False,
                     min_sep: int = 1, _workspace_fill=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """what is said more than once, found without a query: the k best repeats between two sequences of the index ->
        ``(scores int32 [k], pairs int64 [k, 2], spans int64 [k, 2, 2])`` on the device.  Every pair of sequences ``(s, t)`` with
        ``s < t`` is aligned locally (``local_align_unit_strings``: Smith-Waterman with ``match``, ``mismatch``, ``gap``; contract
        in include/sylber_hip.h "Unit repeats") with x = sequence ``s`` and y = sequence ``t``; a pair is kept when ``score >=
        min_score`` (``None``: ``3 * match * W``, three exactly repeated units; else an integer >= 1), and the k best kept pairs
        are returned ordered by (score descending, s, t).  ``pairs[r] = (s, t)``; ``spans[r] = ((a0, a1), (b0, b1))`` are ROW IDS
        of the index (first, one past the last) in sequence ``s`` and in sequence ``t``, so ``provenance`` and
        ``align_phrases(..., free_start=False)`` work on them.  Shorter lists end in score 0, pairs ``(-1, -1)`` and spans -1.

        Sequences are the index's or those of ``sequences=``, as the searches take them; with ``exclude_same_group`` pairs whose
        two sequences share a group (a sequence's group is its first row's) are skipped.  Pairs are enumerated on the host in
        chunks and both windows of a pair point into the one stored ``units`` buffer.

        Exact (small integers): nothing returned depends on ``pair_chunk`` (the pairs per launch; by default as many as keep a
        launch's workspace below ``search.ALIGN_WORKSPACE_BYTES``), on stale workspace contents, on one ``add`` against many or on
        a ``save`` / ``load`` round trip.  ``ValueError`` before any launch: an empty index, ``k < 1``, ``min_score < 1``, a
        parameter outside its range, ``pair_chunk < 1``, a sequence of more than 65 536 rows, ``per_pair`` outside 1 .. 32,
        ``min_sep < 1``.  Fewer than two sequences (one with ``within``): padding only, without a launch.

        Every repeat.  ``per_pair = R > 1`` takes up to R repeats from each pair of sequences, and ``within=True`` adds the pairs
        ``(s, s)``: the repeats INSIDE one sequence, its cells with ``j - i < min_sep`` held at 0 (``local_align_unit_strings_all``,
        "Unit repeats, every one": the rectangle of each found repeat is taken out before the next round of its pair).  Every
        round with ``score >= min_score`` is a candidate, and the k best come back ordered by (score descending, s, t, round), so
        ``pairs[r] = (s, t)`` may repeat and may have ``s == t``; ``exclude_same_group`` never skips ``(s, s)``.  The two spans of a
        repeat inside one sequence may overlap (tandem repetition): ``a1 <= b0`` is the caller's filter.  With ``per_pair=1,
        within=False`` the call is the one-repeat search above, launch for launch.

        Out of scope: path-exact (Waterman-Eggert) blocking, which needs a traceback; non-overlapping spans inside one sequence.
        ``SyllableIndex.find_repeats`` is the one-repeat search on embeddings and still returns one repeat per pair."""
        N, dev, W = len(self), self.device, self.width
        if N == 0:
            raise ValueError("the index is empty")
        if isinstance(k, bool) or int(k) != k or int(k) < 1:
            raise ValueError("k must be an integer >= 1, got %r" % (k,))
        k = int(k)
        params = _local_params(match, mismatch, gap)
        pair_chunk = _check_pair_chunk(pair_chunk)
        floor = _min_score(min_score, params[0], W)
        R, min_sep = _check_best(per_pair, "per_pair"), _check_min_sep(min_sep)
        if not isinstance(within, (bool, np.bool_)):
            raise ValueError("within must be a bool, got %r" % (within,))
        every = R > 1 or bool(within)                       # else the one-repeat entry, as before these arguments
        off = _sequences(sequences, N, self.sequence_offsets)
        S = int(off.size - 1)
        scores = torch.zeros((k,), dtype=torch.int32, device=dev)
        pairs = torch.full((k, 2), -1, dtype=torch.int64, device=dev)
        spans = torch.full((k, 4), -1, dtype=torch.int64, device=dev)
        if S < (1 if within else 2):
            return scores, pairs, spans.reshape(k, 2, 2)
        lib = _lib.load()
        lens = np.diff(off)
        grp = self._g.index_select(0, torch.from_numpy(off[:-1]).to(dev)).cpu().numpy() if exclude_same_group else None
        # pair (s, t), s < t, is number first[s] + t - s - 1 of the enumeration by (s, t); with `within`, s <= t, first[s] + t - s
        idx = np.arange(S, dtype=np.int64)
        d = 0 if within else 1                              # the first t of row s is s + d
        first, total = idx * S - idx * (idx + 2 * d - 1) // 2, S * (S + 1 - 2 * d) // 2
        step = pair_chunk if pair_chunk is not None else REPEAT_PAIRS
        best = None                                         # the kept repeats so far: (scores, (s, t), spans), in the contract's order
        for p0 in range(0, total, step):
            p = np.arange(p0, min(total, p0 + step), dtype=np.int64)
            s = np.searchsorted(first, p, side="right") - 1
            t = p - first[s] + s + d
            if grp is not None:
                other = (grp[s] != grp[t]) | (s == t)
                s, t = s[other], t[other]
            n = int(s.size)
            if n == 0:
                continue
            xw, yw = (np.ascontiguousarray(np.stack([off[q], lens[q]], 1), np.int32) for q in (s, t))
            sc = torch.empty((n, R), dtype=torch.int32, device=dev)
            sp = torch.empty((n, R, 4), dtype=torch.int32, device=dev)
            if every:
                sep = np.where(s == t, min_sep, 0).astype(np.int32)
                _local_all_launch(lib, self._u, self._u, W, xw, yw, sep, params, R, floor, sc, sp, pair_chunk, _workspace_fill, dev)
            else:
                _local_launch(lib, self._u, self._u, W, xw, yw, params, sc, sp, 0, pair_chunk, _workspace_fill, dev)
            sc, sp = sc.reshape(n * R), sp.reshape(n * R, 4)      # candidate c: round c % R of pair c // R
            keep = (sc >= floor).nonzero().flatten()
            if keep.numel() == 0:
                continue
            of = keep // R
            st = torch.from_numpy(np.stack([s, t], 1)).to(dev).index_select(0, of)
            base = torch.from_numpy(np.stack([off[s], off[s], off[t], off[t]], 1)).to(dev).index_select(0, of)
            new = (sc.index_select(0, keep), st, sp.index_select(0, keep).to(torch.int64) + base)
            if best is not None:
                new = tuple(torch.cat([a, b]) for a, b in zip(best, new))
            # what was kept before comes from earlier pairs and is in order: a stable sort by score alone keeps (s, t, round) ascending
            order = torch.sort(-new[0].to(torch.int64), stable=True).indices[:k]
            best = tuple(a.index_select(0, order) for a in new)
        if best is not None:
            n = int(best[0].shape[0])
            scores[:n], pairs[:n], spans[:n] = best
        return scores, pairs, spans.reshape(k, 2, 2)

    # ---- persistence ----------------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """``.npz`` with the units, groups, provenance and a format tag; a round trip gives the same results bit for bit"""
        N, W = len(self), self.width or 1
        np.savez(path, format=np.array(FORMAT), width=np.array(-1 if self.width is None else self.width),
                 units=(self._u.cpu().numpy() if N else np.zeros((0, W), np.int32)),
                 groups=(self._g.cpu().numpy() if N else np.zeros(0, np.int32)), provenance=(self._prov if N else np.zeros((0, 4))),
                 span_int=np.array(self._span_dtype is np.int64))

    @classmethod
    def load(cls, path: str, device="cuda") -> "UnitIndex":
        z = np.load(path, allow_pickle=False)
        if "format" not in z.files or str(z["format"]) != FORMAT:
            raise ValueError("%s is not a saved UnitIndex (%s)" % (path, FORMAT))
        W = int(z["width"])
        idx = cls(width=None if W < 0 else W, device=device)
        if z["units"].shape[0]:
            idx.add(z["units"], groups=z["groups"], _prov=z["provenance"])
        if bool(z["span_int"]):
            idx._span_dtype = np.int64
        return idx


# ---- unit strings -------------------------------------------------------------------------------------------------------------------
def _strings(seq, what: str) -> Tuple[list, np.ndarray, Optional[int]]:
    """a sequence of unit strings (``[n]`` or ``[n, W]`` integer arrays or tensors, or ``tokenize``'s dicts through their
    ``"units"``) -> (the strings as 2-D arrays or tensors where they are, lengths int64 ``[S]``, the width of the non-empty ones or
    ``None``); ids are checked by the caller, once, on the concatenation"""
    if torch.is_tensor(seq) or isinstance(seq, (np.ndarray, dict)):
        raise ValueError("%s must be a sequence of unit strings, got one %s" % (what, type(seq).__name__))
    parts, lens, W = [], [], None
    for i, a in enumerate(seq):
        if isinstance(a, dict):
            a = a["units"]
        if torch.is_tensor(a):
            if a.dtype.is_floating_point or a.dtype.is_complex or a.dtype == torch.bool:
                raise ValueError("%s[%d] must be integers, got %s" % (what, i, a.dtype))
        else:
            a = np.asarray(a)
            kind = a.dtype.kind
            if kind == "u":                                # torch has no wide unsigned types
                if a.size and int(a.max()) > 2 ** 31 - 1:
                    raise ValueError("%s[%d]: unit ids lie in [0, 2**31 - 1], got %d" % (what, i, int(a.max())))
                a = a.astype(np.int64)
            elif kind == "f" and a.size == 0 and a.ndim == 1:      # np.asarray([]) is float64
                a = a.astype(np.int64)
            elif kind != "i":
                raise ValueError("%s[%d] must be integers, got %s" % (what, i, a.dtype))
        shape = tuple(a.shape)
        if len(shape) == 1:
            a, shape = a[:, None], (shape[0], 1)
        elif len(shape) != 2:
            raise ValueError("%s[%d] must be [n] or [n, W], got %s" % (what, i, shape))
        n, w = shape
        if n > MAX_STRING_UNITS:
            raise ValueError("%s[%d] has %d units, more than %d" % (what, i, n, MAX_STRING_UNITS))
        if n:
            if not 1 <= w <= MAX_WIDTH:
                raise ValueError("%s[%d]: the width W must be in [1, %d], got %d" % (what, i, MAX_WIDTH, w))
            if W is not None and w != W:
                raise ValueError("%s[%d]: expected W = %d, got %d" % (what, i, W, w))
            W = w
        parts.append(a)
        lens.append(n)
    return parts, np.array(lens, np.int64), W


def _flat_strings(parts: list, W: int, dev: torch.device, what: str) -> torch.Tensor:
    """the non-empty strings one after another, int32 ``[max(sum n, 1), W]`` on ``dev``; ``ValueError`` for an id outside
    ``0 .. 2**31 - 1`` (one reduction)"""
    parts = [p for p in parts if p.shape[0]]
    if not parts:
        return torch.zeros((1, W), dtype=torch.int32, device=dev)
    if not any(torch.is_tensor(p) for p in parts):
        flat = torch.from_numpy(np.concatenate(parts))     # host arrays, as tokenize returns them: one copy to the device
    else:
        parts = [p if torch.is_tensor(p) else torch.from_numpy(p) for p in parts]
        host = all(p.device.type == "cpu" for p in parts)
        flat = torch.cat([p.to(torch.device("cpu") if host else dev, torch.int64) for p in parts])
    lo, hi = int(flat.min()), int(flat.max())
    if lo < 0 or hi > 2 ** 31 - 1:
        raise ValueError("%s: unit ids lie in [0, 2**31 - 1], got %d .. %d" % (what, lo, hi))
    return flat.to(dev, torch.int32).contiguous()


def unit_strings_workspace_bytes(m, L, pairing: bool) -> np.ndarray:
    """int64: the bytes of workspace that each pair (``m`` reference units, ``L`` hypothesis units; arrays) adds to a launch of
    ``sylber_unit_strings_align`` beyond its 48 B of table: two rows of 12 B per column between strips where ``m > 64``, and with
    ``pairing`` 2 bits per cell of ``ceil(m / 64)`` strips of ``L + 63`` steps, in chunks of 32 steps"""
    m, L = np.asarray(m, np.int64), np.asarray(L, np.int64)
    rows = np.where((m > STRING_ROWS) & (L > 0), (24 * L + 255) // 256 * 256, 0)
    if not pairing:
        return rows
    strips, chunks = (m + STRING_ROWS - 1) // STRING_ROWS, (L + STRING_ROWS - 1 + ALIGN_CHUNK_COLS - 1) // ALIGN_CHUNK_COLS
    return rows + np.where((m > 0) & (L > 0), strips * chunks * 512, 0)


def _align_strings(refs, hyps, pairing, device, pair_chunk, fill, need_ref_units=False):
    """``align_unit_strings`` -> (cols, subs, ops, costs, ref offsets int64 on the host, hyp lengths, W); cols and subs ``None``
    without pairing; ``need_ref_units``: refuse references without a single unit, as everything before any launch"""
    rp, rl, Wr = _strings(refs, "refs")
    hp, hl, Wh = _strings(hyps, "hyps")
    S = int(rl.size)
    if S != int(hl.size):
        raise ValueError("refs and hyps must be equally long, got %d and %d strings" % (S, int(hl.size)))
    if Wr is not None and Wh is not None and Wr != Wh:
        raise ValueError("refs have W = %d, hyps have W = %d" % (Wr, Wh))
    if pair_chunk is not None and (isinstance(pair_chunk, bool) or int(pair_chunk) != pair_chunk or int(pair_chunk) < 1):
        raise ValueError("pair_chunk must be an integer >= 1, got %r" % (pair_chunk,))
    W = Wr or Wh or 1
    pairing = bool(pairing)
    ro, ho = (np.concatenate([[0], np.cumsum(x)]).astype(np.int64) for x in (rl, hl))
    if ro[-1] >= 2 ** 31 or ho[-1] >= 2 ** 31:
        raise ValueError("one call takes fewer than 2^31 units on each side")
    need = unit_strings_workspace_bytes(rl, hl, pairing) + 48
    if S and int(need.max()) + 256 > ALIGN_WORKSPACE_BYTES:
        s = int(need.argmax())
        raise ValueError("pair %d (%d x %d units) needs %d bytes of predecessor codes for its pairing, more than %d; pairing=False "
                         "(counts only) never needs more than 1.5 MiB per pair" % (s, rl[s], hl[s], need[s], ALIGN_WORKSPACE_BYTES))
    if need_ref_units and ro[-1] == 0:
        raise ValueError("the unit error rate needs at least one reference unit")
    dev = _device(device)
    ops = torch.empty((S, 4), dtype=torch.int32, device=dev)
    costs = torch.empty((S,), dtype=torch.int32, device=dev)
    cols = subs = None
    if pairing:
        cols = torch.empty(max(int(ro[-1]), 1), dtype=torch.int32, device=dev)
        subs = torch.empty(max(int(ro[-1]), 1), dtype=torch.int32, device=dev)
    if S:
        # the launches: pair_chunk pairs each, or as many as keep the workspace below ALIGN_WORKSPACE_BYTES
        if pair_chunk is not None:
            cuts = list(range(0, S, int(pair_chunk))) + [S]
        else:
            cuts, acc = [0], np.concatenate([[0], np.cumsum(need)])
            while cuts[-1] < S:
                cuts.append(max(cuts[-1] + 1, int(np.searchsorted(acc, acc[cuts[-1]] + ALIGN_WORKSPACE_BYTES - 256, side="right")) - 1))
        lib = _lib.load()
        rd, hd = _flat_strings(rp, W, dev, "refs"), _flat_strings(hp, W, dev, "hyps")
        groups = []
        for g0, g1 in zip(cuts[:-1], cuts[1:]):
            r32, h32 = (np.ascontiguousarray(o[g0:g1 + 1] - o[g0], np.int32) for o in (ro, ho))
            size = int(lib.sylber_unit_strings_workspace_bytes(r32.ctypes.data_as(_i32p), h32.ctypes.data_as(_i32p), g1 - g0, int(pairing)))
            if size < 0:
                raise _lib.SylberHipError("sylber_unit_strings_workspace_bytes refused the call")
            groups.append((g0, g1, r32, h32, size))

        def at(t, row, width=1):                           # the address of row `row` of a non-empty tensor, also where the slice is empty
            return ctypes.c_void_p(t.data_ptr() + int(row) * width * 4)

        with torch.cuda.device(dev):
            st = _stream(dev)
            ws = torch.empty(max(g[4] for g in groups), dtype=torch.uint8, device=dev)
            if fill is not None:
                ws.fill_(fill)
            for g0, g1, r32, h32, _ in groups:
                _lib.check(lib.sylber_unit_strings_align(at(rd, ro[g0], W), r32.ctypes.data_as(_i32p), at(hd, ho[g0], W),
                                                         h32.ctypes.data_as(_i32p), W, g1 - g0, int(pairing),
                                                         at(cols, ro[g0]) if pairing else None, at(subs, ro[g0]) if pairing else None,
                                                         at(ops, 4 * g0), at(costs, g0), None, _vp(ws), st), "sylber_unit_strings_align")
    if pairing:
        cols, subs = cols[:int(ro[-1])].to(torch.int64), subs[:int(ro[-1])]
    return cols, subs, ops, costs, ro, hl, W


def align_unit_strings(refs, hyps, *, pairing: bool = False, device="cuda", pair_chunk: Optional[int] = None, _workspace_fill=None):
    """how far two tokenisations are from each other: the global alignment of whole unit strings of any length, pair by pair
    (csrc/unit_strings.hip, ``sylber_unit_strings_align``; contract in include/sylber_hip.h "Unit strings", restated in
    tests/unit_strings_ref.py).  ``refs`` and ``hyps``: equally long sequences of ``[m]`` / ``[m, W]`` integer arrays or tensors
    (host or device, empty ones allowed), or the lists of dicts that ``SegmentSynthesis.tokenize`` returns, through their
    ``"units"``.  ``1 <= W <= 8``, ids in ``0 .. 2**31 - 1``, at most 65 536 units per string.

    Without ``pairing``: ``(ops int32 [S, 4], costs int32 [S])`` on the device.  With it: ``(cols int64 [sum m], subs int32 [sum m],
    ops, costs, ref_offsets int64 [S + 1])``, reference ``s`` in rows ``ref_offsets[s] : ref_offsets[s + 1]``.

    For a reference ``r`` of ``m`` units and a hypothesis ``h`` of ``L`` units, ``sub(i, j)`` = the columns in which ``r[i]`` and
    ``h[j]`` differ, all int32::

        E[i][-1] = (i + 1) W        E[-1][j] = (j + 1) W  (predecessor "left")        E[-1][-1] = 0
        E[i][j]  = min(E[i-1][j-1] + sub(i, j), E[i-1][j] + W, E[i][j-1] + W)   the first smallest in that order

    The path is the chain of predecessors from ``(m-1, L-1)`` to the corner.  ``costs = E[m-1][L-1]``, the weighted Levenshtein
    distance; ``ops = (equal, substituted, deleted, inserted)``: diagonal steps with ``sub = 0``, diagonal steps with ``sub > 0``,
    reference units without a partner, hypothesis units without one; ``cols[i]``: the position inside ``h`` (0-based) that
    reference unit ``i`` met on a diagonal step, -1 if it is deleted; ``subs[i]``: that ``sub``, ``W`` for a deleted unit.
    ``m = 0``: cost ``L W``, ops ``(0, 0, 0, L)``; ``L = 0``: cost ``m W``, ops ``(0, 0, m, 0)``, ``cols`` -1, ``subs`` ``W``.
    ``equal + substituted + deleted = m``, ``equal + substituted + inserted = L``, ``costs = subs.sum() + W * inserted``.  For
    ``1 <= m <= 64`` and ``L >= 1`` this is ``UnitIndex(h).align_phrases([r], [[[0, L]]], free_start=False)`` bit for bit.  Only
    the cost is symmetric under exchanging ``r`` and ``h``: ties resolve differently, so the counts need not be.

    Exact (small integers), and nothing depends on ``pair_chunk`` (the pairs per launch; by default as many as keep a launch's
    workspace below ``search.ALIGN_WORKSPACE_BYTES``), on which pairs share a call, on their order or on stale workspace
    contents.  Counts only, a pair needs at most 1.5 MiB of workspace; the pairing keeps 2 bits per cell, about ``m L / 4``
    bytes.  ``ValueError`` before any launch: lists of different length, differing widths, a width outside 1 .. 8, non-integer
    or negative ids, a string of more than 65 536 units, ``pair_chunk < 1``, and with ``pairing`` a single pair whose codes exceed
    ``ALIGN_WORKSPACE_BYTES`` (before anything is allocated).  ``S = 0`` returns empty tensors without a launch."""
    cols, subs, ops, costs, ro, _, _ = _align_strings(refs, hyps, pairing, device, pair_chunk, _workspace_fill)
    if not pairing:
        return ops, costs
    return cols, subs, ops, costs, torch.from_numpy(ro).to(ops.device)


class UnitErrorRate:
    """what ``unit_error_rate`` returns: ``uer`` = (substituted + deleted + inserted) / reference units over all pairs;
    ``weighted`` = the summed costs / (W x reference units), where a substitution counts by the share of its ids that differ; the
    four totals ``equal``, ``substituted``, ``deleted``, ``inserted``; ``ref_units``, ``hyp_units``; the per-pair ``ops`` int32
    ``[S, 4]`` and ``costs`` int32 ``[S]`` on the device"""
    __slots__ = ("uer", "weighted", "equal", "substituted", "deleted", "inserted", "ref_units", "hyp_units", "ops", "costs")

    def __init__(self, ops: torch.Tensor, costs: torch.Tensor, ref_units: int, hyp_units: int, W: int):
        tot = ops.to(torch.int64).sum(0).tolist()
        self.equal, self.substituted, self.deleted, self.inserted = (int(v) for v in tot)
        self.ref_units, self.hyp_units, self.ops, self.costs = int(ref_units), int(hyp_units), ops, costs
        self.uer = (self.substituted + self.deleted + self.inserted) / self.ref_units
        self.weighted = int(costs.to(torch.int64).sum()) / (W * self.ref_units)

    def __repr__(self) -> str:
        return "UnitErrorRate(uer=%.4f, weighted=%.4f, equal=%d, substituted=%d, deleted=%d, inserted=%d, ref_units=%d, hyp_units=%d)" % (
            self.uer, self.weighted, self.equal, self.substituted, self.deleted, self.inserted, self.ref_units, self.hyp_units)


def unit_error_rate(refs, hyps, **kw) -> UnitErrorRate:
    """the corpus-level unit error rate of hypothesis tokenisations against reference ones (clean against noisy, bf16 against
    fp32, one codebook against another): ``align_unit_strings(refs, hyps, **kw)`` summed over the pairs -> ``UnitErrorRate``.
    ``ValueError`` for what ``align_unit_strings`` refuses and for zero reference units in total."""
    kw = dict(kw)
    kw.pop("pairing", None)                                # the counts need no path
    device, pair_chunk, fill = kw.pop("device", "cuda"), kw.pop("pair_chunk", None), kw.pop("_workspace_fill", None)
    if kw:
        raise TypeError("unit_error_rate: unexpected arguments %s" % sorted(kw))
    _, _, ops, costs, ro, hl, W = _align_strings(refs, hyps, False, device, pair_chunk, fill, need_ref_units=True)
    return UnitErrorRate(ops, costs, int(ro[-1]), int(hl.sum()), W)


# ---- unit repeats -------------------------------------------------------------------------------------------------------------------
def unit_local_workspace_bytes(m, L) -> np.ndarray:
    """int64: the bytes of workspace that each pair (``m`` units of x, ``L`` units of y; arrays) adds to a launch of
    ``sylber_unit_local_align`` beyond its 40 B of table: two rows of 12 B per column between strips where ``m > 64``"""
    m, L = np.asarray(m, np.int64), np.asarray(L, np.int64)
    return np.where((m > STRING_ROWS) & (L > 0), (24 * L + 255) // 256 * 256, 0)


def _local_params(match, mismatch, gap) -> Tuple[int, int, int]:
    """the three scores of a local alignment as ints, or ``ValueError``"""
    out = []
    for name, v, lo in (("match", match, 1), ("mismatch", mismatch, 0), ("gap", gap, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= MAX_LOCAL_PARAM:
            raise ValueError("%s must be an integer in [%d, %d], got %r" % (name, lo, MAX_LOCAL_PARAM, v))
        out.append(int(v))
    return tuple(out)


def _check_pair_chunk(pair_chunk) -> Optional[int]:
    if pair_chunk is None:
        return None
    if isinstance(pair_chunk, bool) or int(pair_chunk) != pair_chunk or int(pair_chunk) < 1:
        raise ValueError("pair_chunk must be an integer >= 1, got %r" % (pair_chunk,))
    return int(pair_chunk)


def _local_groups(size_fn, name: str, table: int, xw, yw, pair_chunk) -> list:
    """the launches of a local alignment over the pairs of ``xw`` / ``yw``: ``pair_chunk`` pairs each, or as many as keep a launch's
    workspace (``table`` bytes of table per pair and its two rows) below ``ALIGN_WORKSPACE_BYTES`` -> ``[(g0, g1, xw[g0:g1],
    yw[g0:g1], bytes)]`` with ``bytes`` what ``size_fn`` (the entry's size function, ``name``) says of that launch"""
    n = int(xw.shape[0])
    if pair_chunk is not None:
        cuts = list(range(0, n, pair_chunk)) + [n]
    else:
        need = unit_local_workspace_bytes(xw[:, 1], yw[:, 1]) + table
        cuts, acc = [0], np.concatenate([[0], np.cumsum(need)])
        while cuts[-1] < n:
            cuts.append(max(cuts[-1] + 1, int(np.searchsorted(acc, acc[cuts[-1]] + ALIGN_WORKSPACE_BYTES - 256, side="right")) - 1))
    groups = []
    for g0, g1 in zip(cuts[:-1], cuts[1:]):
        a, b = np.ascontiguousarray(xw[g0:g1]), np.ascontiguousarray(yw[g0:g1])
        size = int(size_fn(a.ctypes.data_as(_i32p), b.ctypes.data_as(_i32p), g1 - g0))
        if size < 0:
            raise _lib.SylberHipError("%s refused the call" % name)
        groups.append((g0, g1, a, b, size))
    return groups


def _local_launch(lib, xd, yd, W, xw, yw, params, scores, spans, at, pair_chunk, fill, dev) -> None:
    """``sylber_unit_local_align`` on the pairs of the windows ``xw`` / ``yw`` (int32 ``[n, 2]`` on the host, ``n >= 1``) into
    ``scores[at : at + n]`` and ``spans[at : at + n]``: ``pair_chunk`` pairs per launch, or as many as keep a launch's workspace
    below ``ALIGN_WORKSPACE_BYTES``"""
    groups = _local_groups(lib.sylber_unit_local_workspace_bytes, "sylber_unit_local_workspace_bytes", 40, xw, yw, pair_chunk)
    with torch.cuda.device(dev):
        st = _stream(dev)
        ws = None
        for g0, g1, a, b, size in groups:
            if ws is None or ws.numel() != size:           # exactly what the size function said, launch by launch
                ws = torch.empty(size, dtype=torch.uint8, device=dev)
                if fill is not None:
                    ws.fill_(fill)
            _lib.check(lib.sylber_unit_local_align(_vp(xd), xd.shape[0], _vp(yd), yd.shape[0], W, a.ctypes.data_as(_i32p),
                                                   b.ctypes.data_as(_i32p), g1 - g0, params[0], params[1], params[2],
                                                   _vp(scores[at + g0:at + g1]), _vp(spans[at + g0:at + g1]), _vp(ws), st),
                       "sylber_unit_local_align")


def _local_all_launch(lib, xd, yd, W, xw, yw, sep, params, n_best, floor, scores, spans, pair_chunk, fill, dev) -> None:
    """``sylber_unit_local_align_all`` on the pairs of the windows ``xw`` / ``yw`` with ``sep`` (int32 ``[n]`` on the host) into
    ``scores [n, n_best]`` and ``spans [n, n_best, 4]``, grouped into launches as ``_local_launch`` groups them"""
    groups = _local_groups(lib.sylber_unit_local_all_workspace_bytes, "sylber_unit_local_all_workspace_bytes", 48, xw, yw, pair_chunk)
    floor = min(floor, 2 ** 31 - 1)                        # an int32 argument; no score reaches 64 * 8 * 65 536
    with torch.cuda.device(dev):
        st = _stream(dev)
        ws = None
        for g0, g1, a, b, size in groups:
            if ws is None or ws.numel() != size:           # exactly what the size function said, launch by launch
                ws = torch.empty(size, dtype=torch.uint8, device=dev)
                if fill is not None:
                    ws.fill_(fill)
            c = np.ascontiguousarray(sep[g0:g1], np.int32)
            _lib.check(lib.sylber_unit_local_align_all(_vp(xd), xd.shape[0], _vp(yd), yd.shape[0], W, a.ctypes.data_as(_i32p),
                                                       b.ctypes.data_as(_i32p), c.ctypes.data_as(_i32p), g1 - g0, params[0], params[1],
                                                       params[2], n_best, floor, _vp(scores[g0:g1]), _vp(spans[g0:g1]), _vp(ws), st),
                       "sylber_unit_local_align_all")


def _check_best(n, what: str) -> int:
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= MAX_BEST:
        raise ValueError("%s must be an integer in [1, %d], got %r" % (what, MAX_BEST, n))
    return int(n)


def _check_min_sep(min_sep) -> int:
    if isinstance(min_sep, bool) or not isinstance(min_sep, (int, np.integer)) or not 1 <= int(min_sep) <= MAX_STRING_UNITS:
        raise ValueError("min_sep must be an integer in [1, %d], got %r" % (MAX_STRING_UNITS, min_sep))
    return int(min_sep)


def _min_score(min_score, match: int, W: int) -> int:
    """the floor of a repeat's score: ``None`` = ``3 * match * W``, three exactly repeated units"""
    if min_score is None:
        return 3 * match * W
    if isinstance(min_score, bool) or not isinstance(min_score, (int, np.integer)) or int(min_score) < 1:
        raise ValueError("min_score must be None or an integer >= 1, got %r" % (min_score,))
    return int(min_score)


def local_align_unit_strings(xs, ys, *, match: int = 2, mismatch: int = 3, gap: int = 4, device="cuda",
                             pair_chunk: Optional[int] = None, _workspace_fill=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """what two unit strings have in common: their local alignment (Smith-Waterman), pair by pair -> ``(scores int32 [S], spans
    int64 [S, 2, 2])`` on the device, ``spans[s] = ((a0, a1), (b0, b1))``: the best-scoring pair of sub-spans is ``xs[s][a0:a1]``
    and ``ys[s][b0:b1]`` (csrc/unit_repeats.hip, ``sylber_unit_local_align``; contract in include/sylber_hip.h "Unit repeats",
    restated in tests/unit_repeats_ref.py).  ``xs`` and ``ys`` are what ``align_unit_strings`` takes: equally long sequences of
    ``[n]`` / ``[n, W]`` integer arrays or tensors (host or device, empty ones allowed), or ``tokenize``'s lists of dicts.
    ``1 <= W <= 8``, ids in ``0 .. 2**31 - 1``, at most 65 536 units per string; ``1 <= match <= 64``, ``0 <= mismatch <= 64``,
    ``1 <= gap <= 64``.

    With ``sub(i, j)`` = the columns in which ``x[i]`` and ``y[j]`` differ, all int32::

        s(i, j)  = match * (W - sub(i, j)) - mismatch * sub(i, j)
        H[i][-1] = H[-1][j] = 0
        c_diag   = H[i-1][j-1] + s(i, j)     start: start[i-1][j-1] if H[i-1][j-1] > 0, else (i, j)
        c_up     = H[i-1][j]   - gap * W     start: start[i-1][j]
        c_left   = H[i][j-1]   - gap * W     start: start[i][j-1]
        v        = the first largest of (c_diag, c_up, c_left), in that order
        H[i][j]  = v if v > 0 else 0         start[i][j] = that candidate's start

    The result is the best cell ``(i, j)``: the largest ``H``, then the smallest ``i``, then the smallest ``j``; ``score = H[i][j]``,
    ``(a0, a1, b0, b1) = (si, i + 1, sj, j + 1)`` with ``(si, sj) = start[i][j]``.  ``x`` is the rows: ties depend on it, so
    exchanging ``xs`` and ``ys`` may move the spans.  A pair without a positive cell -- an empty string included -- has score 0 and
    spans -1.  Both spans of a positive score are non-empty.  When ``gap == mismatch + match / 2`` with ``match`` even, as under
    the defaults, ``score = match * W * ((a1 - a0) + (b1 - b0)) / 2 - (match + mismatch) * cost`` with ``cost`` what
    ``align_unit_strings`` gives for the two spans: under the defaults ``W * (len_x + len_y) - 5 * cost``.

    Exact (small integers), and nothing depends on ``pair_chunk`` (the pairs per launch; by default as many as keep a launch's
    workspace below ``search.ALIGN_WORKSPACE_BYTES``; a pair needs at most 1.5 MiB), on which pairs share a call, on their order
    or on stale workspace contents.  ``ValueError`` before any launch: what ``align_unit_strings`` refuses, and a parameter outside
    its range.  ``S = 0`` returns empty tensors without a launch.

    More than one repeat per pair and the repeats inside one string: ``local_align_unit_strings_all``.  Out of scope: the same on
    embeddings."""
    xp, xl, Wx = _strings(xs, "xs")
    yp, yl, Wy = _strings(ys, "ys")
    S = int(xl.size)
    if S != int(yl.size):
        raise ValueError("xs and ys must be equally long, got %d and %d strings" % (S, int(yl.size)))
    if Wx is not None and Wy is not None and Wx != Wy:
        raise ValueError("xs have W = %d, ys have W = %d" % (Wx, Wy))
    pair_chunk = _check_pair_chunk(pair_chunk)
    params = _local_params(match, mismatch, gap)
    W = Wx or Wy or 1
    xo, yo = (np.concatenate([[0], np.cumsum(v)]).astype(np.int64) for v in (xl, yl))
    if xo[-1] >= 2 ** 31 or yo[-1] >= 2 ** 31:
        raise ValueError("one call takes fewer than 2^31 units on each side")
    dev = _device(device)
    scores = torch.empty((S,), dtype=torch.int32, device=dev)
    spans = torch.empty((S, 4), dtype=torch.int32, device=dev)
    if S:
        xd, yd = _flat_strings(xp, W, dev, "xs"), _flat_strings(yp, W, dev, "ys")
        xw, yw = (np.ascontiguousarray(np.stack([o[:-1], np.diff(o)], 1), np.int32) for o in (xo, yo))
        _local_launch(_lib.load(), xd, yd, W, xw, yw, params, scores, spans, 0, pair_chunk, _workspace_fill, dev)
    return scores, spans.to(torch.int64).reshape(S, 2, 2)


def local_align_unit_strings_all(xs, ys=None, *, n_best: int, min_score=None, min_sep: int = 1, match: int = 2, mismatch: int = 3,
                                 gap: int = 4, device="cuda", pair_chunk: Optional[int] = None,
                                 _workspace_fill=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """EVERY phrase two unit strings share, and the phrases one string says more than once: up to ``n_best`` local alignments per
    pair -> ``(scores int32 [S, n_best], spans int64 [S, n_best, 2, 2])`` on the device (csrc/unit_repeats_all.hip,
    ``sylber_unit_local_align_all``; contract in include/sylber_hip.h "Unit repeats, every one", restated in
    tests/unit_repeats_all_ref.py).  Strings and parameters are ``local_align_unit_strings``'s; ``1 <= n_best <= 32``.

    The rounds ``r = 0 .. n_best - 1`` of a pair run in order, all in one launch.  Round ``r`` is the recurrence of
    ``local_align_unit_strings`` with the cells ``(i, j)``, ``a0 <= i < a1`` and ``b0 <= j < b1``, of every earlier round's
    ``spans[s, q] = ((a0, a1), (b0, b1))`` held at ``H = 0``: the rectangle of a found repeat is taken out, and with it the shadow
    alignments that hug its path.  A round whose score is below ``min_score`` (``None``: ``3 * match * W``, three exactly repeated
    units; else an integer >= 1) ends the pair: it and the later rounds are score 0 and spans -1.  Scores never increase along
    ``n_best``.  Rectangles of different rounds may intersect as rectangles, so two repeats of a pair may share units of ``x`` or
    of ``y``, not both at once: a phrase said once in ``x`` and twice in ``y`` comes back twice with the same ``x`` span.

    ``ys=None`` aligns every string against ITSELF: the cells with ``j - i < min_sep`` (``min_sep >= 1``) are held at 0 as well,
    so only ``j > i`` is left, every repeat is found once and ``spans[s, r]`` has its earlier occurrence first.  Three occurrences
    come back as three repeats, (p1, p2), (p1, p3), (p2, p3).  The two spans of such a repeat may overlap, as in tandem
    repetition: ``[1, 2, 3] * 10`` gives one repeat, ``0:27`` against ``3:30``.  ``a1 <= b0`` is the caller's filter.  With ``ys``
    given ``min_sep`` is ignored.

    With ``ys``, ``min_score=1`` and any ``n_best``, ``scores[:, 0]`` and ``spans[:, 0]`` are ``local_align_unit_strings``'s, bit
    for bit.  Exact (small integers), and nothing depends on ``pair_chunk``, on which pairs share a call, on their order or on stale
    workspace contents.  ``ValueError`` before any launch: what ``local_align_unit_strings`` refuses, ``n_best`` outside 1 .. 32,
    ``min_score < 1``, ``min_sep < 1``.  ``S = 0`` returns empty tensors without a launch.

    Out of scope: path-exact (Waterman-Eggert) blocking, which needs a traceback; non-overlapping spans inside one string; the
    same on embeddings."""
    xp, xl, Wx = _strings(xs, "xs")
    yp, yl, Wy = (xp, xl, Wx) if ys is None else _strings(ys, "ys")
    S = int(xl.size)
    if S != int(yl.size):
        raise ValueError("xs and ys must be equally long, got %d and %d strings" % (S, int(yl.size)))
    if Wx is not None and Wy is not None and Wx != Wy:
        raise ValueError("xs have W = %d, ys have W = %d" % (Wx, Wy))
    pair_chunk = _check_pair_chunk(pair_chunk)
    params = _local_params(match, mismatch, gap)
    n_best = _check_best(n_best, "n_best")
    min_sep = _check_min_sep(min_sep)
    W = Wx or Wy or 1
    floor = _min_score(min_score, params[0], W)
    xo, yo = (np.concatenate([[0], np.cumsum(v)]).astype(np.int64) for v in (xl, yl))
    if xo[-1] >= 2 ** 31 or yo[-1] >= 2 ** 31:
        raise ValueError("one call takes fewer than 2^31 units on each side")
    dev = _device(device)
    scores = torch.empty((S, n_best), dtype=torch.int32, device=dev)
    spans = torch.empty((S, n_best, 4), dtype=torch.int32, device=dev)
    if S:
        xd = _flat_strings(xp, W, dev, "xs")
        yd = xd if ys is None else _flat_strings(yp, W, dev, "ys")
        xw, yw = (np.ascontiguousarray(np.stack([o[:-1], np.diff(o)], 1), np.int32) for o in (xo, yo))
        sep = np.full(S, min_sep if ys is None else 0, np.int32)
        _local_all_launch(_lib.load(), xd, yd, W, xw, yw, sep, params, n_best, floor, scores, spans, pair_chunk, _workspace_fill, dev)
    return scores, spans.to(torch.int64).reshape(S, n_best, 2, 2)

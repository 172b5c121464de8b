"""CPU tier of "Unit repeats, every one" (sylber_amd.local_align_unit_strings_all / UnitIndex.find_repeats with ``per_pair`` or
``within``; include/sylber_hip.h): tests/unit_repeats_all_ref.py against a plain cell-by-cell restatement of the rounds, the
contract's consequences -- round 0 is "Unit repeats", scores never increase, a phrase said twice in y, three occurrences inside one
string, no path cell in an earlier rectangle, the tandem string --, what the library exports, the size function as host arithmetic
and every refusal, none of which needs a device."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unit_repeats_all_ref as aref  # noqa: E402
import unit_repeats_ref as rref  # noqa: E402

PARAMS = [(2, 3, 4), (1, 1, 1), (3, 0, 2), (4, 1, 3)]
NONE = (-1, -1, -1, -1)


def loops(x, y, n_best, min_score=1, sep=0, match=2, mismatch=3, gap=4, paths=False):
    """the contract, cell by cell and round by round -> (scores, spans) as lists; with ``paths`` also the cells of each round's path,
    walked back from the best cell through the candidate each cell chose"""
    x, y = np.asarray(x), np.asarray(y)
    x = x[:, None] if x.ndim == 1 else x
    y = y[:, None] if y.ndim == 1 else y
    m, L = len(x), len(y)
    W = x.shape[1] if m else 1
    scores, spans, walked, rects = [0] * n_best, [NONE] * n_best, [], []
    for r in range(n_best if m and L else 0):
        H = [[0] * (L + 1) for _ in range(m + 1)]          # H[i + 1][j + 1] = the contract's H[i][j]
        start = [[None] * (L + 1) for _ in range(m + 1)]
        came = [[None] * (L + 1) for _ in range(m + 1)]    # the cell the chosen candidate came from, None where the path starts
        best = (0, -1, -1)
        for i in range(m):
            for j in range(L):
                if (sep > 0 and j - i < sep) or any(a0 <= i < a1 and b0 <= j < b1 for a0, a1, b0, b1 in rects):
                    continue                               # blocked: H = 0, no start, never the best
                sub = sum(1 for c in range(W) if x[i][c] != y[j][c])
                cands = [(H[i][j] + match * (W - sub) - mismatch * sub, start[i][j] if H[i][j] > 0 else (i, j), (i - 1, j - 1) if H[i][j] > 0 else None),
                         (H[i][j + 1] - gap * W, start[i][j + 1], (i - 1, j)), (H[i + 1][j] - gap * W, start[i + 1][j], (i, j - 1))]
                v, st, frm = cands[0]
                for c in cands[1:]:
                    if c[0] > v:
                        v, st, frm = c
                if v > 0:
                    H[i + 1][j + 1], start[i + 1][j + 1], came[i + 1][j + 1] = v, st, frm
                    if v > best[0]:                        # rows ascend, columns ascend inside a row: the first largest
                        best = (v, i, j)
        v, i, j = best
        if v < min_score:
            break
        si, sj = start[i + 1][j + 1]
        scores[r], spans[r] = v, (si, i + 1, sj, j + 1)
        rects.append(spans[r])
        cells, at = [], (i, j)
        while at is not None:
            cells.append(at)
            at = came[at[0] + 1][at[1] + 1]
        assert cells[-1] == (si, sj)
        walked.append(cells)
    return (scores, spans, walked) if paths else (scores, spans)


def _random_pairs(n, seed, hi=89):
    rng = np.random.default_rng(seed)
    for e in range(n):
        W = 1 + e % 2
        m, L = int(rng.integers(0, hi + 1)), int(rng.integers(0, hi + 1))
        yield rng.integers(0, 3, (m, W)), rng.integers(0, 3, (L, W)), W


def test_the_reference_is_the_rounds_cell_by_cell():
    """random pairs with m, L < 90, W in (1, 2), alphabet 3, sep in (0, 1, 3); with sep > 0 also a string against itself"""
    rounds = 0
    for e, (x, y, W) in enumerate(_random_pairs(36, 0)):
        par, sep, R = PARAMS[e % len(PARAMS)], (0, 1, 3)[e % 3], (1, 3, 6)[(e // 3) % 3]
        floor = (1, 3 * par[0] * W)[(e // 2) % 2]
        if sep and e % 2:
            y = x
        got, want = aref.local_align_all(x, y, R, floor, sep, *par), loops(x, y, R, floor, sep, *par)
        assert got == want, (x, y, par, sep, R, floor)
        rounds += sum(1 for s in want[0] if s > 0)
    assert rounds > 60


def test_the_reference_takes_300_by_300_by_8_rounds_in_under_a_second():
    rng = np.random.default_rng(1)
    x, y = rng.integers(0, 3, (300, 2)), rng.integers(0, 3, (300, 2))
    t0 = time.perf_counter()
    scores, spans = aref.local_align_all(x, y, 8)
    assert time.perf_counter() - t0 < 1.0 and min(scores) > 0


def test_round_0_without_a_band_is_unit_repeats():
    for e, (x, y, W) in enumerate(_random_pairs(40, 2)):
        par = PARAMS[e % len(PARAMS)]
        scores, spans = aref.local_align_all(x, y, 3, 1, 0, *par)
        assert (scores[0], spans[0]) == rref.local_align(x, y, *par)
        # under a floor: the same where the score reaches it, padding where it does not
        floor = 3 * par[0] * W
        s2, p2 = aref.local_align_all(x, y, 3, floor, 0, *par)
        assert (s2[0], p2[0]) == ((scores[0], spans[0]) if scores[0] >= floor else (0, NONE))


def test_scores_never_increase_and_the_stop_is_final():
    for e, (x, y, W) in enumerate(_random_pairs(30, 3)):
        sep = (0, 1, 3)[e % 3]
        scores, spans = aref.local_align_all(x, x if sep else y, 8, 4, sep)
        assert all(a >= b for a, b in zip(scores, scores[1:]))
        n = sum(1 for s in scores if s > 0)
        assert all(s >= 4 for s in scores[:n]) and scores[n:] == [0] * (8 - n) and spans[n:] == [NONE] * (8 - n)
        for a0, a1, b0, b1 in spans[:n]:
            assert 0 <= a0 < a1 <= len(x) and 0 <= b0 < b1 and (sep == 0 or b1 - 1 - (a1 - 1) >= sep)


def test_a_phrase_said_once_in_x_and_twice_in_y():
    rng = np.random.default_rng(4)
    x, y = rng.integers(0, 50, 60), rng.integers(50, 100, 90)
    y[10:22] = x[30:42]
    y[50:62] = x[30:42]
    scores, spans = aref.local_align_all(x, y, 4, 6)
    assert scores == [24, 24, 0, 0] and spans[:2] == [(30, 42, 10, 22), (30, 42, 50, 62)]


def test_three_occurrences_inside_one_string():
    p = np.arange(10, 15)
    s = np.concatenate([[1, 2], p, [3, 4, 5], p, [6, 7, 8, 9], p, [20]])
    scores, spans = aref.local_align_all(s, s, 5, 6, 1)
    assert scores == [10, 10, 10, 0, 0] and spans[:3] == [(2, 7, 10, 15), (2, 7, 19, 24), (10, 15, 19, 24)]
    # without the band the string matches itself on the diagonal, whole
    assert aref.local_align_all(s, s, 1, 6, 0) == ([2 * len(s)], [(0, len(s), 0, len(s))])


def test_no_path_cell_lies_in_an_earlier_rectangle():
    """rectangles of different rounds may intersect as rectangles; the paths stay out of every earlier one"""
    rng = np.random.default_rng(5)
    crossed = 0
    for e in range(12):
        x, y = rng.integers(0, 3, int(rng.integers(30, 70))), rng.integers(0, 3, int(rng.integers(30, 70)))
        sep = (0, 2)[e % 2]
        scores, spans, walked = loops(x, x if sep else y, 6, 3, sep, paths=True)
        for r, cells in enumerate(walked):
            a0, a1, b0, b1 = spans[r]
            assert all(a0 <= i < a1 and b0 <= j < b1 for i, j in cells)
            for q in range(r):
                c0, c1, d0, d1 = spans[q]
                assert not any(c0 <= i < c1 and d0 <= j < d1 for i, j in cells)
                crossed += int(max(a0, c0) < min(a1, c1) and max(b0, d0) < min(b1, d1))
    assert crossed > 0


def test_the_tandem_string():
    s = np.array([1, 2, 3] * 10)
    assert aref.local_align_all(s, s, 4, 6, 1) == ([54, 0, 0, 0], [(0, 27, 3, 30)] + [NONE] * 3)
    assert loops(s, s, 4, 6, 1) == ([54, 0, 0, 0], [(0, 27, 3, 30)] + [NONE] * 3)


def test_empty_sides_and_the_batch_shapes():
    x, none = np.array([[1, 2], [3, 4], [1, 2], [3, 4]]), np.zeros((0, 2), np.int64)
    for a, b in ((x, none), (none, x), (none, none)):
        assert aref.local_align_all(a, b, 3) == ([0] * 3, [NONE] * 3) == loops(a, b, 3)
    scores, spans = aref.local_align_all_batch([x, none], [x, x], n_best=2, min_score=1)
    assert scores.dtype == np.int32 and spans.dtype == np.int64 and scores.shape == (2, 2) and spans.shape == (2, 2, 2, 2)
    assert scores[0, 0] == 16 and spans[0, 0].tolist() == [[0, 4], [0, 4]] and (scores[1] == 0).all() and (spans[1] == -1).all()
    scores, spans = aref.local_align_all_batch([x], n_best=2, min_score=1)         # against itself: (0:2, 2:4)
    assert scores.tolist() == [[8, 0]] and spans[0, 0].tolist() == [[0, 2], [2, 4]]
    scores, spans = aref.local_align_all_batch([], [], n_best=3)
    assert scores.shape == (0, 3) and spans.shape == (0, 3, 2, 2)


def test_find_repeats_of_the_reference():
    a, b = np.arange(10, 20), np.arange(30, 36)
    seqs = [np.concatenate([[1, 2], a, [3]]), np.array([4]), np.concatenate([b, [5], a, [6, 7], b]), np.concatenate([[8], b])]
    # per_pair = 1 without `within` is the one-repeat search
    for kw in (dict(), dict(min_score=13), dict(groups=[0, 1, 0, 2])):
        for got, want in zip(aref.find_repeats(seqs, 4, **kw), rref.find_repeats(seqs, 4, **kw)):
            assert np.array_equal(got, want)
    scores, pairs, spans = aref.find_repeats(seqs, 6, per_pair=3, within=True)
    # a in 0 and 2; b twice inside 2, and both of them against 3: (2, 2) comes before (2, 3), round 0 before round 1
    assert scores.tolist() == [20, 12, 12, 12, 0, 0] and pairs.tolist() == [[0, 2], [2, 2], [2, 3], [2, 3], [-1, -1], [-1, -1]]
    assert spans[1].tolist() == [[14, 20], [14 + 19, 14 + 25]] and spans[2].tolist() == [[14, 20], [39 + 1, 39 + 7]]
    assert spans[3].tolist() == [[14 + 19, 14 + 25], [39 + 1, 39 + 7]]
    # groups skip (0, 2), never (2, 2)
    assert aref.find_repeats(seqs, 2, per_pair=3, within=True, groups=[0, 1, 0, 2])[1].tolist() == [[2, 2], [2, 3]]
    assert aref.find_repeats(seqs, 9, per_pair=3)[1].tolist()[:4] == [[0, 2], [2, 3], [2, 3], [-1, -1]]


# ---- the library: exports, the size function and the refusals, all without a device -------------------------------------------------
NAMES = ("sylber_unit_local_align_all", "sylber_unit_local_all_workspace_bytes")
_i32p = ctypes.POINTER(ctypes.c_int32)


def _win(values):
    a = np.ascontiguousarray(values, np.int32)
    return a, a.ctypes.data_as(_i32p)


def test_the_entries_are_exported():
    import sylber_amd
    from sylber_amd import _lib, units
    assert "local_align_unit_strings_all" in sylber_amd.__all__ and callable(sylber_amd.local_align_unit_strings_all)
    assert sylber_amd.local_align_unit_strings_all is units.local_align_unit_strings_all
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(lib, n)
    assert units.MAX_BEST == 32


def test_workspace_bytes_is_host_arithmetic():
    """it answers with no device present: nothing but the lengths goes in"""
    from sylber_amd import _lib
    lib = _lib.load()
    size, one = lib.sylber_unit_local_all_workspace_bytes, lib.sylber_unit_local_workspace_bytes

    def need(ms, Ls, fn=size):
        x, y = _win([[7, m] for m in ms]), _win([[0, L] for L in Ls])
        return fn(x[1], y[1], len(ms))

    table = need([0], [0])
    assert table == 256 == need([64], [65536]) == need([5], [0]) == need([65536], [0])      # one strip, or no column: no rows between strips
    assert need([65], [1000]) - table == 24 * 1000 + 64                      # two rows of 12 B per column, rounded up to 256 B
    assert need([65536], [65536]) - table == 24 * 65536 == 3 << 19           # never more than 1.5 MiB per pair, whatever n_best
    ms, Ls = [0, 70, 5, 200, 64], [9, 70, 0, 31, 300]
    assert need(ms, Ls) == 256 + sum(need([m], [L]) - table for m, L in zip(ms, Ls))
    assert need(ms, Ls) - 256 == need(ms, Ls, one) - 256                     # the rows are the one-repeat entry's
    assert need([1] * 5, [1] * 5) == 256 and need([1] * 6, [1] * 6) == 512   # 48 B of table per pair
    good = _win([[0, 3]])
    for x, y, n in ((None, good[1], 1), (good[1], None, 1), (good[1], good[1], 0), (good[1], good[1], -1),
                    (_win([[0, -1]])[1], good[1], 1), (good[1], _win([[0, 65537]])[1], 1), (_win([[0, 65537]])[1], good[1], 1)):
        assert size(x, y, n) == -1


def _good():
    p = 4096                                               # stands for a device pointer: never dereferenced
    return dict(x=p, x_rows=100, y=p, y_rows=80, W=2, xw=[[0, 3], [90, 10], [5, 0]], yw=[[70, 10], [0, 80], [80, 0]], sep=[0, 1, 0],
                pairs=3, match=2, mismatch=3, gap=4, n_best=4, min_score=6, score=p, span=p, ws=p, stream=None)


BAD = [dict(x=None), dict(y=None), dict(xw=None), dict(yw=None), dict(score=None), dict(span=None), dict(ws=None), dict(W=0), dict(W=9),
       dict(W=-1), dict(pairs=0), dict(pairs=-2), dict(match=0), dict(match=65), dict(mismatch=-1), dict(mismatch=65), dict(gap=0),
       dict(gap=65), dict(x_rows=-1), dict(y_rows=-1), dict(xw=[[0, 3], [91, 10], [5, 0]]), dict(yw=[[70, 11], [0, 80], [80, 0]]),
       dict(xw=[[-1, 3], [90, 10], [5, 0]]), dict(yw=[[70, 10], [0, 80], [81, 0]]), dict(xw=[[0, -3], [90, 10], [5, 0]]),
       dict(x_rows=70000, xw=[[0, 65537], [90, 10], [5, 0]]), dict(y_rows=70000, yw=[[70, 10], [0, 65537], [80, 0]]),
       dict(n_best=0), dict(n_best=33), dict(n_best=-1), dict(min_score=0), dict(min_score=-5), dict(sep=[0, 1, -1]), dict(sep=[-3, 0, 0])]


def test_bad_arguments_are_refused_before_any_device_call():
    from sylber_amd import _lib
    lib = _lib.load()
    for case in BAD:
        a = dict(_good(), **case)
        keep = [_win(a[k]) if a[k] is not None else (None, None) for k in ("xw", "yw", "sep")]
        a["xw"], a["yw"], a["sep"] = keep[0][1], keep[1][1], keep[2][1]
        assert lib.sylber_unit_local_align_all(*a.values()) == 1, case
        assert lib.sylber_last_error().decode().startswith("sylber_unit_local_align_all: "), case


def test_host_refusals_need_no_device():
    """what ``local_align_unit_strings_all`` refuses of its strings and parameters it refuses before it looks for a device"""
    from sylber_amd import local_align_unit_strings_all
    one = [np.array([1, 2, 3])]
    for xs, ys, kw, match in ((one, one * 2, {}, "equally long, got 1 and 2"), (one, [np.zeros((2, 2), np.int64)], {}, "xs have W = 1, ys have W = 2"),
                              ([np.zeros((2, 9), np.int64)], None, {}, r"width W must be in \[1, 8\]"),
                              ([np.array([0.5])], one, {}, "must be integers"),
                              (one, [np.zeros(65537, np.int64)], {}, "65537 units, more than 65536"),
                              (np.arange(3), None, {}, "sequence of unit strings"),
                              (one, one, dict(pair_chunk=0), "pair_chunk"),
                              (one, None, dict(match=0), r"match must be an integer in \[1, 64\]"),
                              (one, one, dict(mismatch=-1), r"mismatch must be an integer in \[0, 64\]"),
                              (one, one, dict(gap=65), r"gap must be an integer in \[1, 64\]"),
                              (one, one, dict(n_best=0), r"n_best must be an integer in \[1, 32\]"),
                              (one, None, dict(n_best=33), r"n_best must be an integer in \[1, 32\]"),
                              (one, one, dict(n_best=2.0), r"n_best must be an integer in \[1, 32\]"),
                              (one, one, dict(n_best=True), r"n_best must be an integer in \[1, 32\]"),
                              (one, one, dict(min_score=0), "min_score must be None or an integer >= 1"),
                              (one, None, dict(min_score=1.5), "min_score must be None or an integer >= 1"),
                              (one, None, dict(min_sep=0), r"min_sep must be an integer in \[1, 65536\]"),
                              (one, one, dict(min_sep=-2), r"min_sep must be an integer in \[1, 65536\]")):
        with pytest.raises(ValueError, match=match):
            local_align_unit_strings_all(xs, ys, **dict(dict(n_best=2), **kw))
    with pytest.raises(TypeError):
        local_align_unit_strings_all(one, one)             # n_best has no default


def test_find_repeats_refuses_its_new_arguments_without_a_device():
    """the checks of ``per_pair``, ``within`` and ``min_sep`` come before anything touches the device: an index put together by
    hand over host tensors gets as far as they do"""
    import torch
    from sylber_amd import UnitIndex
    ix = UnitIndex.__new__(UnitIndex)
    ix.device, ix.width, ix._u = torch.device("cpu"), 1, torch.zeros((8, 1), dtype=torch.int32)
    for kw, match in ((dict(per_pair=0), r"per_pair must be an integer in \[1, 32\]"), (dict(per_pair=33), r"per_pair must be an integer in \[1, 32\]"),
                      (dict(per_pair=1.0), r"per_pair must be an integer in \[1, 32\]"), (dict(min_sep=0), r"min_sep must be an integer in \[1, 65536\]"),
                      (dict(within=True, min_sep=-1), r"min_sep must be an integer in \[1, 65536\]"), (dict(within=1), "within must be a bool"),
                      (dict(per_pair=2, min_score=0), "min_score must be None or an integer >= 1")):
        with pytest.raises(ValueError, match=match):
            ix.find_repeats(3, **kw)

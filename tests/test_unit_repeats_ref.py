"""CPU tier of the unit repeats (sylber_amd.local_align_unit_strings / UnitIndex.find_repeats; include/sylber_hip.h "Unit repeats"):
tests/unit_repeats_ref.py against a plain cell-by-cell restatement of the recurrence, the contract's consequences -- the score
identity with the global alignment of the two spans, non-empty spans, the tie order of the best cell, a planted copy recovered,
empty sides --, what the library exports and the C entries' host-only refusals, which need no device."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unit_repeats_ref as rref  # noqa: E402
import unit_strings_ref as sref  # noqa: E402

PARAMS = [(2, 3, 4), (1, 1, 1), (3, 0, 2), (4, 1, 3)]


def loops(x, y, match=2, mismatch=3, gap=4, table=False):
    """the contract, cell by cell -> (score, (a0, a1, b0, b1)), or with ``table`` H as an array [m, L]"""
    x, y = np.asarray(x), np.asarray(y)
    x = x[:, None] if x.ndim == 1 else x
    y = y[:, None] if y.ndim == 1 else y
    m, L = len(x), len(y)
    W = x.shape[1] if m else 1
    H = [[0] * (L + 1) for _ in range(m + 1)]              # H[i + 1][j + 1] = the contract's H[i][j]
    start = [[None] * (L + 1) for _ in range(m + 1)]
    best = (0, -1, -1)
    for i in range(m):
        for j in range(L):
            sub = sum(1 for c in range(W) if x[i][c] != y[j][c])
            cands = [(H[i][j] + match * (W - sub) - mismatch * sub, start[i][j] if H[i][j] > 0 else (i, j)),
                     (H[i][j + 1] - gap * W, start[i][j + 1]), (H[i + 1][j] - gap * W, start[i + 1][j])]
            v, st = cands[0]
            for c in cands[1:]:
                if c[0] > v:
                    v, st = c
            H[i + 1][j + 1], start[i + 1][j + 1] = (v, st) if v > 0 else (0, None)
            if H[i + 1][j + 1] > best[0]:                  # rows ascend, columns ascend inside a row: the first largest
                best = (v, i, j)
    if table:
        return np.array(H, np.int64).reshape(m + 1, L + 1)[1:, 1:]
    if best[0] == 0:
        return 0, (-1, -1, -1, -1)
    v, i, j = best
    si, sj = start[i + 1][j + 1]
    return v, (si, i + 1, sj, j + 1)


def _random_pairs(n, seed, hi=40):
    rng = np.random.default_rng(seed)
    for e in range(n):
        W, A = int(rng.integers(1, 4)), (2, 3, 50)[e % 3]
        m, L = int(rng.integers(0, hi + 1)), int(rng.integers(0, hi + 1))
        x, y = rng.integers(0, A, (m, W)), rng.integers(0, A, (L, W))
        if e % 4 == 0 and m > 8 and L > 8:                 # a shared phrase with an edit in it
            n_c = int(rng.integers(4, min(m, L) - 2))
            a, b = int(rng.integers(0, m - n_c + 1)), int(rng.integers(0, L - n_c + 1))
            y[b:b + n_c] = x[a:a + n_c]
            y[b + n_c // 2] = rng.integers(0, A, W)
        yield x, y, W


def test_the_reference_is_the_recurrence():
    positive = 0
    for e, (x, y, W) in enumerate(_random_pairs(160, 0)):
        par = PARAMS[e % len(PARAMS)]
        got, want = rref.local_align(x, y, *par), loops(x, y, *par)
        assert got == want, (x, y, par)
        positive += int(want[0] > 0)
    assert positive > 100


def test_the_reference_takes_the_longest_strings_in_seconds():
    rng = np.random.default_rng(1)
    x, y = rng.integers(0, 3, (65536, 2)), rng.integers(0, 3, (70, 2))
    t0 = time.perf_counter()
    score, span = rref.local_align(x, y)
    assert time.perf_counter() - t0 < 30 and score > 0
    a0, a1, b0, b1 = span
    assert 0 <= a0 < a1 <= 65536 and 0 <= b0 < b1 <= 70


@pytest.mark.parametrize("par", [(2, 3, 4), (4, 1, 3)])
def test_the_score_identity_with_the_global_alignment(par):
    """gap == mismatch + match / 2, match even: score = match W (len_x + len_y) / 2 - (match + mismatch) cost of the two spans"""
    match, mismatch, gap = par
    assert match % 2 == 0 and gap == mismatch + match // 2
    checked = 0
    for x, y, W in _random_pairs(120, 2):
        score, (a0, a1, b0, b1) = rref.local_align(x, y, *par)
        if score == 0:
            continue
        cost = int(sref.align_batch([x[a0:a1]], [y[b0:b1]])[3][0])
        assert score == match * W * ((a1 - a0) + (b1 - b0)) // 2 - (match + mismatch) * cost, (x, y)
        checked += 1
    assert checked > 80


def test_spans_are_not_empty_and_end_in_matches():
    for e, (x, y, W) in enumerate(_random_pairs(120, 3)):
        par = PARAMS[e % len(PARAMS)]
        score, (a0, a1, b0, b1) = rref.local_align(x, y, *par)
        if score == 0:
            assert (a0, a1, b0, b1) == (-1, -1, -1, -1)
            # no positive cell: no two units with s > 0
            sub = (x[:, None, :] != y[None, :, :]).sum(2) if len(x) and len(y) else np.zeros((0, 0))
            assert not (par[0] * (W - sub) - par[1] * sub > 0).any()
            continue
        assert 0 <= a0 < a1 <= len(x) and 0 <= b0 < b1 <= len(y)
        for i, j in ((a0, b0), (a1 - 1, b1 - 1)):          # the first and the last step: diagonal with s > 0
            sub = int((x[i] != y[j]).sum())
            assert par[0] * (W - sub) - par[1] * sub > 0


def test_the_tie_order_of_the_best_cell():
    """two symbols: the best score is reached in many cells; the result is the first of them by (i, j)"""
    rng = np.random.default_rng(4)
    tied = 0
    for e in range(40):
        x, y = rng.integers(0, 2, int(rng.integers(5, 30))), rng.integers(0, 2, int(rng.integers(5, 30)))
        if e % 2:                                          # all of x twice in y: its full score in two cells at least
            y = np.concatenate([x, y, x])
        score, (a0, a1, b0, b1) = rref.local_align(x, y)
        H = loops(x, y, table=True)
        cells = [tuple(c) for c in np.argwhere(H == H.max()).tolist()]     # in (i, j) order
        assert score == H.max() > 0 and cells[0] == (a1 - 1, b1 - 1)
        tied += int(len(cells) > 1)
    assert tied > 10
    # by hand: "ab" twice in y -> the first column; twice in x -> the first row
    assert rref.local_align([0, 1], [0, 1, 5, 0, 1]) == (4, (0, 2, 0, 2))
    assert rref.local_align([0, 1, 5, 0, 1], [0, 1]) == (4, (0, 2, 0, 2))
    assert rref.local_align([7, 0, 1], [0, 1, 0, 1]) == (4, (1, 3, 0, 2))


@pytest.mark.parametrize("W", [1, 2, 3])
def test_a_planted_copy_is_recovered(W):
    rng = np.random.default_rng(5 + W)
    x, y = rng.integers(0, 50, (300, W)), rng.integers(0, 50, (200, W))
    y[30:90] = x[100:160]
    # make the copy maximal: the units on either side of it differ
    y[29], y[90] = (x[99] + 1) % 50, (x[160] + 1) % 50
    assert rref.local_align(x, y) == (2 * W * 60, (100, 160, 30, 90))


def test_empty_sides():
    x = np.array([[1, 2], [3, 4]])
    none = np.zeros((0, 2), np.int64)
    for a, b in ((x, none), (none, x), (none, none), (np.zeros(0, np.int64), np.zeros(0, np.int64))):
        assert rref.local_align(a, b) == (0, (-1, -1, -1, -1)) == loops(a, b)
    scores, spans = rref.local_align_batch([x, none, x], [x, x, none])
    assert scores.tolist() == [8, 0, 0] and spans.tolist() == [[[0, 2], [0, 2]], [[-1, -1]] * 2, [[-1, -1]] * 2]
    assert scores.dtype == np.int32 and spans.dtype == np.int64
    scores, spans = rref.local_align_batch([], [])
    assert scores.shape == (0,) and spans.shape == (0, 2, 2)


def test_find_repeats_of_the_reference():
    a, b = np.arange(10, 20), np.arange(30, 36)
    seqs = [np.concatenate([[1, 2], a, [3]]), np.array([4]), np.concatenate([b, [5], a]), np.concatenate([[6], b])]
    scores, pairs, spans = rref.find_repeats(seqs, 4)
    assert scores.tolist() == [20, 12, 0, 0] and pairs.tolist() == [[0, 2], [2, 3], [-1, -1], [-1, -1]]
    assert spans[0].tolist() == [[2, 12], [14 + 7, 14 + 17]] and spans[1].tolist() == [[14, 20], [31 + 1, 31 + 7]]
    assert (spans[2:] == -1).all()
    assert rref.find_repeats(seqs, 1)[1].tolist() == [[0, 2]]
    assert rref.find_repeats(seqs, 2, min_score=13)[0].tolist() == [20, 0]
    assert rref.find_repeats(seqs, 2, groups=[0, 1, 0, 2])[1].tolist() == [[2, 3], [-1, -1]]


# ---- the library: exports and host-only refusals ------------------------------------------------------------------------------------
NAMES = ("sylber_unit_local_align", "sylber_unit_local_workspace_bytes")
_i32p = ctypes.POINTER(ctypes.c_int32)


def _win(values):
    a = np.ascontiguousarray(values, np.int32)
    return a, a.ctypes.data_as(_i32p)


def test_the_entries_are_exported():
    import sylber_amd
    from sylber_amd import _lib, units
    assert "local_align_unit_strings" in sylber_amd.__all__ and callable(sylber_amd.local_align_unit_strings)
    assert sylber_amd.local_align_unit_strings is units.local_align_unit_strings
    assert callable(sylber_amd.UnitIndex.find_repeats)
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(lib, n)
    assert units.MAX_LOCAL_PARAM == 64


def test_workspace_bytes_is_host_arithmetic():
    from sylber_amd import _lib, units
    size = _lib.load().sylber_unit_local_workspace_bytes

    def need(ms, Ls):
        x, y = _win([[7, m] for m in ms]), _win([[0, L] for L in Ls])
        return size(x[1], y[1], len(ms))

    table = need([0], [0])
    assert table == 256 == need([64], [65536]) == need([5], [0]) == need([65536], [0])      # one strip, or no column: no rows between strips
    assert need([65], [1000]) - table == 24 * 1000 + 64                      # two rows of 12 B per column, rounded up to 256 B
    assert need([65536], [65536]) - table == 24 * 65536 == 3 << 19           # never more than 1.5 MiB per pair
    ms, Ls = [0, 70, 5, 200, 64], [9, 70, 0, 31, 300]
    assert need(ms, Ls) == 256 + sum(need([m], [L]) - table for m, L in zip(ms, Ls))      # 5 x 40 B of table; a pair's slice is its own
    assert np.array_equal(units.unit_local_workspace_bytes(ms, Ls), [need([m], [L]) - table for m, L in zip(ms, Ls)])
    assert need([1] * 6, [1] * 6) == 256 and need([1] * 7, [1] * 7) == 512   # 40 B of table per pair
    good = _win([[0, 3]])
    for x, y, n in ((None, good[1], 1), (good[1], None, 1), (good[1], good[1], 0), (good[1], good[1], -1),
                    (_win([[0, -1]])[1], good[1], 1), (good[1], _win([[0, 65537]])[1], 1), (_win([[0, 65537]])[1], good[1], 1)):
        assert size(x, y, n) == -1


def _good():
    p = 4096                                               # stands for a device pointer: never dereferenced
    return dict(x=p, x_rows=100, y=p, y_rows=80, W=2, xw=[[0, 3], [90, 10], [5, 0]], yw=[[70, 10], [0, 80], [80, 0]], pairs=3, match=2,
                mismatch=3, gap=4, score=p, span=p, ws=p, stream=None)


BAD = [dict(x=None), dict(y=None), dict(xw=None), dict(yw=None), dict(score=None), dict(span=None), dict(ws=None), dict(W=0), dict(W=9),
       dict(W=-1), dict(pairs=0), dict(pairs=-2), dict(match=0), dict(match=65), dict(mismatch=-1), dict(mismatch=65), dict(gap=0),
       dict(gap=65), dict(x_rows=-1), dict(y_rows=-1), dict(xw=[[0, 3], [91, 10], [5, 0]]), dict(yw=[[70, 11], [0, 80], [80, 0]]),
       dict(xw=[[-1, 3], [90, 10], [5, 0]]), dict(yw=[[70, 10], [0, 80], [81, 0]]), dict(xw=[[0, -3], [90, 10], [5, 0]]),
       dict(x_rows=70000, xw=[[0, 65537], [90, 10], [5, 0]]), dict(y_rows=70000, yw=[[70, 10], [0, 65537], [80, 0]])]


def test_bad_arguments_are_refused_before_any_device_call():
    from sylber_amd import _lib
    lib = _lib.load()
    for case in BAD:
        a = dict(_good(), **case)
        keep = [_win(a[k]) if a[k] is not None else (None, None) for k in ("xw", "yw")]
        a["xw"], a["yw"] = keep[0][1], keep[1][1]
        assert lib.sylber_unit_local_align(*a.values()) == 1, case
        assert lib.sylber_last_error().decode().startswith("sylber_unit_local_align: "), case


def test_host_refusals_need_no_device():
    """what ``local_align_unit_strings`` refuses of its strings and parameters it refuses before it looks for a device"""
    from sylber_amd import local_align_unit_strings
    one = [np.array([1, 2, 3])]
    for xs, ys, kw, match in ((one, one * 2, {}, "equally long, got 1 and 2"), (one, [np.zeros((2, 2), np.int64)], {}, "xs have W = 1, ys have W = 2"),
                              ([np.zeros((2, 9), np.int64)], one, {}, r"width W must be in \[1, 8\]"),
                              ([np.array([1, 2]), np.zeros((2, 2), np.int64)], one * 2, {}, "expected W = 1, got 2"),
                              ([np.array([0.5])], one, {}, "must be integers"),
                              (one, [np.zeros(65537, np.int64)], {}, "65537 units, more than 65536"),
                              (np.arange(3), one, {}, "sequence of unit strings"),
                              (one, one, dict(pair_chunk=0), "pair_chunk"), (one, one, dict(pair_chunk=1.5), "pair_chunk"),
                              (one, one, dict(match=0), r"match must be an integer in \[1, 64\]"),
                              (one, one, dict(match=65), r"match must be an integer in \[1, 64\]"),
                              (one, one, dict(mismatch=-1), r"mismatch must be an integer in \[0, 64\]"),
                              (one, one, dict(gap=0), r"gap must be an integer in \[1, 64\]"),
                              (one, one, dict(gap=2.0), r"gap must be an integer in \[1, 64\]"),
                              (one, one, dict(match=True), r"match must be an integer in \[1, 64\]")):
        with pytest.raises(ValueError, match=match):
            local_align_unit_strings(xs, ys, **kw)

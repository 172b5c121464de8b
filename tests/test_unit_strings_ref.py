"""CPU tier of the unit strings (sylber_amd.align_unit_strings / unit_error_rate; include/sylber_hip.h "Unit strings"): the two
restatements of tests/unit_strings_ref.py against each other -- the definition with its walk back and the carried counters that
the kernel computes its counts in --, the cost against an independent Levenshtein distance, the three identities, the
strip-by-strip form against the whole table, what the library exports and the C entries' host-only refusals, which need no
device."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unit_strings_ref as sref  # noqa: E402


def _random_pairs(n, seed, hi=150):
    rng = np.random.default_rng(seed)
    for e in range(n):
        W, A = int(rng.integers(1, 4)), (2, 3, 50)[e % 3]
        m, L = int(rng.integers(0, hi + 1)), int(rng.integers(0, hi + 1))
        if e % 10 == 0:                                    # a hypothesis that is the reference with a few edits: long diagonal runs
            r = rng.integers(0, A, (max(m, 1), W))
            h = np.delete(r, rng.integers(len(r)), 0)
            h = np.insert(h, rng.integers(len(h) + 1), rng.integers(0, A, W), 0)
        else:
            r, h = rng.integers(0, A, (m, W)), rng.integers(0, A, (L, W))
        yield r, h, W


def test_the_two_restatements_agree_and_the_identities_hold():
    empty = 0
    for r, h, W in _random_pairs(240, 0):
        cols, subs, ops, cost = sref.align(r, h)
        ops2, cost2 = sref.counters(r, h)
        assert np.array_equal(ops, ops2) and cost == cost2, (r, h)
        m, L = len(r), len(h)
        assert ops[:3].sum() == m and ops[[0, 1, 3]].sum() == L and cost == subs.sum() + W * ops[3]
        assert cols.shape == (m,) and subs.shape == (m,) and (cols < 0).sum() == ops[2] and ((cols >= 0) & (subs > 0)).sum() == ops[1]
        assert np.array_equal(subs[cols < 0], np.full(ops[2], W)) and np.all(np.diff(cols[cols >= 0]) > 0)
        assert all(subs[i] == (r[i] != h[cols[i]]).sum() for i in np.nonzero(cols >= 0)[0])
        empty += int(m == 0 or L == 0)
    assert empty > 0


def test_empty_sides():
    r = np.array([[1, 2], [3, 4], [5, 6]])
    none = np.zeros((0, 2), np.int64)
    cols, subs, ops, cost = sref.align(r, none)
    assert cols.tolist() == [-1] * 3 and subs.tolist() == [2] * 3 and ops.tolist() == [0, 0, 3, 0] and cost == 6
    cols, subs, ops, cost = sref.align(none, r)
    assert cols.shape == (0,) and subs.shape == (0,) and ops.tolist() == [0, 0, 0, 3] and cost == 6
    cols, subs, ops, cost = sref.align(np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert ops.tolist() == [0, 0, 0, 0] and cost == 0
    for a, b in ((r, none), (none, r), (none, none)):
        o, c = sref.counters(a, b)
        assert np.array_equal(o, sref.align(a, b)[2]) and c == sref.align(a, b)[3]


def test_the_cost_is_the_levenshtein_distance_and_symmetric():
    """the cost alone: exchanged, ties resolve differently and the counts may change with them"""
    for r, h, W in _random_pairs(150, 1, hi=60):
        assert sref.align(r, h)[3] == sref.align(h, r)[3] == sref.lev(r, h, W) == sref.lev(h, r, W)


def test_strip_by_strip_equals_the_whole_table():
    rng = np.random.default_rng(2)
    for m in (63, 64, 65, 128, 129, 200):
        for W, A, L in ((1, 2, 70), (2, 3, 33), (3, 50, 90)):
            r, h = rng.integers(0, A, (m, W)), rng.integers(0, A, (L, W))
            whole, cut = sref.counters(r, h), sref.strips(r, h, 64)
            assert np.array_equal(whole[0], cut[0]) and whole[1] == cut[1], (m, W)
            ops, cost = sref.align(r, h)[2:]
            assert np.array_equal(ops, cut[0]) and cost == cut[1], (m, W)


def test_align_batch_is_flat():
    refs = [np.array([1, 2, 3]), np.zeros(0, np.int64), np.array([4, 4])]
    hyps = [np.array([1, 3]), np.array([7]), np.zeros(0, np.int64)]
    cols, subs, ops, costs, off = sref.align_batch(refs, hyps)
    assert off.tolist() == [0, 3, 3, 5] and cols.tolist() == [0, -1, 1, -1, -1] and subs.tolist() == [0, 1, 0, 1, 1]
    assert ops.tolist() == [[2, 0, 1, 0], [0, 0, 0, 1], [0, 0, 2, 0]] and costs.tolist() == [1, 1, 2]
    assert cols.dtype == np.int64 and subs.dtype == ops.dtype == costs.dtype == np.int32


# ---- the library: exports and host-only refusals ------------------------------------------------------------------------------------
NAMES = ("sylber_unit_strings_align", "sylber_unit_strings_workspace_bytes")
_i32p = ctypes.POINTER(ctypes.c_int32)


def _off(values):
    a = np.ascontiguousarray(values, np.int32)
    return a, a.ctypes.data_as(_i32p)


def test_the_entries_are_exported():
    import sylber_amd
    from sylber_amd import _lib, units
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(lib, n)
    assert units.STRING_ROWS == 64 and units.MAX_STRING_UNITS == 65536
    for n in ("align_unit_strings", "unit_error_rate"):
        assert callable(getattr(sylber_amd, n)) and n in sylber_amd.__all__


def test_workspace_bytes_is_host_arithmetic():
    from sylber_amd import _lib, units
    size = _lib.load().sylber_unit_strings_workspace_bytes

    def need(ms, Ls, pairing):
        r, h = _off(np.concatenate([[0], np.cumsum(ms)])), _off(np.concatenate([[0], np.cumsum(Ls)]))
        return size(r[1], h[1], len(ms), pairing)

    table = need([0], [0], 0)
    assert table == 256 == need([0], [0], 1) == need([64], [65536], 0) == need([5], [0], 1) == need([0], [5], 1)      # one strip: no rows between strips
    assert need([65], [1000], 0) - table == 24 * 1000 + 64                  # two rows of 12 B per column, rounded up to 256 B
    assert need([65536], [65536], 0) - table == 24 * 65536 == 3 << 19       # counts only: never more than 1.5 MiB per pair
    assert need([64], [1], 1) - table == 2 * 512 and need([64], [2], 1) - table == 3 * 512      # chunks of 32 of L + 63 steps
    assert need([65], [2], 1) - table == 256 + 2 * 3 * 512                  # two strips
    assert need([3000], [2900], 1) - table == 24 * 2900 + 32 + 47 * 93 * 512
    ms, Ls = [0, 70, 5, 200, 64], [9, 70, 0, 31, 300]
    for pairing in (0, 1):
        each = sum(need([m], [L], pairing) - table for m, L in zip(ms, Ls))
        assert need(ms, Ls, pairing) == 256 + each                          # 5 x 48 B of table; a pair's slice is its own
        assert np.array_equal(units.unit_strings_workspace_bytes(ms, Ls, bool(pairing)),
                              [need([m], [L], pairing) - table for m, L in zip(ms, Ls)])
    assert need([1] * 6, [1] * 6, 0) == 512                                 # 6 x 48 B of table
    good = _off([0, 3])
    for r, h, n, pairing in ((None, good[1], 1, 0), (good[1], None, 1, 0), (good[1], good[1], 0, 0), (good[1], good[1], -1, 0),
                             (good[1], good[1], 1, 2), (good[1], good[1], 1, -1), (_off([1, 3])[1], good[1], 1, 0),
                             (good[1], _off([3, 0])[1], 1, 0), (_off([0, 65537])[1], good[1], 1, 0), (good[1], _off([0, 65537])[1], 1, 1)):
        assert size(r, h, n, pairing) == -1
    assert need([65536], [65536], 1) > 0


def _good():
    p = 4096                                               # stands for a device pointer: never dereferenced
    return dict(r=p, ro=[0, 3, 3, 70], h=p, ho=[0, 0, 5, 9], W=2, pairs=3, pairing=1, cols=p, subs=p, ops=p, cost=p, walk=None, ws=p,
                stream=None)


BAD = [dict(r=None), dict(ro=None), dict(h=None), dict(ho=None), dict(ops=None), dict(cost=None), dict(ws=None), dict(cols=None),
       dict(subs=None), dict(W=0), dict(W=9), dict(W=-1), dict(pairs=0), dict(pairs=-2), dict(pairing=2), dict(pairing=-1),
       dict(ro=[0, 3, 2, 70]), dict(ho=[0, 6, 5, 9]), dict(ro=[1, 3, 3, 70]), dict(ho=[-1, 0, 5, 9]), dict(ro=[0, 3, 3, 65540]),
       dict(ho=[0, 0, 5, 65542]), dict(pairing=0, ro=[0, 3, 3, 65540]), dict(pairing=0, ops=None)]


def test_bad_arguments_are_refused_before_any_device_call():
    from sylber_amd import _lib
    lib = _lib.load()
    for case in BAD:
        a = dict(_good(), **case)
        keep = [_off(a[k]) if a[k] is not None else (None, None) for k in ("ro", "ho")]
        a["ro"], a["ho"] = keep[0][1], keep[1][1]
        assert lib.sylber_unit_strings_align(*a.values()) != 0, case
        assert lib.sylber_last_error().decode().startswith("sylber_unit_strings_align: "), case


def test_host_refusals_need_no_device():
    """what ``align_unit_strings`` refuses it refuses before it looks for a device"""
    import pytest
    from sylber_amd import align_unit_strings, unit_error_rate
    one = [np.array([1, 2, 3])]
    for refs, hyps, kw, match in ((one, one * 2, {}, "equally long"), (one, [np.zeros((2, 2), np.int64)], {}, "refs have W = 1, hyps have W = 2"),
                                  ([np.zeros((2, 9), np.int64)], one, {}, r"width W must be in \[1, 8\]"),
                                  ([np.array([1, 2]), np.zeros((2, 2), np.int64)], one * 2, {}, "expected W = 1, got 2"),
                                  ([np.array([0.5])], one, {}, "must be integers"), ([np.array([True])], one, {}, "must be integers"),
                                  (one, [np.zeros(65537, np.int64)], {}, "65537 units, more than 65536"),
                                  (one, [np.zeros((2, 2, 2), np.int64)], {}, r"must be \[n\] or \[n, W\]"),
                                  (np.arange(3), one, {}, "sequence of unit strings"),
                                  (one, one, dict(pair_chunk=0), "pair_chunk"), (one, one, dict(pair_chunk=1.5), "pair_chunk"),
                                  ([np.zeros(40000, np.int64)], [np.zeros(40000, np.int64)], dict(pairing=True), "pairing=False")):
        with pytest.raises(ValueError, match=match):
            align_unit_strings(refs, hyps, **kw)
    with pytest.raises(ValueError, match="equally long"):
        unit_error_rate(one, one * 2)
    with pytest.raises(ValueError, match="pair_chunk"):
        unit_error_rate(one, one, pair_chunk=-3)
    for refs, hyps in (([], []), ([np.zeros(0, np.int64)], one)):
        with pytest.raises(ValueError, match="at least one reference unit"):
            unit_error_rate(refs, hyps)

"""CPU tier of the unit search (sylber_amd.UnitIndex; include/sylber_hip.h "Unit search"): the numpy restatement
tests/unit_search_ref.py against an independent brute force -- textbook weighted Levenshtein distance over all substrings -- on
random pairs over alphabets of 2 to 4 symbols (ties everywhere) and W = 1 .. 3; what the package exports; the C entries' host-only
refusals, which need no device."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unit_search_ref as ref  # noqa: E402


def lev(a, b, W):
    """textbook global edit distance of unit strings a [m, W], b [n, W]: substitution = differing columns, indel = W"""
    m, n = len(a), len(b)
    D = np.zeros((m + 1, n + 1), np.int64)
    D[:, 0] = np.arange(m + 1) * W
    D[0, :] = np.arange(n + 1) * W
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            D[i, j] = min(D[i - 1, j - 1] + int((a[i - 1] != b[j - 1]).sum()), D[i - 1, j] + W, D[i, j - 1] + W)
    return int(D[m, n])


def _pairs(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        W, A = int(rng.integers(1, 4)), int(rng.integers(2, 5))
        m, L = int(rng.integers(1, 6)), int(rng.integers(1, 11))
        yield rng.integers(0, A, (m, W)), rng.integers(0, A, (L, W)), W


@pytest.fixture(scope="module")
def rows():
    """(p, t, W, E, st) of 500 random pairs, E / st from the vectorised last_rows"""
    out = []
    for p, t, W in _pairs(500, 0):
        E, ST = ref.last_rows([p], [t])
        out.append((p, t, W, E[0, 0], ST[0, 0]))
    return out


def test_the_vectorised_rows_are_the_contract_cell_by_cell(rows):
    for p, t, W, E, st in rows[:200]:
        E2, st2 = ref.last_row_loop(p, t)
        assert np.array_equal(E, E2) and np.array_equal(st, st2)
        E3, st3 = ref.last_row_scan(p, t)                                 # the row-wise form that long sequences use
        assert np.array_equal(E, E3) and np.array_equal(st, st3)
    # all pairs of a batch at once, mixed lengths
    rng = np.random.default_rng(1)
    ph = [rng.integers(0, 3, (m, 2)) for m in (1, 4, 2, 6)]
    sq = [rng.integers(0, 3, (L, 2)) for L in (3, 9, 1)]
    E, ST = ref.last_rows(ph, sq)
    for a, p in enumerate(ph):
        for b, t in enumerate(sq):
            E2, st2 = ref.last_row_loop(p, t)
            assert np.array_equal(E[a, b, :len(t)], E2) and np.array_equal(ST[a, b, :len(t)], st2)


def test_starts_ascend_and_no_admissible_span_is_empty(rows):
    for p, t, W, E, st in rows:
        assert np.all(np.diff(st) >= 0)
        adm = E <= len(p) * W - 1
        assert np.all(st[adm] <= np.arange(len(t))[adm])


def test_cost_is_the_brute_force_minimum_and_spans_attain_it(rows):
    for p, t, W, E, st in rows:
        m, L = len(p), len(t)
        brute = min([m * W] + [lev(p, t[a:b], W) for a in range(L) for b in range(a + 1, L + 1)])
        assert min(int(E.min()), m * W) == brute
        for j in np.nonzero(E <= m * W - 1)[0]:                           # every admissible column is a real alignment of its span
            assert lev(p, t[st[j]:j + 1], W) == E[j]


def test_occurrences_are_disjoint_and_the_best_is_search_phrases(rows):
    some = 0
    for p, t, W, E, st in rows:
        thr = len(p) * W - 1
        occ = ref.one_pass(ref.families(E, st, thr))
        assert occ == ref.one_pass_columns(E, st, thr)                    # the per-column form the kernel runs
        for a, b in zip(occ, occ[1:]):
            assert a[2] < b[1]
        best = ref.best_match(E, st, thr)
        assert (best is None) == (not occ)
        if occ:
            assert min(occ, key=lambda o: (o[0], o[1])) == best
            some += len(occ) > 1
    assert some > 50


def test_exact_substring_and_phrase_longer_than_the_sequence():
    rng = np.random.default_rng(2)
    corpus = rng.integers(0, 50, (40, 2))
    off = [0, 15, 40]
    ph = [corpus[20:25], corpus[3:4]]
    c, q, sp, n = ref.search_phrases(corpus, off, ph, 2)
    assert c[0, 0] == 0 and q[0, 0] == 1 and tuple(sp[0, 0]) == (20, 25)
    assert c[1, 0] == 0 and q[1, 0] == 0 and tuple(sp[1, 0]) == (3, 4)
    # m > L: the three-unit sequence inside a five-unit phrase costs two deletions
    t = corpus[:3]
    p = np.concatenate([corpus[30:31], t, corpus[31:32]])
    c, q, sp, n = ref.search_phrases(t, [0, 3], [p], 1)
    assert c[0, 0] == 2 * 2 and tuple(sp[0, 0]) == (0, 3)


def test_max_cost_only_removes_results_and_padding():
    rng = np.random.default_rng(3)
    corpus = rng.integers(0, 3, 60)
    off = np.arange(0, 61, 12)                             # at most 60 occurrences: nothing is cut off at k
    ph = [rng.integers(0, 3, m) for m in (3, 5, 4)]
    for fn in (ref.search_phrases, ref.search_occurrences):
        full = fn(corpus, off, ph, 128)
        for mc in (0, 1, [2, 0, 1]):
            cut = fn(corpus, off, ph, 128, max_cost=mc)
            for p in range(3):
                thr = np.broadcast_to(mc, 3)[p]
                keep = full[0][p] <= thr
                n = int(keep.sum())
                assert cut[3][p] == n
                assert np.array_equal(cut[0][p, :n], full[0][p][keep]) and np.array_equal(cut[2][p, :n], full[2][p][keep])
                assert np.all(cut[0][p, n:] == 2 ** 31 - 1) and np.all(cut[1][p, n:] == -1) and np.all(cut[2][p, n:] == -1)
    assert full[0].dtype == np.int32 and full[1].dtype == np.int64 and full[2].dtype == np.int64


def test_one_pass_is_not_greedy_suppression():
    """A - B - C with A and C disjoint, both overlapping B, costs A > B > C: only C is emitted"""
    fams = [(3, 0, 4), (2, 3, 8), (1, 7, 11)]
    assert ref.one_pass(fams) == [(1, 7, 11)]


# ---- the package and the C ABI ------------------------------------------------------------------------------------------------------
NAMES = ("sylber_unit_search", "sylber_unit_occurrences", "sylber_unit_workspace_bytes")


def test_the_index_and_the_entries_are_exported():
    import sylber_amd
    from sylber_amd import _lib, units
    assert "UnitIndex" in sylber_amd.__all__ and sylber_amd.UnitIndex is units.UnitIndex
    assert units.TILE_COLS == 256
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(lib, n)
    assert _lib.EXPORTS["sylber_unit_search"] == _lib.EXPORTS["sylber_unit_occurrences"]


def _i32(a):
    return (ctypes.c_int32 * len(a))(*a)


def _good():
    p = 4096                                               # stands for a device pointer: never dereferenced
    return dict(q=p, R=5, W=2, prow=_i32([0, 2]), plen=_i32([2, 3]), thr=_i32([3, 5]), P=2, x=p, N=30, off=_i32([0, 10, 30]), S=2, seqid=p,
                pgrp=None, sgrp=None, splits=0, k=10, cost=p, seq=p, span=p, ws=p, stream=None)


BAD = [dict(q=None), dict(prow=None), dict(plen=None), dict(thr=None), dict(x=None), dict(off=None), dict(seqid=None), dict(cost=None),
       dict(seq=None), dict(span=None), dict(ws=None), dict(W=0), dict(W=9), dict(k=0), dict(k=129), dict(P=0), dict(S=0), dict(N=0),
       dict(R=0), dict(splits=-1), dict(plen=_i32([0, 3])), dict(plen=_i32([2, 65])), dict(plen=_i32([2, 4])), dict(prow=_i32([-1, 2])),
       dict(off=_i32([0, 10, 10])), dict(off=_i32([0, 20, 10])), dict(off=_i32([1, 10, 30])), dict(off=_i32([0, 10, 29])),
       dict(off=_i32([0, 10, 65547]), N=65547), dict(thr=_i32([3, -1])), dict(pgrp=_i32([0, 1])), dict(sgrp=4096)]


@pytest.mark.parametrize("name", NAMES[:2])
def test_bad_arguments_are_refused_before_any_device_call(name):
    from sylber_amd import _lib
    lib = _lib.load()
    for case in BAD:
        args = dict(_good(), **case)
        assert getattr(lib, name)(*args.values()) != 0, case
        assert lib.sylber_last_error().decode().startswith(name + ": "), case


def test_workspace_bytes_is_host_arithmetic():
    from sylber_amd import _lib
    lib = _lib.load()
    g = _good()
    size = lambda **kw: lib.sylber_unit_workspace_bytes(*dict(dict(plen=g["plen"], P=2, off=_i32([0, 20, 30]), S=2, k=10, splits=0), **kw).values())
    one = size()
    assert one > 0 and one % 256 == 0
    assert size(splits=2) > one                            # two cuts (row 20 is the first sequence start at or after 30 / 2): two partial lists per phrase
    assert size(splits=7) == size(splits=2)                # cuts fall on sequence starts: two sequences give at most two
    for bad in (dict(plen=None), dict(off=None), dict(P=0), dict(S=0), dict(k=0), dict(k=129), dict(splits=-1), dict(plen=_i32([2, 65])),
                dict(off=_i32([0, 10, 10]))):
        assert size(**bad) == -1, bad

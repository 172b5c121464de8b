"""CPU tier of the edit scripts (sylber_amd.UnitIndex.align_phrases; include/sylber_hip.h "Edit scripts"): the theorem -- the
window DP on a span that a unit search returned starts in the span's first row, costs what was reported and takes the scan's own
path, in both modes -- on more than 20 000 returned spans of tests/unit_search_ref.py; the global mode against an independent
Levenshtein distance; the two forms of the reference against each other; what the library exports and the C entry's host-only
refusals, which need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unit_align_ref as aref  # noqa: E402
import unit_search_ref as ref  # noqa: E402


def _corrupted(rng, corpus, off, A, n):
    """n phrases cut from sequences of the corpus; each in turn untouched, with a unit substituted, one deleted, one inserted, or all
    three"""
    out = []
    for e in range(n):
        s = int(rng.integers(len(off) - 1))
        L = int(off[s + 1] - off[s])
        m = int(rng.integers(1, min(L, 7) + 1))
        a = int(off[s] + rng.integers(0, L - m + 1))
        p = np.array(corpus[a:a + m], copy=True)
        kind = e % 5
        if kind in (1, 4):
            p[rng.integers(len(p))] = rng.integers(0, A, p.shape[1])
        if kind in (2, 4) and len(p) > 1:
            p = np.delete(p, rng.integers(len(p)), 0)                              # the window holds a row more: an insertion
        if kind in (3, 4):
            p = np.insert(p, rng.integers(len(p) + 1), rng.integers(0, A, p.shape[1]), 0)      # ... a unit more: a deletion
        out.append(p)
    return out


def test_the_theorem_on_returned_spans():
    """first row = a, cost = the reported cost, the pairing = the full DP's own walk back, both modes alike, the three identities"""
    rng = np.random.default_rng(0)
    spans_seen = with_del = with_ins = 0
    for W in (1, 2, 3):
        for A in (2, 3, 50):
            lens = rng.integers(4, 17, 14)
            off = np.concatenate([[0], np.cumsum(lens)])
            corpus = rng.integers(0, A, (int(off[-1]), W))
            phrases = _corrupted(rng, corpus, off, A, 20)
            seqs = [corpus[off[s]:off[s + 1]] for s in range(len(lens))]
            rows = ref.last_rows(phrases, seqs)
            tables = {}                                    # (phrase, sequence) -> the full DP, made once
            for mc in (None, 0, 1, 2, 3, 4):
                for fn in (ref.search_phrases, ref.search_occurrences):
                    cost, seq, span, _ = fn(corpus, off, phrases, 40, rows=rows, max_cost=mc)
                    for pi, p in enumerate(phrases):
                        m = len(p)
                        for r in np.nonzero(seq[pi] >= 0)[0]:
                            a, b = (int(v) for v in span[pi, r])
                            s = int(seq[pi, r])
                            free = aref.window_loop(p, corpus[a:b], True)
                            glob = aref.window_loop(p, corpus[a:b], False)
                            for c, sb, ops, E, first in (free, glob):
                                assert first == 0 and E == cost[pi, r]
                                assert ops[:3].sum() == m and (b - a) - ops[[0, 1, 3]].sum() == first
                                assert E == sb.sum() + W * ops[3]
                            assert all(np.array_equal(x, y) for x, y in zip(free[:3], glob[:3]))
                            if (pi, s) not in tables:
                                tables[pi, s] = aref.window_table(p, seqs[s], True)
                            Ef, pred = tables[pi, s]
                            o = int(off[s])
                            own = aref.walk_back(pred, lambda i, j: int((p[i] != seqs[s][j]).sum()), W, m - 1, b - 1 - o, True)
                            assert Ef[m - 1][b - 1 - o] == cost[pi, r] and own[3] == a - o
                            assert np.array_equal(np.where(own[0] >= 0, own[0] + o - a, -1), free[0])
                            assert np.array_equal(own[1], free[1]) and np.array_equal(own[2], free[2])
                            spans_seen += 1
                            with_del += int(free[2][2] > 0)
                            with_ins += int(free[2][3] > 0)
    assert spans_seen >= 20000, spans_seen
    assert with_del > 0 and with_ins > 0, (with_del, with_ins)


def lev(a, b, W):
    """textbook global edit distance of unit strings a [m, W], b [n, W]: substitution = differing columns, indel = W"""
    prev = [j * W for j in range(len(b) + 1)]
    for i in range(1, len(a) + 1):
        cur = [i * W]
        for j in range(1, len(b) + 1):
            cur.append(min(prev[j - 1] + int((a[i - 1] != b[j - 1]).sum()), prev[j] + W, cur[j - 1] + W))
        prev = cur
    return prev[-1]


def _pairs(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        W, A = int(rng.integers(1, 4)), int(rng.integers(2, 5))
        m, L = int(rng.integers(1, 8)), int(rng.integers(1, 13))
        yield rng.integers(0, A, (m, W)), rng.integers(0, A, (L, W)), W


def test_global_mode_is_the_levenshtein_distance():
    for p, t, W in _pairs(600, 1):
        c, sb, ops, E, first = aref.window_loop(p, t, False)
        assert E == lev(p, t, W) and first == 0
        assert ops[:3].sum() == len(p) and ops[[0, 1, 3]].sum() == len(t) and E == sb.sum() + W * ops[3]
        assert np.array_equal(sb[c < 0], np.full((c < 0).sum(), W)) and all(sb[i] == (p[i] != t[c[i]]).sum() for i in np.nonzero(c >= 0)[0])
        assert np.all(np.diff(c[c >= 0]) > 0)              # the pairing is monotone


def test_free_start_on_any_window():
    """a window that no search returned: the path may begin inside it, and the cost is the last cell of the searches' last row"""
    inside = 0
    for p, t, W in _pairs(600, 2):
        c, sb, ops, E, first = aref.window_loop(p, t, True)
        E2, st2 = ref.last_row_loop(p, t)
        assert E == E2[-1] and first == st2[-1]            # the walk back ends where the scan's start tracking says
        assert ops[:3].sum() == len(p) and len(t) - ops[[0, 1, 3]].sum() == first and E == sb.sum() + W * ops[3]
        inside += int(first > 0)
        # the full DP's walk back from every column of the last row ends where the scan's start tracking says, at its cost
        for end in range(len(t)):
            own = aref.scan_path(p, t, end)
            assert own[3] == E2[end] and own[4] == st2[end]
        assert all(np.array_equal(x, y) for x, y in zip(own, (c, sb, ops, E, first)))
    assert inside > 100


def test_the_two_forms_of_the_reference_agree():
    for mode in (True, False):
        for p, t, W in _pairs(300, 3):
            one, two = aref.window_loop(p, t, mode), aref.window_scan(p, t, mode)
            assert all(np.array_equal(x, y) for x, y in zip(one, two)), (p, t, mode)
    rng = np.random.default_rng(4)                         # longer, over two symbols: ties everywhere
    for m, L in ((64, 300), (5, 1000), (64, 3)):
        p, t = rng.integers(0, 2, (m, 2)), rng.integers(0, 2, (L, 2))
        for mode in (True, False):
            assert all(np.array_equal(x, y) for x, y in zip(aref.window_loop(p, t, mode), aref.window_scan(p, t, mode)))


def test_align_phrases_pads():
    corpus = np.arange(12) % 3
    spans = np.array([[[2, 5], [-1, -1]], [[0, 12], [4, 5]]])
    cols, subs, ops, costs, first = aref.align_phrases(corpus, [np.array([2, 0, 1]), np.array([1])], spans)
    assert cols.shape == (2, 2, 3) and cols[0, 0].tolist() == [2, 3, 4] and costs[0].tolist() == [0, ref.PAD]
    assert cols[0, 1].tolist() == [-1] * 3 and subs[0, 1].tolist() == [-1] * 3 and not ops[0, 1].any() and first[0, 1] == -1
    assert cols[1, 1].tolist() == [4, -1, -1] and subs[1, 0].tolist() == [1, -1, -1] and first[1].tolist() == [11, 4]


# ---- the library: exports and host-only refusals ------------------------------------------------------------------------------------
NAMES = ("sylber_unit_align", "sylber_unit_align_workspace_bytes")


def test_the_entries_are_exported():
    from sylber_amd import _lib, units
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(lib, n)
    assert units.ALIGN_CHUNK_COLS == 32 and hasattr(units.UnitIndex, "align_phrases")


def _good():
    p = 4096                                               # stands for a device pointer: never dereferenced
    return dict(q=p, R=5, W=2, prow=p, plen=p, P=2, x=p, N=30, pp=p, win=p, pairs=3, max_cols=12, max_rows=3, free=1, cols=p, subs=p,
                ops=p, cost=p, start=None, ws=p, stream=None)


BAD = [dict(q=None), dict(prow=None), dict(plen=None), dict(x=None), dict(pp=None), dict(win=None), dict(cols=None), dict(subs=None),
       dict(ops=None), dict(cost=None), dict(ws=None), dict(W=0), dict(W=9), dict(R=0), dict(N=0), dict(P=0), dict(pairs=0), dict(max_cols=0),
       dict(max_cols=65537), dict(max_rows=0), dict(max_rows=65), dict(free=-1), dict(free=2)]


def test_bad_arguments_are_refused_before_any_device_call():
    from sylber_amd import _lib
    lib = _lib.load()
    for case in BAD:
        args = dict(_good(), **case)
        assert lib.sylber_unit_align(*args.values()) != 0, case
        assert lib.sylber_last_error().decode().startswith("sylber_unit_align: "), case


def test_workspace_bytes_is_host_arithmetic():
    from sylber_amd import _lib
    lib = _lib.load()
    size = lib.sylber_unit_align_workspace_bytes
    one = size(1, 1)
    assert one > 0 and one % 512 == 0                      # whole rows of 64 words
    assert size(2, 1) == 2 * one and size(1, 65536) > size(1, 1000) > size(1, 100) > one
    assert size(1, 65536) >= 16 * 65536 and size(7, 65536) == 7 * size(1, 65536)
    for bad in ((0, 10), (-1, 10), (1, 0), (1, 65537), (1, -5)):
        assert size(*bad) == -1, bad

"""GPU tier of the edit scripts (sylber_amd.UnitIndex.align_phrases, csrc/unit_align.hip) against tests/unit_align_ref.py: cols,
subs, ops and costs equal bit for bit -- everything is a small integer, no tolerance is involved.  Shapes are the smallest at which
the kernel can go wrong: phrases of 1, 2, 63 and 64 units, windows around the chunk of anti-diagonal steps, a phrase longer than
its window, one window of 65 536 columns, widths that fill their padded row and widths that do not, alphabets of 2 (ties
everywhere) and 20 000 symbols, spans at both ends of the corpus and on a sequence start."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unit_align_ref as aref  # noqa: E402
import unit_search_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

from sylber_amd import UnitIndex  # noqa: E402
from sylber_amd.units import ALIGN_CHUNK_COLS, TILE_COLS  # noqa: E402

T, CH = TILE_COLS, ALIGN_CHUNK_COLS


def _np(out):
    return tuple(o.cpu().numpy() for o in out)


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def _index(corpus, off):
    """an index whose default sequences are ``off``: one group per sequence"""
    g = np.repeat(np.arange(len(off) - 1), np.diff(off)).astype(np.int32)
    return UnitIndex(corpus, groups=g), g


def _raw(idx, phrases, spans, free_start, pair_phrase=None, tables=None, max_cols=None):
    """``sylber_unit_align`` itself, all pairs in one launch -> (cols, subs, ops, costs, start) as int32 arrays; ``pair_phrase [P, k]``
    and ``tables = (phrase rows, phrase lengths)`` stand in for the ones that belong to ``phrases``"""
    from sylber_amd import _lib
    from sylber_amd.kmeans import _stream, _vp
    lib, dev = _lib.load(), idx.device
    q, lens = idx._phrases(phrases, None)
    P, k, Mx = len(lens), spans.shape[1], int(lens.max())
    n = P * k
    qd = q.to(dev, torch.int32).contiguous()
    rows, lens = tables if tables is not None else (np.cumsum(lens) - lens, lens)
    row_d = torch.from_numpy(np.asarray(rows).astype(np.int32)).to(dev)
    len_d = torch.from_numpy(np.asarray(lens).astype(np.int32)).to(dev)
    pp = torch.arange(P, dtype=torch.int32, device=dev).repeat_interleave(k)
    if pair_phrase is not None:
        pp = torch.from_numpy(np.asarray(pair_phrase, np.int32).reshape(n)).to(dev)
    win = torch.from_numpy(np.ascontiguousarray(spans.reshape(n, 2), np.int32)).to(dev)
    widest = max_cols if max_cols is not None else int((spans[..., 1] - spans[..., 0]).max())
    cols, subs = (torch.full((n, Mx), 7, dtype=torch.int32, device=dev) for _ in range(2))
    ops = torch.full((n, 4), 7, dtype=torch.int32, device=dev)
    cost, start = (torch.full((n,), 7, dtype=torch.int32, device=dev) for _ in range(2))
    ws = torch.empty(int(lib.sylber_unit_align_workspace_bytes(n, widest)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.sylber_unit_align(_vp(qd), qd.shape[0], idx.width, _vp(row_d), _vp(len_d), P, _vp(idx.units), len(idx), _vp(pp), _vp(win),
                                         n, widest, Mx, int(free_start), _vp(cols), _vp(subs), _vp(ops), _vp(cost), _vp(start), _vp(ws),
                                         _stream(dev)), "sylber_unit_align")
    return tuple(t.cpu().numpy().reshape((P, k) + t.shape[1:]) for t in (cols, subs, ops, cost, start))


def _check(idx, corpus, phrases, spans, searched=None):
    """``align_phrases`` on ``spans`` (int64 [P, k, 2], numpy) equals the reference in both modes, and so does the raw entry, whose
    tracked start is the first row of the path walked back.  ``searched``: the costs of the search that returned the spans -- then
    the theorem holds too: the first row is the span's, the cost the reported one, both modes alike.  Returns the free-start result."""
    out = []
    for mode in (True, False):
        want = aref.align_phrases(corpus, phrases, spans, mode)
        got = _np(idx.align_phrases(phrases, torch.from_numpy(spans), free_start=mode))
        assert got[0].dtype == np.int64 and _same(got, want[:4]), mode
        raw = _raw(idx, phrases, spans, mode)
        assert all(np.array_equal(x, y) for x, y in zip(raw, want)), mode
        if searched is not None:
            assert np.array_equal(want[4], spans[..., 0]) and np.array_equal(got[3], searched)
        out.append(got)
    if searched is not None:
        assert _same(out[0], out[1])
    return out[0]


def _both(idx, corpus, phrases, k, **kw):
    """the spans of both searches, aligned; returns them"""
    spans = []
    for name in ("search_phrases", "search_occurrences"):
        c, s, sp = _np(getattr(idx, name)(phrases, k, **kw))
        assert (s >= 0).any()
        _check(idx, corpus, phrases, sp, searched=c)
        spans.append(sp)
    return spans


def _corrupt(rng, piece, A):
    """a copy of a corpus substring with one substitution (two units or more) and one deletion (four or more)"""
    p = np.array(piece, copy=True)
    if len(p) < 2:
        return p
    p[rng.integers(len(p))] = rng.integers(0, A, p.shape[1:])
    return np.delete(p, rng.integers(len(p)), 0) if len(p) > 3 else p


# ---- spans of both searches ----------------------------------------------------------------------------------------------------------
TILE_LENGTHS = [T, T - 1, 1, 2, T - 1, T + 1, 3 * T + 5, 1, 40]


@pytest.fixture(scope="module")
def tiles():
    rng = np.random.default_rng(10)
    off = np.concatenate([[0], np.cumsum(TILE_LENGTHS)])
    corpus = rng.integers(0, 2, int(off[-1]))              # two symbols: ties everywhere
    return corpus, off, _index(corpus, off)[0]


def test_spans_of_both_searches_phrase_lengths(tiles):
    corpus, off, idx = tiles
    rng = np.random.default_rng(7)
    N = len(corpus)
    phrases = [rng.integers(0, 2, m) for m in (1, 2, 63, 64, 5)]       # includes m > L against the sequences of 1 and 2 units
    phrases += [corpus[:17].copy(), corpus[N - 9:].copy(), corpus[off[6]:off[6] + 64].copy()]
    for kw in (dict(), dict(max_cost=2)):
        for sp in _both(idx, corpus, phrases, 10, **kw):
            assert 0 in sp[5, :, 0] and N in sp[6, :, 1] and off[6] in sp[7, :, 0]     # row 0, row N, a sequence start


@pytest.mark.parametrize("W, A", [(1, 20000), (2, 2), (2, 20000), (3, 2), (8, 2), (8, 20000)])
def test_spans_of_both_searches_widths_and_alphabets(W, A):
    rng = np.random.default_rng(100 * W + A % 7)
    lens = rng.integers(20, 61, 14)
    off = np.concatenate([[0], np.cumsum(lens)])
    corpus = rng.integers(0, A, (int(off[-1]), W))
    if W == 1:
        corpus = corpus[:, 0]
    phrases = []
    for m in (1, 2, 5, 9, 16, 33, 64, 3, 7):
        a = int(rng.integers(0, len(corpus) - m))
        phrases.append(_corrupt(rng, corpus[a:a + m], A))
    idx, _ = _index(corpus, off)
    _both(idx, corpus, phrases, 6)
    _both(idx, corpus, phrases, 6, max_cost=W)


@pytest.fixture(scope="module")
def many():
    """200 short sequences over two symbols: far more admissible sequences and occurrences than any k"""
    rng = np.random.default_rng(12)
    lens = rng.integers(3, 11, 200)
    off = np.concatenate([[0], np.cumsum(lens)])
    corpus = rng.integers(0, 2, (int(off[-1]), 2))
    phrases = [rng.integers(0, 2, (m, 2)) for m in rng.integers(1, 7, 40)]
    idx, g = _index(corpus, off)
    return corpus, off, phrases, idx, g


def test_spans_under_max_cost_and_exclude_same_group(many):
    corpus, off, phrases, idx, g = many
    _both(idx, corpus, phrases, 10)
    sp0 = _both(idx, corpus, phrases, 10, max_cost=0)      # exact matches only: lists that end in padding
    assert (sp0[0] == -1).any() and (sp0[0] >= 0).any()
    sg = np.arange(200) % 5
    gidx = UnitIndex(corpus, groups=np.repeat(sg, np.diff(off)).astype(np.int32))
    _both(gidx, corpus, phrases, 10, groups=np.arange(len(phrases)) % 5, exclude_same_group=True, sequences=off, max_cost=np.arange(len(phrases)) % 4)


# ---- planted scripts ---------------------------------------------------------------------------------------------------------------
def test_planted_scripts():
    rng = np.random.default_rng(13)
    word = rng.integers(0, 20000, (6, 2))
    corpus = rng.integers(0, 20000, (300, 2))
    off = np.array([0, 100, 200, 300])
    corpus[100:106] = word                                 # on a sequence start
    idx, _ = _index(corpus, off)
    removed = np.delete(word, 3, 0)                        # the window holds a row that the phrase does not: an insertion
    foreign = np.concatenate([[[20001, 20002]], word])     # a first unit that nothing matches: deleted through the boundary column
    changed = word.copy()
    changed[2, 1] = 20003                                  # one id of two: sub = 1
    phrases = [removed, foreign, changed, word]
    c, s, sp = _np(idx.search_phrases(phrases, 1))
    assert c[:, 0].tolist() == [2, 2, 1, 0] and s[:, 0].tolist() == [1] * 4 and sp[:, 0].tolist() == [[100, 106]] * 4
    cols, subs, ops, costs = _check(idx, corpus, phrases, sp, searched=c)
    assert cols[0, 0].tolist() == [100, 101, 102, 104, 105, -1, -1] and subs[0, 0].tolist() == [0] * 5 + [-1, -1]
    assert ops[0, 0].tolist() == [5, 0, 0, 1]
    assert cols[1, 0].tolist() == [-1, 100, 101, 102, 103, 104, 105] and subs[1, 0].tolist() == [2] + [0] * 6
    assert ops[1, 0].tolist() == [6, 0, 1, 0]
    assert cols[2, 0].tolist() == [100, 101, 102, 103, 104, 105, -1] and subs[2, 0].tolist() == [0, 0, 1, 0, 0, 0, -1]
    assert ops[2, 0].tolist() == [5, 1, 0, 0]
    assert cols[3, 0].tolist() == cols[2, 0].tolist() and ops[3, 0].tolist() == [6, 0, 0, 0] and costs[:, 0].tolist() == [2, 2, 1, 0]
    assert idx.provenance(cols[0, 0, :5]) == [None] * 5    # rows added without provenance


# ---- windows of the caller's own -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, A", [(1, 2), (2, 2), (3, 3), (8, 2)])
def test_windows_around_the_chunk(W, A):
    rng = np.random.default_rng(20 + W)
    off = np.array([0, 50, 51, 200, 400])
    corpus = rng.integers(0, A, (400, W))
    idx, _ = _index(corpus, off)
    phrases = [rng.integers(0, A, (m, W)) for m in (1, 64, 2, 63)]
    lengths = [1, 2, CH - 1, CH, CH + 1, 2 * CH + 1, 3, CH + 2]
    starts = [0, 49, 60, 399 - CH, 200, 7, 48, 30]          # (49, 51), (48, 51) and (30, 30 + CH + 2) cross sequence boundaries
    starts[3] = 400 - CH                                    # ends at row N
    spans = np.array([[[a, a + L] for a, L in zip(starts, lengths)]] * len(phrases), np.int64)
    assert spans.max() == 400 and (spans[..., 1] - spans[..., 0]).min() == 1
    _check(idx, corpus, phrases, spans)


def test_one_window_of_65536_columns():
    rng = np.random.default_rng(11)
    corpus = rng.integers(0, 3, 65536)
    p = rng.integers(0, 3, 64)
    idx = UnitIndex(corpus)
    spans = np.array([[[0, 65536]]], np.int64)
    for mode in (True, False):
        c, s, o, cost, first = aref.window_scan(p, corpus, mode)
        got = _np(idx.align_phrases([p], spans, free_start=mode))
        assert np.array_equal(got[0][0, 0], c) and np.array_equal(got[1][0, 0], s) and np.array_equal(got[2][0, 0], o) and got[3][0, 0] == cost
        assert 65536 - o[[0, 1, 3]].sum() == first and (first == 0 or mode)
        assert _raw(idx, [p], spans, mode)[4][0, 0] == first


# ---- invariance -------------------------------------------------------------------------------------------------------------------
def test_nothing_depends_on_chunks_workspace_placement_adds_or_a_round_trip(many, tmp_path):
    corpus, off, phrases, idx, g = many
    spans = idx.search_occurrences(phrases, 7)[2]
    for mode in (True, False):
        base = _np(idx.align_phrases(phrases, spans, free_start=mode))
        assert _same(base, aref.align_phrases(corpus, phrases, spans.cpu().numpy(), mode)[:4])
        for kw in (dict(pair_chunk=1), dict(pair_chunk=3), dict(_workspace_fill=0xA5), dict(_workspace_fill=0xFF), dict(pair_chunk=3, _workspace_fill=0xFF)):
            assert _same(_np(idx.align_phrases(phrases, spans, free_start=mode, **kw)), base), kw
        assert _same(_np(idx.align_phrases(phrases, spans.cpu(), free_start=mode)), base)                # spans on the host
        assert _same(_np(idx.align_phrases(phrases, spans.cpu().numpy(), free_start=mode)), base)
        packed, lens = np.concatenate(phrases), [len(p) for p in phrases]
        assert _same(_np(idx.align_phrases(packed, spans, lengths=lens, free_start=mode)), base)
    parts = UnitIndex(width=2)
    for a in range(0, 200, 37):                            # many adds against one
        lo, hi = off[a], off[min(a + 37, 200)]
        parts.add(torch.from_numpy(corpus[lo:hi]), groups=g[lo:hi])
    path = str(tmp_path / "units.npz")
    idx.save(path)
    for other in (parts, UnitIndex.load(path)):
        assert _same(_np(other.align_phrases(phrases, spans)), _np(idx.align_phrases(phrases, spans)))


# ---- padding and refusals -----------------------------------------------------------------------------------------------------------
def test_padding():
    corpus = np.arange(40) % 3
    idx = UnitIndex(corpus)
    phrases = [np.array([1, 2, 0, 1]), np.array([2])]
    spans = np.array([[[-1, -1], [3, 8], [-1, -1]], [[0, 40], [-1, -1], [39, 40]]], np.int64)       # padding inside the lists
    cols, subs, ops, costs = _check(idx, corpus, phrases, spans)
    assert cols[0, 0].tolist() == [-1] * 4 and subs[0, 2].tolist() == [-1] * 4 and not ops[1, 1].any() and costs[1, 1] == ref.PAD
    assert costs[0, 1] < ref.PAD and subs[1, 2].tolist() == [1, -1, -1, -1]
    # all padding and nothing at all: shaped results, no launch
    cols, subs, ops, costs = idx.align_phrases(phrases, np.full((2, 3, 2), -1, np.int64))
    assert cols.shape == (2, 3, 4) and cols.dtype == torch.int64 and int(cols.max()) == -1 and int(subs.max()) == -1
    assert subs.dtype == ops.dtype == costs.dtype == torch.int32 and not ops.any() and int(costs.min()) == ref.PAD
    cols, subs, ops, costs = idx.align_phrases([], np.zeros((0, 3, 2), np.int64))
    assert cols.shape == (0, 3, 0) and subs.shape == (0, 3, 0) and ops.shape == (0, 3, 4) and costs.shape == (0, 3)
    cols, subs, ops, costs = idx.align_phrases(phrases, np.zeros((2, 0, 2), np.int64))
    assert cols.shape == (2, 0, 4) and ops.shape == (2, 0, 4) and costs.shape == (2, 0) and cols.is_cuda


def test_bad_pairs_of_the_raw_entry_come_back_as_padding():
    """what the entry cannot see on the host -- a phrase number, a phrase's rows or length, a window out of range -- makes that pair
    padding and leaves its neighbours alone"""
    corpus = np.arange(40) % 3
    idx = UnitIndex(corpus)
    phrases = [np.array([1, 2, 0, 1]), np.array([2])]      # R = 5 rows, Mx = 4
    bad = [[5, 5], [6, 5], [-2, 3], [30, 41], [0, 13]]     # empty, reversed, before row 0, past row N, longer than max_cols = 12
    spans = np.array([[[3, 8]] + bad + [[28, 40]]] * 2, np.int64)
    legal = spans.copy()
    legal[:, 1:6] = -1

    def padded(want, which):
        want = [w.copy() for w in want]
        for w, v in zip(want, (-1, -1, 0, ref.PAD, -1)):
            w[which] = v
        return want

    for mode in (True, False):
        want = aref.align_phrases(corpus, phrases, legal, mode)
        assert (want[3][:, [0, 6]] < ref.PAD).all()
        got = _raw(idx, phrases, spans, mode, max_cols=12)
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
        pp = np.array([[0, -1, 2, 0, 0, 0, 0], [1, 1, 1, 1, 1, 2 ** 31 - 1, 1]])
        which = (pp < 0) | (pp > 1)
        got = _raw(idx, phrases, np.where(which[..., None], spans[:, :1], spans), mode, pair_phrase=pp, max_cols=12)
        keep = np.where(which[..., None], spans[:, :1], legal)
        assert all(np.array_equal(x, y) for x, y in zip(got, padded(aref.align_phrases(corpus, phrases, keep, mode), which)))
        # a phrase of 0 or 65 units, one that begins before its rows, one that runs past them, one longer than the outputs' pitch
        for tables, p in ((([0, 4], [0, 1]), 0), (([0, 4], [65, 1]), 0), (([-1, 4], [4, 1]), 0), (([0, 4], [4, 2]), 1), (([0, 0], [4, 5]), 1)):
            which = np.zeros((2, 7), bool)
            which[p] = True
            got = _raw(idx, phrases, spans, mode, tables=tables, max_cols=12)
            assert all(np.array_equal(x, y) for x, y in zip(got, padded(want, which))), tables


def test_refusals():
    idx = UnitIndex(np.arange(20) % 3)
    one = [np.array([1, 2])]
    ok = np.array([[[0, 5]]], np.int64)
    with pytest.raises(ValueError, match="expected W = 1, got 2"):
        idx.align_phrases([np.zeros((2, 2), np.int64)], ok)
    with pytest.raises(ValueError, match="from 65 to 65"):
        idx.align_phrases([np.zeros(65, np.int64)], ok)
    with pytest.raises(ValueError, match="need lengths"):
        idx.align_phrases(np.array([1, 2]), ok)
    with pytest.raises(ValueError, match="lengths sum to 3"):
        idx.align_phrases(np.array([1, 2]), ok, lengths=[3])
    for bad in (ok.astype(np.int32), ok[0], np.zeros((2, 1, 2), np.int64), np.zeros((1, 1, 3), np.int64)):
        with pytest.raises(ValueError, match=r"spans must be int64 \[1 phrases, k, 2\]"):
            idx.align_phrases(one, bad)
    for bad in ([[[5, 5]]], [[[6, 5]]], [[[-1, 5]]], [[[0, 21]]], [[[-1, -1], [-2, -2]]], [[[3, -1]]]):
        with pytest.raises(ValueError, match="1 spans are neither"):
            idx.align_phrases(one, np.array(bad, np.int64))
        with pytest.raises(ValueError, match="1 spans are neither"):
            idx.align_phrases(one, torch.tensor(bad, device="cuda"))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="pair_chunk must be an integer >= 1"):
            idx.align_phrases(one, ok, pair_chunk=bad)
    with pytest.raises(ValueError, match="a window has 65537 rows, more than 65536"):
        UnitIndex(np.zeros(65537, np.int64)).align_phrases(one, np.array([[[0, 65537]]], np.int64))
    with pytest.raises(ValueError, match="empty"):
        UnitIndex(width=1).align_phrases(one, ok)

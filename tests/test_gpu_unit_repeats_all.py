"""GPU tier of "Unit repeats, every one" (sylber_amd.local_align_unit_strings_all / UnitIndex.find_repeats with ``per_pair`` or
``within``, csrc/unit_repeats_all.hip) against tests/unit_repeats_all_ref.py: scores, pairs and spans equal bit for bit, dtype
included -- everything is a small integer, no tolerance is involved.  The rounds of a pair run in order, so the reference of
``n_best = 32`` holds the reference of every smaller ``n_best`` in its first columns: it is made once per configuration.

Shapes: no strip, one strip, two with their carried rows, five; y around the chunk of 32 steps and the ring of 128 columns; widths
that fill their padded row and one that does not; an alphabet of 3 (ties everywhere, 32 rounds and more to find) and of 1000 (only
what was planted).  Planted repeats put a rectangle across a strip edge, a chunk edge, the ring's wrap, at row 0 / column 0, in the
last row / column, over three strips, and two rectangles on the same rows."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unit_repeats_all_ref as aref  # noqa: E402

pytestmark = pytest.mark.gpu

from sylber_amd import UnitIndex, local_align_unit_strings, local_align_unit_strings_all  # noqa: E402

SHAPES = ((0, 5), (1, 0), (33, 40), (65, 257), (129, 127), (300, 129))
# W, alphabet, (match, mismatch, gap), min_score: None = 3 * match * W; 1 where that floor would leave random strings nothing
CONFIGS = [(1, 3, (2, 3, 4), None), (2, 3, (1, 1, 1), None), (3, 3, (2, 3, 4), 1), (8, 3, (1, 1, 1), 1), (1, 1000, (1, 1, 1), None),
           (8, 1000, (2, 3, 4), None)]
BESTS = (1, 2, 7, 32)


def _np(out):
    return tuple(o.cpu().numpy() for o in out)


def _same(a, b):
    assert len(a) == len(b)
    return all(np.array_equal(x, y) and x.dtype == y.dtype and x.shape == y.shape for x, y in zip(a, b))


def _cut(want, R):
    return want[0][:, :R], want[1][:, :R]


_BATCHES, _WANT = {}, {}


def _batch(W, A):
    """the pairs of SHAPES; with the alphabet of 1000, where nothing repeats by chance, a phrase of x three times in y, once with
    an edit"""
    if (W, A) not in _BATCHES:
        rng = np.random.default_rng(100 * W + A)
        xs = [rng.integers(0, A, (m, W)) for m, _ in SHAPES]
        ys = [rng.integers(0, A, (L, W)) for _, L in SHAPES]
        if A == 1000:
            for x, y in zip(xs, ys):
                if len(x) >= 30 and len(y) >= 40:
                    n, a = 9, len(x) - 12
                    for b in (1, 14, len(y) - n):
                        y[b:b + n] = x[a:a + n]
                    y[18] = (y[18] + 1) % A
        _BATCHES[W, A] = (xs, ys)
    return _BATCHES[W, A]


def _want(W, A, par, floor):
    if (W, A, par, floor) not in _WANT:
        xs, ys = _batch(W, A)
        _WANT[W, A, par, floor] = aref.local_align_all_batch(xs, ys, 32, floor, 1, *par)
    return _WANT[W, A, par, floor]


# ---- random pairs at every shape ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", BESTS)
@pytest.mark.parametrize("W, A, par, floor", CONFIGS)
def test_every_shape(W, A, par, floor, R):
    xs, ys = _batch(W, A)
    want = _want(W, A, par, floor)
    rounds = (want[0] > 0).sum(1)
    assert rounds[:2].tolist() == [0, 0] and (rounds[3:] >= (20 if A == 3 else 3)).all()
    got = _np(local_align_unit_strings_all(xs, ys, n_best=R, min_score=floor, match=par[0], mismatch=par[1], gap=par[2]))
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and got[1].shape == (len(xs), R, 2, 2)
    assert _same(got, _cut(want, R))


@pytest.mark.parametrize("W, A, par, floor", CONFIGS)
def test_column_0_is_the_one_repeat_entry(W, A, par, floor):
    """``min_score=1``: round 0 without a band is "Unit repeats" bit for bit, for every pair and any ``n_best``"""
    xs, ys = _batch(W, A)
    kw = dict(match=par[0], mismatch=par[1], gap=par[2])
    one = _np(local_align_unit_strings(xs, ys, **kw))
    assert (one[0] > 0).sum() == 4
    for R in (1, 7):
        got = _np(local_align_unit_strings_all(xs, ys, n_best=R, min_score=1, **kw))
        assert _same((got[0][:, 0], got[1][:, 0]), one)
    # under the default floor: the same where the score reaches it, padding where it does not
    got = _np(local_align_unit_strings_all(xs, ys, n_best=2, **kw))
    kept = one[0] >= 3 * par[0] * W
    assert np.array_equal(got[0][:, 0], np.where(kept, one[0], 0)) and np.array_equal(got[1][:, 0], np.where(kept[:, None, None], one[1], -1))


# ---- planted repeats: where a rectangle lies -----------------------------------------------------------------------------------------
M, L = 200, 190
# (rows of x, [columns of y]) of a phrase and its copies, 0-based and inclusive as the cases are named
PLANTED = {"strip edge": ((58, 72), [5, 100]), "chunk edge": ((10, 24), [25, 90]), "ring wrap": ((10, 24), [120, 60]),
           "row 0, column 0": ((0, 14), [0, 100]), "last row, last column": ((M - 15, M - 1), [L - 15, 40]),
           "three strips": ((30, 169), [40]), "shared rows": ((58, 72), [5, 150, 80])}


def _planted():
    if "planted" not in _BATCHES:
        rng = np.random.default_rng(7)
        xs, ys = [], []
        for (r0, r1), cols in PLANTED.values():
            x, y = rng.integers(0, 3, (M, 2)), rng.integers(0, 3, (L, 2))
            for b in cols:
                y[b:b + r1 - r0 + 1] = x[r0:r1 + 1]
            xs.append(x)
            ys.append(y)
        _BATCHES["planted"] = (xs, ys)
        _WANT["planted"] = aref.local_align_all_batch(xs, ys, 6)
    return _BATCHES["planted"], _WANT["planted"]


def test_planted_rectangles():
    """W = 2 over an alphabet of 3: the planted copies come first, each blocked by its rectangle in the rounds after it, and the
    rounds go on into what repeats by chance around them"""
    (xs, ys), want = _planted()
    for e, ((r0, r1), cols) in enumerate(PLANTED.values()):
        n = r1 - r0 + 1
        for r in range(len(cols)):                         # the copies: found whole or longer, the x span the same rows each time
            a0, a1 = want[1][e, r, 0]
            assert want[0][e, r] >= 4 * n and a0 <= r0 and a1 >= r1 + 1, (e, r)
        for b in cols:                                     # every copy lies in the y span of one of those rounds
            assert any(b0 <= b and b1 >= b + n for b0, b1 in want[1][e, :len(cols), 1].tolist()), (e, b)
        assert (want[0][e] >= 12).all()                    # six rounds, all found
    assert _same(_np(local_align_unit_strings_all(xs, ys, n_best=6)), want)


def test_more_rounds_than_repeats():
    """one planted phrase over an alphabet of 1000: one repeat, then padding; a floor above its score: padding only; and the stop
    at ``min_score`` among chance repeats"""
    rng = np.random.default_rng(8)
    x, y = rng.integers(0, 1000, 150), rng.integers(0, 1000, 140)
    y[70:90] = x[60:80]
    for floor in (None, 40, 41):
        want = aref.local_align_all_batch([x], [y], 7, floor)
        assert want[0][0].tolist() == ([40] + [0] * 6 if floor != 41 else [0] * 7)
        assert _same(_np(local_align_unit_strings_all([x], [y], n_best=7, min_score=floor)), want)
    x, y = rng.integers(0, 3, 150), rng.integers(0, 3, 140)
    want = aref.local_align_all_batch([x], [y], 32, 14)
    assert 0 < (want[0] > 0).sum() < 32
    assert _same(_np(local_align_unit_strings_all([x], [y], n_best=32, min_score=14)), want)


# ---- inside one string --------------------------------------------------------------------------------------------------------------
def _selves():
    rng = np.random.default_rng(9)
    three = rng.integers(0, 1000, 200)
    p = three[20:32].copy()
    three[90:102], three[150:162] = p, p                   # the third occurrence lies in another strip than the first two
    return [three, np.array([1, 2, 3] * 10), rng.integers(0, 3, 129), np.zeros(0, np.int64), np.array([5]), rng.integers(0, 3, (70, 2))[:, 0]]


@pytest.mark.parametrize("min_sep", [1, 5])
def test_repeats_inside_one_string(min_sep):
    xs = _selves()
    want = aref.local_align_all_batch(xs, None, 5, None, min_sep)
    assert want[0][0].tolist() == [24, 24, 24, 0, 0]
    assert want[1][0, :3].tolist() == [[[20, 32], [90, 102]], [[20, 32], [150, 162]], [[90, 102], [150, 162]]]
    assert want[0][1].tolist() == [54 - 6 * ((min_sep - 1) // 3), 0, 0, 0, 0]          # the tandem string: one repeat, its spans overlap
    if min_sep == 1:
        assert want[1][1, 0].tolist() == [[0, 27], [3, 30]]
    assert (want[0][2] > 0).all() and (want[0][3:5] == 0).all()
    got = _np(local_align_unit_strings_all(xs, n_best=5, min_sep=min_sep))
    assert _same(got, want)
    # ys given: min_sep is ignored, and a string against itself without a band is its diagonal
    got = _np(local_align_unit_strings_all(xs[:2], xs[:2], n_best=1, min_sep=min_sep))
    assert got[0][:, 0].tolist() == [400, 60] and got[1][:, 0].tolist() == [[[0, 200], [0, 200]], [[0, 30], [0, 30]]]


# ---- independence -------------------------------------------------------------------------------------------------------------------
def test_nothing_depends_on_chunks_stale_workspace_company_or_where_the_inputs_lie():
    xs, ys = _batch(1, 3)
    want = _cut(_want(1, 3, (2, 3, 4), None), 7)
    kw = dict(n_best=7)
    for chunk in (1, 2, 5):
        for fill in (None, 0xFF, 0x00):
            assert _same(_np(local_align_unit_strings_all(xs, ys, pair_chunk=chunk, _workspace_fill=fill, **kw)), want), (chunk, fill)
    for fill in (0xFF, 0x7F):
        assert _same(_np(local_align_unit_strings_all(xs, ys, _workspace_fill=fill, **kw)), want)
    for e in range(len(xs)):                               # a pair alone, and the pairs in another order
        got = _np(local_align_unit_strings_all(xs[e:e + 1], ys[e:e + 1], _workspace_fill=0xFF, **kw))
        assert _same(got, (want[0][e:e + 1], want[1][e:e + 1]))
    got = _np(local_align_unit_strings_all(xs[::-1], ys[::-1], **kw))
    assert _same(got, (want[0][::-1], want[1][::-1]))
    xd = [torch.from_numpy(x).cuda() for x in xs]          # device strings on one side, int32 host tensors on the other
    yt = [torch.from_numpy(y.astype(np.int32)) for y in ys]
    assert _same(_np(local_align_unit_strings_all(xd, yt, **kw)), want)
    selves, sw = _selves(), aref.local_align_all_batch(_selves(), None, 5)
    for chunk, fill in ((1, 0xFF), (4, 0x00)):
        assert _same(_np(local_align_unit_strings_all(selves, n_best=5, pair_chunk=chunk, _workspace_fill=fill)), sw)


# ---- find_repeats -------------------------------------------------------------------------------------------------------------------
LENS = (3, 70, 1, 65, 130, 200)
GROUPS = (0, 1, 2, 1, 3, 3)


def _corpus():
    """six sequences; phrase A (ids 100 ..) three times inside sequence 5, phrase B (ids 200 ..) once in sequence 1 and twice in
    sequence 4; the rest over an alphabet of 6"""
    if "corpus" not in _BATCHES:
        rng = np.random.default_rng(10)
        seqs = [rng.integers(0, 6, n) for n in LENS]
        A, B = np.arange(100, 118), np.arange(200, 220)
        fence = iter(range(300, 400))                      # a unit of its own on either side of a copy: it ends there
        for s, at, p in ((5, 10, A), (5, 75, A), (5, 170, A), (1, 40, B), (4, 5, B), (4, 100, B)):
            seqs[s][at:at + len(p)] = p
            seqs[s][at - 1], seqs[s][at + len(p)] = next(fence), next(fence)
        _BATCHES["corpus"] = seqs
    return _BATCHES["corpus"]


def _corpus_want(k, **kw):
    key = ("corpus", k, tuple(sorted(kw.items())))
    if key not in _WANT:
        _WANT[key] = aref.find_repeats(_corpus(), k, **kw)
    return _WANT[key]


def _index():
    seqs = _corpus()
    return UnitIndex(np.concatenate(seqs), groups=np.repeat(np.arange(len(LENS)), LENS))


def test_find_repeats_every_repeat(tmp_path):
    ix = _index()
    off = np.concatenate([[0], np.cumsum(LENS)])
    want = _corpus_want(12, per_pair=4, within=True)
    # the planted phrases come first: B (score 40) in (1, 4) twice and inside 4 once, then A (36) three times inside 5
    assert want[0][:6].tolist() == [40, 40, 40, 36, 36, 36] and want[1][:6].tolist() == [[1, 4], [1, 4], [4, 4], [5, 5], [5, 5], [5, 5]]
    assert (want[2][:2, 0] == off[1] + np.array([40, 60])).all() and want[2][:2, 1, 0].tolist() == [off[4] + 5, off[4] + 100]
    assert want[2][3:6, :, 0].tolist() == [[off[5] + 10, off[5] + 75], [off[5] + 10, off[5] + 170], [off[5] + 75, off[5] + 170]]
    assert (want[0] >= 6).all()
    got = _np(ix.find_repeats(12, per_pair=4, within=True))
    assert got[0].dtype == np.int32 and got[1].dtype == got[2].dtype == np.int64
    assert _same(got, want)
    for chunk, fill in ((1, 0xFF), (4, 0x00)):             # pairs per launch and per host chunk, stale workspace
        assert _same(_np(ix.find_repeats(12, per_pair=4, within=True, pair_chunk=chunk, _workspace_fill=fill)), want)
    assert _same(_np(ix.find_repeats(40, per_pair=4, within=True, min_score=14)), _corpus_want(40, per_pair=4, within=True, min_score=14))
    assert _same(_np(ix.find_repeats(12, per_pair=2, min_sep=7, within=True)), _corpus_want(12, per_pair=2, within=True, min_sep=7))
    assert _same(_np(ix.find_repeats(12, per_pair=3)), _corpus_want(12, per_pair=3))
    # with groups: (1, 3) and (4, 5) are skipped, (s, s) never
    seq_groups = list(GROUPS)
    ig = UnitIndex(np.concatenate(_corpus()), groups=np.repeat(np.array(GROUPS), LENS))
    assert ig.sequence_offsets().tolist() != off.tolist()   # 4 and 5 share a group and run together: cut them apart
    want_g = _corpus_want(12, per_pair=4, within=True, groups=tuple(seq_groups))
    assert want_g[1][:6].tolist() == want[1][:6].tolist() and not _same(want_g, want)
    assert _same(_np(ig.find_repeats(12, per_pair=4, within=True, exclude_same_group=True, sequences=off)), want_g)
    # after a save / load round trip
    path = str(tmp_path / "units.npz")
    ix.save(path)
    assert _same(_np(UnitIndex.load(path).find_repeats(12, per_pair=4, within=True)), want)
    # one sequence alone: its repeats inside
    alone = UnitIndex(_corpus()[5])
    assert _same(_np(alone.find_repeats(5, per_pair=4, within=True)), aref.find_repeats([_corpus()[5]], 5, per_pair=4, within=True))
    assert (_np(alone.find_repeats(5, per_pair=4))[0] == 0).all()


def test_find_repeats_with_the_defaults_spelled_out_is_find_repeats():
    ix = _index()
    for kw in (dict(), dict(exclude_same_group=True), dict(min_score=1, pair_chunk=3)):
        plain = _np(ix.find_repeats(9, **kw))
        assert (plain[0] > 0).sum() >= 3
        assert _same(_np(ix.find_repeats(9, per_pair=1, within=False, **kw)), plain)
        assert _same(_np(ix.find_repeats(9, per_pair=1, within=False, min_sep=4, **kw)), plain)

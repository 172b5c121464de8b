"""GPU tier of the unit repeats (sylber_amd.local_align_unit_strings / UnitIndex.find_repeats, csrc/unit_repeats.hip) against
tests/unit_repeats_ref.py: scores, pairs and spans equal bit for bit, dtype included -- everything is a small integer, no tolerance
is involved.  Shapes are the smallest at which the kernel can go wrong: strings of x around one, two and three strips of 64 rows,
strings of y around the chunk of 32 anti-diagonal steps and the 128-column ring, empty sides, widths that fill their padded row and
widths that do not, alphabets of 2 (ties everywhere) and 50, one pair of 47 strips, a planted copy whose start is carried across
six strips, and the longest string on either side."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unit_repeats_ref as rref  # noqa: E402

pytestmark = pytest.mark.gpu

from sylber_amd import UnitIndex, _lib, align_unit_strings, local_align_unit_strings  # noqa: E402
from sylber_amd import units as units_mod  # noqa: E402

MS = (0, 1, 63, 64, 65, 127, 128, 129, 200)
LS = (0, 1, 31, 32, 33, 64, 65, 96, 129, 300)
CONFIGS = [(1, 2), (2, 3), (3, 3), (8, 50)]               # (W, alphabet): W = 3 is padded to 4 words
PARAMS = [(2, 3, 4), (1, 1, 1), (3, 0, 2)]                # match, mismatch, gap
_i32p = ctypes.POINTER(ctypes.c_int32)


def _np(out):
    return tuple(o.cpu().numpy() for o in out)


def _same(a, b):
    assert len(a) == len(b)
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def _strings(rng, n, W, A):
    s = rng.integers(0, A, (n, W))
    return s[:, 0] if W == 1 else s


_BATCHES, _WANT = {}, {}


def _boundary_batch(W, A):
    """every m of MS against every L of LS; every third pair has y cut from x with 80 % of its units kept"""
    if (W, A) not in _BATCHES:
        rng = np.random.default_rng(2000 * W + A)
        xs, ys = [], []
        for m in MS:
            for L in LS:
                xs.append(_strings(rng, m, W, A))
                if m and L and (m + L) % 3 == 0:
                    base = np.resize(xs[-1], (L,) + xs[-1].shape[1:])
                    noise = _strings(rng, L, W, A)
                    keep = rng.random(L) < 0.8
                    ys.append(np.where(keep.reshape((L,) + (1,) * (base.ndim - 1)), base, noise))
                else:
                    ys.append(_strings(rng, L, W, A))
        _BATCHES[W, A] = (xs, ys)
    return _BATCHES[W, A]


def _boundary_want(W, A, par):
    """the reference's result of the batch under ``par``, made once"""
    if (W, A, par) not in _WANT:
        xs, ys = _boundary_batch(W, A)
        _WANT[W, A, par] = rref.local_align_batch(xs, ys, *par)
    return _WANT[W, A, par]


def _raw(xs, ys, W, par=(2, 3, 4), fill=None, one_buffer=False):
    """``sylber_unit_local_align`` itself, all pairs in one launch, into sentinel-filled outputs one element longer than needed
    -> (scores int32 [S], spans int32 [S, 4]); ``one_buffer``: both sides' windows point into the same buffer"""
    from sylber_amd.kmeans import _stream, _vp
    lib, dev = _lib.load(), torch.device("cuda", torch.cuda.current_device())

    def flat(strings, base=0):
        lens = np.array([len(s) for s in strings], np.int64)
        win = np.stack([base + np.cumsum(lens) - lens, lens], 1).astype(np.int32)
        rows = np.concatenate([np.asarray(s, np.int64).reshape(len(s), W) for s in strings] + [np.zeros((1, W), np.int64)])
        return rows.astype(np.int32), np.ascontiguousarray(win)

    xr, xw = flat(xs)
    yr, yw = flat(ys, base=len(xr) if one_buffer else 0)
    if one_buffer:
        xd = yd = torch.from_numpy(np.concatenate([xr, yr])).to(dev)
    else:
        xd, yd = torch.from_numpy(xr).to(dev), torch.from_numpy(yr).to(dev)
    S = len(xs)
    score = torch.full((S + 1,), 7, dtype=torch.int32, device=dev)
    span = torch.full((4 * S + 1,), 7, dtype=torch.int32, device=dev)
    size = int(lib.sylber_unit_local_workspace_bytes(xw.ctypes.data_as(_i32p), yw.ctypes.data_as(_i32p), S))
    assert size > 0
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    with torch.cuda.device(dev):
        _lib.check(lib.sylber_unit_local_align(_vp(xd), xd.shape[0], _vp(yd), yd.shape[0], W, xw.ctypes.data_as(_i32p),
                                               yw.ctypes.data_as(_i32p), S, par[0], par[1], par[2], _vp(score), _vp(span), _vp(ws),
                                               _stream(dev)), "sylber_unit_local_align")
    score, span = score.cpu().numpy(), span.cpu().numpy()
    assert score[S] == 7 and span[4 * S] == 7              # nothing past the last pair
    return score[:S], span[:4 * S].reshape(S, 4)


# ---- one call with every boundary ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("par", PARAMS)
@pytest.mark.parametrize("W, A", CONFIGS)
def test_one_call_with_every_boundary(W, A, par):
    xs, ys = _boundary_batch(W, A)
    want = _boundary_want(W, A, par)
    assert (want[0] > 0).sum() >= 20 and (want[0] == 0).sum() >= 18          # the pairs cut from x; the pairs with an empty side
    got = _np(local_align_unit_strings(xs, ys, match=par[0], mismatch=par[1], gap=par[2]))
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and got[1].shape == (len(xs), 2, 2)
    assert _same(got, want)
    for one_buffer in (False, True):
        score, span = _raw(xs, ys, W, par, one_buffer=one_buffer)
        assert np.array_equal(score, want[0]) and np.array_equal(span.reshape(-1, 2, 2), want[1])


@pytest.mark.parametrize("W, A", CONFIGS)
def test_against_the_existing_kernel(W, A):
    """under the defaults: score == W * (len_x + len_y) - 5 * cost, cost = ``align_unit_strings`` of the two returned spans"""
    xs, ys = _boundary_batch(W, A)
    scores, spans = _np(local_align_unit_strings(xs, ys))
    pick = np.nonzero(scores > 0)[0]
    assert len(pick) >= 20                                 # the pairs with y cut from x at least
    assert (spans[pick, :, 0] < spans[pick, :, 1]).all() and (spans[pick] >= 0).all()      # both spans are non-empty
    assert (spans[scores == 0] == -1).all()
    sx = [np.asarray(xs[s])[spans[s, 0, 0]:spans[s, 0, 1]] for s in pick]
    sy = [np.asarray(ys[s])[spans[s, 1, 0]:spans[s, 1, 1]] for s in pick]
    _, costs = _np(align_unit_strings(sx, sy))
    lens = (spans[pick, :, 1] - spans[pick, :, 0]).sum(1)
    assert np.array_equal(scores[pick].astype(np.int64), W * lens - 5 * costs.astype(np.int64))


# ---- long strings -------------------------------------------------------------------------------------------------------------------
def test_one_pair_of_47_strips():
    rng = np.random.default_rng(5)
    x, y = rng.integers(0, 2, 3000), rng.integers(0, 2, 2900)      # two symbols: ties everywhere
    want = rref.local_align_batch([x], [y])
    assert want[0][0] > 0
    assert _same(_np(local_align_unit_strings([x], [y])), want)
    score, span = _raw([x], [y], 1, fill=0xFF)
    assert np.array_equal(score, want[0]) and np.array_equal(span.reshape(-1, 2, 2), want[1])


def test_a_start_carried_across_six_strips():
    rng = np.random.default_rng(6)
    x, y = rng.integers(0, 50, (1500, 2)), rng.integers(0, 50, (700, 2))
    y[200:600] = x[1000:1400]
    y[199], y[600] = (x[999] + 1) % 50, (x[1400] + 1) % 50         # the copy is maximal
    scores, spans = _np(local_align_unit_strings([x], [y]))
    assert scores.tolist() == [2 * 2 * 400] and spans.tolist() == [[[1000, 1400], [200, 600]]]
    assert _same((scores, spans), rref.local_align_batch([x], [y]))


@pytest.mark.parametrize("m, L", [(65536, 70), (70, 65536)])
def test_the_longest_string_on_either_side(m, L):
    rng = np.random.default_rng(m % 7)
    x, y = rng.integers(0, 3, (m, 2)), rng.integers(0, 3, (L, 2))
    want = rref.local_align_batch([x], [y])
    assert want[0][0] > 0
    assert _same(_np(local_align_unit_strings([x], [y])), want)


# ---- independence -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    """40 pairs over two symbols, from empty to four strips, with their reference result"""
    rng = np.random.default_rng(7)
    ms = rng.integers(0, 260, 40)
    Ls = rng.integers(0, 200, 40)
    ms[3], Ls[5], ms[8], Ls[8] = 0, 0, 0, 0
    xs = [rng.integers(0, 2, int(m)) for m in ms]
    ys = [rng.integers(0, 2, int(L)) for L in Ls]
    return xs, ys, rref.local_align_batch(xs, ys)


def test_nothing_depends_on_chunks_order_company_or_the_workspace(mixed, monkeypatch):
    xs, ys, want = mixed
    S = len(xs)
    assert _same(_np(local_align_unit_strings(xs, ys)), want)
    for kw in (dict(pair_chunk=1), dict(pair_chunk=7), dict(_workspace_fill=0x00), dict(_workspace_fill=0xFF),
               dict(pair_chunk=7, _workspace_fill=0xFF), dict(pair_chunk=1000)):
        assert _same(_np(local_align_unit_strings(xs, ys, **kw)), want), kw
    # launches cut by the workspace bound, not by pair_chunk
    need = units_mod.unit_local_workspace_bytes([len(x) for x in xs], [len(y) for y in ys])
    with monkeypatch.context() as mp:
        mp.setattr(units_mod, "ALIGN_WORKSPACE_BYTES", int(need.max()) + 40 + 256 + 4096)
        assert _same(_np(local_align_unit_strings(xs, ys, _workspace_fill=0xFF)), want)
    perm = np.random.default_rng(8).permutation(S)
    got = _np(local_align_unit_strings([xs[s] for s in perm], [ys[s] for s in perm]))
    assert np.array_equal(got[0], want[0][perm]) and np.array_equal(got[1], want[1][perm])
    for s in range(S):                                     # each pair alone
        got = _np(local_align_unit_strings([xs[s]], [ys[s]]))
        assert got[0][0] == want[0][s] and np.array_equal(got[1][0], want[1][s]), s
    for fill in (0x00, 0xFF):
        score, span = _raw(xs, ys, 1, fill=fill)
        assert np.array_equal(score, want[0]) and np.array_equal(span.reshape(-1, 2, 2), want[1])


def test_inputs_on_the_device_and_in_either_form(mixed):
    xs, ys, want = mixed
    dev = [torch.from_numpy(np.asarray(x)).cuda() for x in xs]
    wide = [np.asarray(y).reshape(-1, 1).astype(np.int32) for y in ys]
    assert _same(_np(local_align_unit_strings(dev, wide)), want)
    mixed_in = [d if i % 2 else x for i, (d, x) in enumerate(zip(dev, xs))]
    assert _same(_np(local_align_unit_strings(mixed_in, [{"units": y} for y in ys])), want)
    assert _same(_np(local_align_unit_strings(tuple(xs), tuple(ys), device="cuda:0")), want)


def _no_launch(monkeypatch):
    def refuse(*a):
        raise AssertionError("a launch")
    monkeypatch.setattr(_lib.load(), "sylber_unit_local_align", refuse)


def test_no_pairs_no_launch(monkeypatch):
    _no_launch(monkeypatch)
    scores, spans = local_align_unit_strings([], [])
    assert scores.shape == (0,) and spans.shape == (0, 2, 2) and scores.dtype == torch.int32 and spans.dtype == torch.int64
    assert scores.is_cuda and spans.is_cuda
    ix = UnitIndex(np.arange(9), groups=np.zeros(9, np.int32))      # one sequence: no pair
    scores, pairs, spans = ix.find_repeats(3)
    assert scores.tolist() == [0] * 3 and pairs.tolist() == [[-1, -1]] * 3 and spans.tolist() == [[[-1, -1]] * 2] * 3
    assert scores.dtype == torch.int32 and pairs.dtype == spans.dtype == torch.int64 and scores.is_cuda
    ix = UnitIndex(np.arange(9), groups=np.array([0, 0, 0, 1, 1, 2, 2, 2, 0], np.int32))
    assert ix.find_repeats(2, sequences=np.array([0, 9]))[0].tolist() == [0, 0]


# ---- find_repeats -------------------------------------------------------------------------------------------------------------------
W_CORPUS = 2
LENS = (40, 5, 150, 1, 33, 64, 90, 70, 12, 129, 25, 48)
GROUPS = (0, 1, 2, 3, 4, 5, 6, 2, 8, 9, 10, 11)           # sequences 2 and 7 share a group


def _corpus():
    rng = np.random.default_rng(9)
    seqs = [rng.integers(0, 6, (n, W_CORPUS)) for n in LENS]
    seqs[9][100:106] = seqs[0][10:16]
    seqs[7][40:60] = seqs[2][30:50]
    seqs[10][11:21] = seqs[4][3:13]
    return seqs


@pytest.fixture(scope="module")
def corpus():
    seqs = _corpus()
    u = np.concatenate(seqs)
    g = np.repeat(np.array(GROUPS, np.int32), LENS)
    return seqs, u, g, UnitIndex(u, groups=g)


def _held(got, want):
    got = _np(got)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and got[2].dtype == np.int64
    assert _same(got, want), (got, want)


def test_find_repeats_against_the_reference(corpus):
    seqs, u, g, ix = corpus
    assert len(seqs) == 12 and min(LENS) == 1 and max(LENS) == 150
    assert np.array_equal(ix.sequence_offsets(), np.concatenate([[0], np.cumsum(LENS)]))
    full = rref.find_repeats(seqs, 100)
    kept = int((full[0] > 0).sum())
    assert 3 < kept < 66                                   # k = 100 pads, k = 3 cuts
    found = {tuple(p) for p in full[1][:kept].tolist()}
    assert {(0, 9), (2, 7), (4, 10)} <= found              # the three planted repeats
    assert full[0][0] >= 2 * W_CORPUS * 20 and tuple(full[1][0]) == (2, 7)
    for k in (1, 3, kept, 100):
        _held(ix.find_repeats(k), rref.find_repeats(seqs, k))
    for ms in (1, 13, 30, 10 ** 6):
        _held(ix.find_repeats(20, min_score=ms), rref.find_repeats(seqs, 20, min_score=ms))
    for par in ((1, 1, 1), (3, 0, 2)):
        _held(ix.find_repeats(20, match=par[0], mismatch=par[1], gap=par[2]), rref.find_repeats(seqs, 20, None, *par))
    got = ix.find_repeats(20, exclude_same_group=True)
    _held(got, rref.find_repeats(seqs, 20, groups=GROUPS))
    assert [2, 7] not in got[1].tolist() and [2, 7] in ix.find_repeats(20)[1].tolist()
    for kw in (dict(pair_chunk=1), dict(pair_chunk=7), dict(pair_chunk=1000), dict(_workspace_fill=0x00), dict(_workspace_fill=0xFF),
               dict(pair_chunk=5, _workspace_fill=0xFF)):
        _held(ix.find_repeats(20, **kw), rref.find_repeats(seqs, 20))


def test_find_repeats_in_chunks_of_the_enumeration(corpus, monkeypatch):
    seqs, u, g, ix = corpus
    monkeypatch.setattr(units_mod, "REPEAT_PAIRS", 10)
    _held(ix.find_repeats(4), rref.find_repeats(seqs, 4))
    _held(ix.find_repeats(100, exclude_same_group=True), rref.find_repeats(seqs, 100, groups=GROUPS))


def test_find_repeats_with_other_cuts(corpus):
    seqs, u, g, ix = corpus
    N = len(u)
    off = np.array([0, 100, 101, 230, 400, 520, N])
    cut = [u[a:b] for a, b in zip(off[:-1], off[1:])]
    grp = g[off[:-1]]
    _held(ix.find_repeats(10, sequences=off), rref.find_repeats(cut, 10, offsets=off))
    _held(ix.find_repeats(10, sequences=torch.from_numpy(off), exclude_same_group=True),
          rref.find_repeats(cut, 10, groups=grp, offsets=off))


def test_find_repeats_after_many_adds_and_a_round_trip(corpus, tmp_path):
    seqs, u, g, ix = corpus
    want = rref.find_repeats(seqs, 20)
    many = UnitIndex(width=W_CORPUS)
    for s, grp in zip(seqs, GROUPS):
        many.add(s, groups=np.full(len(s), grp, np.int32))
    _held(many.find_repeats(20), want)
    path = str(tmp_path / "units.npz")
    ix.save(path)
    _held(UnitIndex.load(path).find_repeats(20), want)


def test_the_spans_feed_provenance_and_align_phrases(corpus):
    """the spans are row ids: ``provenance`` takes them, and for the repeats of at most 64 units the global alignment of the x span
    against the y span costs ``(W * (len_x + len_y) - score) / 5``"""
    seqs, u, g, ix = corpus
    scores, pairs, spans = _np(ix.find_repeats(100))
    kept = int((scores > 0).sum())
    off = ix.sequence_offsets()
    phrases, windows, want = [], [], []
    for r in range(kept):
        (a0, a1), (b0, b1) = spans[r].tolist()
        s, t = pairs[r].tolist()
        assert off[s] <= a0 < a1 <= off[s + 1] and off[t] <= b0 < b1 <= off[t + 1]
        assert len(ix.provenance(range(a0, a1))) == a1 - a0 and len(ix.provenance(range(b0, b1))) == b1 - b0
        if a1 - a0 <= 64:
            phrases.append(u[a0:a1])
            windows.append([[b0, b1]])
            total = W_CORPUS * ((a1 - a0) + (b1 - b0)) - int(scores[r])
            assert total % 5 == 0
            want.append(total // 5)
    assert len(phrases) >= 3 and 20 in [len(p) for p in phrases]
    costs = ix.align_phrases(phrases, torch.tensor(windows), free_start=False)[3].cpu().numpy()
    assert costs[:, 0].tolist() == want


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(corpus, monkeypatch):
    _no_launch(monkeypatch)
    one = [np.array([1, 2, 3])]
    for kw, name, lo in ((dict(match=0), "match", 1), (dict(match=65), "match", 1), (dict(mismatch=-1), "mismatch", 0),
                         (dict(mismatch=65), "mismatch", 0), (dict(gap=0), "gap", 1), (dict(gap=65), "gap", 1), (dict(gap=1.0), "gap", 1)):
        with pytest.raises(ValueError, match=r"%s must be an integer in \[%d, 64\]" % (name, lo)):
            local_align_unit_strings(one, one, **kw)
        with pytest.raises(ValueError, match=r"%s must be an integer in \[%d, 64\]" % (name, lo)):
            corpus[3].find_repeats(3, **kw)
    with pytest.raises(ValueError, match="equally long, got 1 and 2"):
        local_align_unit_strings(one, one * 2)
    with pytest.raises(ValueError, match="xs have W = 1, ys have W = 2"):
        local_align_unit_strings(one, [np.zeros((2, 2), np.int64)])
    with pytest.raises(ValueError, match="expected W = 2, got 3"):
        local_align_unit_strings([np.zeros((2, 2), np.int64), np.zeros((2, 3), np.int64)], one * 2)
    for bad in (np.array([0.5, 1.0]), np.array([True, False]), torch.tensor([1.0], device="cuda")):
        with pytest.raises(ValueError, match="must be integers"):
            local_align_unit_strings(one, [bad])
    for bad in (np.array([1, -1]), torch.tensor([3, -2], device="cuda"), np.array([2 ** 31])):
        with pytest.raises(ValueError, match=r"unit ids lie in \[0, 2\*\*31 - 1\]"):
            local_align_unit_strings([bad], one)
    with pytest.raises(ValueError, match="ys\\[0\\] has 65537 units, more than 65536"):
        local_align_unit_strings(one, [np.zeros(65537, np.int64)])
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="pair_chunk must be an integer >= 1"):
            local_align_unit_strings(one, one, pair_chunk=bad)
        with pytest.raises(ValueError, match="pair_chunk must be an integer >= 1"):
            corpus[3].find_repeats(3, pair_chunk=bad)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="k must be an integer >= 1"):
            corpus[3].find_repeats(bad)
    for bad in (0, -5, 2.5, True):
        with pytest.raises(ValueError, match="min_score must be None or an integer >= 1"):
            corpus[3].find_repeats(3, min_score=bad)
    with pytest.raises(ValueError, match="the index is empty"):
        UnitIndex(width=2).find_repeats(3)
    with pytest.raises(ValueError, match="a sequence has 65537 rows, more than 65536"):
        UnitIndex(np.zeros(65537, np.int64)).find_repeats(3)
    with pytest.raises(ValueError, match="sequences must ascend"):
        corpus[3].find_repeats(3, sequences=np.array([0, 5, 5, len(corpus[1])]))


def test_the_raw_entry_refuses_bad_arguments():
    """no pointer that the device would dereference is passed: every case is refused on the host"""
    lib = _lib.load()
    p = 4096

    def win(v):
        a = np.ascontiguousarray(v, np.int32)
        return a, a.ctypes.data_as(_i32p)

    good = dict(x=p, x_rows=100, y=p, y_rows=80, W=2, xw=[[0, 3], [90, 10]], yw=[[70, 10], [0, 80]], pairs=2, match=2, mismatch=3, gap=4,
                score=p, span=p, ws=p, stream=None)
    for case in (dict(x=None), dict(y=None), dict(xw=None), dict(yw=None), dict(score=None), dict(span=None), dict(ws=None), dict(W=0),
                 dict(W=9), dict(pairs=0), dict(match=0), dict(match=65), dict(mismatch=-1), dict(mismatch=65), dict(gap=0), dict(gap=65),
                 dict(xw=[[0, 3], [91, 10]]), dict(yw=[[-1, 10], [0, 80]]), dict(yw=[[70, 10], [0, 81]]),
                 dict(x_rows=70000, xw=[[0, 3], [0, 65537]])):
        a = dict(good, **case)
        keep = [win(a[k]) if a[k] is not None else (None, None) for k in ("xw", "yw")]
        a["xw"], a["yw"] = keep[0][1], keep[1][1]
        assert lib.sylber_unit_local_align(*a.values()) == 1, case
        assert lib.sylber_last_error().decode().startswith("sylber_unit_local_align: "), case

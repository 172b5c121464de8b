"""GPU tier, embedding strings (csrc/dtw_strings.hip behind ``align_sequences`` and ``SyllableIndex.align_sequences``), bitwise against
tests/dtw_strings_ref.py.  The local costs come from numpy where they are exact (integer rows under L2) and otherwise from the
library's fp32 search on pieces of at most 128 rows, as tests/test_gpu_align.py takes them (``test_gpu_phrase._local_costs``: code from
before this kernel, never the code under test); the fp32 global DP and the walk of dtw_strings_ref run over them, and the call must
return exactly those cost bits, steps and runs.

Shapes (m, L): one cell, one row, one column, inside one strip and tile, exactly one strip and tile (64, 128), the second strip and
the second tile (65, 129), a whole super-strip (128, 128), the second super-strip with its carried rows in the workspace (129, 127),
three super-strips with a short last one over three tiles (300, 257).

A stale window table cannot be produced by a caller: the windows are host arrays that the entry checks and copies into the table
itself before the launch, so there is no test of one."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dtw_ref as R
import dtw_strings_ref as G
from test_gpu_phrase import _groups_of, _local_costs, _np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((1, 1), (1, 40), (40, 1), (33, 40), (64, 128), (65, 129), (128, 128), (129, 127), (300, 257))
SHAPES_768 = ((33, 40), (65, 129), (129, 127))


def _pieces(L):
    return np.array(sorted(set(list(range(0, L, 128)) + [L])), np.int64)


@functools.lru_cache(maxsize=None)
def _case(D, integer, metric):
    """the pairs of one group with their reference, computed once: (xs, ys, d per pair, reference of align_sequences)"""
    rng = np.random.default_rng(D + 7 * integer)
    xs, ys, ds = [], [], []
    for m, L in (SHAPES if D == 32 else SHAPES_768):
        if integer:
            x, y = (rng.integers(-2, 3, (n, D)).astype(np.float32) for n in (m, L))
        else:
            x, y = (rng.standard_normal((n, D)).astype(np.float32) for n in (m, L))
            if m > 1 and L > 1:                                   # the two recordings say the same thing at different speeds
                y = (x[np.minimum(np.arange(L) * m // L, m - 1)] + 0.5 * y).astype(np.float32)
        if L >= 30:
            y[10:20] = y[9]                                       # a run of equal rows: ties along a row of the DP
        if integer and metric == "l2":                            # every term is a small integer: numpy is exact and needs nothing from the GPU
            xn, yn = (x * x).sum(1), (y * y).sum(1)
            d = np.maximum(np.float32(0), xn[:, None] + (np.float32(-2) * (x @ y.T) + yn[None, :])).astype(np.float32)
        else:
            d = _local_costs(y, _pieces(L), x, metric)
        xs.append(x); ys.append(y); ds.append(d)
    ref = G.align_sequences(lambda s: ds[s], [len(x) for x in xs], [len(y) for y in ys])
    return xs, ys, ds, ref


def _assert_same(got, ref):
    rows, costs, steps, xo = got
    assert rows.dtype == torch.int64 and costs.dtype == torch.float32 and steps.dtype == torch.int32 and xo.dtype == torch.int64
    assert rows.device.type == "cuda" and costs.device.type == "cuda"
    assert np.array_equal(_np(costs).view(np.uint32), ref[1].astype(np.float32).view(np.uint32))
    assert np.array_equal(_np(steps), ref[2])
    assert np.array_equal(_np(rows), ref[0])
    assert np.array_equal(_np(xo), ref[3])


def _equal(a, b, what=None):
    assert len(a) == len(b)
    for s, t in zip(a, b):
        assert s.dtype == t.dtype and s.shape == t.shape and torch.equal(s.contiguous().view(-1).view(torch.uint8), t.contiguous().view(-1).view(torch.uint8)), what


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,integer", [(32, True), (32, False), (768, False)])
def test_bitwise_against_the_contract(D, integer, metric):
    from sylber_amd import align_sequences
    xs, ys, ds, ref = _case(D, integer, metric)
    got = align_sequences(xs, ys, metric=metric, path=True, device=DEV, _steps_walk=True)
    _assert_same(got[:4], ref)
    assert torch.equal(got[4], got[2])                            # the walk over the codes counts the cells that formed them
    steps = _np(got[2])
    for s, (x, y) in enumerate(zip(xs, ys)):
        assert max(len(x), len(y)) <= steps[s] <= len(x) + len(y) - 1
    costs, csteps = align_sequences(xs, ys, metric=metric, device=DEV)       # counts only: no codes, the same cells
    assert torch.equal(costs.view(torch.int32), got[1].view(torch.int32)) and torch.equal(csteps, got[2])
    xo = ref[3]
    for s in range(len(xs)):                                      # one pair per call
        rows, c, n, _ = align_sequences(xs[s:s + 1], ys[s:s + 1], metric=metric, path=True, device=DEV)
        assert torch.equal(rows, got[0][xo[s]:xo[s + 1]]) and torch.equal(c.view(torch.int32), got[1][s:s + 1].view(torch.int32))
        assert torch.equal(n, got[2][s:s + 1])


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D", [32, 768])
def test_costs_against_float64(D, metric):
    """Gaussian rows: |cost32 - cost64| within ``dtw_strings_ref.cost_error_bound``, which is derived there (per-cell rounding of the
    chain and of dt_cost, one rounding per addition along a path), not fitted; the float64 DP runs on the rows as the kernel reads
    them"""
    from sylber_amd import align_sequences
    from sylber_amd._index import _prep
    xs, ys, _, _ = _case(D, False, metric)
    costs, steps = align_sequences(xs, ys, metric=metric, device=DEV)
    costs = _np(costs).astype(np.float64)
    for s, (x, y) in enumerate(zip(xs, ys)):
        xp, yp = (_np(_prep(torch.from_numpy(a), metric, torch.device(DEV))) for a in (x, y))
        cost64 = G.align(R.local_costs(xp, yp, metric), np.float64)[0]
        bound = G.cost_error_bound(xp, yp, cost64, metric)
        print("D=%d %s %dx%d: cost32 %.9g cost64 %.9g |diff| %.3g bound %.3g" % (D, metric, len(x), len(y), costs[s], cost64, abs(costs[s] - cost64), bound))
        assert abs(costs[s] - cost64) <= bound
        assert bound < 1e-2 * max(cost64, 1.0)                    # and the bound says something


@functools.lru_cache(maxsize=None)
def _searched(metric):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(21)
    lens = [90, 40, 130, 7, 70]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N, D = int(offsets[-1]), 32
    x = rng.standard_normal((N, D)).astype(np.float32)
    phrases = []
    for m, a in ((5, 20), (33, 100), (64, 150)):
        p = x[a:a + m + 1].copy() + 0.2 * rng.standard_normal((m + 1, D)).astype(np.float32)
        phrases.append(np.delete(p, m // 2, 0))                  # a row left out: the match has to warp
    return x, offsets, phrases, SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_the_theorem_on_spans_of_a_phrase_search(metric):
    """phrases of 5, 33 and 64 rows: on every span ``search_phrases`` returns, the global alignment of the phrase against those rows is
    ``align_phrases``'s -- cost bits, steps, runs; on windows that are no span its cost is at least ``align_phrases``'s"""
    from sylber_amd import align_sequences
    x, offsets, phrases, idx = _searched(metric)
    k = 3
    costs, seqs, spans = idx.search_phrases(phrases, k)
    rows, steps, acost = idx.align_phrases(phrases, spans)
    sp, hit = _np(spans), _np(seqs) >= 0
    assert hit.all()
    xs = [phrases[p] for p in range(len(phrases)) for r in range(k)]
    ys = [x[sp[p, r, 0]:sp[p, r, 1]] for p in range(len(phrases)) for r in range(k)]
    grows, gcost, gsteps, xo = align_sequences(xs, ys, metric=metric, path=True, device=DEV)
    assert torch.equal(gcost.view(torch.int32), acost.reshape(-1).view(torch.int32))
    assert torch.equal(gcost.view(torch.int32), costs.reshape(-1).view(torch.int32))
    assert torch.equal(gsteps, steps.reshape(-1))
    grows, xo = _np(grows), _np(xo)
    for p in range(len(phrases)):
        for r in range(k):
            e, m = p * k + r, len(phrases[p])
            assert np.array_equal(grows[xo[e]:xo[e + 1]] + sp[p, r, 0], _np(rows[p, r, :m])), (p, r)
    # windows that are no span: wider on both sides, and cut short
    wide = np.stack([np.maximum(sp[..., 0] - 3, 0), np.minimum(sp[..., 1] + 2, len(x))], -1)
    short = np.stack([sp[..., 0], np.maximum(sp[..., 0] + 1, sp[..., 1] - 2)], -1)
    for win in (wide, short):
        _, _, wcost = idx.align_phrases(phrases, win)
        ys = [x[win[p, r, 0]:win[p, r, 1]] for p in range(len(phrases)) for r in range(k)]
        gc, _ = align_sequences(xs, ys, metric=metric, device=DEV)
        assert (gc >= wcost.reshape(-1)).all() and torch.isfinite(gc).all()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_the_index_method_is_the_free_function_on_its_rows(metric):
    from sylber_amd import IVFSyllableIndex, align_sequences
    x, offsets, _, idx = _searched(metric)
    pairs = np.array([[0, 1], [2, 4], [2, 2], [3, 0], [4, 2], [1, 1]], np.int64)
    xs = [x[offsets[a]:offsets[a + 1]] for a, _ in pairs]
    ys = [x[offsets[b]:offsets[b + 1]] for _, b in pairs]
    want = align_sequences(xs, ys, metric=metric, path=True, device=DEV)
    got = idx.align_sequences(pairs, path=True)
    shift = torch.from_numpy(np.repeat(offsets[pairs[:, 1]], [len(a) for a in xs])).to(DEV)[:, None]
    _equal((got[0] - shift,) + got[1:], want)
    assert int(got[0][0, 0]) == offsets[1] and int(got[0][-1, 1]) == offsets[2]          # row ids of the index
    _equal(idx.align_sequences(pairs), want[1:3])
    _equal(idx.align_sequences(torch.from_numpy(pairs).to(DEV), path=True, pair_chunk=2), got)
    cut = np.array([0, 64, 200, len(x)], np.int64)                # explicit sequences
    a = idx.align_sequences([[0, 1], [1, 2]], path=True, sequences=cut)
    b = align_sequences([x[0:64], x[64:200]], [x[64:200], x[200:]], metric=metric, path=True, device=DEV)
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2])
    ivf = IVFSyllableIndex.build(idx, 4, seed=1)
    _equal(ivf.align_sequences(pairs, path=True), got)


def test_nan_rows_and_empty_sides_are_padding():
    from sylber_amd import align_sequences
    rng = np.random.default_rng(5)
    D = 32
    mk = lambda n: rng.standard_normal((n, D)).astype(np.float32)
    xs, ys = [mk(70), mk(70), mk(0), mk(5), mk(0), mk(140), mk(9)], [mk(150), mk(150), mk(5), mk(0), mk(0), mk(30), mk(9)]
    ys[5][7] = np.inf                                             # inf - inf in the norms: NaN costs
    for metric in ("l2", "cosine"):
        # a NaN row as the kernel reads it.  Under "cosine" the rows pass through sylber_knn_unit_rows first, as in every cosine
        # search of the library: it keeps a row whose squared norm is not above 0 -- a row with a NaN in it too -- as the zero
        # row, and turns a row of inf into a NaN row; the entry itself is held on NaN rows under IP below
        xs[0][66] = np.nan if metric == "l2" else np.inf         # a NaN row of x in the second strip: every path crosses it
        ys[1][140] = np.nan if metric == "l2" else np.inf        # a NaN row of y in the second tile
        rows, costs, steps, xo = align_sequences(xs, ys, metric=metric, path=True, device=DEV, _steps_walk=True)[:4]
        assert torch.isposinf(costs[:6]).all() and (steps[:6] == 0).all() and (rows[:int(xo[6])] == -1).all()
        assert torch.isfinite(costs[6]) and int(steps[6]) >= 9 and (rows[int(xo[6]):] >= 0).all()
        c2, s2 = align_sequences(xs, ys, metric=metric, device=DEV)
        assert torch.equal(c2.view(torch.int32), costs.view(torch.int32)) and torch.equal(s2, steps)
        assert xo.tolist() == [0, 70, 140, 140, 145, 145, 285, 294]
    # the entry under IP on a buffer of unit rows with one NaN row (row 12): in x's window, in y's window, in neither
    from sylber_amd import _lib
    from sylber_amd.kmeans import _stream, _vp
    lib, dev = _lib.load(), torch.device(DEV)
    u = mk(40)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u[12, 5] = np.nan
    buf = torch.from_numpy(u).to(dev)
    xw, yw = np.array([[10, 5], [20, 6], [20, 6]], np.int32), np.array([[20, 9], [5, 10], [30, 10]], np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    ws = torch.empty(int(lib.sylber_dtw_strings_workspace_bytes(xw.ctypes.data_as(i32p), yw.ctypes.data_as(i32p), 3, 0)), dtype=torch.uint8, device=dev)
    steps, costs = torch.full((3,), 7, dtype=torch.int32, device=dev), torch.zeros(3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        assert lib.sylber_dtw_strings_align(_vp(buf), 40, None, _vp(buf), 40, None, 32, 1, xw.ctypes.data_as(i32p), yw.ctypes.data_as(i32p), 3, 0,
                                            None, None, _vp(steps), _vp(costs), None, _vp(ws), _stream(dev)) == 0
    assert torch.isposinf(costs[:2]).all() and steps.tolist()[:2] == [0, 0] and torch.isfinite(costs[2]) and 10 <= int(steps[2]) <= 15


def test_invariance_is_bitwise():
    from sylber_amd import align_sequences
    from sylber_amd import _lib
    from sylber_amd._index import _row_norms
    from sylber_amd.kmeans import _stream, _vp
    xs, ys, _, _ = _case(32, True, "l2")
    base = align_sequences(xs, ys, path=True, device=DEV)
    counts = align_sequences(xs, ys, device=DEV)
    for kw in ({"pair_chunk": 1}, {"pair_chunk": 3}, {"_workspace_fill": 0x00}, {"_workspace_fill": 0xFF}, {"pair_chunk": 3, "_workspace_fill": 0xFF}):
        _equal(base, align_sequences(xs, ys, path=True, device=DEV, **kw), kw)
        _equal(counts, align_sequences(xs, ys, device=DEV, **kw), kw)
    xd, yd = [torch.from_numpy(a).to(DEV) for a in xs], [torch.from_numpy(a).double() for a in ys]
    _equal(base, align_sequences(xd, yd, path=True, device=DEV), "device and float64 host inputs")
    order = [8, 0, 7, 3, 5, 1, 6, 2, 4]                           # the order of the pairs
    perm = align_sequences([xs[s] for s in order], [ys[s] for s in order], path=True, device=DEV)
    xo, po = _np(base[3]), _np(perm[3])
    for e, s in enumerate(order):
        assert torch.equal(perm[0][po[e]:po[e + 1]], base[0][xo[s]:xo[s + 1]]), s
        assert torch.equal(perm[1][e:e + 1].view(torch.int32), base[1][s:s + 1].view(torch.int32)) and perm[2][e] == base[2][s]
    # x and y windows in ONE shared buffer, overlapping and repeated, straight through the entry
    lib, dev = _lib.load(), torch.device(DEV)
    buf = torch.from_numpy(np.concatenate([xs[8], ys[8]])).to(dev)               # 300 + 257 rows
    nrm = _row_norms(buf)
    xw = np.array([[0, 300], [100, 150], [100, 150], [200, 129]], np.int32)
    yw = np.array([[300, 257], [150, 200], [100, 150], [0, 557]], np.int32)
    ro = np.array([0, 300, 450, 600], np.int64)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    size = int(lib.sylber_dtw_strings_workspace_bytes(xw.ctypes.data_as(i32p), yw.ctypes.data_as(i32p), 4, 1))
    assert size == 256 + sum(G.workspace_bytes(int(m), int(L), True) for m, L in zip(xw[:, 1], yw[:, 1]))
    outs = []
    for fill in (0x00, 0xFF):
        ws = torch.full((size,), fill, dtype=torch.uint8, device=dev)
        rows = torch.full((729, 2), 7, dtype=torch.int32, device=dev)
        steps, walk = torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        costs = torch.zeros(4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            assert lib.sylber_dtw_strings_align(_vp(buf), 557, _vp(nrm), _vp(buf), 557, _vp(nrm), 32, 0, xw.ctypes.data_as(i32p),
                                                yw.ctypes.data_as(i32p), 4, 1, ro.ctypes.data_as(i64p), _vp(rows), _vp(steps), _vp(costs),
                                                _vp(walk), _vp(ws), _stream(dev)) == 0
        assert torch.equal(walk, steps)
        outs.append((rows, steps, costs))
    _equal(*outs)
    rows, steps, costs = outs[0]
    b = _np(buf)
    want = align_sequences([b[a:a + n] for a, n in xw], [b[a:a + n] for a, n in yw], path=True, device=DEV)
    _equal((rows.to(torch.int64), costs, steps), want[:3])
    assert torch.equal(costs[:1].view(torch.int32), base[1][8:9].view(torch.int32)) and float(costs[2]) == 0.0 and int(steps[2]) == 150


def test_every_refusal_comes_before_a_launch(monkeypatch):
    from sylber_amd import SyllableIndex, _lib, align_sequences
    from sylber_amd import search as S
    rng = np.random.default_rng(10)
    x = rng.standard_normal((40, 16)).astype(np.float32)
    idx = SyllableIndex(x, groups=np.repeat(np.arange(4), 10), device=DEV)
    lib = _lib.load()

    def fail(*a):
        raise AssertionError("launched")
    entries = {"sylber_dtw_strings_align", "sylber_dtw_strings_workspace_bytes", "sylber_knn_row_norms", "sylber_knn_unit_rows"}
    monkeypatch.setattr(_lib, "_LIB", type("L", (), {"__getattr__": lambda self, n: fail if n in entries else getattr(lib, n)})())
    a, b = [x[:3]], [x[3:9]]
    bad = [dict(xs=a + a, ys=b), dict(xs=a, ys=[np.zeros((4, 32), np.float32)]), dict(xs=[np.zeros((4, 24), np.float32)], ys=[np.zeros((4, 24), np.float32)]),
           dict(xs=[np.zeros((4, 8), np.float32)], ys=[np.zeros((4, 8), np.float32)]), dict(xs=[x[:3].astype(np.int32)], ys=b),
           dict(xs=a, ys=[torch.zeros((3, 16), dtype=torch.int64)]), dict(xs=[x[0]], ys=b), dict(xs=x[:3], ys=x[3:9]),
           dict(xs=[np.zeros((65537, 16), np.float32)], ys=b), dict(xs=a, ys=[np.zeros((65537, 16), np.float32)]),
           dict(xs=a, ys=b, pair_chunk=0), dict(xs=a, ys=b, pair_chunk=1.5), dict(xs=a, ys=b, pair_chunk=True), dict(xs=a, ys=b, metric="ip"),
           dict(xs=[np.zeros((65536, 16), np.float32)], ys=[np.zeros((65536, 16), np.float32)], path=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            align_sequences(device=DEV, **kw)
    with pytest.raises(ValueError, match=r"pair 1 .*path=False never needs more than 1 MiB"):
        align_sequences(a + [np.zeros((40000, 16), np.float32)], b + [np.zeros((40000, 16), np.float32)], path=True, device=DEV)
    # 2^31 rows in total on a side: the lengths alone decide, so the check is held on them
    with pytest.raises(ValueError, match="2\\^31"):
        S._check_sequence_pairs(np.full(32768, 65536, np.int64), np.ones(32768, np.int64), False, None)
    for kw in (dict(pairs=[[0, 4]]), dict(pairs=[[-1, 0]]), dict(pairs=[0, 1]), dict(pairs=[[0.0, 1.0]]), dict(pairs=[[0, 1]], pair_chunk=0),
               dict(pairs=[[0, 1]], sequences=[0, 10, 41])):
        with pytest.raises(ValueError):
            idx.align_sequences(**kw)
    with pytest.raises(ValueError):
        SyllableIndex(device=DEV).align_sequences([[0, 0]])
    for path in (False, True):                                    # no pair: empty outputs without a launch
        out = align_sequences([], [], path=path, device=DEV)
        assert [tuple(t.shape) for t in out] == ([(0, 2), (0,), (0,), (1,)] if path else [(0,), (0,)])
        out = idx.align_sequences(np.zeros((0, 2), np.int64), path=path)
        assert [tuple(t.shape) for t in out] == ([(0, 2), (0,), (0,), (1,)] if path else [(0,), (0,)])
    monkeypatch.undo()
    costs, steps = align_sequences([np.zeros((65536, 16), np.float32)], [np.zeros((2, 16), np.float32)], device=DEV)    # the longest side does launch
    assert float(costs[0]) == 0.0 and int(steps[0]) == 65536


def test_the_entry_refuses_bad_arguments():
    """the C ABI by itself: status 1 with ``sylber_last_error`` for everything the entry can see, and that is everything -- the
    windows are host data"""
    from sylber_amd import _lib
    from sylber_amd._index import _row_norms
    from sylber_amd.kmeans import _stream, _vp
    lib, dev = _lib.load(), torch.device(DEV)
    x = torch.from_numpy(np.random.default_rng(12).standard_normal((40, 16)).astype(np.float32)).to(dev)
    nrm = _row_norms(x)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    win = lambda *w: np.array(w, np.int32).reshape(-1, 2)
    xw, yw, ro = win(0, 10, 5, 0), win(10, 30, 0, 5), np.array([0, 10], np.int64)
    p32 = lambda a: a.ctypes.data_as(i32p) if a is not None else None
    size = int(lib.sylber_dtw_strings_workspace_bytes(p32(xw), p32(yw), 2, 1))
    assert size == 256 + 2048
    assert int(lib.sylber_dtw_strings_workspace_bytes(p32(xw), p32(yw), 2, 0)) == 256
    for args in ((None, p32(yw), 2, 1), (p32(xw), None, 2, 1), (p32(xw), p32(yw), 0, 1), (p32(xw), p32(yw), 2, 2), (p32(win(0, -1)), p32(yw), 1, 0),
                 (p32(xw), p32(win(0, 65537)), 1, 0)):
        assert int(lib.sylber_dtw_strings_workspace_bytes(*args)) == -1
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    rows = torch.full((10, 2), 7, dtype=torch.int32, device=dev)
    steps = torch.full((2,), 7, dtype=torch.int32, device=dev)
    costs = torch.zeros(2, dtype=torch.float32, device=dev)
    good = dict(x=_vp(x), xr=40, xn=_vp(nrm), y=_vp(x), yr=40, yn=_vp(nrm), D=16, metric=0, xw=xw, yw=yw, n=2, path=1, ro=ro, rows=_vp(rows),
                steps=_vp(steps), costs=_vp(costs), walk=None, ws=_vp(ws))

    def call(**over):
        a = dict(good, **over)
        a["xw"], a["yw"] = p32(a["xw"]), p32(a["yw"])
        a["ro"] = a["ro"].ctypes.data_as(i64p) if a["ro"] is not None else None
        with torch.cuda.device(dev):
            return lib.sylber_dtw_strings_align(*a.values(), _stream(dev))
    for over in (dict(x=None), dict(y=None), dict(steps=None), dict(costs=None), dict(ws=None), dict(xw=None), dict(yw=None), dict(ro=None),
                 dict(rows=None), dict(D=8), dict(D=24), dict(D=0), dict(metric=5), dict(xn=None), dict(yn=None), dict(n=0), dict(n=-1),
                 dict(path=2), dict(path=-1), dict(xw=win(0, -1, 5, 0)), dict(yw=win(10, 65537, 0, 5)), dict(xw=win(-1, 10, 5, 0)),
                 dict(xw=win(35, 10, 5, 0)), dict(yw=win(10, 31, 0, 5)), dict(xr=9), dict(yr=39), dict(ro=np.array([0, -1], np.int64))):
        assert call(**over) == 1, over
        assert lib.sylber_last_error().decode().startswith("sylber_dtw_strings_align"), over
    torch.cuda.synchronize()
    assert (rows == 7).all() and (steps == 7).all()               # a refused call wrote nothing
    assert call() == 0 and call(metric=1, xn=None, yn=None) == 0 and call(path=0, ro=None, rows=None) == 0
    torch.cuda.synchronize()
    assert (rows >= 0).all() and int(steps[0]) >= 30 and int(steps[1]) == 0 and torch.isposinf(costs[1])

"""GPU tier, embedding strings, local (csrc/dtw_strings_local.hip behind ``local_align_sequences`` and
``SyllableIndex.local_align_sequences``), bitwise against tests/dtw_strings_local_ref.py.  The local costs come from numpy where they
are exact (integer rows under L2) and otherwise from the library's fp32 search on pieces of at most 128 rows
(``test_gpu_phrase._local_costs``: code from before this kernel, never the code under test); the rounds of dtw_strings_local_ref run
over them, and the call must return exactly those score bits and spans.

Shapes (m, L): one cell, one row, one column, inside one strip and tile, exactly one strip and tile (64, 128), the second strip and
the second tile (65, 129), a whole super-strip (128, 128), the second super-strip with its carried rows (129, 127), three
super-strips with a short last one over three tiles (300, 257), and the empty sides.  ``PLANTS`` puts repeats across a strip edge,
a tile edge and a super-strip edge, into the first and the last row and column, and a copy of 150 rows across two super-strip edges;
every case asserts through ``dtw_strings_local_ref.assert_not_vacuous`` that the reference alone has as many rounds as copies, paths
with up and left steps, and exact ties between c_diag and c_up / c_left: at gap = 0 every path's first cell ties, at gap > 0 the
doubled rows of a "double" copy tie where numpy's d is exact (integer rows under L2); rows whose d is not exactly 0 cannot be made
to tie at gap > 0."""
import functools

import numpy as np
import pytest
import torch

import dtw_ref as R
import dtw_strings_local_ref as G
from test_gpu_phrase import _groups_of, _local_costs, _np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
# (m, L): [(first row of x, rows, first row of y, how)]
PLANTS = {
    (1, 1): [(0, 1, 0, "same")],
    (1, 40): [(0, 1, 7, "same")],                                  # a best cell in row 0
    (40, 1): [(9, 1, 0, "same")],                                  # a best cell in column 0
    (33, 40): [(2, 12, 20, "drop"), (18, 12, 3, "double")],
    (64, 128): [(50, 14, 114, "same"), (5, 14, 20, "drop"), (25, 12, 60, "double")],       # a best cell in the last row and column
    (65, 129): [(55, 10, 119, "same"), (10, 14, 40, "double")],    # across the strip edge and the tile edge
    (128, 128): [(0, 14, 100, "same"), (100, 16, 0, "drop"), (40, 12, 50, "double")],      # starts in row 0 and in column 0
    (129, 127): [(115, 14, 20, "same"), (20, 14, 100, "double")],  # across the super-strip edge
    (300, 257): [(120, 150, 60, "drop"), (10, 16, 230, "double"), (280, 16, 5, "same")],    # a start carried across two super-strips
    (0, 5): [],
    (1, 0): [],
}
SHAPES = tuple(PLANTS)
SHAPES_768 = ((33, 40), (65, 129), (129, 127))
CONFIGS = [(32, True, "l2"), (32, True, "cosine"), (32, False, "l2"), (32, False, "cosine"), (768, False, "l2"), (768, False, "cosine")]


def _radius(D, integer, metric):
    """between the d of a planted row (0, or the copy's noise) and the d of unrelated rows: 4 D (integer), 2 D (gaussian), 1 (cosine)"""
    return f32(0.5) if metric == "cosine" else f32(48.0 if integer else 0.75 * D)


def _pieces(L):
    return np.array(sorted(set(list(range(0, L, 128)) + [L])), np.int64)


def _d_int(x, y):
    """every term is a small integer: numpy is exact and needs nothing from the GPU"""
    xn, yn = (x * x).sum(1), (y * y).sum(1)
    return np.maximum(f32(0), xn[:, None] + (f32(-2) * (x @ y.T) + yn[None, :])).astype(np.float32)


def _costs(x, y, integer, metric):
    if len(x) == 0 or len(y) == 0:
        return np.zeros((len(x), len(y)), np.float32)
    return _d_int(x, y) if integer and metric == "l2" else _local_costs(y, _pieces(len(y)), x, metric)


@functools.lru_cache(maxsize=None)
def _case(D, integer, metric):
    """the pairs of one group, made once: (xs, ys, d per pair, radius)"""
    rng = np.random.default_rng(D + 7 * integer)
    xs, ys, ds = [], [], []
    for m, L in (SHAPES if D == 32 else SHAPES_768):
        x, y = G.planted(rng, m, L, D, PLANTS[(m, L)], integer)
        xs.append(x); ys.append(y); ds.append(_costs(x, y, integer, metric))
    return xs, ys, ds, _radius(D, integer, metric)


@functools.lru_cache(maxsize=None)
def _ref(D, integer, metric, gap_mul):
    """the reference of every pair at 32 rounds, computed once: (scores [S, 32], spans [S, 32, 2, 2]); fewer rounds are its prefix"""
    xs, ys, ds, radius = _case(D, integer, metric)
    gap, min_score = f32(gap_mul) * radius, f32(0.5) * radius
    out = []
    for x, y, d in zip(xs, ys, ds):
        copies = PLANTS[(len(x), len(y))]
        if copies:
            ties = gap_mul == 0 or (integer and metric == "l2" and any(c[3] == "double" for c in copies))
            sc, sp, info = G.assert_not_vacuous(d, radius, gap, min_score, G.MAX_BEST, copies, need_ties=ties)
            assert len(copies) < 3 or len(info) >= 3
        else:
            sc, sp = G.rounds(d, radius, gap, min_score, G.MAX_BEST, strip=None)
        out.append((sc, sp))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), gap, min_score


def _assert_same(got, scores, spans, what=None):
    sc, sp = got
    assert sc.dtype == torch.float32 and sp.dtype == torch.int64 and sc.device.type == "cuda" and sp.device.type == "cuda"
    assert tuple(sc.shape) == scores.shape and tuple(sp.shape) == spans.shape, what
    assert np.array_equal(_np(sc).view(np.uint32), np.ascontiguousarray(scores, np.float32).view(np.uint32)), what
    assert np.array_equal(_np(sp), spans), what


def _equal(a, b, what=None):
    assert len(a) == len(b)
    for s, t in zip(a, b):
        assert s.dtype == t.dtype and s.shape == t.shape and torch.equal(s.contiguous().view(-1).view(torch.uint8), t.contiguous().view(-1).view(torch.uint8)), what


@pytest.mark.parametrize("gap_mul", [0, 1, 2])
@pytest.mark.parametrize("D,integer,metric", CONFIGS)
def test_bitwise_against_the_contract(D, integer, metric, gap_mul):
    from sylber_amd import local_align_sequences
    xs, ys, _, radius = _case(D, integer, metric)
    scores, spans, gap, min_score = _ref(D, integer, metric, gap_mul)
    for n_best in (32, 7, 2, 1):
        got = local_align_sequences(xs, ys, radius=radius, gap=gap, min_score=min_score, n_best=n_best, metric=metric, device=DEV)
        _assert_same(got, scores[:, :n_best], spans[:, :n_best], n_best)
    s = len(xs) - 1 if D == 768 else SHAPES.index((300, 257))     # one pair per call
    got = local_align_sequences(xs[s:s + 1], ys[s:s + 1], radius=radius, gap=gap, min_score=min_score, n_best=7, metric=metric, device=DEV)
    _assert_same(got, scores[s:s + 1, :7], spans[s:s + 1, :7])


def test_thirty_two_rounds():
    """a floor so low that all 32 rounds run: every bit of a lane's mask is in use and rectangles pile up"""
    from sylber_amd import local_align_sequences
    xs, ys, ds, _ = _case(32, True, "l2")
    radius = f32(96.0)                                             # unrelated rows are about 128 +- 26 apart: positive cells everywhere
    for s in (SHAPES.index((129, 127)), SHAPES.index((65, 129))):
        sc, sp = G.rounds(ds[s], radius, radius, f32(1), 32, strip=None)
        assert (sc > 0).all() and (np.diff(sc) <= 0).all()
        got = local_align_sequences(xs[s:s + 1], ys[s:s + 1], radius=radius, gap=radius, min_score=1.0, n_best=32, device=DEV)
        _assert_same(got, sc[None], sp[None])


@functools.lru_cache(maxsize=None)
def _self_case():
    """one sequence of 300 rows that says a phrase of 20 rows three times"""
    rng = np.random.default_rng(31)
    x = rng.integers(-2, 3, (300, 32)).astype(np.float32)
    x[130:150] = x[20:40]
    x[260:280] = x[20:40]
    return x, _d_int(x, x), f32(48.0)


@pytest.mark.parametrize("min_sep", [1, 5, 200])
def test_a_sequence_against_itself(min_sep):
    """three occurrences give the three pairs, nothing on or below the diagonal; min_sep = 200 leaves one pair and skips whole
    tiles (all of the third super-strip's)"""
    from sylber_amd import SyllableIndex, local_align_sequences
    x, d, radius = _self_case()
    min_score = f32(3) * radius
    sc, sp, info = G.rounds(d, radius, radius, min_score, 7, min_sep, strip=None, info=True)
    pairs = sorted((int(a[0]), int(b[0])) for a, b in sp[:len(info)] if a[1] - a[0] == 20)
    assert pairs == ([(20, 130), (20, 260), (130, 260)] if min_sep < 200 else [(20, 260)])
    assert all(j - i >= min_sep for p in info for i, j in p["path"])
    got = local_align_sequences([x], radius=radius, gap=radius, min_score=min_score, n_best=7, min_sep=min_sep, device=DEV)
    _assert_same(got, sc[None], sp[None])
    assert (got[1][0, :len(info), 1, 0] - got[1][0, :len(info), 0, 0] >= min_sep).all()
    # the same through the index: a pair (s, s) among others, row ids shifted by the sequence's first row
    other = np.random.default_rng(1).integers(-2, 3, (50, 32)).astype(np.float32)
    idx = SyllableIndex(np.concatenate([other, x]), groups=np.repeat([0, 1], [50, 300]), device=DEV)
    isc, isp = idx.local_align_sequences([[1, 1], [0, 1]], radius, gap=radius, min_score=min_score, n_best=7, min_sep=min_sep)
    want = torch.from_numpy(np.where(sp >= 0, sp + 50, sp)).to(DEV)
    assert torch.equal(isc[0].view(torch.int32), got[0][0].view(torch.int32)) and torch.equal(isp[0], want)
    cross = local_align_sequences([other], [x], radius=radius, gap=radius, min_score=min_score, n_best=7, device=DEV)     # (0, 1) has no band
    assert torch.equal(isc[1].view(torch.int32), cross[0][0].view(torch.int32))


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_round_0_is_search_repeats(metric):
    """for m <= 64: a probe against an index that holds one sequence -- score bits and both spans"""
    from sylber_amd import SyllableIndex, local_align_sequences
    rng = np.random.default_rng(17)
    D = 32
    seq = rng.standard_normal((200, D)).astype(np.float32)
    radius = f32(24.0) if metric == "l2" else f32(0.5)
    idx = SyllableIndex(seq, metric=metric, groups=np.zeros(200, np.int32), device=DEV)
    for m, a in ((5, 20), (33, 100), (64, 130)):
        p = seq[a:a + m + 1].copy() + 0.1 * rng.standard_normal((m + 1, D)).astype(np.float32)
        p = np.delete(p, m // 2, 0)                                # a row left out: the match has to warp
        for gap in (f32(0), radius):
            sc, sq, sp = idx.search_repeats([p], 1, radius, gap=gap, min_score=radius)
            gsc, gsp = local_align_sequences([p], [seq], radius=radius, gap=gap, min_score=radius, metric=metric, device=DEV)
            assert int(sq[0, 0]) == 0 and float(sc[0, 0]) > 2 * float(radius)
            assert torch.equal(gsc[0].view(torch.int32), sc[0].view(torch.int32)) and torch.equal(gsp[0, 0], sp[0, 0]), (m, gap)


def test_the_pairs_of_find_repeats():
    """``find_repeats``' pairs fed to ``local_align_sequences``: round 0 never scores less, and where the whole sequences' best
    alignment covers at most window - hop + 1 = 33 rows of s (the window theorem's condition) it is that result, bit for bit"""
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(23)
    D, lens = 32, [90, 100, 130, 70]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = rng.standard_normal((int(off[-1]), D)).astype(np.float32)
    x[off[2] + 50:off[2] + 70] = x[off[0] + 30:off[0] + 50] + 0.05 * rng.standard_normal((20, D)).astype(np.float32)     # 20 rows: inside a window
    x[off[3] + 5:off[3] + 65] = x[off[1] + 20:off[1] + 80] + 0.05 * rng.standard_normal((60, D)).astype(np.float32)      # 60 rows: in no window
    idx = SyllableIndex(x, groups=_groups_of(off), device=DEV)
    radius = f32(24.0)
    fsc, fpairs, fsp = idx.find_repeats(4, radius, gap=radius)
    n = int((fpairs[:, 0] >= 0).sum())
    assert n >= 2 and sorted(map(tuple, _np(fpairs[:2]).tolist())) == [(0, 2), (1, 3)]
    sc, sp = idx.local_align_sequences(fpairs[:n], radius, gap=radius)
    assert (sc[:, 0] >= fsc[:n]).all()
    rows = _np(sp[:, 0, 0, 1] - sp[:, 0, 0, 0])
    held = rows <= 33
    assert held.any() and (~held).any()
    for e in range(n):
        if held[e]:
            assert torch.equal(sc[e, :1].view(torch.int32), fsc[e:e + 1].view(torch.int32)) and torch.equal(sp[e, 0], fsp[e]), e
        else:
            assert float(sc[e, 0]) > float(fsc[e])                 # the full extent of the repeat whose window find_repeats found
    pr, spn = _np(fpairs[:n]), _np(sp[:, 0])                       # the spans are row ids inside the pair's two sequences
    assert (off[pr] <= spn[..., 0]).all() and (spn[..., 1] <= off[pr + 1]).all() and len(idx.provenance(sp[0, 0, 0])) == 2


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D", [32, 768])
def test_scores_against_float64(D, metric):
    """Gaussian rows: |score32 - score64| of round 0 within ``dtw_strings_local_ref.score_error_bound`` (``repeats_ref``'s, whose
    derivation takes the path length m + L - 1 from the shapes; derived, not fitted), and the bound small against the score; the
    float64 DP runs on the rows as the kernel reads them"""
    from sylber_amd import local_align_sequences
    from sylber_amd._index import _prep
    xs, ys, _, radius = _case(D, False, metric)
    scores, _ = local_align_sequences(xs, ys, radius=radius, gap=radius, min_score=f32(0.5) * radius, metric=metric, device=DEV)
    scores = _np(scores).astype(np.float64)[:, 0]
    for s, (x, y) in enumerate(zip(xs, ys)):
        if len(x) == 0 or len(y) == 0:
            assert scores[s] == 0
            continue
        xp, yp = (_np(_prep(torch.from_numpy(a), metric, torch.device(DEV))) for a in (x, y))
        s64 = float(G.rounds(R.local_costs(xp, yp, metric), radius, radius, f32(0.5) * radius, 1, dtype=np.float64, strip=None)[0][0])
        bound = G.score_error_bound(xp, yp, s64, radius, radius, metric)
        print("D=%d %s %dx%d: score32 %.9g score64 %.9g |diff| %.3g bound %.3g" % (D, metric, len(x), len(y), scores[s], s64, abs(scores[s] - s64), bound))
        assert s64 > 0 and abs(scores[s] - s64) <= bound
        assert bound < 1e-2 * s64                                  # and the bound says something


def test_invariance_is_bitwise(tmp_path):
    from sylber_amd import IVFSyllableIndex, SyllableIndex, local_align_sequences
    xs, ys, _, radius = _case(32, True, "l2")
    kw = dict(radius=radius, gap=radius, min_score=f32(0.5) * radius, n_best=4, device=DEV)
    base = local_align_sequences(xs, ys, **kw)
    for more in ({"pair_chunk": 1}, {"pair_chunk": 3}, {"_workspace_fill": 0x00}, {"_workspace_fill": 0xFF}, {"pair_chunk": 3, "_workspace_fill": 0xFF}):
        _equal(base, local_align_sequences(xs, ys, **kw, **more), more)
    xd, yd = [torch.from_numpy(a).to(DEV) for a in xs], [torch.from_numpy(a).double() for a in ys]
    _equal(base, local_align_sequences(xd, yd, **kw), "device and float64 host inputs")
    order = [8, 0, 10, 7, 3, 5, 1, 9, 6, 2, 4]                     # the order of the pairs
    perm = local_align_sequences([xs[s] for s in order], [ys[s] for s in order], **kw)
    _equal([t[order] for t in base], perm, "order")
    # the index method on the same rows: one buffer, windows into it, spans as row ids
    keep = [s for s in range(len(xs)) if len(xs[s]) and len(ys[s])]                # an index holds no empty sequence
    parts = [a for s in keep for a in (xs[s], ys[s])]
    rows = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum([len(a) for a in parts])]).astype(np.int64)
    pairs = np.array([[2 * e, 2 * e + 1] for e in range(len(keep))], np.int64)
    idx = SyllableIndex(rows, groups=_groups_of(off), device=DEV)
    shift = torch.from_numpy(off[:-1][pairs]).to(DEV)[:, None, :, None]
    want = (base[0][keep], torch.where(base[1][keep] >= 0, base[1][keep] + shift, base[1][keep]))
    ikw = dict(gap=radius, min_score=f32(0.5) * radius, n_best=4)
    got = idx.local_align_sequences(pairs, radius, **ikw)
    _equal(got, want, "index")
    _equal(idx.local_align_sequences(torch.from_numpy(pairs).to(DEV), radius, pair_chunk=2, _workspace_fill=0xFF, **ikw), want)
    _equal(IVFSyllableIndex.build(idx, 4, seed=1).local_align_sequences(pairs, radius, **ikw), want, "ivf")
    idx.save(str(tmp_path / "idx.npz"))
    _equal(SyllableIndex.load(str(tmp_path / "idx.npz"), device=DEV).local_align_sequences(pairs, radius, **ikw), want, "save / load")
    cut = np.array([0, 64, 200, len(rows)], np.int64)              # explicit sequences
    a = idx.local_align_sequences([[0, 1], [1, 1]], radius, sequences=cut, **ikw)
    b0 = local_align_sequences([rows[0:64]], [rows[64:200]], **kw)
    b1 = local_align_sequences([rows[64:200]], **kw)
    assert torch.equal(a[0].view(torch.int32), torch.cat([b0[0], b1[0]]).view(torch.int32))


def test_every_refusal_comes_before_a_launch(monkeypatch):
    from sylber_amd import IVFSyllableIndex, SyllableIndex, _lib, local_align_sequences
    rng = np.random.default_rng(10)
    x = rng.standard_normal((40, 16)).astype(np.float32)
    idx = SyllableIndex(x, groups=np.repeat(np.arange(4), 10), device=DEV)
    lib = _lib.load()

    def fail(*a):
        raise AssertionError("launched")
    entries = {"sylber_dtw_strings_local", "sylber_dtw_strings_local_workspace_bytes", "sylber_knn_row_norms", "sylber_knn_unit_rows"}
    monkeypatch.setattr(_lib, "_LIB", type("L", (), {"__getattr__": lambda self, n: fail if n in entries else getattr(lib, n)})())
    a, b = [x[:3]], [x[3:9]]
    nan, inf = float("nan"), float("inf")
    bad = [dict(xs=a + a, ys=b), dict(xs=a, ys=[np.zeros((4, 32), np.float32)]), dict(xs=[np.zeros((4, 24), np.float32)], ys=[np.zeros((4, 24), np.float32)]),
           dict(xs=[np.zeros((4, 8), np.float32)]), dict(xs=[x[:3].astype(np.int32)], ys=b), dict(xs=[x[0]], ys=b), dict(xs=x[:3], ys=x[3:9]),
           dict(xs=[np.zeros((65537, 16), np.float32)], ys=b), dict(xs=a, ys=[np.zeros((65537, 16), np.float32)]),
           dict(xs=a, ys=b, pair_chunk=0), dict(xs=a, ys=b, pair_chunk=1.5), dict(xs=a, ys=b, metric="ip"),
           dict(xs=a, ys=b, radius=0.0), dict(xs=a, ys=b, radius=-1.0), dict(xs=a, ys=b, radius=nan), dict(xs=a, ys=b, radius=inf),
           dict(xs=a, ys=b, radius="1"), dict(xs=a, ys=b, gap=-1.0), dict(xs=a, ys=b, gap=nan), dict(xs=a, ys=b, min_score=0.0),
           dict(xs=a, ys=b, min_score=inf), dict(xs=a, ys=b, n_best=0), dict(xs=a, ys=b, n_best=33), dict(xs=a, ys=b, n_best=2.0),
           dict(xs=a, ys=b, n_best=True), dict(xs=a, min_sep=0), dict(xs=a, min_sep=-3), dict(xs=a, min_sep=1.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            local_align_sequences(**dict(dict(radius=1.0, device=DEV), **kw))
    for kw in (dict(pairs=[[0, 4]]), dict(pairs=[[-1, 0]]), dict(pairs=[0, 1]), dict(pairs=[[0.0, 1.0]]), dict(pairs=[[0, 1]], pair_chunk=0),
               dict(pairs=[[0, 1]], sequences=[0, 10, 41]), dict(pairs=[[0, 1]], radius=0.0), dict(pairs=[[0, 1]], gap=-1.0),
               dict(pairs=[[0, 1]], min_score=nan), dict(pairs=[[0, 1]], n_best=33), dict(pairs=[[0, 0]], min_sep=0)):
        with pytest.raises(ValueError):
            idx.local_align_sequences(**dict(dict(radius=1.0), **kw))
    with pytest.raises(ValueError):
        SyllableIndex(device=DEV).local_align_sequences([[0, 0]], 1.0)
    for out in (local_align_sequences([], [], radius=1.0, n_best=3, device=DEV), local_align_sequences([], radius=1.0, n_best=3, device=DEV),
                idx.local_align_sequences(np.zeros((0, 2), np.int64), 1.0, n_best=3)):      # no pair: empty outputs without a launch
        assert [tuple(t.shape) for t in out] == [(0, 3), (0, 3, 2, 2)] and out[0].dtype == torch.float32 and out[1].dtype == torch.int64
    monkeypatch.undo()
    sc, sp = local_align_sequences(a, b, radius=1.0, device=DEV)  # and the good call does launch: unrelated rows, no repeat
    assert sc.tolist() == [[0.0]] and (sp == -1).all()


def test_the_entry_refuses_bad_arguments():
    """the C ABI by itself: status 1 with ``sylber_last_error`` for everything the entry can see, and that is everything -- the
    windows and sep are host data"""
    import ctypes
    from sylber_amd import _lib
    from sylber_amd._index import _row_norms
    from sylber_amd.kmeans import _stream, _vp
    lib, dev = _lib.load(), torch.device(DEV)
    x = torch.from_numpy(np.random.default_rng(12).standard_normal((40, 16)).astype(np.float32)).to(dev)
    nrm = _row_norms(x)
    i32p = ctypes.POINTER(ctypes.c_int32)
    win = lambda *w: np.array(w, np.int32).reshape(-1, 2)
    xw, yw, sep = win(0, 10, 5, 0), win(10, 30, 0, 5), np.array([0, 3], np.int32)
    p32 = lambda a: a.ctypes.data_as(i32p) if a is not None else None
    size = int(lib.sylber_dtw_strings_local_workspace_bytes(p32(xw), p32(yw), 2))
    assert size == 256
    assert int(lib.sylber_dtw_strings_local_workspace_bytes(p32(win(0, 129)), p32(win(0, 40)), 1)) == 256 + 768
    for args in ((None, p32(yw), 2), (p32(xw), None, 2), (p32(xw), p32(yw), 0), (p32(win(0, -1)), p32(yw), 1), (p32(xw), p32(win(0, 65537)), 1)):
        assert int(lib.sylber_dtw_strings_local_workspace_bytes(*args)) == -1
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    scores = torch.full((2, 3), 7.0, dtype=torch.float32, device=dev)
    spans = torch.full((2, 3, 4), 7, dtype=torch.int32, device=dev)
    good = dict(x=_vp(x), xr=40, xn=_vp(nrm), y=_vp(x), yr=40, yn=_vp(nrm), D=16, metric=0, xw=xw, yw=yw, sep=sep, n=2, radius=40.0, gap=40.0,
                min_score=40.0, n_best=3, scores=_vp(scores), spans=_vp(spans), ws=_vp(ws))

    def call(**over):
        a = dict(good, **over)
        a["xw"], a["yw"], a["sep"] = p32(a["xw"]), p32(a["yw"]), p32(a["sep"])
        with torch.cuda.device(dev):
            return lib.sylber_dtw_strings_local(*a.values(), _stream(dev))
    nan, inf = float("nan"), float("inf")
    for over in (dict(x=None), dict(y=None), dict(scores=None), dict(spans=None), dict(ws=None), dict(xw=None), dict(yw=None), dict(D=8), dict(D=24),
                 dict(D=0), dict(metric=5), dict(xn=None), dict(yn=None), dict(n=0), dict(n=-1), dict(xw=win(0, -1, 5, 0)),
                 dict(yw=win(10, 65537, 0, 5)), dict(xw=win(-1, 10, 5, 0)), dict(xw=win(35, 10, 5, 0)), dict(yw=win(10, 31, 0, 5)), dict(xr=9),
                 dict(yr=39), dict(sep=np.array([0, -1], np.int32)), dict(radius=0.0), dict(radius=nan), dict(radius=inf), dict(gap=-1.0),
                 dict(gap=nan), dict(min_score=0.0), dict(min_score=inf), dict(n_best=0), dict(n_best=33)):
        assert call(**over) == 1, over
        assert lib.sylber_last_error().decode().startswith("sylber_dtw_strings_local"), over
    torch.cuda.synchronize()
    assert (scores == 7).all() and (spans == 7).all()             # a refused call wrote nothing
    assert call() == 0 and call(metric=1, xn=None, yn=None) == 0 and call(sep=None) == 0
    torch.cuda.synchronize()
    assert (scores[1] == 0).all() and (spans[1] == -1).all() and (spans[0][scores[0] == 0] == -1).all()

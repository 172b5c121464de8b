"""GPU tier, embedding strings with one pair split across workgroups (csrc/dtw_strings_split.hip behind ``align_sequences(split=...)``
and ``SyllableIndex.align_sequences(split=...)``): bit for bit the one-workgroup kernel (``split=False``) and the numpy contract of
tests/dtw_strings_ref.py, whatever the block sizes, the company of a pair, the order and the workspace's contents.

Shapes (m, L) at blocks of 128 x 128: one block (128, 128); 2 x 2 blocks with one-row and one-column edge blocks (129, 129); one band
of one row (1, 300) and one chunk of one column (300, 1); a half-live strip over three chunks (64, 257); 3 x 4 blocks, ragged both ways
(300, 400); 4 x 3 (385, 257).  D = 16 is one K step of the contraction, D = 48 three.  The local costs of the reference come from numpy
where they are exact (small-integer rows under L2) and otherwise from the library's fp32 search on pieces of at most 128 rows
(``test_gpu_phrase._local_costs``: code from before this kernel)."""
import functools

import numpy as np
import pytest
import torch

import dtw_strings_ref as G
from test_gpu_dtw_strings import _assert_same, _equal, _pieces
from test_gpu_phrase import _local_costs, _np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((128, 128), (129, 129), (1, 300), (300, 1), (64, 257), (300, 400), (385, 257))
BLOCKS = ((256, 128), (128, 384), (256, 256))


@functools.lru_cache(maxsize=None)
def _case(D, metric):
    """the pairs with their reference, computed once: (xs, ys, reference of align_sequences)"""
    rng = np.random.default_rng(100 + D)
    xs, ys, ds = [], [], []
    for m, L in SHAPES:
        x, y = (rng.standard_normal((n, D)).astype(np.float32) for n in (m, L))
        if m > 1 and L > 1:                                       # the two recordings say the same thing at different speeds
            y = (x[np.minimum(np.arange(L) * m // L, m - 1)] + 0.5 * y).astype(np.float32)
        xs.append(x); ys.append(y); ds.append(_local_costs(y, _pieces(L), x, metric))
    return xs, ys, G.align_sequences(lambda s: ds[s], [len(x) for x in xs], [len(y) for y in ys])


@functools.lru_cache(maxsize=None)
def _unsplit(D, metric, path):
    from sylber_amd import align_sequences
    xs, ys, _ = _case(D, metric)
    return align_sequences(xs, ys, metric=metric, path=path, device=DEV, split=False, _steps_walk=path)


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D", [16, 48])
def test_bitwise_the_one_workgroup_kernel_and_the_contract(D, metric):
    from sylber_amd import align_sequences
    xs, ys, ref = _case(D, metric)
    got = align_sequences(xs, ys, metric=metric, path=True, device=DEV, split=(128, 128), _steps_walk=True)
    _assert_same(got[:4], ref)
    assert torch.equal(got[4], got[2])                            # the walk over the codes counts the cells that formed them
    _equal(got, _unsplit(D, metric, True), "path")
    counts = align_sequences(xs, ys, metric=metric, device=DEV, split=(128, 128))
    _equal(counts, _unsplit(D, metric, False), "counts")
    assert torch.equal(counts[0].view(torch.int32), got[1].view(torch.int32)) and torch.equal(counts[1], got[2])
    for s in (1, 5):                                              # one pair per call
        rows, c, n, _ = align_sequences(xs[s:s + 1], ys[s:s + 1], metric=metric, path=True, device=DEV, split=(128, 128))
        xo = ref[3]
        assert np.array_equal(_np(rows), ref[0][xo[s]:xo[s + 1]]) and torch.equal(c.view(torch.int32), got[1][s:s + 1].view(torch.int32))
        assert torch.equal(n, got[2][s:s + 1])


@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("D", [16, 48])
def test_nothing_depends_on_the_block_size(D, blocks):
    """(256, 128) and (256, 256) carry a row between a block's own super-strips; (128, 384) walks three tiles per block"""
    from sylber_amd import align_sequences
    for metric in ("l2", "cosine"):
        xs, ys, ref = _case(D, metric)
        got = align_sequences(xs, ys, metric=metric, path=True, device=DEV, split=blocks, _steps_walk=True)
        _equal(got, _unsplit(D, metric, True), (blocks, metric))
        _assert_same(got[:4], ref)
        _equal(align_sequences(xs, ys, metric=metric, device=DEV, split=blocks), _unsplit(D, metric, False), (blocks, metric))


def test_ties_keep_the_first_smallest_across_block_edges():
    """rows of {-1, 0, 1}: every cost is a small integer that numpy computes exactly, and many cells tie"""
    from sylber_amd import align_sequences
    rng = np.random.default_rng(41)
    D = 16
    xs, ys, ds = [], [], []
    for m, L in SHAPES:
        x, y = (rng.integers(-1, 2, (n, D)).astype(np.float32) for n in (m, L))
        if L >= 140:
            y[120:136] = y[119]                                   # a run of equal rows across the first chunk's edge
        xn, yn = (x * x).sum(1), (y * y).sum(1)
        xs.append(x); ys.append(y)
        ds.append(np.maximum(np.float32(0), xn[:, None] + (np.float32(-2) * (x @ y.T) + yn[None, :])).astype(np.float32))
    ref = G.align_sequences(lambda s: ds[s], [len(x) for x in xs], [len(y) for y in ys])
    base = align_sequences(xs, ys, path=True, device=DEV, split=False)
    for blocks in ((128, 128),) + BLOCKS:
        got = align_sequences(xs, ys, path=True, device=DEV, split=blocks, _steps_walk=True)
        _assert_same(got[:4], ref)
        assert torch.equal(got[4], got[2])
        _equal(got[:4], base, blocks)


def test_nan_rows_on_block_edges_are_padding():
    """a NaN row of x (rows 127, 128, 255) or of y (rows 127, 128) is a row or a column of +inf costs on a block's edge: every path
    crosses it, the reference's cost is +inf and the pair is padding"""
    from sylber_amd import align_sequences
    rng = np.random.default_rng(42)
    D = 16
    mk = lambda n: rng.standard_normal((n, D)).astype(np.float32)
    xs, ys = [mk(300) for _ in range(6)], [mk(257) for _ in range(6)]
    for metric in ("l2", "cosine"):
        bad = np.nan if metric == "l2" else np.inf                # under "cosine" a row of inf becomes the NaN row (see test_gpu_dtw_strings)
        for s, i in enumerate((127, 128, 255)):
            xs[s][i] = bad
        for s, j in ((3, 127), (4, 128)):
            ys[s][j] = bad
        for blocks in ((128, 128), (256, 128)):
            rows, costs, steps, xo = align_sequences(xs, ys, metric=metric, path=True, device=DEV, split=blocks)
            assert torch.isposinf(costs[:5]).all() and (steps[:5] == 0).all() and (rows[:int(xo[5])] == -1).all()
            assert torch.isfinite(costs[5]) and int(steps[5]) >= 300 and (rows[int(xo[5]):] >= 0).all()
            _equal((rows, costs, steps, xo), align_sequences(xs, ys, metric=metric, path=True, device=DEV, split=False), (metric, blocks))
            _equal(align_sequences(xs, ys, metric=metric, device=DEV, split=blocks), (costs, steps), (metric, blocks))


@functools.lru_cache(maxsize=None)
def _mixed():
    """three pairs of 3 x 4, 2 x 2 and 1 x 3 blocks among five short pairs and a pair with an empty side"""
    rng = np.random.default_rng(43)
    D = 16
    shapes = ((40, 33), (300, 400), (5, 128), (129, 129), (0, 9), (128, 100), (64, 257), (1, 1), (77, 3))
    xs = [rng.standard_normal((m, D)).astype(np.float32) for m, _ in shapes]
    ys = [rng.standard_normal((L, D)).astype(np.float32) for _, L in shapes]
    return xs, ys


def test_company_order_and_grouping_change_nothing():
    from sylber_amd import align_sequences
    from sylber_amd import search as S
    xs, ys = _mixed()
    ml, Ll = np.array([len(x) for x in xs]), np.array([len(y) for y in ys])
    assert S._split_plan(ml, Ll, True, None)[0].tolist() == [False, True, False, True, False, False, True, False, False]
    base = align_sequences(xs, ys, path=True, device=DEV, split=False)
    counts = align_sequences(xs, ys, device=DEV, split=False)
    for kw in ({}, {"pair_chunk": 1}, {"pair_chunk": 2}, {"_workspace_fill": 0x00}, {"_workspace_fill": 0xFF}, {"pair_chunk": 2, "_workspace_fill": 0xFF}):
        _equal(base, align_sequences(xs, ys, path=True, device=DEV, split=True, **kw), kw)
        _equal(counts, align_sequences(xs, ys, device=DEV, split=True, **kw), kw)
    order = [6, 0, 8, 3, 5, 1, 7, 2, 4]
    perm = align_sequences([xs[s] for s in order], [ys[s] for s in order], path=True, device=DEV, split=True)
    xo, po = _np(base[3]), _np(perm[3])
    for e, s in enumerate(order):
        assert torch.equal(perm[0][po[e]:po[e + 1]], base[0][xo[s]:xo[s + 1]]), s
        assert torch.equal(perm[1][e:e + 1].view(torch.int32), base[1][s:s + 1].view(torch.int32)) and perm[2][e] == base[2][s]
    assert torch.isposinf(base[1][4]) and int(base[2][4]) == 0


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_no_read_of_unwritten_workspace(fill):
    from sylber_amd import align_sequences
    xs, ys, _ = _case(16, "l2")
    for blocks in ((128, 128), (256, 256)):
        _equal(align_sequences(xs, ys, path=True, device=DEV, split=blocks, _workspace_fill=fill, _steps_walk=True), _unsplit(16, "l2", True), blocks)
        _equal(align_sequences(xs, ys, device=DEV, split=blocks, _workspace_fill=fill), _unsplit(16, "l2", False), blocks)


def test_the_index_method_splits_with_the_same_bits():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(44)
    lens = (300, 400, 129, 40)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = SyllableIndex(rng.standard_normal((int(off[-1]), 16)).astype(np.float32), groups=np.repeat(np.arange(4), lens).astype(np.int32), device=DEV)
    pairs = np.array([[0, 1], [3, 2], [2, 0], [1, 1]], np.int64)
    for path in (False, True):
        base = idx.align_sequences(pairs, path=path, split=False)
        for split in (True, None, (128, 128), (256, 128)):
            _equal(idx.align_sequences(pairs, path=path, split=split), base, split)


def test_bad_block_sizes_are_refused_before_any_launch(monkeypatch):
    from sylber_amd import SyllableIndex, _lib, align_sequences
    rng = np.random.default_rng(45)
    x = rng.standard_normal((300, 16)).astype(np.float32)
    idx = SyllableIndex(x, groups=np.repeat(np.arange(2), 150).astype(np.int32), device=DEV)
    lib = _lib.load()

    def fail(*a):
        raise AssertionError("launched")
    entries = {"sylber_dtw_strings_align", "sylber_dtw_strings_align_split", "sylber_dtw_strings_workspace_bytes",
               "sylber_dtw_strings_split_workspace_bytes", "sylber_knn_row_norms", "sylber_knn_unit_rows"}
    monkeypatch.setattr(_lib, "_LIB", type("L", (), {"__getattr__": lambda self, n: fail if n in entries else getattr(lib, n)})())
    for bad in ((100, 128), (128, 0), (0, 128), (-128, 128), (128, -128), (-128, -128), (128,), "yes", 3):
        with pytest.raises(ValueError):
            align_sequences([x], [x[:200]], device=DEV, split=bad)
        with pytest.raises(ValueError):
            idx.align_sequences([[0, 1]], split=bad)
    monkeypatch.undo()
    # the entry itself: status 1 with sylber_last_error, nothing written
    import ctypes
    from sylber_amd._index import _row_norms
    from sylber_amd.kmeans import _stream, _vp
    dev = torch.device(DEV)
    xd = torch.from_numpy(x).to(dev)
    nrm = _row_norms(xd)
    i32p = ctypes.POINTER(ctypes.c_int32)
    xw, yw = np.array([[0, 300]], np.int32), np.array([[0, 200]], np.int32)
    ws = torch.empty(int(lib.sylber_dtw_strings_split_workspace_bytes(xw.ctypes.data_as(i32p), yw.ctypes.data_as(i32p), 1, 0, 128, 128)), dtype=torch.uint8, device=dev)
    steps, costs = torch.full((1,), 7, dtype=torch.int32, device=dev), torch.full((1,), 7.0, dtype=torch.float32, device=dev)

    def call(BR, BC):
        with torch.cuda.device(dev):
            return lib.sylber_dtw_strings_align_split(_vp(xd), 300, _vp(nrm), _vp(xd), 300, _vp(nrm), 16, 0, xw.ctypes.data_as(i32p), yw.ctypes.data_as(i32p),
                                                      1, 0, None, None, _vp(steps), _vp(costs), None, BR, BC, _vp(ws), _stream(dev))
    for BR, BC in ((100, 128), (128, 100), (-128, 128), (128, -128), (65664, 128)):
        assert call(BR, BC) == 1 and lib.sylber_last_error().decode().startswith("sylber_dtw_strings_align_split")
    torch.cuda.synchronize()
    assert int(steps[0]) == 7 and float(costs[0]) == 7.0
    assert call(128, 128) == 0
    c1, s1 = costs.clone(), steps.clone()
    assert call(0, 0) == 0                                        # 0: the library's choice
    want = align_sequences([x], [x[:200]], device=DEV, split=False)
    _equal((c1, s1), want)
    _equal((costs, steps), want)


def test_a_realistic_pair_with_automatic_blocks():
    """one pair of 2048 x 2048 at D = 768: the automatic rule splits it, and the bits are the one-workgroup kernel's"""
    from sylber_amd import align_sequences
    from sylber_amd import search as S
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn((2048, 768), generator=g, device=DEV)
    y = x + 0.5 * torch.randn((2048, 768), generator=g, device=DEV)
    dev = torch.device(DEV)
    plan = S._split_plan(np.array([2048]), np.array([2048]), None, None, dev)
    assert plan is not None and plan[0].tolist() == [True] and plan[1:] == S.SPLIT_BLOCK
    # the rule: at least 2 x 2 blocks and SPLIT_MIN_CELLS cells, in a launch of fewer pairs than CUs
    ml, Ll = np.array([256, 255, 64, 4096, 500]), np.array([256, 255, 4096, 128, 500])
    assert S._split_plan(ml, Ll, None, None, dev)[0].tolist() == [True, False, False, False, True]
    assert S._split_plan(ml, Ll, None, 2, dev)[0].tolist() == [True, False, False, False, True]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert S._split_plan(np.full(cus, 500), np.full(cus, 500), None, None, dev) is None
    assert S._split_plan(np.full(cus, 500), np.full(cus, 500), None, cus - 1, dev) is not None
    base = align_sequences([x], [y], path=True, device=DEV, split=False)
    _equal(align_sequences([x], [y], path=True, device=DEV), base)
    _equal(align_sequences([x], [y], device=DEV), base[1:3])
    assert torch.isfinite(base[1]).all() and 2048 <= int(base[2][0]) <= 4095

"""CPU tier for the inverted-file search: the numpy restatement (tests/ivf_ref.py) against the exact restatement (tests/knn_ref.py),
and the library's host-only work-item table (``sylber_ivf_work_items``) against its Python restatement and its covering property."""
import ctypes

import numpy as np
import pytest

import ivf_ref as I
import knn_ref as R


def _data(seed, N=700, D=16, n=25, ncent=12):
    rng = np.random.default_rng(seed)
    cent = 3.0 * rng.standard_normal((ncent, D))
    w = rng.dirichlet(np.full(ncent, 0.6))
    x = (cent[rng.choice(ncent, N, p=w)] + rng.standard_normal((N, D))).astype(np.float32)
    q = (cent[rng.choice(ncent, n)] + rng.standard_normal((n, D))).astype(np.float32)
    c = x[rng.choice(N, ncent, replace=False)]
    d_x = ((x[:, None, :].astype(np.float64) - c[None]) ** 2).sum(2)
    d_q = ((q[:, None, :].astype(np.float64) - c[None]) ** 2).sum(2)
    return x, q, np.argmin(d_x, 1), np.argsort(d_q, 1, kind="stable")


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_all_lists_is_the_exact_search(metric):
    x, q, labels, probe = _data(1)
    g = np.arange(len(x)) % 7
    for kw in ({}, {"q_group": np.arange(len(q)) % 7, "x_group": g}):
        s, i = I.search(q, x, 9, labels, probe, metric, **kw)
        s0, i0 = R.search(q, x, 9, metric, **kw)
        assert np.array_equal(i, i0) and np.array_equal(s, s0)


def test_candidates_are_nested_and_recall_never_decreases():
    x, q, labels, probe = _data(2)
    k = 10
    _, exact = R.search(q, x, k)
    prev_recall = np.zeros(len(q))
    prev = [set()] * len(q)
    for nprobe in range(1, probe.shape[1] + 1):
        _, ids = I.search(q, x, k, labels, probe[:, :nprobe])
        for r in range(len(q)):
            cand = set(I.candidates(labels, probe[r, :nprobe]).tolist())
            assert prev[r] <= cand
            prev[r] = cand
            assert set(ids[r][ids[r] >= 0].tolist()) <= cand
        recall = np.array([len(set(ids[r].tolist()) & set(exact[r].tolist())) / k for r in range(len(q))])
        assert np.all(recall >= prev_recall)
        prev_recall = recall
    assert np.all(prev_recall == 1.0)


def test_unlisted_rows_and_missing_probe_slots():
    x, q, labels, probe = _data(3)
    labels = labels.copy()
    labels[:50] = -1
    probe = probe[:, :3].copy()
    probe[0] = -1
    s, i = I.search(q, x, 5, labels, probe)
    assert np.all(i[0] == -1) and np.all(np.isinf(s[0]))
    assert not (set(i.ravel().tolist()) & set(range(50)))


def _lib_items(lib, pc, off, item_tiles):
    i32p = ctypes.POINTER(ctypes.c_int32)
    pc = np.ascontiguousarray(pc, np.int32)
    off = np.ascontiguousarray(off, np.int32)
    cuts = ctypes.c_int32(0)
    W = lib.sylber_ivf_work_items(pc.ctypes.data_as(i32p), off.ctypes.data_as(i32p), len(pc), item_tiles, None, 0, ctypes.byref(cuts))
    assert W >= 0
    items = np.full((max(W, 1), 8), -7, np.int32)
    assert lib.sylber_ivf_work_items(pc.ctypes.data_as(i32p), off.ctypes.data_as(i32p), len(pc), item_tiles, items.ctypes.data_as(i32p), W,
                                     ctypes.byref(cuts)) == W
    if W:       # one item too few is refused, nothing is written behind the capacity
        assert lib.sylber_ivf_work_items(pc.ctypes.data_as(i32p), off.ctypes.data_as(i32p), len(pc), item_tiles, items.ctypes.data_as(i32p),
                                         W - 1, ctypes.byref(cuts)) == -1
    return items[:W], cuts.value


def _check_cover(items, cuts, pc, off):
    """every pair of every probed list is in exactly one item per cut, and the cuts of its list tile the list's rows exactly once"""
    pc, off = np.asarray(pc, np.int64), np.asarray(off, np.int64)
    begin = np.concatenate([[0], np.cumsum(pc)])
    ranges = {}
    for l, pb, cnt, r0, r1, c, last, t0 in items.tolist():
        assert 1 <= cnt <= 128 and pc[l] > 0 and begin[l] <= pb and pb + cnt <= begin[l + 1]
        assert r0 == min(off[l] + 128 * t0, max(off[l + 1], off[l])) or r0 == off[l] + 128 * t0
        assert off[l] <= r0 <= r1 <= off[l + 1] and 0 <= c < cuts
        for p in range(pb, pb + cnt):
            ranges.setdefault(p, []).append((c, r0, r1, last))
    assert sorted(ranges) == list(range(int(pc.sum())))
    for p, rs in ranges.items():
        l = int(np.searchsorted(begin, p, side="right") - 1)
        rs.sort()
        assert [r[0] for r in rs] == list(range(len(rs))) and [r[3] for r in rs] == [0] * (len(rs) - 1) + [1]
        assert rs[0][1] == off[l] and rs[-1][2] == off[l + 1]
        for a, b in zip(rs, rs[1:]):
            assert a[2] == b[1] and (a[2] - a[1]) % 128 == 0 and a[2] > a[1]


CASES = {
    # name: (list sizes, pair counts)
    "empty lists, an unprobed list, > 128 queries": ([0, 1, 127, 128, 129, 0, 5000, 300], [3, 1, 0, 130, 128, 0, 257, 1]),
    "one query": ([40, 0, 900], [0, 0, 1]),
    "one query on an empty list": ([0, 10], [1, 0]),
    "a list of 100 tiles": ([12800, 12801, 1], [5, 200, 1]),
    "nothing probed": ([5, 6], [0, 0]),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("item_tiles", [0, 1, 2, 16])
def test_work_items_cover_every_pair_and_tile_once(case, item_tiles):
    from sylber_amd import _lib, build
    build.build()
    lib = _lib.load()
    sizes, pc = CASES[case]
    off = np.concatenate([[0], np.cumsum(sizes)])
    items, cuts = _lib_items(lib, pc, off, item_tiles)
    ref, ref_cuts = I.work_items(pc, off, item_tiles)
    assert np.array_equal(items, ref) and cuts == ref_cuts and 1 <= cuts <= 16
    _check_cover(items, cuts, pc, off)
    if item_tiles:      # items hold item_tiles tiles at most, more only where a probed list would otherwise need more than 16 cuts
        longest = max([-(-s // 128) for s, p in zip(sizes, pc) if p] + [0])
        assert all((r1 - r0 + 127) // 128 <= max(item_tiles, -(-longest // 16)) for _, _, _, r0, r1, _, _, _ in items.tolist())


@pytest.mark.parametrize("seed", range(6))
def test_work_items_seeded(seed):
    from sylber_amd import _lib, build
    build.build()
    lib = _lib.load()
    rng = np.random.default_rng(seed)
    nlist = int(rng.integers(1, 60))
    sizes = (rng.integers(0, 3, nlist) * rng.integers(0, 2500, nlist)).astype(np.int64)
    pc = (rng.integers(0, 2, nlist) * rng.integers(0, 400, nlist)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for item_tiles in (0, 1, 3):
        items, cuts = _lib_items(lib, pc, off, item_tiles)
        ref, ref_cuts = I.work_items(pc, off, item_tiles)
        assert np.array_equal(items, ref) and cuts == ref_cuts
        _check_cover(items, cuts, pc, off)


def test_work_items_refuses_bad_arguments():
    from sylber_amd import _lib, build
    build.build()
    lib = _lib.load()
    i32p = ctypes.POINTER(ctypes.c_int32)
    a = np.array([1, -1], np.int32)
    off = np.array([0, 5, 3], np.int32)
    assert lib.sylber_ivf_work_items(a.ctypes.data_as(i32p), off.ctypes.data_as(i32p), 2, 0, None, 0, None) == -1
    assert lib.sylber_ivf_work_items(None, off.ctypes.data_as(i32p), 2, 0, None, 0, None) == -1
    assert lib.sylber_ivf_workspace_bytes(0, 1, 1, 1) == -1 and lib.sylber_ivf_workspace_bytes(1, 129, 1, 1) == -1
    assert lib.sylber_ivf_workspace_bytes(100, 32, 10, 2) >= 100 * 32 * 2 * 10 * 8


def test_new_symbols_are_exported():
    from sylber_amd import _lib
    assert {"sylber_ivf_work_items", "sylber_ivf_workspace_bytes", "sylber_ivf_search"} <= set(_lib.EXPORTS)
    import sylber_amd
    assert "IVFSyllableIndex" in sylber_amd.__all__ and hasattr(sylber_amd.IVFSyllableIndex, "build")

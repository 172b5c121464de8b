"""GPU tier, inverted-file syllable search (csrc/knn.hip ``sylber_ivf_search`` behind sylber_amd.IVFSyllableIndex).  Everything is
checked bit for bit, against the exact search (``SyllableIndex``) or against float64 where the fp32 arithmetic is exact:

* ``nprobe == nlist`` is ``SyllableIndex.search``; for any ``nprobe`` every query row is the exact search on the sub-database of
  its probed lists (ids mapped back), lists of 0, 1, 127, 128 and 129 rows and one case of 100 000 rows included;
* the probed lists are the coarse search's ids, the membership is ``sylber_kmeans_assign``'s labels;
* independence of the query chunking, of the cut of lists into work items, of stale workspace contents and of build versus add;
* group exclusion, padding, NaN rows and queries, a NaN row right behind a list's end;
* integer data in [-2, 2] against the float64 restatement (tests/ivf_ref.py), ties included;
* save / load, the ValueErrors, and Segmenter outputs end to end."""
import numpy as np
import pytest
import torch

import ivf_ref as I

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _np(t):
    return t.cpu().numpy()


def _mixture(seed, N, D, n, ncent, spread=0.5):
    """seeded mixture of Gaussians around random centres with uneven weights; queries from the same mixture"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((ncent, D)).astype(np.float32)
    w = rng.dirichlet(np.full(ncent, 0.5))
    x = cent[rng.choice(ncent, N, p=w)] + spread * rng.standard_normal((N, D)).astype(np.float32)
    q = cent[rng.choice(ncent, n)] + spread * rng.standard_normal((n, D)).astype(np.float32)
    return x.astype(np.float32), q.astype(np.float32)


FORCED_SIZES = [0, 1, 127, 128, 129, 300, 128]


def _forced(seed, D, metric, n=96):
    """lists of exactly FORCED_SIZES rows around far-apart centroids (list 0 stays empty); the rows of the lists are interleaved"""
    rng = np.random.default_rng(seed)
    nl = len(FORCED_SIZES)
    cent = np.zeros((nl, D), np.float32)
    cent[np.arange(nl), np.arange(nl)] = 1.0 if metric == "cosine" else 40.0
    lab = rng.permutation(np.repeat(np.arange(nl), FORCED_SIZES))
    scale = 0.02 if metric == "cosine" else 1.0
    x = cent[lab] + scale * rng.standard_normal((len(lab), D)).astype(np.float32)
    # queries between centroids, so that the probe order varies
    a, b = rng.integers(0, nl, n), rng.integers(0, nl, n)
    t = rng.uniform(0, 1, (n, 1)).astype(np.float32)
    q = t * cent[a] + (1 - t) * cent[b] + scale * rng.standard_normal((n, D)).astype(np.float32)
    return x.astype(np.float32), q.astype(np.float32), cent, lab


def _sub_index(index, cand):
    """the exact index over the STORED rows ``cand`` of ``index`` (stored rows, norms and groups as they are: no second normalisation)"""
    from sylber_amd import SyllableIndex
    sub = SyllableIndex(metric=index.metric, device=index.device)
    c = torch.from_numpy(np.asarray(cand, np.int64)).to(index.device)
    sub.dim, sub._x, sub._g = index.dim, index._x.index_select(0, c).contiguous(), index._g.index_select(0, c).contiguous()
    sub._c = index._c.index_select(0, c).contiguous() if index._c is not None else None
    sub._prov = np.full((len(cand), 4), -1.0)
    return sub


def _check_rows_are_exact_on_probed_lists(ivf, q, k, nprobe, s, i, rows=None, groups=None):
    labels = _np(ivf.labels)
    probe = _np(ivf.probe(q, nprobe))
    s, i = _np(s), _np(i)
    for r in (range(q.shape[0]) if rows is None else rows):
        cand = I.candidates(labels, probe[r])
        if len(cand) == 0:
            assert np.all(i[r] == -1) and np.all(np.isinf(s[r])), r
            continue
        kw = {} if groups is None else {"groups": groups[r:r + 1], "exclude_same_group": True}
        es, ei = _sub_index(ivf.index, cand).search(q[r:r + 1], k, **kw)
        es, ei = _np(es)[0], _np(ei)[0]
        ei = np.where(ei >= 0, cand[np.maximum(ei, 0)], -1)
        assert np.array_equal(i[r], ei) and np.array_equal(s[r].view(np.uint32), es.view(np.uint32)), (r, nprobe)


@pytest.mark.parametrize("D", [16, 768])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_all_lists_probed_is_the_exact_search_bitwise(metric, D):
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    x, q = _mixture(D, 4099, D, 200, 30)
    index = SyllableIndex(x, metric=metric, device=DEV)
    ivf = IVFSyllableIndex.build(index, nlist=24, seed=1, max_iter=5)
    assert ivf.nlist == 24 and len(ivf) == 4099 and tuple(ivf.centroids.shape) == (24, D)
    assert ivf.list_sizes.dtype == torch.int64 and int(ivf.list_sizes.sum()) == 4099
    for k in (1, 10, 128):
        es, ei = index.search(q, k)
        s, i = ivf.search(q, k, nprobe=24)
        assert s.dtype == torch.float32 and i.dtype == torch.int64
        assert torch.equal(i, ei) and torch.equal(s.view(torch.int32), es.view(torch.int32)), k
        assert ivf.last_search["pairs"] == 200 * 4099 and ivf.last_search["fraction"] == 1.0


@pytest.mark.parametrize("D", [16, 768])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_every_row_is_exact_on_its_probed_lists(metric, D):
    from sylber_amd import IVFSyllableIndex
    x, q = _mixture(100 + D, 4099, D, 120, 50)
    ivf = IVFSyllableIndex.build(x, nlist=40, seed=2, max_iter=4, metric=metric, device=DEV)
    sizes = _np(ivf.list_sizes)
    assert sizes.max() > 2 * sizes.mean()                    # uneven lists
    for nprobe in (1, 3, 32):
        for k in (1, 10):
            s, i = ivf.search(q, k, nprobe=nprobe)
            _check_rows_are_exact_on_probed_lists(ivf, q, k, nprobe, s, i)
        assert 0 < ivf.last_search["fraction"] < 1.0


@pytest.mark.parametrize("D", [16, 768])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_forced_list_sizes_0_1_127_128_129(metric, D):
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    x, q, cent, lab = _forced(5, D, metric)
    index = SyllableIndex(x, metric=metric, device=DEV)
    ivf = IVFSyllableIndex.build(index, centroids=cent)
    assert _np(ivf.list_sizes).tolist() == FORCED_SIZES and np.array_equal(_np(ivf.labels), lab)
    nl = len(FORCED_SIZES)
    for k in (1, 10, 128):
        es, ei = index.search(q, k)
        s, i = ivf.search(q, k, nprobe=nl)
        assert torch.equal(i, ei) and torch.equal(s, es)
        for nprobe in (1, 3):
            for item_tiles in (0, 1):
                s, i = ivf.search(q, k, nprobe=nprobe, item_tiles=item_tiles)
                _check_rows_are_exact_on_probed_lists(ivf, q, k, nprobe, s, i)
    # a query whose only list holds one row, k = 10: one hit, then (-1, +inf); the empty list gives nothing at all
    one = cent[1:2].copy()
    s, i = ivf.search(one, 10, nprobe=1)
    assert _np(i)[0, 0] == np.nonzero(lab == 1)[0][0] and bool((i[0, 1:] == -1).all()) and bool(torch.isinf(s[0, 1:]).all())
    s, i = ivf.search(cent[0:1].copy(), 10, nprobe=1)
    if int(ivf.probe(cent[0:1].copy(), 1)[0, 0]) == 0:
        assert bool((i == -1).all()) and bool(torch.isinf(s).all())


def test_large_index_sampled_rows():
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    N, D, n = 100003, 768, 1500
    x, q = _mixture(7, N, D, n, 300)
    index = SyllableIndex(x, device=DEV)
    ivf = IVFSyllableIndex.build(index, nlist=256, seed=0, max_iter=3, train_rows=20000)
    sample = np.sort(np.random.default_rng(8).choice(n, 256, replace=False))
    k = 10
    _, exact = index.search(q, k)
    recall = []
    for nprobe in (1, 3, 32):
        s, i = ivf.search(q, k, nprobe=nprobe)
        _check_rows_are_exact_on_probed_lists(ivf, q, k, nprobe, s, i, rows=sample)
        recall.append(float((i[:, :, None] == exact[:, None, :]).any(2).float().mean()))
        assert ivf.last_search["fraction"] == ivf.last_search["pairs"] / (n * N) and 0 < ivf.last_search["fraction"] < 1
        print("N = %d, nlist = 256, nprobe = %d: recall@10 %.3f, fraction %.4f" % (N, nprobe, recall[-1], ivf.last_search["fraction"]))
    assert recall[0] <= recall[1] <= recall[2], recall            # the candidate sets are nested
    # some list is probed by more than 128 of the 1 500 queries and some list is longer than one tile
    probe = _np(ivf.probe(q, 32))
    assert np.bincount(probe.ravel(), minlength=256).max() > 128 and int(ivf.list_sizes.max()) > 129
    s2, i2 = ivf.search(q, k, nprobe=32, item_tiles=1, query_chunk=700)
    assert torch.equal(i2, i) and torch.equal(s2, s)


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_probes_and_membership(metric):
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    from sylber_amd import kmeans as KM
    x, q = _mixture(9, 3000, 64, 100, 20)
    index = SyllableIndex(x, metric=metric, device=DEV)
    ivf = IVFSyllableIndex.build(index, nlist=17, seed=3, max_iter=6)
    fit = KM.fit_kmeans(index.features, 17, seed=3, max_iter=6)
    assert torch.equal(ivf.centroids, fit.centroids)
    lab = KM.assign(index.features, ivf.centroids)[0].to(torch.int64)
    assert torch.equal(ivf.labels, lab) and torch.equal(ivf.list_sizes, torch.bincount(lab, minlength=17))
    for l in range(17):
        assert torch.equal(ivf.list_ids(l), torch.nonzero(lab == l)[:, 0])
    qd = index._prep(torch.from_numpy(q))
    for nprobe in (1, 3, 17):
        want = SyllableIndex(ivf.centroids, metric="l2", device=DEV).search(qd, nprobe)[1]
        assert torch.equal(ivf.probe(q, nprobe), want)
    assert torch.equal(ivf.probe(q, 17)[:, :3], ivf.probe(q, 3))          # nested in nprobe


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_bitwise_independent_of_chunks_work_items_workspace_and_adds(metric):
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    N, D, n, k = 20000, 128, 300, 17
    x, q = _mixture(11, N, D, n, 40)
    x[5000:5100] = x[4000:4100]                                            # exact ties
    q[:20] = x[4000:4020]
    g = np.arange(N) % 11
    ivf = IVFSyllableIndex.build(SyllableIndex(x, metric=metric, groups=g, device=DEV), nlist=32, seed=4, max_iter=5)
    assert int(ivf.list_sizes.max()) > 3 * 128
    for nprobe in (1, 5, 32):
        ref = ivf.search(q, k, nprobe=nprobe)
        for kw in ({"query_chunk": 1}, {"query_chunk": 77}, {"item_tiles": 1}, {"item_tiles": 2, "query_chunk": 100},
                   {"_workspace_fill": 0xFF}, {"_workspace_fill": 0x7F, "item_tiles": 3}):
            s, i = ivf.search(q, k, nprobe=nprobe, **kw)
            assert torch.equal(i, ref[1]) and torch.equal(s.view(torch.int32), ref[0].view(torch.int32)), (nprobe, kw)
    grown = IVFSyllableIndex.build(SyllableIndex(x[:7000], metric=metric, groups=g[:7000], device=DEV), centroids=ivf.centroids)
    assert grown.add(x[7000:7129], groups=g[7000:7129]) == range(7000, 7129)
    assert grown.add(x[7129:], groups=g[7129:]) == range(7129, N)
    assert torch.equal(grown.labels, ivf.labels) and torch.equal(grown.list_sizes, ivf.list_sizes)
    qg = np.arange(n) % 11
    for kw in ({}, {"groups": qg, "exclude_same_group": True}):
        a, b = ivf.search(q, k, nprobe=5, **kw), grown.search(q, k, nprobe=5, **kw)
        assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def test_group_exclusion_and_padding():
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    x, q = _mixture(12, 3000, 64, 60, 15)
    xg = np.random.default_rng(12).integers(0, 5, 3000)
    q = x[:60] + 0.01 * q
    qg = xg[:60]
    ivf = IVFSyllableIndex.build(SyllableIndex(x, groups=xg, device=DEV), nlist=12, seed=0, max_iter=5)
    for nprobe in (2, 12):
        s, i = ivf.search(q, 20, nprobe=nprobe, groups=qg, exclude_same_group=True)
        ii = _np(i)
        assert np.all(xg[np.maximum(ii, 0)][ii >= 0] != np.broadcast_to(qg[:, None], ii.shape)[ii >= 0])
        _check_rows_are_exact_on_probed_lists(ivf, q, 20, nprobe, s, i, groups=qg)
    es, ei = ivf.index.search(q, 20, groups=qg, exclude_same_group=True)
    assert torch.equal(i, ei) and torch.equal(s, es)
    whole = IVFSyllableIndex.build(SyllableIndex(x, groups=np.full(3000, 9), device=DEV), centroids=ivf.centroids)
    s, i = whole.search(q[:3], 5, nprobe=4, groups=[9, 9, 9], exclude_same_group=True)
    assert bool((i == -1).all()) and bool(torch.isinf(s).all())


def test_nan_rows_nan_queries_and_a_nan_row_behind_a_lists_end(tmp_path):
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    x, q, cent, lab = _forced(6, 32, "l2", n=64)
    ivf = IVFSyllableIndex.build(SyllableIndex(x, device=DEV), centroids=cent)
    k = 8
    clean = {p: ivf.search(q, k, nprobe=p) for p in (1, 3)}
    # NaN rows at build time are in no list and never returned; the other rows keep their places
    xb = x.copy()
    bad = [int(v) for v in _np(clean[1][1])[:5, 0]]
    xb[bad] = np.nan
    ivb = IVFSyllableIndex.build(SyllableIndex(xb, device=DEV), centroids=cent)
    assert bool((ivb.labels[bad] == -1).all()) and int(ivb.list_sizes.sum()) == len(x) - len(set(bad))
    for p in (1, 3):
        s, i = ivb.search(q, k, nprobe=p)
        assert not (set(_np(i).ravel().tolist()) & set(bad))
        _check_rows_are_exact_on_probed_lists(ivb, q, k, p, s, i)
    # NaN queries get nothing and disturb nobody
    qb = q.copy()
    qb[[2, 40]] = np.nan
    keep = [r for r in range(64) if r not in (2, 40)]
    for p in (1, 3):
        s, i = ivf.search(qb, k, nprobe=p, _workspace_fill=0xFF)
        assert bool((i[[2, 40]] == -1).all()) and bool(torch.isinf(s[[2, 40]]).all())
        assert torch.equal(i[keep], clean[p][1][keep]) and torch.equal(s[keep], clean[p][0][keep])
    # a row that is NaN and lies right behind the end of the 127-row list (the first row of the next list): a saved index whose
    # rows are edited keeps its list assignment on load, so the NaN row stays in its list
    path = str(tmp_path / "ivf.npz")
    ivf.save(path)
    z = dict(np.load(path))
    first_of_3 = int(np.nonzero(lab == 3)[0][0])
    z["features"][first_of_3] = np.nan
    np.savez(path, **z)
    back = IVFSyllableIndex.load(path, device=DEV)
    assert int(back.labels[first_of_3]) == 3 and int(back.list_ids(3)[0]) == first_of_3
    only2 = np.nonzero(_np(ivf.probe(q, 1))[:, 0] == 2)[0]
    assert len(only2) > 0
    s, i = back.search(q, k, nprobe=1)
    assert torch.equal(i[only2], clean[1][1][only2]) and torch.equal(s[only2], clean[1][0][only2])
    assert first_of_3 not in set(_np(i).ravel().tolist())
    s, i = back.search(q, 128, nprobe=len(FORCED_SIZES))
    assert first_of_3 not in set(_np(i).ravel().tolist())
    _check_rows_are_exact_on_probed_lists(back, q, 128, len(FORCED_SIZES), s, i)


def test_integer_data_equals_float64_exactly():
    """entries in [-2, 2], D = 768: every product and partial sum is an integer of magnitude <= 4 x 768 = 3 072 < 2^24, so the fp32
    scores are exact and the float64 restatement gives identical ids and scores, ties included"""
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    rng = np.random.default_rng(21)
    N, D, n, nlist = 5000, 768, 80, 16
    proto = rng.integers(-2, 3, (nlist, D))
    x = proto[rng.integers(0, nlist, N)].copy()
    flip = rng.random((N, D)) < 0.02
    x[flip] = rng.integers(-2, 3, int(flip.sum()))
    x[100:140] = x[60:100]                                                 # exact duplicates: ties by id
    q = x[rng.integers(0, N, n)].copy()
    flip = rng.random((n, D)) < 0.02
    q[flip] = rng.integers(-2, 3, int(flip.sum()))
    q[:10] = x[60:70]                                                      # distance 0 to rows 60 + r and 100 + r
    x, q = x.astype(np.float32), q.astype(np.float32)
    xg, qg = rng.integers(0, 4, N), rng.integers(0, 4, n)
    ivf = IVFSyllableIndex.build(SyllableIndex(x, groups=xg, device=DEV), centroids=proto.astype(np.float32))
    labels = _np(ivf.labels)
    ties = 0
    for nprobe in (1, 3, 16):
        probe = _np(ivf.probe(q, nprobe))
        for k in (1, 10, 128):
            for kw, rkw in (({}, {}), ({"groups": qg, "exclude_same_group": True}, {"q_group": qg, "x_group": xg})):
                s, i = ivf.search(q, k, nprobe=nprobe, **kw)
                rs, ri = I.search(q, x, k, labels, probe, "l2", **rkw)
                assert np.array_equal(_np(i), ri) and np.array_equal(_np(s).astype(np.float64), rs), (nprobe, k)
                ties += int((rs[:, 1:] == rs[:, :-1])[np.isfinite(rs[:, 1:])].sum())
    assert ties > 0


def test_save_load_round_trip(tmp_path):
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    x, q = _mixture(13, 2500, 48, 70, 12)
    g = np.arange(2500) % 9
    for metric in ("l2", "cosine"):
        ivf = IVFSyllableIndex.build(SyllableIndex(x, metric=metric, groups=g, device=DEV), nlist=10, seed=5, max_iter=4)
        p = str(tmp_path / ("ivf_%s.npz" % metric))
        ivf.save(p)
        back = IVFSyllableIndex.load(p, device=DEV)
        assert back.metric == metric and back.nlist == 10 and len(back) == 2500
        assert torch.equal(back.centroids, ivf.centroids) and torch.equal(back.labels, ivf.labels) and torch.equal(back.list_sizes, ivf.list_sizes)
        assert torch.equal(back.index.features, ivf.index.features)
        for kw in ({}, {"groups": np.arange(70) % 9, "exclude_same_group": True}):
            a, b = ivf.search(q, 10, nprobe=3, **kw), back.search(q, 10, nprobe=3, **kw)
            assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    plain = str(tmp_path / "plain.npz")
    ivf.index.save(plain)
    with pytest.raises(ValueError):
        IVFSyllableIndex.load(plain, device=DEV)


def test_value_errors():
    from sylber_amd import IVFSyllableIndex, SyllableIndex
    x = np.random.default_rng(0).standard_normal((200, 16)).astype(np.float32)
    index = SyllableIndex(x, groups=np.arange(200), device=DEV)
    q = x[:2]
    for nlist in (0, -1, 201, 2.5, None):
        with pytest.raises(ValueError):
            IVFSyllableIndex.build(index, nlist=nlist)
    with pytest.raises(ValueError):
        IVFSyllableIndex.build(SyllableIndex(device=DEV), nlist=1)                       # empty
    with pytest.raises(ValueError):
        IVFSyllableIndex.build(np.ones((40, 24), np.float32), nlist=2, device=DEV)        # D % 16
    with pytest.raises(ValueError):
        IVFSyllableIndex.build(index, centroids=np.ones((3, 32), np.float32))
    with pytest.raises(ValueError):
        IVFSyllableIndex.build(index, centroids=np.full((3, 16), np.nan, np.float32))
    with pytest.raises(ValueError):
        IVFSyllableIndex.build(index, nlist=4, centroids=np.ones((3, 16), np.float32))
    ivf = IVFSyllableIndex.build(index, nlist=8, seed=0)
    for nprobe in (0, 9, 1.5, True):
        with pytest.raises(ValueError):
            ivf.search(q, 1, nprobe=nprobe)
    for k in (0, 129, 1.5, True):
        with pytest.raises(ValueError):
            ivf.search(q, k, nprobe=2)
    with pytest.raises(ValueError):
        ivf.search(np.ones((2, 32), np.float32), 1, nprobe=2)
    with pytest.raises(ValueError):
        ivf.search(q, 1, nprobe=2, exclude_same_group=True)
    with pytest.raises(ValueError):
        ivf.search(q, 1, nprobe=2, groups=[1, 2, 3], exclude_same_group=True)
    with pytest.raises(ValueError):
        ivf.add(np.ones((3, 32), np.float32))
    big = IVFSyllableIndex.build(np.random.default_rng(1).standard_normal((400, 16)).astype(np.float32), nlist=200, max_iter=2, device=DEV)
    with pytest.raises(ValueError):
        big.search(q, 1, nprobe=129)
    s, i = big.search(q, 3, nprobe=128)
    assert tuple(i.shape) == (2, 3)


def test_segmenter_outputs_end_to_end():
    from sylber_amd import IVFSyllableIndex, Segmenter, SyllableIndex
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_state_dict
    seg = Segmenter(model_ckpt=synthetic_state_dict(0), device=DEV)
    wavs = [syllable_wave(int(m), s) for s, m in enumerate([32000, 24000, 40000, 28000], start=70)]
    outs = seg(wav=wavs, in_second=False)
    counts = [len(o["segments"]) for o in outs]
    assert sum(c > 0 for c in counts) >= 3, counts
    index = SyllableIndex.from_outputs(outs)
    ivf = IVFSyllableIndex.build(index, nlist=3, seed=0)
    assert len(ivf) == sum(counts)
    feats = np.concatenate([o["segment_features"] for o in outs if len(o["segments"])])
    clip = np.concatenate([np.full(c, ci) for ci, c in enumerate(counts)])
    k = 5
    s, i = ivf.search(feats, k, nprobe=2, groups=clip, exclude_same_group=True)
    _check_rows_are_exact_on_probed_lists(ivf, feats, k, 2, s, i, groups=clip)
    hits = 0
    for r in range(len(feats)):
        for j in _np(i)[r]:
            if j < 0:
                continue
            c, sg, st, en = ivf.provenance([j])[0]
            assert c != clip[r] and [st, en] == outs[c]["segments"][sg].tolist()
            hits += 1
    assert hits > 0
    es, ei = index.search(feats, k, groups=clip, exclude_same_group=True)
    s, i = ivf.search(feats, k, nprobe=3, groups=clip, exclude_same_group=True)
    assert torch.equal(i, ei) and torch.equal(s, es)

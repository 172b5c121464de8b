"""CPU tier: the numpy restatement of the product-quantization contract (tests/pq_ref.py) is itself checked -- its encode and
decode against each other, its composition against knn_ref.search, its fp32 scan against an explicit loop, the chain bound against an
explicit fp32 fmaf chain, and the share of decisions the GPU tier's float64 encode test may leave undecided."""
import numpy as np
import pytest

import knn_ref as R
import pq_ref as P


def test_encoding_the_centroids_returns_their_indices_and_decode_is_exact():
    rng = np.random.default_rng(0)
    M, dsub = 3, 16
    C = rng.standard_normal((M, P.KSUB, dsub)).astype(np.float32)
    own = np.concatenate([C[m] for m in range(M)], 1)                    # row c = centroid c of every sub-space
    codes, bad = P.encode(own, C)
    assert np.array_equal(codes, np.repeat(np.arange(256, dtype=np.uint8)[:, None], M, 1)) and not bad.any()
    pick = rng.integers(0, P.KSUB, (500, M))
    x = P.decode(pick, C)
    assert x.dtype == np.float32 and x.shape == (500, M * dsub)
    codes, bad = P.encode(x, C)
    assert np.array_equal(codes, pick) and not bad.any()
    assert np.array_equal(P.decode(codes, C).view(np.uint32), x.view(np.uint32))
    # ties go to the smaller index; a NaN anywhere in a sub-row gives code 0 and masks the row, the other sub-rows keep their codes
    C2 = C.copy()
    C2[1, 200] = C2[1, 7]
    assert P.encode(P.decode(np.array([[3, 200, 5]]), C2), C2)[0].tolist() == [[3, 7, 5]]
    y = x[:4].copy()
    y[1, dsub + 2] = np.nan
    codes, bad = P.encode(y, C)
    assert bad.tolist() == [False, True, False, False] and codes[1].tolist() == [pick[1, 0], 0, pick[1, 2]]


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_rerank_with_enough_candidates_is_the_exact_reference(metric):
    rng = np.random.default_rng(3)
    q, x, C = P.clustered(3, 37, 32, 2, 9, noise=0.5)
    x[5] = np.nan
    x[11] = 0
    xg, qg = rng.integers(0, 3, 37), rng.integers(0, 3, 9)
    for groups in (False, True):
        kw = dict(q_group=qg, x_group=xg) if groups else {}
        s, i, cand = P.search(q, x, C, 10, 4, metric, **kw)              # m_c = 40 >= 37
        es, ei = R.search(q, x, 10, metric, **kw)
        assert np.array_equal(i, ei) and np.array_equal(s, es) and cand.shape == (9, 40)
        assert metric == "cosine" or not np.isin(5, cand)               # knn_ref.unit_rows makes the NaN row a zero row under cosine
    # a short list is the exact order restricted to the candidates; without re-ranking it is the scan's own order and values
    s, i, cand = P.search(q, x, C, 3, 2, metric)
    full = R.scores(q, x, metric)
    for r in range(9):
        c = cand[r][cand[r] >= 0]
        assert i[r].tolist() == c[np.lexsort((c, full[r, c]))][:3].tolist()
    s, i, cand = P.search(q, x, C, 5, metric=metric, rerank=False)
    assert cand.shape == (9, 5) and np.array_equal(i, cand)
    assert np.all(np.diff(s, axis=1) >= 0) if metric == "l2" else np.all(np.diff(s, axis=1) <= 0)


def test_scan_t_is_the_ascending_fp32_sum():
    rng = np.random.default_rng(4)
    table = (rng.standard_normal((3, 5, P.KSUB)) * 10.0 ** rng.integers(-3, 4, (3, 5, 1))).astype(np.float32)
    codes = rng.integers(0, P.KSUB, (40, 5)).astype(np.uint8)
    t = P.scan_t(table, codes)
    assert t.dtype == np.float32
    for i in range(3):
        for j in range(40):
            acc = table[i, 0, codes[j, 0]]
            for m in range(1, 5):
                acc = np.float32(acc + table[i, m, codes[j, m]])
            assert acc.view(np.uint32) == t[i, j].view(np.uint32)
    bad = np.zeros(40, bool)
    bad[int(np.argmin(t[0]))] = True
    tc, cand = P.candidates(t, 50, bad)
    assert (cand[:, 39:] == -1).all() and np.isinf(tc[:, 39:]).all() and not np.isin(np.nonzero(bad)[0][0], cand)
    assert np.all(np.diff(tc[:, :39], axis=1) >= 0)


def test_chain_bound_covers_an_fp32_fmaf_chain_and_few_decisions_stay_open():
    """standard-normal rows and centroids at dsub = 16: the bound holds for an explicit chain (float64 products rounded once per
    step = fmaf), and the float64 gap decides all but a handful of 12 000 decisions (the GPU tier's encode test allows 1 %)"""
    rng = np.random.default_rng(5)
    M, dsub, n = 48, 16, 250
    C = rng.standard_normal((M, P.KSUB, dsub)).astype(np.float32)
    x = rng.standard_normal((n, M * dsub)).astype(np.float32)
    ok = P.decided(x, C)
    print("undecided: %d of %d" % (int((~ok).sum()), ok.size))
    assert (~ok).sum() <= 0.01 * ok.size
    xs = x.reshape(n, M, dsub)[:8]
    dot = np.zeros((8, M, P.KSUB), np.float32)
    for k in range(dsub):
        dot = (xs[:, :, None, k].astype(np.float64) * C[None, :, :, k].astype(np.float64) + dot.astype(np.float64)).astype(np.float32)
    cn = np.zeros((M, P.KSUB), np.float32)
    for k in range(dsub):
        cn = (C[:, :, k].astype(np.float64) ** 2 + cn.astype(np.float64)).astype(np.float32)
    got = (-2.0 * dot.astype(np.float64) + cn[None].astype(np.float64)).astype(np.float32).astype(np.float64)
    assert np.all(np.abs(got - P.sub_scores(x[:8], C)) <= P.chain_bound(x[:8], C))

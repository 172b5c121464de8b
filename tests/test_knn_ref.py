"""CPU tier: tests/knn_ref.py (the k-NN search contract in float64) against brute force and hand-built ties."""
import numpy as np
import pytest

import knn_ref as R


def _brute(q, x, k, metric="l2", qg=None, xg=None):
    s = R.scores(q, x, metric)
    ids = []
    for i in range(len(q)):
        cand = [(s[i, j], j) for j in range(len(x)) if not np.isnan(s[i, j]) and (qg is None or xg[j] != qg[i])]
        cand.sort()
        ids.append([j for _, j in cand[:k]] + [-1] * (k - min(k, len(cand))))
    return np.array(ids, np.int64)


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("k", [1, 3, 10, 40])
def test_search_matches_stable_argsort(metric, k):
    rng = np.random.default_rng(k)
    q, x = rng.standard_normal((7, 16)), rng.standard_normal((33, 16))
    got_s, got_i = R.search(q, x, k, metric)
    s = R.scores(q, x, metric)
    for i in range(7):
        exp = np.argsort(s[i], kind="stable")[:k]
        m = min(k, 33)
        assert np.array_equal(got_i[i, :m], exp)
        assert np.all(got_i[i, m:] == -1) and np.all(np.isinf(got_s[i, m:]))
    assert np.array_equal(got_i, _brute(q, x, k, metric))
    if metric == "l2":
        d = ((q[:, None, :] - x[None, :, :]) ** 2).sum(2)
        m = min(k, 33)
        assert np.allclose(got_s[:, :m], np.take_along_axis(d, got_i[:, :m], 1))


def test_ties_go_to_the_smaller_id():
    x = np.array([[1.0, 0], [0, 1], [1, 0], [1, 0], [0, 1]])
    q = np.array([[1.0, 0.0]])
    _, i = R.search(q, x, 5)
    assert i.tolist() == [[0, 2, 3, 1, 4]]
    _, i = R.search(q, x, 7)
    assert i.tolist() == [[0, 2, 3, 1, 4, -1, -1]]
    s, i = R.search(q, x, 3, "cosine")
    assert i.tolist() == [[0, 2, 3]] and np.allclose(s, 1.0)


def test_nan_rows_are_never_returned():
    x = np.array([[1.0, 0], [np.nan, 0], [2, 0]])
    _, i = R.search(np.array([[1.0, 0.0]]), x, 3)
    assert i.tolist() == [[0, 2, -1]]
    s, i = R.search(np.array([[np.nan, 0.0], [0.0, 0.0]]), x, 2)
    assert i[0].tolist() == [-1, -1] and np.all(np.isinf(s[0])) and i[1].tolist() == [0, 2]


def test_group_exclusion():
    rng = np.random.default_rng(1)
    q, x = rng.standard_normal((6, 8)), rng.standard_normal((20, 8))
    qg, xg = rng.integers(0, 3, 6), rng.integers(0, 3, 20)
    s, i = R.search(q, x, 25, q_group=qg, x_group=xg)
    assert np.array_equal(i, _brute(q, x, 25, qg=qg, xg=xg))
    for r in range(6):
        got = i[r][i[r] >= 0]
        assert np.all(xg[got] != qg[r]) and len(got) == (xg != qg[r]).sum()
    _, i = R.search(q[:1], x, 4, q_group=[7], x_group=np.full(20, 7))
    assert i.tolist() == [[-1, -1, -1, -1]]


def test_cosine_on_unit_rows_and_zero_rows():
    x = np.array([[3.0, 4], [0, 0], [-1, -1], [0, 0], [1, 0]])
    s, i = R.search(np.array([[0.0, 2.0]]), x, 5, "cosine")
    assert i.tolist() == [[0, 1, 3, 4, 2]]                  # similarity 0 (zero rows and an orthogonal row) ties by id
    assert np.allclose(s, [[0.8, 0.0, 0.0, 0.0, -np.sqrt(0.5)]])
    u = R.unit_rows(x)
    assert np.allclose((u ** 2).sum(1), [1, 0, 1, 0, 1])


def test_dot_error_bound_covers_fp32():
    rng = np.random.default_rng(2)
    q, x = rng.standard_normal((5, 768)).astype(np.float32), rng.standard_normal((50, 768)).astype(np.float32)
    s64 = R.scores(q, x)
    dots = np.zeros((5, 50), np.float32)
    for kk in range(768):                                    # the fmaf chain, one rounding per step (fp64 product is exact)
        dots = (dots.astype(np.float64) + q[:, kk:kk + 1].astype(np.float64) * x[None, :, kk].astype(np.float64)).astype(np.float32)
    cn = (x.astype(np.float64) ** 2).sum(1).astype(np.float32)
    s32 = (cn[None, :].astype(np.float64) - 2.0 * dots.astype(np.float64)).astype(np.float32)
    assert np.all(np.abs(s32 - s64) <= R.dot_error_bound(q, x))

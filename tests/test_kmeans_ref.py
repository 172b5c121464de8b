"""CPU tier: the numpy restatement of the k-means fit (tests/kmeans_ref.py) that the GPU tests compare against -- monotone inertia,
agreement with scikit-learn's Lloyd iterations from the same seeds, exact k-means++ picks on integer data, argument errors -- and the
host-side argument checks of ``sylber_amd.fit_kmeans`` that run before any device work."""
import numpy as np
import pytest

import kmeans_ref as R


def blobs(n_per, K, D, sep=20.0, seed=0):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((K, D)) * sep
    x = np.concatenate([centers[k] + rng.standard_normal((n_per, D)) for k in range(K)]).astype(np.float32)
    truth = np.repeat(np.arange(K), n_per)
    return x, truth


def test_inertia_never_increases():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((600, 16)).astype(np.float32)
    f = R.fit(x, 12, max_iter=30, tol=0.0, init="random", seed=3)
    inert = [h[0] for h in f["history"]] + [f["inertia"]]
    assert all(b <= a * (1 + 1e-12) for a, b in zip(inert, inert[1:])), inert
    assert f["n_iter"] >= 2


def test_matches_sklearn_lloyd_from_the_same_seeds():
    KMeans = pytest.importorskip("sklearn.cluster").KMeans
    x, truth = blobs(50, 6, 16, seed=2)
    c0 = R.init_centroids(x, 6, "k-means++", seed=5)
    f = R.fit(x, 6, max_iter=50, tol=0.0, init=c0)
    sk = KMeans(n_clusters=6, init=c0.astype(np.float64), n_init=1, algorithm="lloyd", max_iter=50, tol=0.0).fit(x.astype(np.float64))
    assert np.array_equal(f["labels"], sk.labels_)
    np.testing.assert_allclose(f["centroids"], sk.cluster_centers_, rtol=1e-5, atol=1e-5)
    # the blobs are recovered up to a permutation
    perm = {int(t): int(l) for t, l in zip(truth, f["labels"])}
    assert len(set(perm.values())) == 6 and all(perm[int(t)] == int(l) for t, l in zip(truth, f["labels"]))


def test_kmeanspp_exact_on_integer_data():
    rng = np.random.default_rng(4)
    x = rng.integers(-3, 4, (300, 16)).astype(np.float32)
    u = np.random.default_rng(9).random(20)
    picks = R.kmeans_plusplus(x, 20, u)
    assert len(set(picks.tolist())) == 20
    # restated by hand: integer distances, exact prefix sums
    xi = x.astype(np.int64)
    chosen = [int(np.floor(u[0] * len(x)))]
    dist = np.full(len(x), 1 << 60, np.int64)
    for j in range(1, 20):
        dist = np.minimum(dist, ((xi - xi[chosen[-1]]) ** 2).sum(1))
        cum = np.cumsum(dist)
        chosen.append(int(np.nonzero(cum > u[j] * cum[-1])[0][0]))
    assert picks.tolist() == chosen


def test_kmeanspp_refuses_too_few_distinct_rows():
    x = np.repeat(np.eye(16, dtype=np.float32)[:3], 10, axis=0)
    R.kmeans_plusplus(x, 3, np.random.default_rng(0).random(3))
    with pytest.raises(ValueError, match="distinct"):
        R.kmeans_plusplus(x, 4, np.random.default_rng(0).random(4))


def test_update_keeps_empty_clusters_and_uses_pieces():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((1300, 16)).astype(np.float32)
    labels = np.zeros(1300, np.int64)
    labels[::7] = 2
    c = rng.standard_normal((3, 16)).astype(np.float32)
    new, counts = R.update(x, labels, c)
    assert counts.tolist() == [1300 - len(labels[::7]), 0, len(labels[::7])]
    assert np.array_equal(new[1], c[1])
    for k in (0, 2):
        exp = x[labels == k].astype(np.float64).mean(0)
        assert np.all(np.abs(new[k] - exp) <= np.spacing(np.abs(exp).astype(np.float32)))


def test_reference_argument_errors():
    x = np.zeros((5, 16), np.float32)
    with pytest.raises(ValueError):
        R.fit(x, 0)
    with pytest.raises(ValueError):
        R.fit(x, 6)
    bad = x.copy(); bad[0, 0] = np.nan
    with pytest.raises(ValueError):
        R.fit(bad, 2)


def test_fit_kmeans_argument_errors_before_device_work():
    """``fit_kmeans`` converts and checks its arguments first; on a machine without a GPU it refuses with SylberHipError"""
    import torch
    from sylber_amd import _lib, fit_kmeans
    if not torch.cuda.is_available():
        with pytest.raises(_lib.SylberHipError):
            fit_kmeans(np.zeros((8, 16), np.float32), 2)
        return
    with pytest.raises(ValueError, match="multiple of 16"):
        fit_kmeans(np.zeros((8, 12), np.float32), 2)

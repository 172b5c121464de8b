"""GPU tier, fitting k-means unit codebooks (csrc/kmeans.hip behind sylber_amd/kmeans.py):

* the fused assign gives ``sylber_km_assign``'s labels bit for bit (K from 1 to 4 099, D 16 / 768, normalised or not, any row
  chunking), with d_min and the inertia within 1e-5 of float64;
* the centroid update is the restatement's fp64 piece sums bit for bit (within 1 ulp of numpy's mean), keeps empty clusters, handles
  a 2 M-row cluster beside 1-row clusters, and repeats bitwise;
* k-means++ picks the restatement's rows on small-integer data (all sums exact) and refuses fewer than K distinct rows;
* a fit follows the restatement iteration by iteration, recovers separated blobs and repeats bitwise;
* fitted quantizers map their training rows to the fit's labels (through ``.npy`` too), the residual fit both columns;
* end to end: Segmenter features -> ``fit_residual_km_quantizer`` -> ``SegmentSynthesis.tokenize`` / ``synthesize_units``."""
import numpy as np
import pytest
import torch

import kmeans_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


@pytest.mark.parametrize("D", [16, 768])
@pytest.mark.parametrize("K", [4, 5, 64, 1000, 4099])
@pytest.mark.parametrize("normalize", [False, True])
def test_fused_assign_bitwise_km_assign(K, D, normalize):
    from sylber_amd import KMQuantizer
    from sylber_amd import kmeans as KM
    n = 4097 + 3 * K % 61                                   # not a multiple of 64
    rng = np.random.default_rng(K * 7 + D)
    x = rng.standard_normal((n, D)).astype(np.float32)
    c = (x[rng.choice(n, K, replace=K > n)] + 0.3 * rng.standard_normal((K, D))).astype(np.float32)
    q = KMQuantizer(c, normalize=normalize, device=DEV)
    exp = q.get_indices(_t(x)).cpu().numpy()[:, 0]
    xd = _t(x)
    if normalize:
        xd = KM._normalize(xd)
    lab, dmin, inertia, _ = KM.assign(xd, _t(c))
    got = lab.cpu().numpy()
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    lab2, dmin2, inertia2, _ = KM.assign(xd, _t(c), row_chunk=1000)
    assert torch.equal(lab2, lab) and torch.equal(dmin2, dmin)
    assert abs(inertia2 - inertia) <= 1e-9 * abs(inertia)
    # d_min and the inertia against float64 on the device's own (normalised) rows and labels
    xr = xd.cpu().numpy().astype(np.float64)
    c64 = c.astype(np.float64)
    sc = (c64[got] ** 2).sum(1) - 2 * (xr * c64[got]).sum(1)
    scale = (xr ** 2).sum(1) + (c64[got] ** 2).sum(1)
    assert np.all(np.abs(dmin.cpu().numpy() - sc) <= 1e-5 * scale)
    ref_inertia = float(np.maximum(0, (xr ** 2).sum(1) + sc).sum())
    assert abs(inertia - ref_inertia) <= 1e-5 * ref_inertia


@pytest.mark.parametrize("K", [1, 3])
def test_fused_assign_small_k_against_restatement(K):
    from sylber_amd import kmeans as KM
    rng = np.random.default_rng(K)
    c = (rng.standard_normal((K, 32)) * 10).astype(np.float32)
    x = (c[rng.integers(0, K, 999)] + rng.standard_normal((999, 32))).astype(np.float32)
    lab, _, inertia, _ = KM.assign(_t(x), _t(c))
    exp, _, ref_inertia = R.assign(x, c)
    assert np.array_equal(lab.cpu().numpy(), exp)
    assert abs(inertia - ref_inertia) <= 1e-5 * ref_inertia


def test_assign_counts_changed_rows():
    from sylber_amd import kmeans as KM
    rng = np.random.default_rng(3)
    x, c = _t(rng.standard_normal((3000, 64))), _t(rng.standard_normal((40, 64)))
    lab, _, _, _ = KM.assign(x, c)
    prev = lab.clone()
    prev[::10] = (prev[::10] + 1) % 40
    _, _, _, ch = KM.assign(x, c, prev)
    assert ch == 300
    _, _, _, ch = KM.assign(x, c, prev, row_chunk=777)
    assert ch == 300


def test_update_matches_restatement_and_repeats():
    from sylber_amd import kmeans as KM
    rng = np.random.default_rng(5)
    n, D, K = 20000, 768, 50
    x = (rng.standard_normal((n, D)) * 3 + 1).astype(np.float32)
    labels = rng.integers(0, K, n)
    labels[labels == 7] = 8                                  # cluster 7 is empty
    c0 = rng.standard_normal((K, D)).astype(np.float32)
    exp, counts = R.update(x, labels, c0)
    xd, ld = _t(x), torch.from_numpy(labels.astype(np.int32)).to(DEV)
    outs = []
    for _ in range(2):
        c = _t(c0)
        cnt = KM.update(xd, ld, c)
        outs.append(c.cpu().numpy())
        assert np.array_equal(cnt.cpu().numpy(), counts)
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0][7], c0[7])
    assert np.array_equal(outs[0], exp)
    for k in range(K):
        if counts[k]:
            m = x[labels == k].astype(np.float64).mean(0)
            assert np.all(np.abs(outs[0][k] - m) <= np.spacing(np.abs(m).astype(np.float32)))


def test_update_one_huge_cluster_beside_singletons():
    from sylber_amd import kmeans as KM
    rng = np.random.default_rng(8)
    n, D, K = 2_000_003, 16, 4
    x = (rng.standard_normal((n, D)) + 5).astype(np.float32)
    labels = np.zeros(n, np.int32)
    labels[[17, 1_000_001, n - 1]] = [1, 2, 3]
    c = _t(np.zeros((K, D)))
    cnt = KM.update(_t(x), torch.from_numpy(labels).to(DEV), c)
    assert cnt.cpu().tolist() == [n - 3, 1, 1, 1]
    got = c.cpu().numpy()
    exp, _ = R.update(x, labels.astype(np.int64), np.zeros((K, D), np.float32))
    assert np.array_equal(got, exp)
    m = x[labels == 0].astype(np.float64).mean(0)
    assert np.all(np.abs(got[0] - m) <= np.spacing(np.abs(m).astype(np.float32)))
    assert np.array_equal(got[1:], x[[17, 1_000_001, n - 1]])


@pytest.mark.parametrize("D", [16, 768])
def test_kmeanspp_equals_restatement_on_integer_data(D):
    from sylber_amd import kmeans as KM
    rng = np.random.default_rng(D)
    x = rng.integers(-2, 3, (3001, D)).astype(np.float32)
    u = np.random.default_rng(11).random(40)
    got = KM.kmeans_plusplus(_t(x), 40, u).cpu().numpy()
    assert got.tolist() == R.kmeans_plusplus(x, 40, u).tolist()
    # through fit_kmeans, with and without init_rows
    from sylber_amd import fit_kmeans
    for rows in (None, 1000):
        f = fit_kmeans(x, 40, max_iter=0, seed=4, init_rows=rows, device=DEV)
        assert np.array_equal(f.centroids.cpu().numpy(), R.init_centroids(x, 40, seed=4, init_rows=rows))


def test_kmeanspp_refuses_too_few_distinct_rows():
    from sylber_amd import fit_kmeans
    x = np.repeat(np.eye(16, dtype=np.float32)[:5], 40, axis=0)
    assert fit_kmeans(x, 5, max_iter=3, device=DEV).inertia == 0.0
    with pytest.raises(ValueError, match="distinct"):
        fit_kmeans(x, 6, device=DEV)


def test_argument_errors():
    from sylber_amd import fit_kmeans
    x = np.random.default_rng(0).standard_normal((10, 16)).astype(np.float32)
    for K in (0, 11):
        with pytest.raises(ValueError):
            fit_kmeans(x, K, device=DEV)
    bad = x.copy(); bad[3, 3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        fit_kmeans(bad, 2, device=DEV)
    with pytest.raises(ValueError, match="multiple of 16"):
        fit_kmeans(x[:, :12], 2, device=DEV)
    with pytest.raises(ValueError):
        fit_kmeans(x, 2, init=np.zeros((3, 16)), device=DEV)


def test_fit_follows_restatement_per_iteration():
    from sylber_amd import fit_kmeans
    rng = np.random.default_rng(21)
    x = rng.standard_normal((2000, 32)).astype(np.float32)
    c0 = x[rng.choice(2000, 16, replace=False)] + 0.1
    for it in range(0, 7):
        f = fit_kmeans(x, 16, max_iter=it, tol=0.0, init=c0, device=DEV)
        r = R.fit(x, 16, max_iter=it, tol=0.0, init=c0)
        assert np.array_equal(f.labels.cpu().numpy(), r["labels"]), it
        np.testing.assert_allclose(f.centroids.cpu().numpy(), r["centroids"], rtol=1e-5, atol=1e-6)
        assert f.n_iter == r["n_iter"] and abs(f.inertia - r["inertia"]) <= 1e-5 * r["inertia"]
        assert [h[1:] for h in f.history] == [h[1:] for h in r["history"]]
    f = fit_kmeans(x, 16, max_iter=300, tol=0.0, init=c0, device=DEV)
    assert f.converged and f.n_iter < 300
    inert = [h[0] for h in f.history]
    assert all(b <= a * (1 + 1e-6) for a, b in zip(inert, inert[1:]))


def test_fit_recovers_blobs_and_repeats_bitwise():
    from sylber_amd import fit_kmeans
    rng = np.random.default_rng(2)
    K, D, m = 12, 768, 300
    centers = rng.standard_normal((K, D)) * 100               # far apart: k-means++ puts one seed in each blob
    x = np.concatenate([centers[k] + rng.standard_normal((m, D)) * 0.5 for k in range(K)]).astype(np.float32)
    truth = np.repeat(np.arange(K), m)
    feats = [torch.from_numpy(x[i:i + 500]).to(torch.bfloat16).float().numpy() for i in range(0, len(x), 500)] + [np.array([])]
    xb = np.concatenate(feats[:-1])
    f1 = fit_kmeans(feats, K, seed=1, device=DEV)
    f2 = fit_kmeans(torch.from_numpy(xb).to(DEV), K, seed=1, device=DEV)
    assert torch.equal(f1.centroids, f2.centroids) and torch.equal(f1.labels, f2.labels) and f1.history == f2.history
    lab = f1.labels.cpu().numpy()
    mapping = {}
    for t, l in zip(truth, lab):
        assert mapping.setdefault(int(t), int(l)) == int(l)
    assert len(set(mapping.values())) == K
    f3 = fit_kmeans(torch.from_numpy(xb).to(torch.bfloat16), K, seed=1, device=DEV)   # bf16 in: the same rows
    assert torch.equal(f3.labels, f1.labels)


@pytest.mark.parametrize("normalize", [False, True])
def test_quantizer_round_trip(normalize, tmp_path):
    from sylber_amd import KMQuantizer, fit_km_quantizer, load_km_quantizer
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((5000, 768)) + rng.standard_normal((1, 768))).astype(np.float32)
    q = fit_km_quantizer(x, 37, normalize=normalize, max_iter=20, device=DEV)
    assert isinstance(q, KMQuantizer) and q.normalize == normalize
    ids = q.get_indices(_t(x))[:, 0]
    assert torch.equal(ids, q.fit.labels)
    p = str(tmp_path / "units.npy")
    q.fit.save(p)
    c = np.load(p)
    assert c.dtype == np.float32 and c.shape == (37, 768)
    assert torch.equal(load_km_quantizer(p, normalize=normalize, device=DEV).get_indices(_t(x))[:, 0], ids)


def test_residual_round_trip():
    from sylber_amd import ResidualKMQuantizer, fit_residual_km_quantizer
    rng = np.random.default_rng(10)
    x = rng.standard_normal((4000, 768)).astype(np.float32)
    rkm = fit_residual_km_quantizer(x, 20, 9, max_iter=15, device=DEV)
    assert isinstance(rkm, ResidualKMQuantizer)
    f1, f2 = rkm.fits
    ids = rkm.get_indices(_t(x))
    assert torch.equal(ids[:, 0], f1.labels) and torch.equal(ids[:, 1], f2.labels)
    with pytest.raises(ValueError, match="normalize"):
        fit_residual_km_quantizer(x, 4, 4, normalize=True, device=DEV)


def test_end_to_end_segment_features_to_units():
    from sylber_amd import Segmenter, SegmentSynthesis, fit_residual_km_quantizer
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_state_dict
    from test_gpu_units import _checkpoint
    seg = Segmenter(model_ckpt=synthetic_state_dict(0), device=DEV, batch_invariant=True)
    wavs = [syllable_wave(int(n), s)[0] for s, n in enumerate([32000, 24000, 40000, 16000, 28000, 36000], start=50)]
    outs = seg(wav=[w[None] for w in wavs])
    feats = [o["segment_features"] for o in outs] + [np.array([])]
    n = sum(len(f) for f in feats)
    assert n >= 10, n
    rkm = fit_residual_km_quantizer(feats, 6, 4, device=DEV)
    syn = SegmentSynthesis(model_ckpt=_checkpoint(), device=DEV, quantizer=rkm, batch_invariant=True)
    clips = wavs[:3]
    L = max(len(w) for w in clips)
    x, mask = torch.zeros(3, L), torch.zeros(3, L)
    for i, w in enumerate(clips):
        x[i, :len(w)] = w
        mask[i, :len(w)] = 1
    x, mask = x.to(DEV), mask.to(DEV)
    lengths = [len(w) for w in clips]
    # the synthetic encoder's hidden-state norms sit below the default threshold: take one inside their range (as test_gpu_units)
    hidden = syn.speech_model.forward(x.contiguous(), lengths)
    frames = syn.speech_model.frame_counts(lengths)
    norms = torch.cat([torch.sqrt((hidden[b, :f].double() ** 2).sum(-1) + 1e-8) for b, f in enumerate(frames)])
    thr = float(np.round(torch.quantile(norms, 0.4).item(), 2))
    toks = syn.tokenize(x, attention_mask=mask, normthreshold=thr)
    assert len(toks) == 3 and sum(len(t["units"]) for t in toks) > 0
    for t in toks:
        u = t["units"]
        assert u.shape[1] == 2 and u.dtype == np.int64
        assert np.all((u[:, 0] >= 0) & (u[:, 0] < 6) & (u[:, 1] >= 0) & (u[:, 1] < 4))
    art = syn.synthesize_units([t["units"] for t in toks], [t["segments"] for t in toks], frames=[t["frames"] for t in toks])
    assert art.shape[0] == 3 and art.shape[-1] == 14 and bool(torch.isfinite(art).all())

"""CPU tier: the numpy restatement of the two-stage search contract (tests/knn16_ref.py) is itself checked -- its 16-bit roundings
against torch's casts bit for bit, its composition against knn_ref.search, and the inputs of the GPU tier's 'equality where the
bound decides it' test against their cap."""
import numpy as np
import pytest
import torch

import knn16_ref as R16
import knn_ref as R


def _values():
    rng = np.random.default_rng(0)
    a = [rng.standard_normal(4000) * 10.0 ** rng.integers(-8, 5, 4000), rng.standard_normal(2000)]
    # exact ties of both formats (a half-ulp above a representable value, even and odd neighbours), subnormals, zeros, NaN, inf
    base16 = np.arange(1024, 1024 + 64, dtype=np.float32) / 1024.0                    # fp16 grid in [1, 2): step 2^-10
    a.append(base16 + np.float32(2.0 ** -11))
    base_bf = np.arange(128, 128 + 64, dtype=np.float32) / 128.0                      # bf16 grid in [1, 2): step 2^-7
    a.append(base_bf + np.float32(2.0 ** -8))
    a.append(np.array([2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3 * 2.0 ** -25, 6e-8, 5.96e-8, 1e-7, 6.1e-5, 6.0e-5, 2.0 ** -14]))
    a.append(np.array([1e-40, -1e-40, 2.0 ** -133, 2.0 ** -134, 1.5 * 2.0 ** -133, 9.2e-41, 1e-45]))
    a.append(np.array([0.0, -0.0, np.nan, 65504.0, -65504.0, 65503.9, 1.0, -1.0]))
    v = np.concatenate([np.asarray(p, np.float64) for p in a]).astype(np.float32)
    return np.concatenate([v, -v])


def _bits(a):
    """the bit patterns, with every NaN mapped to one pattern (a NaN's payload and sign are not part of the contract)"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def test_round16_is_torchs_cast_bitwise():
    v = _values()
    t = torch.from_numpy(v)
    assert np.array_equal(_bits(R16.round16(v, "fp16")), _bits(t.to(torch.float16).to(torch.float32).numpy()))     # all within +-65504
    big = np.array([3.4e38, -3.4e38, 1e30, np.inf, -np.inf, 1e-30], np.float32)
    vb = np.concatenate([v, big])
    assert np.array_equal(_bits(R16.round16(vb, "bf16")), _bits(torch.from_numpy(vb).to(torch.bfloat16).to(torch.float32).numpy()))
    # fp16 saturates where torch overflows, NaN stays NaN
    sat = R16.round16(np.array([65504.1, 65519.9, 65520.0, 1e5, -1e5, np.inf, -np.inf, np.nan], np.float32), "fp16")
    assert sat[:7].tolist() == [65504.0, 65504.0, 65504.0, 65504.0, -65504.0, 65504.0, -65504.0] and np.isnan(sat[7])


@pytest.mark.parametrize("storage", R16.STORAGES)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_reference_with_m_at_least_N_is_the_exact_reference(storage, metric):
    rng = np.random.default_rng(3)
    N, D, n, k = 37, 32, 9, 10
    x = rng.standard_normal((N, D)).astype(np.float32)
    x[5] = np.nan
    x[11] = 0
    q = rng.standard_normal((n, D)).astype(np.float32)
    xg, qg = rng.integers(0, 3, N), rng.integers(0, 3, n)
    for groups in (False, True):
        kw = dict(q_group=qg, x_group=xg) if groups else {}
        s, i, cand = R16.two_stage(q, x, k, 4, storage, metric, **kw)          # m = 40 >= 37
        es, ei = R.search(q, x, k, metric, **kw)
        assert np.array_equal(i, ei) and np.array_equal(s, es)
        assert cand.shape == (n, 40)
        assert metric == "cosine" or not np.isin(5, cand)       # knn_ref.unit_rows makes the NaN row a zero row under cosine
    # and with a short list it is the exact order restricted to the candidates
    s, i, cand = R16.two_stage(q, x, 3, 2, storage, metric)
    full = R.scores(q, x, metric)
    for r in range(n):
        c = cand[r][cand[r] >= 0]
        assert i[r].tolist() == c[np.lexsort((c, full[r, c]))][:3].tolist()


def test_coarse_bound_covers_an_fp32_chain():
    """the bound holds for an explicit fp32 accumulation of the exact 16-bit products, in ascending and in pairwise order"""
    rng = np.random.default_rng(5)
    D = 768
    q = rng.standard_normal((4, D)).astype(np.float32)
    x = (rng.standard_normal((6, D)) * 3).astype(np.float32)
    for storage in R16.STORAGES:
        t = R16.coarse_scores(q, x, storage)
        b = R16.coarse_error_bound(q, x, storage)
        qr, xr = R16.round16(q, storage), R16.round16(x, storage)
        c = np.zeros(6, np.float32)
        for kk in range(D):
            c = (c.astype(np.float64) + x[:, kk].astype(np.float64) ** 2).astype(np.float32)       # one rounding per step
        for i in range(4):
            p = qr[i][None, :] * xr                                                   # exact in fp32
            assert np.array_equal(p.astype(np.float64), qr[i][None, :].astype(np.float64) * xr.astype(np.float64))
            chain = np.zeros(6, np.float32)
            for kk in range(D):
                chain = chain + p[:, kk]
            tree = p.copy()
            while tree.shape[1] > 1:
                if tree.shape[1] % 2:
                    tree = np.concatenate([tree, np.zeros((6, 1), np.float32)], 1)
                tree = tree[:, 0::2] + tree[:, 1::2]
            for dot in (chain, tree[:, 0]):
                got = (np.float32(-2.0) * dot).astype(np.float64) + c.astype(np.float64)
                got = got.astype(np.float32).astype(np.float64)                        # the fmaf's single rounding
                assert np.all(np.abs(got - t[i]) <= b[i])


@pytest.mark.parametrize("storage", R16.STORAGES)
def test_checkable_inputs_meet_their_cap(storage):
    q, x, k, refine = R16.checkable_inputs()
    ok = R16.checkable(q, x, k, refine, storage)
    print("checkable %s: %d of %d" % (storage, int(ok.sum()), len(ok)))
    assert (~ok).sum() <= 0.10 * len(ok)
    # refine = 1 is not enough on the same data: that is why refine exists
    assert R16.checkable(q, x, k, 1, storage).sum() < ok.sum()

"""CPU tier for tests/tokenizer_ref.py: the bounds must reject every planted defect, the fp32 numpy restatement alone must pass them,
and the inputs the GPU module (tests/test_gpu_tokenizers_f64.py) draws must be hard enough: in each random case at least 95 % of
the rows are decided (gap > 2 bnd), and at least 90 % of the near-tie rows land 4x to 16x their bound away from a tie."""
import numpy as np
import pytest

import tokenizer_ref as T


_linear_case = T.linear_case


def _km_case(D, K, n, seed, normalize=False):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((K, D)).astype(np.float32)
    return c, T.random_tokens(rng, c, n), rng


_near_ties = T.near_ties


# ---- the restatement clears the bounds, and the inputs are hard enough -----------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(65, 48, 768), (33, 80, 48), (129, 16, 16)])
def test_linear_restatement_within_bound(M, N, K):
    x, W, b = _linear_case(M, N, K, M + N + K)
    bad = T.judge_elements(T.linear32(x, W, b), T.linear64(x, W, b), T.linear_bound(x, W, b))
    assert len(bad) == 0, bad[:5]


def test_ffenc_restatement_within_propagated_bound():
    dims = (48, 80, 32)
    x, weights = T.ffenc_case(65, dims)
    layers = T.ffenc_layers(dims, weights)
    ref, bound = T.ffenc64(x, layers)
    assert len(T.judge_elements(T.ffenc32(x, layers), ref, bound)) == 0
    # the propagated bound is a worst case over four layers, yet it still rejects a K step dropped in the middle of the chain
    h = T.ffenc32(x, layers[:2])
    W, b, _ = layers[2]
    short = T.ffenc32(T.linear32(h, W, b, steps=80 - 16), layers[3:])
    assert len(T.judge_elements(short, ref, bound)) > 0


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("D", T.KM_D)
def test_kmeans_inputs_and_restatement(D, normalize):
    """the very pools the GPU module runs: decided rows, near ties in their band, and the fp32 restatement under the id rule"""
    for K in T.KM_K:
        c, x, dups = T.km_pool(D, K, normalize)
        s, bnd = T.km_bounds(x, c, normalize)
        ratio = T.gaps(s)[1] / bnd
        dup_ids = [i for p in dups for i in p]
        rand = np.array([r for r in range(42, 130) if s[r].argmin() not in dup_ids])      # a duplicated best row is a planted tie
        decided = (ratio[rand] > 2).mean()
        tie = ratio[T.KM_TIES]
        in_band = ((tie >= 4) & (tie <= 16)).mean()
        print("D=%d K=%d normalize=%d: %.1f %% decided, %.1f %% of near ties in the 4x-16x band" % (D, K, normalize, 100 * decided, 100 * in_band))
        assert decided >= 0.95, (K, decided)
        assert in_band >= 0.9, (K, in_band, np.sort(tie)[:5], np.sort(tie)[-5:])
        if K in (5, 8, 257) or (K == 1002 and D < 768):
            ids = T.argmin32(T.km_normalize32(x) if normalize else x, c)
            assert T.judge_ids(s, bnd, ids) == []
            for lo, hi in dups:
                assert not (ids == hi).any()
            if not normalize:
                c2 = T.km_second_book(D, K)
                r = (x - c[ids]).astype(np.float32)
                s2, b2 = T.km_bounds(r, c2, False)
                assert (T.gaps(s2)[1] > 2 * b2).mean() >= 0.95
                assert T.judge_ids(s2, b2, T.argmin32(r, c2)) == []


@pytest.mark.parametrize("d,K,Q", [(8, 1024, 4), (64, 1024, 2), (5, 5, 3), (20, 64, 1)])
def test_rvq_inputs_and_restatement(d, K, Q):
    books, x = T.rvq_case(d, K, Q)
    ids = T.rvq_assign32(x, books)
    bad, decided = T.rvq_judge(x, books, ids)
    assert bad == [] and decided >= 0.95, (bad[:3], decided)


def test_exact_tables_restatement():
    rng = np.random.default_rng(9)
    x, c = T.int_table(rng, 130, 257, 16)
    s = T.scores64(x, c)
    assert (T.gaps(s)[1] == 0).any()                               # the table does hold ties
    assert T.judge_ids(s, 0.0, T.argmin32(x, c), exact=True) == []


def test_norm_restatement_within_bound():
    rng = np.random.default_rng(2)
    for D in (1, 8, 63, 64, 65, 72, 130):
        x = (rng.standard_normal((40, D)) * rng.choice([1e-4, 1.0, 1e3], (40, 1))).astype(np.float32)
        for split in (0, 1, D - 1):
            ref = T.lq_norm64(x, split)
            assert len(T.judge_elements(T.lq_norm32(x, split), ref, T.NORM_REL(D) * np.abs(ref))) == 0
    tiny = np.full((1, 8), 2.0 ** -81, np.float32)
    assert T.blank_rows32(np.concatenate([tiny, np.zeros((1, 8), np.float32), np.full((1, 8), np.nan, np.float32),
                                          np.ones((1, 8), np.float32)])).tolist() == [True, True, True, False]


# ---- planted defects: each must be rejected ------------------------------------------------------------------------------------------
def test_dropped_k_step_is_rejected():
    x, W, b = _linear_case(33, 48, 768, 1)
    ref, bound = T.linear64(x, W, b), T.linear_bound(x, W, b)
    assert len(T.judge_elements(T.linear32(x, W, b, steps=768 - 16), ref, bound)) > 0
    # and in an arg-min: on near-tie rows the ids of the short contraction break the id rule
    c, _, rng = _km_case(64, 65, 8, 5)
    nt = _near_ties(c, 64, rng)
    s, bnd = T.scores64(nt, c), T.row_bounds(nt, c, 64)
    assert T.judge_ids(s, bnd, T.argmin32(nt, c)) == []
    assert T.judge_ids(s, bnd, T.argmin32(nt, c, steps=48)) != []


def test_shifted_bias_is_rejected():
    x, W, b = _linear_case(33, 48, 48, 2)
    got = (T.fma_chain32(x, W) + np.roll(b, 1)[None, :]).astype(np.float32)
    assert len(T.judge_elements(got, T.linear64(x, W, b), T.linear_bound(x, W, b))) > 0


def test_clamped_row_copied_over_another_is_rejected():
    x, W, b = _linear_case(65, 48, 48, 3)                           # the last 64-row tile holds row 64 alone; 129 -> rows 128 and 127
    got = T.linear32(x, W, b)
    got[63] = got[64]
    bad = T.judge_elements(got, T.linear64(x, W, b), T.linear_bound(x, W, b))
    assert len(bad) > 0 and set(bad[:, 0]) == {63}


def test_tie_to_the_larger_index_is_rejected():
    rng = np.random.default_rng(9)
    x, c = T.int_table(rng, 130, 257, 16)
    assert T.judge_ids(T.scores64(x, c), 0.0, T.argmin32(x, c, larger_on_tie=True), exact=True) != []
    # duplicated rows in a random codebook: both are within the bound, so the smaller index is asserted directly by the GPU tests
    c2, x2, _ = _km_case(64, 260, 16, 6)
    c2[259] = c2[3]
    x2[:] = c2[3]
    assert (T.argmin32(x2, c2) == 3).all() and (T.argmin32(x2, c2, larger_on_tie=True) == 259).all()


def test_out_of_range_ids_are_rejected():
    c, x, _ = _km_case(16, 5, 8, 7)
    s, bnd = T.scores64(x, c), T.row_bounds(x, c, 16)
    ids = T.argmin32(x, c)
    for wrong in (5, 7, T.INT_MAX, -1):                            # a zero-padded row K..Kp-1, INT_MAX of an all-NaN row
        planted = ids.copy(); planted[3] = wrong
        bad = T.judge_ids(s, bnd, planted)
        assert [r for r, _ in bad] == [3], (wrong, bad)
    # a zero token scores the padded rows 0, below every real row: an arg-min over Kp rows returns one of them
    books = T.pad_books([c])[0]
    assert T.argmin32(np.zeros((1, 16), np.float32), books)[0] >= 5
    assert T.argmin32(np.zeros((1, 16), np.float32), books, K=5)[0] < 5


def test_wrong_constant_under_the_root_is_rejected():
    v = np.float32(3e-4)
    thr = np.sqrt(v * v + np.float32(1e-8))
    cand = T.ulp_neighbours(v, 3)
    for t in T.ulp_neighbours(thr, 1):
        assert not np.array_equal(T.silent_hidden32(cand, t, 1e-5), T.silent_hidden32(cand, t))
    # the k-means normalisation of a quiet row, and the learned quantizer's unit norm with the other constant
    x = (np.random.default_rng(0).standard_normal((4, 64)) * 1e-3).astype(np.float32)
    ref = T.km_normalize64(x)
    assert len(T.judge_elements(T.km_normalize32(x), ref, T.NORM_REL(64) * np.abs(ref))) == 0
    assert len(T.judge_elements(T.km_normalize32(x, 1e-5), ref, T.NORM_REL(64) * np.abs(ref))) > 0
    ref = T.lq_norm64(x)
    assert len(T.judge_elements(T.lq_norm32(x, 0, 1e-8), ref, T.NORM_REL(64) * np.abs(ref))) > 0


def test_features_crossing_sits_on_the_threshold():
    v = T.features_crossing()
    cand = T.ulp_neighbours(v, 3)
    m = T.silent_features32(cand)
    assert m[:3].all() and not m[3:].any()

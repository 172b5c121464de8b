"""CPU tier: tests/dtw16_ref.py (the numpy restatement of ``SyllableIndex.search_phrases_refined``) against dtw_ref, its candidate and
padding rules, the decided share of the fixed input set that the GPU tier relies on, and the refusals of the C entry points, which
come before any launch and so need no device."""
import numpy as np
import pytest

import dtw16_ref as R
import dtw_ref as DR


def _small(metric, seed=5):
    rng = np.random.default_rng(seed)
    D = 16
    lens = [4, 9, 1, 6, 3, 7, 5]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = rng.standard_normal((int(offsets[-1]), D)).astype(np.float32)
    phrases = [(x[a:a + m] + 0.2 * rng.standard_normal((m, D))).astype(np.float32) for m, a in ((1, 3), (3, 5), (5, 20), (8, 0))]
    return x, offsets, phrases


@pytest.mark.parametrize("storage", R.STORAGES)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_every_sequence_a_candidate_is_search_phrases(metric, storage):
    x, offsets, phrases = _small(metric)
    S = len(offsets) - 1
    qs, xs = R.stored(phrases, x, metric)
    d_of = lambda p, s: DR.local_costs(qs[p], xs[offsets[s]:offsets[s + 1]], metric)
    for k, refine in ((S, 1), (3, 3), (2, 4)):                # m = 7, 9, 8 >= S
        want = DR.search_phrases(d_of, len(phrases), offsets, k, np.float64)
        got = R.two_stage(phrases, x, offsets, k, refine, storage, metric)
        for a, b in zip(got[:3], want):
            assert np.array_equal(a, b)
        assert got[3].shape == (len(phrases), k * refine) and (np.sort(got[3][:, :S], 1) == np.arange(S)).all()
        assert (got[3][:, S:] == -1).all() and np.isinf(got[4][:, S:]).all() and np.isfinite(got[4][:, :S]).all()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_candidate_and_padding_rules(metric):
    x, offsets, phrases = _small(metric, 6)
    x = x.copy()
    x[offsets[2]:offsets[3]] = np.nan                         # sequence 2 is NaN throughout: under l2 its cost is +inf
    S = len(offsets) - 1
    qs, xs = R.stored(phrases, x, metric)
    cc = R.coarse_costs(qs, xs, offsets, "fp16", metric)
    ec = R.exact_results(qs, xs, offsets, metric)
    sgrp = np.array([0, 1, 2, 0, 3, 1, 4])
    pgrp = np.array([0, 1, 4, 9])
    for pg, sg in ((None, None), (pgrp, sgrp)):
        k, refine = 2, 2
        c, q, sp, cand, co = R.two_stage(phrases, x, offsets, k, refine, "fp16", metric, pg, sg, coarse=cc, exact=ec)
        for p in range(len(phrases)):
            adm = (np.ones(S, bool) if pg is None else sg != pg[p]) & np.isfinite(cc[p])
            order = np.nonzero(adm)[0]
            order = order[np.lexsort((order, cc[p, order]))][:k * refine]
            assert cand[p, :order.size].tolist() == order.tolist() and (cand[p, order.size:] == -1).all()
            assert np.array_equal(co[p, :order.size], cc[p, order]) and np.isinf(co[p, order.size:]).all()
            # the result is the exact ranking restricted to the candidates
            inside = order[np.isfinite(ec[0][p, order])]
            best = inside[np.lexsort((inside, ec[0][p, inside]))][:k]
            assert q[p, :best.size].tolist() == best.tolist() and (q[p, best.size:] == -1).all()
            assert np.array_equal(c[p, :best.size], ec[0][p, best]) and np.isinf(c[p, best.size:]).all()
            assert (sp[p, best.size:] == -1).all()
            assert np.array_equal(sp[p, :best.size, 0], offsets[best] + ec[1][p, best])
            assert np.array_equal(sp[p, :best.size, 1], offsets[best] + ec[2][p, best] + 1)
            if pg is not None:
                assert not np.isin(cand[p], np.nonzero(sg == pg[p])[0]).any()
        if metric == "l2":
            assert 2 not in cand and np.isinf(cc[:, 2]).all()
    # fewer admissible sequences than k: the lists end in (+inf, -1, (-1, -1)), cand in -1, coarse in +inf
    c, q, sp, cand, co = R.two_stage(phrases[:1], x, offsets, 5, 2, "bf16", metric, np.array([1]), np.array([1, 1, 1, 0, 1, 1, 5]))
    assert sorted(cand[0, :2].tolist()) == [3, 6] and (cand[0, 2:] == -1).all() and np.isinf(co[0, 2:]).all()
    assert (q[0, 2:] == -1).all() and np.isinf(c[0, 2:]).all() and (sp[0, 2:] == -1).all() and (q[0, :2] >= 0).all()


def test_the_fixed_input_set_is_the_recipe():
    x, offsets, phrases, k, refine = R.checkable_inputs()
    assert x.shape == (int(offsets[-1]), 64) and x.dtype == np.float32 and len(offsets) == 61 and len(phrases) == 24
    assert sorted(len(p) for p in phrases) == sorted([1, 2, 3, 5, 8, 13] * 4) and (k, refine) == (3, 4)
    assert 5 <= np.diff(offsets).min() and np.diff(offsets).max() <= 40
    assert int(offsets[-1]) // 128 >= 8                       # sequences straddle many 128-row tile edges
    cc, cb, (ec, _, _) = R.checkable_reference("fp16", "l2")
    assert np.isfinite(cc).all() and (cc >= 0).all() and (cb > 0).all() and np.isfinite(ec).all()


@pytest.mark.parametrize("storage", R.STORAGES)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_decided_share_of_the_fixed_input_set(metric, storage):
    """at most 2 of the 24 phrases may be left out by the GPU tier, per combination"""
    x, offsets, phrases, k, refine = R.checkable_inputs()
    qs, xs = R.stored(phrases, x, metric)
    cc, cb, exact = R.checkable_reference(storage, metric)
    decided, inside, top = R.checkable(qs, xs, offsets, k, refine, storage, metric, coarse=(cc, cb), exact=exact)
    print("decided", int(decided.sum()), "exact top-k inside", int(inside.sum()), "both", int((decided & inside).sum()), "of", len(phrases))
    assert decided.sum() >= len(phrases) - 2
    assert (decided & inside).sum() >= len(phrases) - 2
    got = R.two_stage(phrases, x, offsets, k, refine, storage, metric, coarse=cc, exact=exact)
    assert np.array_equal(got[3], top)
    want = DR.rank
    for p in np.nonzero(inside)[0]:                           # where the top-k is inside, the restriction changes nothing
        c, q, sp = want(exact[0][p], exact[1][p], exact[2][p], offsets, k)
        assert np.array_equal(got[0][p], c) and np.array_equal(got[1][p], q) and np.array_equal(got[2][p], sp)


def test_entry_points_refuse_bad_arguments_without_a_device():
    from sylber_amd import build, _lib
    build.build()
    lib = _lib.load()
    wb = lib.sylber_dtw16_workspace_bytes
    al = lambda b: (b + 255) // 256 * 256
    assert wb(10, 12, 5) == 2 * al(10 * 5 * 12 * 4) + 2 * al(10 * 3 * 12 * 4)       # the partial lists [P][C][m] and [P][ceil(C/2)][m]
    assert wb(10, 12, 1) == max(4 * al(10 * 12 * 4), al(10 * 12 * 4) + al(10 * 12 * 8))
    assert wb(1, 128, 1) > 0
    for bad in ((0, 12, 5), (10, 0, 5), (10, 129, 5), (10, 12, 0), (-1, 12, 5)):
        assert wb(*bad) == -1, bad
    p = 4096                                                  # never dereferenced: every refusal comes before a launch
    good = dict(q16=p, nb=1, meta=p, slot=p, rows=p, P=3, bp=3, db16=p, N=100, D=64, cn=p, qn=p, metric=0, storage=0, m=12, seqid=p,
                cut=p, cuts=2, pg=None, sg=None, cand=p, coarse=p, ws=p, stream=None)
    cases = [dict(q16=None), dict(meta=None), dict(slot=None), dict(rows=None), dict(db16=None), dict(seqid=None), dict(cut=None),
             dict(cand=None), dict(coarse=None), dict(ws=None), dict(nb=0), dict(P=0), dict(N=0), dict(D=8), dict(D=72), dict(m=0),
             dict(m=129), dict(bp=0), dict(bp=129), dict(m=128, bp=33), dict(cuts=0), dict(cuts=65536), dict(metric=2), dict(storage=2),
             dict(cn=None), dict(qn=None), dict(pg=p), dict(sg=p), dict(P=2 ** 20, cuts=1024)]
    for c in cases:
        a = dict(good, **c)
        assert lib.sylber_dtw16_scan(*a.values()) == 1, c
        assert lib.sylber_last_error().decode().startswith("sylber_dtw16_scan: "), c
    good = dict(q=p, nb=1, qn=p, prow=p, plen=p, P=3, db=p, N=100, D=64, cn=p, metric=0, cand=p, m=12, soff=p, S=7, k=3, cost=p, seq=p,
                span=p, ws=p, stream=None)
    cases = [dict(q=None), dict(prow=None), dict(plen=None), dict(db=None), dict(cand=None), dict(soff=None), dict(cost=None),
             dict(seq=None), dict(span=None), dict(ws=None), dict(nb=0), dict(P=0), dict(N=0), dict(S=0), dict(D=8), dict(D=72), dict(m=0),
             dict(m=129), dict(k=0), dict(k=13), dict(metric=2), dict(cn=None), dict(qn=None)]
    for c in cases:
        a = dict(good, **c)
        assert lib.sylber_dtw_rerank(*a.values()) == 1, c
        assert lib.sylber_last_error().decode().startswith("sylber_dtw_rerank: "), c

"""numpy restatement of the compressed phrase-search contract of sylber_amd.PQSyllableIndex.search_phrases / csrc/dtwpq.hip, built on
pq_ref (codes, decode), dtw16_ref (the two-stage phrase search) and dtw_ref (the recurrence, the ranking).

    x^_j      = pq_ref.decode(code_j): the fp32 reconstruction of stored row j (of the unit row under "cosine", not renormalised);
                a masked row (pq_ref.encode's ``bad``) is a NaN row
    stage 1   = dtw16_ref's stage 1 fed x^ in place of the stored rows: t(i, j) = c_j - 2 q~_i . round16(x^_j), c_j = ||x^_j||^2 (l2)
                or 0 (cosine); a NaN row's local cost is +inf against every phrase row
    stage 2   rerank=True:  dtw_ref's exact (cost, start, end) on the STORED rows for each candidate
              rerank=False: the same on x^ (masked rows NaN)
    ordered by (cost, sequence), the best k reported and padded as dtw_ref.search_phrases reports them

so it is ``dtw16_ref.two_stage`` / ``checkable`` with other rows behind the two stages.  Everything is float64, as there."""
import numpy as np

import dtw16_ref as R16
import pq_ref as PQ

STORAGES = R16.STORAGES


def codebooks_from_rows(xs, M, seed=7):
    """explicit codebooks [M, 256, D / M] without k-means: sub-space mm is columns [mm dsub, (mm + 1) dsub) of the stored rows
    ``np.sort(default_rng(seed).choice(N, 256, replace=False))``"""
    xs = np.asarray(xs, np.float32)
    N, D = xs.shape
    rows = np.sort(np.random.default_rng(seed).choice(N, PQ.KSUB, replace=False))
    dsub = D // M
    return np.stack([xs[rows, mm * dsub:(mm + 1) * dsub] for mm in range(M)]).astype(np.float32)


def decoded(xs, C, codes=None, bad=None):
    """the fp32 rows behind stage 1 from stored rows ``xs``: pq_ref.decode of pq_ref.encode's codes (or of ``codes`` / ``bad`` as
    given, e.g. the index's own), masked rows NaN -> (x^ [N, D] float32, codes, bad)"""
    if codes is None:
        codes, bad = PQ.encode(xs, C)
    xh = PQ.decode(codes, C).astype(np.float32)
    xh[np.asarray(bad, bool)] = np.nan
    return xh, np.asarray(codes), np.asarray(bad, bool)


def references(phrases, x, C, offsets, storage, metric="l2", rerank=True, codes=None, bad=None, bounds=False):
    """(stored phrases, x^, coarse costs [P, S] (with their bounds if ``bounds``), exact (cost, start, end) of every pair): the two
    inputs of ``dtw16_ref.two_stage`` / ``checkable``"""
    qs, xs = R16.stored(phrases, x, metric)
    xh = decoded(xs, C, codes, bad)[0]
    coarse = R16.coarse_costs(qs, xh, offsets, storage, metric, bounds=bounds)
    return qs, xh, coarse, R16.exact_results(qs, xs if rerank else xh, offsets, metric)


def two_stage(phrases, x, C, offsets, k, refine, storage="fp16", metric="l2", rerank=True, phrase_groups=None, seq_groups=None,
              codes=None, bad=None):
    """(costs [P, k], seqs [P, k], spans [P, k, 2], cand [P, m], coarse [P, m]) of the contract in float64, from raw phrases and rows"""
    _, _, coarse, exact = references(phrases, x, C, offsets, storage, metric, rerank, codes, bad)
    return R16.two_stage(phrases, x, offsets, k, refine, storage, metric, phrase_groups, seq_groups, coarse=coarse, exact=exact)


def checkable(phrases, x, C, offsets, k, refine, storage, metric="l2", codes=None, bad=None):
    """``dtw16_ref.checkable`` with stage 1 on x^ and the exact stage on the stored rows (``rerank=True``) -> (decided [P], inside [P],
    top [P, m], coarse costs, bounds): where decided and inside, ``pq.search_phrases(rerank=True)`` must equal ``search_phrases``"""
    qs, xh, (cc, cb), exact = references(phrases, x, C, offsets, storage, metric, True, codes, bad, bounds=True)
    decided, inside, top = R16.checkable(qs, xh, offsets, k, refine, storage, metric, coarse=(cc, cb), exact=exact)
    return decided, inside, top, cc, cb

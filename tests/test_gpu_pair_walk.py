"""The chunk walk that the three wave-per-pair kernels share (csrc/dtw_pair.h: ``dtw_rerank_kernel``, ``dtw_occ_rerank_kernel``,
``dtw_align_kernel``), pinned at the edges of its 32-column chunk across all three users: sequences of 1, 2, 31, 32, 33, 63, 64, 65,
96 and 97 rows against phrases of 1, 2, 31, 32, 33 and 64 rows (so ``m > L`` occurs), integer-valued rows, every sequence a
candidate (``k = 10`` sequences, ``refine = 1``).  Bitwise: each two-stage search against its scan, the alignment against the search
whose spans it is given, and all three against the numpy restatements (tests/dtw_ref.py, occ_ref.py, align_ref.py), which a CPU test
first holds against each other on the same inputs."""
import functools

import numpy as np
import pytest
import torch

import align_ref as A
import dtw_ref as R
import occ_ref as O

DEV = "cuda:0"
SEQ_LENS = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97)
PHRASE_LENS = (1, 2, 31, 32, 33, 64)
OFFSETS = np.concatenate([[0], np.cumsum(SEQ_LENS)]).astype(np.int64)
K = len(SEQ_LENS)


@functools.lru_cache(maxsize=None)
def _corpus(D):
    """484 rows of small integers and six phrases: stretches of the corpus (exact matches, ties in every sum) with every third row
    replaced, taken where they cross chunk edges of their sequence"""
    rng = np.random.default_rng(D)
    x = rng.integers(-2, 3, (int(OFFSETS[-1]), D)).astype(np.float32)
    x[OFFSETS[8] + 30:OFFSETS[8] + 36] = x[OFFSETS[8] + 29]   # a run of equal rows across the first chunk edge of the 96-row sequence
    phrases = []
    for m, s, a in zip(PHRASE_LENS, (3, 6, 7, 8, 9, 9), (31, 31, 20, 40, 50, 16)):
        p = x[OFFSETS[s] + a:OFFSETS[s] + a + m].copy()
        p[1::3] = rng.integers(-2, 3, p[1::3].shape).astype(np.float32)
        phrases.append(p)
    return x, phrases


def _references(d, phrases):
    """(search_phrases, search_occurrences, align_phrases on the first's spans) of the restatements over local costs d [sum m, N]"""
    lens = [len(p) for p in phrases]
    r0 = np.concatenate([[0], np.cumsum(lens)])
    by_seq = lambda p, s: d[r0[p]:r0[p + 1], OFFSETS[s]:OFFSETS[s + 1]]  # noqa: E731
    ref = R.search_phrases(by_seq, len(phrases), OFFSETS, K)
    occ = O.search_occurrences(by_seq, len(phrases), OFFSETS, K)[:3]
    ali = A.align_phrases(lambda p, a, b: d[r0[p]:r0[p + 1], a:b], lens, ref[2])
    return ref, occ, ali


def _exact_l2(x, phrases):
    """the "l2" local costs of integer rows: every product, sum and the final ``||q||^2 + fmaf(-2, q . x, ||x||^2)`` is an integer
    below 2^24, so fp32 gives ``||q - x||^2`` exactly whatever the order"""
    q = np.concatenate(phrases).astype(np.float64)
    return ((q[:, None, :] - x[None].astype(np.float64)) ** 2).sum(2).astype(np.float32)


def test_the_references_agree_on_these_inputs():
    x, phrases = _corpus(16)
    d = _exact_l2(x, phrases)
    ref, occ, ali = _references(d, phrases)
    assert (ref[1] >= 0).all() and np.isfinite(ref[0]).all()         # every sequence is returned for every phrase, m > L included
    # alignment against search: the path of a returned span starts and ends where the span does and has the search's cost bits
    lens = np.array([len(p) for p in phrases])
    assert np.array_equal(ali[2].view(np.uint32), ref[0].view(np.uint32))
    assert np.array_equal(ali[0][:, :, 0, 0], ref[2][:, :, 0])
    assert np.array_equal(ali[0][np.arange(len(lens)), :, lens - 1, 1], ref[2][:, :, 1])
    # occurrences against search: the first occurrence of each sequence under (cost, start row) is the sequence's match
    r0 = np.concatenate([[0], np.cumsum(lens)])
    full = O.search_occurrences(lambda p, s: d[r0[p]:r0[p + 1], OFFSETS[s]:OFFSETS[s + 1]], len(phrases), OFFSETS, 1024)
    for p in range(len(phrases)):
        seqs = full[1][p]
        first = [int(np.nonzero(seqs == s)[0][0]) for s in ref[1][p]]
        assert first == sorted(first)
        assert np.array_equal(full[0][p][first].view(np.uint32), ref[0][p].view(np.uint32)) and np.array_equal(full[2][p][first], ref[2][p])
        assert np.array_equal(full[0][p][:K].view(np.uint32), occ[0][p].view(np.uint32))


def _same(got, ref):
    for g, r in zip(got, ref):
        g = g.cpu().numpy()
        r = np.asarray(r).astype(g.dtype)
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, r.view(np.uint32) if r.dtype == np.float32 else r)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D", [16, 48])
def test_chunk_edges_across_the_three_pair_kernels(D, metric):
    from sylber_amd import SyllableIndex
    from test_gpu_phrase import _groups_of, _local_costs
    x, phrases = _corpus(D)
    idx = SyllableIndex(x, metric=metric, groups=_groups_of(OFFSETS), device=DEV)
    assert np.array_equal(idx.sequence_offsets(), OFFSETS)
    scan = idx.search_phrases(phrases, K)
    occ = idx.search_occurrences(phrases, K)
    # the two-stage searches with every sequence a candidate are their scans
    for a, b in zip(idx.search_phrases_refined(phrases, K, 1), scan):
        assert torch.equal(a, b)
    for a, b in zip(idx.search_occurrences_refined(phrases, K, 1), occ):
        assert torch.equal(a, b)
    # the alignment on the scan's spans: its cost bits, its starts, and the start the walk tracked
    rows, steps, costs, start = idx.align_phrases(phrases, scan[2], _tracked_start=True)
    assert torch.equal(costs.view(torch.int32), scan[0].view(torch.int32))
    assert torch.equal(rows[:, :, 0, 0], scan[2][:, :, 0])
    assert torch.equal(start, rows[:, :, 0, 0])
    # and the restatements, over the library's own local costs
    d = _local_costs(x, OFFSETS, np.concatenate(phrases), metric)
    if metric == "l2":
        assert np.array_equal(d, _exact_l2(x, phrases))
    ref, ref_occ, ref_ali = _references(d, phrases)
    assert (ref[1] >= 0).all()
    _same(scan, ref)
    _same(occ, ref_occ)
    _same((rows, steps, costs), ref_ali)

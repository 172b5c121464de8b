"""CPU tier of phrase search on the compressed inverted file: the numpy composition (tests/ivfpq_phrase_ref.py) recovers the planted
phrases at the settings the GPU tier uses, its ``rerank=False`` costs are the cell-by-cell DTW on the reconstruction, its alignment
of its own spans has the search's bits, and the two C entries refuse bad arguments before any device call."""
import functools

import numpy as np
import pytest

import dtw_ref as T
import ivfpq_phrase_ref as Q
import phrase_vote_ref as V


@functools.lru_cache(maxsize=None)
def _ix(residual):
    return Q.planted_index(residual)


@functools.lru_cache(maxsize=None)
def _search(residual, rerank, nprobe, seeds):
    ix = _ix(residual)
    return Q.search_phrases(ix, ix["phrases"], Q.K, nprobe, seeds, Q.REFINE, rerank)


def test_the_settings_are_the_planted_ones():
    assert (Q.M, Q.K, Q.REFINE) == (2, V.PLANTED["k"], V.PLANTED["refine"]) and V.PLANTED["D"] % (16 * Q.M) == 0
    assert (V.PLANTED["nprobe"], V.PLANTED["seeds"]) in Q.SETTINGS and max(n for n, _ in Q.SETTINGS) == V.PLANTED["nlist"]
    for residual in (False, True):
        ix = _ix(residual)
        assert not ix["bad"].any() and (ix["labels"] >= 0).all() and np.isfinite(ix["xhat"]).all()
        assert ix["codebooks"].shape == (Q.M, 256, V.PLANTED["D"] // Q.M)


@pytest.mark.parametrize("nprobe,seeds", Q.SETTINGS)
@pytest.mark.parametrize("rerank", [True, False])
@pytest.mark.parametrize("residual", [False, True])
def test_planted_phrases_come_first(residual, rerank, nprobe, seeds):
    ix = _ix(residual)
    costs, seqs, spans, cand, bound = _search(residual, rerank, nprobe, seeds)
    assert np.array_equal(seqs[:, 0], ix["truth"]), (residual, rerank, nprobe, seeds)
    off, t = ix["offsets"], ix["truth"]
    assert ((spans[:, 0, 0] >= off[t]) & (spans[:, 0, 1] <= off[t + 1])).all()
    assert (costs[:, 0] < costs[:, 1]).all() and np.isfinite(bound[:, 0]).all()
    assert cand.shape == (len(t), Q.K * Q.REFINE) and cand.dtype == np.int32


@pytest.mark.parametrize("residual", [False, True])
def test_codes_only_costs_are_the_dtw_on_the_reconstruction(residual):
    ix = _ix(residual)
    costs, seqs, spans, _, _ = _search(residual, False, 3, 32)
    off = ix["offsets"]
    for p, ph in enumerate(ix["phrases"]):
        for r in range(Q.K):
            s = int(seqs[p, r])
            assert s >= 0
            cost, start, end, _ = T.dtw_loop(T.local_costs(ph, ix["xhat"][off[s]:off[s + 1]]), np.float32)
            assert cost.view(np.uint32) == costs[p, r].view(np.uint32)
            assert (off[s] + start, off[s] + end + 1) == tuple(spans[p, r])
    # the rows' own costs differ: the reconstruction is not the row
    held = _search(residual, True, 3, 32)
    assert np.array_equal(held[1][:, 0], seqs[:, 0]) and not np.array_equal(held[0], costs)


@pytest.mark.parametrize("rerank", [True, False])
def test_alignment_of_the_search_spans_has_its_costs(rerank):
    ix = _ix(True)
    costs, _, spans, _, _ = _search(True, rerank, 3, 32)
    rows, steps, acosts = Q.align(ix, ix["phrases"], spans, rerank)
    assert np.array_equal(acosts.view(np.uint32), costs.view(np.uint32))
    assert np.array_equal(rows[:, :, 0, 0], spans[:, :, 0]) and (steps >= np.array([len(p) for p in ix["phrases"]])[:, None]).all()


def test_a_masked_row_costs_infinity():
    case = V.planted_case()
    x = case["x"].copy()
    t = int(case["truth"][0])
    x[int(case["offsets"][t]) + 1, 5] = np.nan
    ix = Q.planted_index(True, case=dict(case, x=x))
    bad = int(case["offsets"][t]) + 1
    assert ix["bad"][bad] and ix["labels"][bad] == -1 and np.isnan(ix["xhat"][bad]).all() and ix["bad"].sum() == 1
    got = Q.search_phrases(ix, ix["phrases"], Q.K, 3, 32, Q.REFINE, False)
    assert np.isfinite(got[0][1:, 0]).all() and np.array_equal(got[1][1:, 0], ix["truth"][1:])
    hit = got[1][0] == t
    assert not ((got[2][0, hit, 0] <= bad) & (bad < got[2][0, hit, 1])).any()            # no span crosses the masked row


# ---- the C ABI's refusals: host checks only, nothing is dereferenced ----------------------------------------------------------------
def test_the_entries_refuse_bad_arguments_before_any_launch():
    from sylber_amd import build, _lib
    build.build()
    lib = _lib.load()
    for name, good, cases in Q.abi_refusals():
        for c in cases:
            assert getattr(lib, name)(*dict(good, **c).values()) == 1, (name, c)
            assert lib.sylber_last_error().decode().startswith(name + ": "), (name, c)

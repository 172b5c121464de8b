"""CPU tier: the consequences of the "Embedding strings, local" contract on tests/dtw_strings_local_ref.py itself, the kernel's
anti-diagonal / strip / tile / skipped-tile form against the cell-by-cell form, and the planted misreadings that the restatement
must reject.  The fixtures assert their own non-vacuity (``dtw_strings_local_ref.assert_not_vacuous``)."""
import functools

import numpy as np
import pytest

import dtw_strings_local_ref as G
import repeats_ref

f32 = np.float32


def _d_int(x, y):
    """exact in numpy: integer rows under L2"""
    xn, yn = (x * x).sum(1), (y * y).sum(1)
    return np.maximum(f32(0), xn[:, None] + (f32(-2) * (x @ y.T) + yn[None, :])).astype(np.float32)


# name: (m, L, copies, integer rows)
CASES = {
    "three": (60, 90, [(2, 14, 65, "same"), (20, 16, 35, "drop"), (40, 16, 5, "double")], True),
    "gauss": (33, 40, [(0, 16, 22, "drop"), (17, 16, 2, "double")], False),
    "edges": (40, 48, [(0, 14, 34, "same"), (24, 16, 0, "drop"), (10, 12, 16, "double")], True),
    "strips": (150, 140, [(55, 20, 10, "drop"), (120, 14, 120, "double")], True),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    m, L, copies, integer = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x, y = G.planted(rng, m, L, 16, copies, integer)
    d = _d_int(x, y) if integer else repeats_ref.local_costs32(x, y)
    radius = f32(24.0) if integer else f32(12.0)
    return d, radius, copies


@functools.lru_cache(maxsize=None)
def _self_case():
    """one sequence holding a phrase three times: against itself the three pairs of occurrences repeat"""
    rng = np.random.default_rng(3)
    x = rng.integers(-2, 3, (90, 16)).astype(np.float32)
    x[40:50] = x[5:15]
    x[70:80] = x[5:15]
    return _d_int(x, x), f32(24.0)


@pytest.mark.parametrize("gap_mul", [0, 1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_consequences_and_the_two_forms(name, gap_mul):
    d, radius, copies = _case(name)
    gap, min_score, R = f32(gap_mul) * radius, f32(3) * radius, 5
    integer = CASES[name][3]
    scores, spans, info = G.assert_not_vacuous(d, radius, gap, min_score, R, copies, need_ties=integer or gap_mul == 0)
    n = len(info)
    assert n >= len(copies) and (name != "three" or n >= 3)
    loop = G.rounds_loop(d, radius, gap, min_score, R)             # cell by cell: the same results, paths and ties
    assert np.array_equal(loop[0].view(np.uint32), scores.view(np.uint32)) and np.array_equal(loop[1], spans) and loop[2] == info
    # round 0 without a band is the "Embedding repeats" recurrence on a probe of any length
    sc, pa, pb, _, _ = repeats_ref.local_loop(d, radius, gap)
    assert sc.view(np.uint32) == scores[0].view(np.uint32) and (pa, pb) == (tuple(spans[0, 0]), tuple(spans[0, 1]))
    assert (np.diff(scores) <= 0).all() and (scores[n:] == 0).all() and (spans[n:] == -1).all() and (scores[:n] >= min_score).all()
    for r in range(n):                                             # no path cell of a round lies in an earlier rectangle
        assert info[r]["path"][0] == (spans[r, 0, 0], spans[r, 1, 0]) and info[r]["path"][-1] == (spans[r, 0, 1] - 1, spans[r, 1, 1] - 1)
        for q in range(r):
            (a0, a1), (b0, b1) = spans[q]
            assert not any(a0 <= i < a1 and b0 <= j < b1 for i, j in info[r]["path"]), (r, q)
    # the kernel's form, at its own strip and tile, at small ones that put every edge into a small matrix, and as one strip
    for kw in (dict(), dict(strip=4, tile=8, per_super=2), dict(strip=5, tile=3, per_super=2), dict(strip=None)):
        s2, p2 = G.rounds(d, radius, gap, min_score, R, **kw)
        assert np.array_equal(s2.view(np.uint32), scores.view(np.uint32)) and np.array_equal(p2, spans), kw
    for k in (1, 2):                                               # fewer rounds are a prefix
        s2, p2 = G.rounds(d, radius, gap, min_score, k, strip=None)
        assert np.array_equal(s2, scores[:k]) and np.array_equal(p2, spans[:k])


@pytest.mark.parametrize("sep", [1, 5, 30])
def test_a_sequence_against_itself(sep):
    d, radius = _self_case()
    gap, min_score = radius, f32(3) * radius
    scores, spans, info = G.rounds_loop(d, radius, gap, min_score, 6, sep)
    assert len(info) >= 3 and (scores[:3] == f32(10) * radius).all()
    got = sorted((int(a0), int(b0)) for (a0, _), (b0, _) in spans[:3])
    assert got == [(5, 40), (5, 70), (40, 70)]
    for r in range(len(info)):
        assert all(j - i >= sep for i, j in info[r]["path"])       # nothing on or below the band
    for kw in (dict(strip=4, tile=8, per_super=2), dict(strip=8, tile=4, per_super=2), dict(), dict(strip=None)):
        s2, p2 = G.rounds(d, radius, gap, min_score, 6, sep, **kw)  # small tiles: whole tiles lie in the band and are skipped
        assert np.array_equal(s2.view(np.uint32), scores.view(np.uint32)) and np.array_equal(p2, spans), kw
    # a band that blocks every cell, and one that leaves a corner
    assert G.rounds_loop(d, radius, gap, min_score, 2, 90)[0].tolist() == [0, 0]
    assert G.rounds(d, radius, gap, min_score, 2, 90, strip=4, tile=8)[0].tolist() == [0, 0]


def test_random_matrices_with_holes():
    rng = np.random.default_rng(8)
    for trial in range(6):
        m, L = int(rng.integers(1, 30)), int(rng.integers(1, 40))
        d = rng.integers(0, 6, (m, L)).astype(np.float32)          # small integers: ties everywhere
        d[rng.random((m, L)) < 0.05] = np.inf
        d[rng.random((m, L)) < 0.02] = np.nan
        sep = int(rng.integers(0, 4))
        radius, gap = f32(3), f32(rng.integers(0, 3))
        want = G.rounds_loop(d, radius, gap, f32(4), 7, sep)
        for kw in (dict(strip=4, tile=8, per_super=2), dict(strip=3, tile=5, per_super=2), dict(strip=None)):
            got = G.rounds(d, radius, gap, f32(4), 7, sep, **kw)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1]), (trial, kw)
        assert (np.diff(want[0]) <= 0).all()
    for d in (np.zeros((0, 5), np.float32), np.zeros((1, 0), np.float32)):       # an empty side: padding
        for fn in (G.rounds_loop, G.rounds):
            out = fn(d, f32(1), f32(1), f32(1), 3)
            assert out[0].tolist() == [0, 0, 0] and (out[1] == -1).all()


@pytest.mark.parametrize("defect", ["rect", "band", "zero_start", "tie"])
def test_planted_misreadings_are_rejected(defect):
    """each wrong reading of the contract changes a result on these fixtures, so agreement with them means something"""
    differs = False
    for name in ("three", "edges"):
        d, radius, _ = _case(name)
        for gap in (f32(0), radius):
            good = G.rounds_loop(d, radius, gap, f32(1), 5)          # a low floor: the rounds go on into single cells
            bad = G.rounds_loop(d, radius, gap, f32(1), 5, _defect=defect)
            differs |= not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1]))
    d, radius = _self_case()
    for sep in (1, 30):                                            # 30: the second and third occurrence lie on the band's edge
        good = G.rounds_loop(d, radius, f32(0), f32(3) * radius, 5, sep)
        bad = G.rounds_loop(d, radius, f32(0), f32(3) * radius, 5, sep, _defect=defect)
        differs |= not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1]))
    assert differs, defect


def test_float64_bound_is_small_against_the_score():
    rng = np.random.default_rng(4)
    x, y = G.planted(rng, 150, 200, 32, [(20, 100, 40, "drop")], False)
    import dtw_ref
    d64 = dtw_ref.local_costs(x.astype(np.float64), y.astype(np.float64), "l2")
    radius = f32(16.0)
    s64 = float(G.rounds(d64, radius, radius, f32(1), 1, dtype=np.float64, strip=None)[0][0])
    s32 = float(G.rounds(repeats_ref.local_costs32(x, y), radius, radius, f32(1), 1, strip=None)[0][0])
    bound = G.score_error_bound(x, y, s64, radius, radius)
    assert s64 > 50 * float(radius) and abs(s32 - s64) <= bound < 1e-3 * s64


def test_the_public_names():
    import sylber_amd
    from sylber_amd import search
    assert "local_align_sequences" in sylber_amd.__all__ and sylber_amd.local_align_sequences is search.local_align_sequences
    assert callable(search.SyllableIndex.local_align_sequences) and callable(search.IVFSyllableIndex.local_align_sequences)
    assert search.MAX_LOCAL_BEST == G.MAX_BEST
    for bad in (dict(n_best=0), dict(n_best=33), dict(n_best=True), dict(n_best=1.5), dict(min_sep=0), dict(min_sep=-1)):
        with pytest.raises(ValueError):
            search._local_rounds(**dict(dict(n_best=1, min_sep=1), **bad))

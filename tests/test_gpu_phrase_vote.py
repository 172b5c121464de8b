"""GPU tier, the vote of the seeded phrase search (csrc/phrase_vote.hip, ``sylber_phrase_vote``), called through the C ABI with hand-made
seeds: ``cand`` and ``bound`` are bitwise those of tests/phrase_vote_ref.py.

* phrase lengths {1, 2, 63, 64} x seeds {1, 7, 32, 33, 128} (32 | 33 is where the launcher goes from 256 to 1 024 threads; 64 x 128 is
  the full 8 192-seed phrase), both metrics, ``-1`` / NaN / ``+inf`` seeds in the middle of rows, duplicates, outputs pre-filled;
* all seeds in one sequence; 8 192 seeds in 8 192 one-row sequences; equal bounds; a row without a valid seed; a phrase without one;
  shuffled seeds and duplicates; group exclusion; m above and below the number of seen sequences;
* bad arguments return 1 and name the entry."""
import numpy as np
import pytest
import torch

import phrase_vote_ref as V

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
METRIC = {"l2": 0, "cosine": 1}


def _vote(sc, ids, rows, lens, off, metric, m, pg=None, sg=None):
    """the library's (cand int32 [P, m], bound fp32 [P, m]) as numpy, from outputs pre-filled with garbage"""
    from sylber_amd import _lib
    from sylber_amd.kmeans import _stream, _vp
    lib = _lib.load()
    dev = torch.device(DEV)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    sc_d, id_d = t(sc, np.float32), t(ids, np.int64)
    row_d, len_d, off_d = t(rows, np.int32), t(lens, np.int32), t(off, np.int32)
    pg_d = t(pg, np.int32) if pg is not None else None
    sg_d = t(sg, np.int32) if sg is not None else None
    P = len(lens)
    cand = torch.full((P, m), 12345, dtype=torch.int32, device=dev)
    bound = torch.full((P, m), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.sylber_phrase_vote(_vp(sc_d), _vp(id_d), sc.shape[1], _vp(row_d), _vp(len_d), P, _vp(off_d), len(off) - 1,
                                          METRIC[metric], _vp(pg_d), _vp(sg_d), m, _vp(cand), _vp(bound), _stream(dev)),
                   "sylber_phrase_vote")
    torch.cuda.synchronize(dev)
    return cand.cpu().numpy(), bound.cpu().numpy()


def _check(sc, ids, rows, lens, off, metric, m, pg=None, sg=None):
    want = V.vote(sc, ids, rows, lens, off, metric, m, pg, sg)
    got = _vote(sc, ids, rows, lens, off, metric, m, pg, sg)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (got[1], want[1])
    return got


def _random_seeds(rng, R, seeds, N, metric, spoil=True):
    ids = rng.integers(0, N, (R, seeds)).astype(np.int64)
    sc = (rng.random((R, seeds)) * (2.0 if metric == "cosine" else 9.0) - (1.0 if metric == "cosine" else 0.0)).astype(np.float32)
    sc = np.round(sc * 8) / np.float32(8) if rng.random() < 0.5 else sc          # coarse values: equal costs and equal bounds happen
    if spoil and seeds >= 3:                                                  # ignored seeds in the middle of rows
        c = seeds // 2
        ids[0::3, c] = -1
        sc[1::3, c] = np.nan
        sc[2::3, c] = -np.inf if metric == "cosine" else np.inf
    return sc.astype(np.float32), ids


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("seeds", [1, 7, 32, 33, 128])
def test_lengths_and_seed_counts(metric, seeds):
    """phrases of 1, 2, 63 and 64 rows (and a few between) in one launch, against 37 sequences of 1 .. 40 rows"""
    rng = np.random.default_rng(seeds)
    off = np.concatenate([[0], np.cumsum(rng.integers(1, 41, 37))])
    lens = np.array([1, 2, 63, 64, 5, 17, 64, 1])
    rows = np.cumsum(lens) - lens
    sc, ids = _random_seeds(rng, int(lens.sum()), seeds, int(off[-1]), metric)
    for m in (1, 16, 128):
        cand, bound = _check(sc, ids, rows, lens, off, metric, m)
    assert (cand >= 0).sum() > 0
    # phrases launched one at a time, in another order, give the same rows
    for p in (3, 0, 6):
        c1, b1 = _vote(sc, ids, rows[p:p + 1], lens[p:p + 1], off, metric, 128)
        assert np.array_equal(c1[0], cand[p]) and np.array_equal(b1[0].view(np.uint32), bound[p].view(np.uint32))


def test_all_seeds_in_one_sequence():
    rng = np.random.default_rng(0)
    off = np.array([0, 10, 5000, 5003])
    ids = rng.integers(10, 5000, (64, 128)).astype(np.int64)
    sc = rng.random((64, 128)).astype(np.float32)
    cand, bound = _check(sc, ids, [0], [64], off, "l2", 4)
    assert cand[0].tolist() == [1, -1, -1, -1]
    assert bound[0, 0] == np.add.accumulate(np.concatenate([[np.float32(0)], sc.min(1)]), dtype=np.float32)[-1]


def test_8192_seeds_in_8192_one_row_sequences():
    rng = np.random.default_rng(1)
    off = np.arange(8193)
    ids = rng.permutation(8192).reshape(64, 128).astype(np.int64)
    sc = (rng.integers(0, 50, (64, 128)) / 4).astype(np.float32)               # many equal bounds: the smaller sequence number wins
    for m in (128, 3):
        cand, bound = _check(sc, ids, [0], [64], off, "l2", m)
    assert (cand >= 0).all()


def test_equal_bounds_take_the_smaller_sequence():
    off = np.array([0, 2, 4, 6, 8])
    sc = np.array([[1, 1, 2, 1]], np.float32)
    ids = np.array([[6, 2, 0, 5]], np.int64)
    cand, bound = _check(sc, ids, [0], [1], off, "l2", 6)                    # m above the number of seen sequences
    assert cand[0].tolist() == [1, 2, 3, 0, -1, -1] and bound[0].tolist() == [1, 1, 1, 2, np.inf, np.inf]
    cand, bound = _check(sc, ids, [0], [1], off, "l2", 2)                    # and below
    assert cand[0].tolist() == [1, 2]


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_rows_and_phrases_without_valid_seeds(metric):
    off = np.array([0, 4, 8])
    bad = -np.inf if metric == "cosine" else np.inf
    # phrase 0: row 1 has no valid seed; phrase 1: no valid seed at all; phrase 2: an ordinary one behind it
    sc = np.array([[0.5, 0.75], [bad, np.nan], [0.25, bad],
                   [np.nan, np.nan], [bad, 0.5],
                   [0.5, 0.25]], np.float32)
    ids = np.array([[1, 5], [-1, 3], [6, -1],
                    [2, 3], [1, -1],
                    [7, 0]], np.int64)
    cand, bound = _check(sc, ids, [0, 3, 5], [3, 2, 1], off, metric, 3)
    assert cand[0].tolist() == ([1, 0, -1] if metric == "cosine" else [0, 1, -1])
    assert (cand[1] == -1).all() and np.isposinf(bound[1]).all()
    assert (cand[2, :2] >= 0).all()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_duplicates_shuffles_and_exclusion(metric):
    rng = np.random.default_rng(5)
    off = np.concatenate([[0], np.cumsum(rng.integers(1, 9, 50))])
    lens = np.array([9, 64, 3])
    rows = np.cumsum(lens) - lens
    R, seeds = int(lens.sum()), 20
    sc, ids = _random_seeds(rng, R, seeds, int(off[-1]), metric)
    base = _check(sc, ids, rows, lens, off, metric, 24)
    perm = np.stack([rng.permutation(seeds) for _ in range(R)])
    sh = _check(np.take_along_axis(sc, perm, 1), np.take_along_axis(ids, perm, 1), rows, lens, off, metric, 24)
    dup = _check(np.concatenate([sc, sc], 1), np.concatenate([ids, ids], 1), rows, lens, off, metric, 24)
    for other in (sh, dup):
        assert np.array_equal(base[0], other[0]) and np.array_equal(base[1].view(np.uint32), other[1].view(np.uint32))
    sg = rng.integers(0, 4, 50).astype(np.int32)
    pg = np.array([0, 3, 1], np.int32)
    ex = _check(sc, ids, rows, lens, off, metric, 24, pg, sg)
    for p in range(3):
        got = ex[0][p][ex[0][p] >= 0]
        assert (sg[got] != pg[p]).all() and got.size


def test_bad_arguments_return_1_without_a_launch():
    from sylber_amd import _lib
    lib = _lib.load()
    names = ["seed_score", "seed_id", "seeds", "phrase_row", "phrase_len", "n_phrases", "seq_offsets", "n_seq", "metric", "phrase_group",
             "seq_group", "m", "cand", "bound", "stream"]
    assert len(names) == len(_lib.EXPORTS["sylber_phrase_vote"][1])
    buf = torch.zeros(64, dtype=torch.int64, device=DEV)
    ptr = buf.data_ptr()
    good = dict(seed_score=ptr, seed_id=ptr, seeds=2, phrase_row=ptr, phrase_len=ptr, n_phrases=1, seq_offsets=ptr, n_seq=1, metric=0,
                phrase_group=None, seq_group=None, m=2, cand=ptr, bound=ptr, stream=None)
    bad = [dict(seed_score=None), dict(seed_id=None), dict(phrase_row=None), dict(phrase_len=None), dict(seq_offsets=None),
           dict(cand=None), dict(bound=None), dict(seeds=0), dict(seeds=129), dict(n_phrases=0), dict(n_seq=0), dict(metric=2),
           dict(m=0), dict(m=129), dict(phrase_group=ptr), dict(seq_group=ptr)]
    torch.cuda.synchronize()
    for kw in bad:
        a = dict(good, **kw)
        assert lib.sylber_phrase_vote(*[a[n] for n in names]) == 1, kw
        assert lib.sylber_last_error().decode().startswith("sylber_phrase_vote: "), kw
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0                                         # nothing was written

"""GPU tier, repeated phrases on embeddings (csrc/dtw_local.hip behind ``SyllableIndex.search_repeats`` / ``find_repeats``): local
alignment of probes against every sequence of the index.

* bitwise against the contract, by the method of tests/test_gpu_phrase.py: the local costs are taken from the library itself
  (``SyllableIndex.search`` over pieces of at most 128 rows gives every d[i][j]), the fp32 reference of tests/repeats_ref.py runs
  over them, and scores (as uint32), sequences, spans and order must be exactly those;
* planted copies whose best cell lies where the gather over the lanes of a probe can go wrong;
* long sequences under every cut; invariance under the hooks, one ``add`` against many and ``save`` / ``load``; NaN and zero rows,
  group exclusion, explicit sequences, short lists; every refusal; float64 within ``repeats_ref.score_error_bound``;
* ``find_repeats`` whole against the reference built from the contract, the window theorem on a planted pair, ``hop = window`` and
  ``hop = 1``, group exclusion, fewer than two sequences, and end to end from ``Segmenter`` outputs."""
import numpy as np
import pytest
import torch

import dtw_ref
import repeats_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
INF = np.float32(np.inf)


def _np(t):
    return t.cpu().numpy()


def _local_costs(x, offsets, rows, metric):
    """d [R, N] fp32 of the probe rows against every database row, from ``search`` on pieces of one sequence (<= 128 rows)"""
    from sylber_amd import SyllableIndex
    N = x.shape[0]
    d = np.full((rows.shape[0], N), INF, np.float32)
    for s in range(len(offsets) - 1):
        for lo in range(int(offsets[s]), int(offsets[s + 1]), 128):
            hi = min(lo + 128, int(offsets[s + 1]))
            sc, ids = SyllableIndex(x[lo:hi], metric=metric, device=DEV).search(rows, hi - lo)
            sc, ids = _np(sc), _np(ids)
            v = sc if metric == "l2" else np.maximum(np.float32(0), np.float32(1) - sc)
            r, c = np.nonzero(ids >= 0)                      # a NaN score is never returned: that cell stays +inf
            d[r, lo + ids[r, c]] = v[r, c]
    return d


def _d_of(x, offsets, probes, metric):
    d = _local_costs(x, offsets, np.concatenate(probes), metric)
    r0 = np.concatenate([[0], np.cumsum([len(p) for p in probes])])
    return lambda p, s: d[r0[p]:r0[p + 1], offsets[s]:offsets[s + 1]]


def _assert_same(got, ref, what=""):
    c, q, sp = (_np(t) for t in got)
    assert np.array_equal(q, ref[1]), what
    assert np.array_equal(c.view(np.uint32), ref[0].astype(np.float32).view(np.uint32)), what
    assert np.array_equal(sp, ref[2]), what


def _groups_of(offsets):
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets)).astype(np.int32)


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


SEQ_LENS = [128, 1, 127, 5, 123, 128, 2, 60, 66, 100, 28, 128, 37, 1, 1, 90, 126, 3, 64, 64, 128, 128, 17, 111]
# a cell of two unrelated rows is closer than the radius with a probability of about 0.1: most (probe, sequence) pairs have a
# positive cell, a short probe against a short sequence often has none
RADIUS = {(16, True, "l2"): 40.0, (16, False, "l2"): 20.0, (768, True, "l2"): 2900.0, (768, False, "l2"): 1400.0,
          (16, True, "cosine"): 0.75, (16, False, "cosine"): 0.75, (768, True, "cosine"): 0.953125, (768, False, "cosine"): 0.953125}


def _corpus(D, integer, seed):
    """tests/test_gpu_phrase.py's corpus: sequences of 1 .. 128 rows whose edges fall inside and on 128-row tile edges, whole
    duplicated sequences and a run of equal rows; probes of 1, 2, 7, 63 and 64 rows and five that share a 64-row half"""
    rng = np.random.default_rng(seed)
    offsets = _offsets(SEQ_LENS)
    N = int(offsets[-1])
    x = rng.integers(-2, 3, (N, D)).astype(np.float32) if integer else rng.standard_normal((N, D)).astype(np.float32)
    x[offsets[5]:offsets[6]] = x[offsets[0]:offsets[1]]       # sequence 5 = sequence 0; 20 and 21 = 11
    x[offsets[20]:offsets[21]] = x[offsets[11]:offsets[12]]
    x[offsets[21]:offsets[22]] = x[offsets[11]:offsets[12]]
    x[offsets[9] + 10:offsets[9] + 20] = x[offsets[9] + 9]    # a run of equal rows
    probes = []
    for m in (1, 2, 7, 63, 64):
        a = int(rng.integers(0, N - m))
        p = x[a:a + m].copy()
        if not integer:
            p += 0.3 * rng.standard_normal(p.shape).astype(np.float32)
        probes.append(p)
    probes.append(x[offsets[11] + 3:offsets[11] + 10].copy())  # exact copies: equal scores in sequences 11, 20, 21
    probes.append(np.repeat(x[offsets[9] + 9][None], 5, 0))
    for m, a in ((20, offsets[2] + 100), (30, offsets[15] + 70), (2, offsets[13])):       # ... across sequence ends
        probes.append(x[a:a + m].copy())
    return x, offsets, probes


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,integer", [(16, True), (16, False), (768, False), (768, True)])
def test_bitwise_against_the_contract(D, integer, metric):
    from sylber_amd import SyllableIndex
    x, offsets, probes = _corpus(D, integer, D + integer)
    S, P = len(offsets) - 1, len(probes)
    idx = SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)
    assert np.array_equal(idx.sequence_offsets(), offsets)
    d_of = _d_of(x, offsets, probes, metric)
    radius = F(RADIUS[(D, integer, metric)])
    low = F(0.5) if metric == "l2" else F(2.0 ** -10)          # a min_score that keeps nearly every positive pair
    for gap in (F(0), radius, F(2) * radius):
        ref = R.search_repeats(d_of, P, offsets, 128, radius, gap, low)
        pos = ref[3]
        print("positive pairs", D, integer, metric, "gap", float(gap), int(pos.sum()), "of", pos.size)
        assert pos.sum() > 0.5 * pos.size and (~pos).sum() >= 3              # most pairs have a result, some have none
        _assert_same(idx.search_repeats(probes, S, radius, gap=gap, min_score=low), [r[:, :S] for r in ref[:3]], "k = S")
        _assert_same(idx.search_repeats(probes, 128, radius, gap=gap, min_score=low), ref[:3], "k = 128")
    # the defaults: gap = 2 radius, min_score = 3 radius
    ref = R.search_repeats(d_of, P, offsets, S, radius, F(2) * radius, F(3) * radius)
    got = idx.search_repeats(probes, S, float(radius))
    _assert_same(got, ref[:3], "defaults")
    assert (ref[1] >= 0).any() and (ref[1] < 0).any()
    got2 = idx.search_repeats(np.concatenate(probes), S, radius, lengths=[len(p) for p in probes])
    for a, b in zip(got, got2):
        assert torch.equal(a, b)


def test_where_the_gather_can_go_wrong():
    """planted copies whose best cell lies in the probe's first, a middle and its last row; in a sequence's first and last column;
    in the last column before a tile edge and the first after it; in a one-row sequence; two sequences ending in neighbouring
    columns"""
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(21)
    D = 16
    lens = [100, 80, 1, 1, 30, 44, 64, 1, 63, 100, 1, 60]     # tile edges 127 | 128 and 511 | 512 lie inside sequences 1 and 11;
    offsets = _offsets(lens)                                  # sequences 5 and 8 end at 255 and 383, sequences 6 and 9 begin behind them
    assert offsets.tolist() == [0, 100, 180, 181, 182, 212, 256, 320, 321, 384, 484, 485, 545]
    N, S = int(offsets[-1]), len(lens)
    x = (3 * rng.standard_normal((N, D))).astype(np.float32)
    probes = [(3 * rng.standard_normal((m, D))).astype(np.float32) for m in (20, 20, 64, 9, 1, 33)]
    want, used = {}, np.zeros(N, bool)

    def plant(p, i0, i1, j1):
        """rows i0 .. i1 of probe p end at row j1 of the index: the best cell of (p, that sequence) is (i1, j1)"""
        j0 = j1 - (i1 - i0)
        s = int(np.searchsorted(offsets, j1, side="right")) - 1
        assert offsets[s] <= j0 and not used[j0:j1 + 1].any() and (p, s) not in want
        x[j0:j1 + 1], used[j0:j1 + 1] = probes[p][i0:i1 + 1], True
        want[(p, s)] = (i0, i1, j1)
    plant(0, 0, 0, 50)                                        # the probe's first row
    plant(0, 5, 11, 127)                                      # a middle row; the last column before a tile edge
    plant(1, 3, 10, 135)                                      # begins in the first column after that edge
    plant(0, 7, 7, 180)                                       # a one-row sequence ...
    plant(0, 9, 9, 181)                                       # ... and its one-row neighbour
    plant(0, 12, 19, 211)                                     # the probe's last row in a sequence's last column
    plant(1, 0, 0, 212)                                       # a sequence's first column, the probe's first row
    plant(3, 0, 8, 255)                                       # a sequence's last column = the last column before a tile edge
    plant(2, 0, 63, 319)                                      # 64 rows behind a tile edge, ending in the sequence's last column ...
    plant(2, 63, 63, 320)                                     # ... and the same lane again in the next column: a one-row sequence
    plant(5, 1, 32, 383)                                      # the last row in the last column before a tile edge
    plant(5, 0, 0, 384)                                       # the first row in the first column behind it
    plant(1, 19, 19, 483)                                     # two sequences ending in neighbouring columns: 483 ...
    plant(4, 0, 0, 484)                                       # ... and 484, a one-row probe
    plant(3, 2, 8, 512)                                       # the last row in the first column behind a tile edge, inside a sequence
    for metric, radius in (("l2", F(8)), ("cosine", F(0.125))):
        idx = SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)
        d_of = _d_of(x, offsets, probes, metric)
        for gap in (F(0), F(2) * radius):
            ref = R.search_repeats(d_of, len(probes), offsets, S, radius, gap, F(radius / 2))
            for (p, s), (i0, i1, j1) in want.items():         # the reference finds what was planted
                r = np.nonzero(ref[1][p] == s)[0]
                assert r.size == 1, (p, s)
                sp = ref[2][p, r[0]]
                assert sp[0, 1] == i1 + 1 and sp[1, 1] == j1 + 1 and sp[0, 0] <= i0 and sp[1, 1] - sp[1, 0] >= i1 - i0 + 1, (p, s, sp)
            for kw in ({}, {"splits": N}, {"splits": 3}, {"block_phrases": 1}):
                _assert_same(idx.search_repeats(probes, S, radius, gap=gap, min_score=F(radius / 2), **kw), ref[:3], (metric, gap, kw))


@pytest.mark.parametrize("D,metric", [(16, "l2"), (768, "cosine")])
def test_long_sequences_under_every_cut(D, metric):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(D)
    lens = [3000, 70, 1500, 128, 2049, 1, 700]
    offsets = _offsets(lens)
    N, S = int(offsets[-1]), len(lens)
    x = rng.standard_normal((N, D)).astype(np.float32)
    probes = []
    for m, a in ((1, 5), (7, 2990), (64, 4000), (33, 7000), (12, 3060)):
        p = x[a:a + m] + 0.2 * rng.standard_normal((m, D)).astype(np.float32)
        probes.append(np.delete(p, m // 2, 0) if m > 2 else p)
    idx = SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)
    radius = F(RADIUS[(D, False, metric)])
    low = F(radius / 8) if metric == "l2" else F(2.0 ** -10)
    ref = R.search_repeats(_d_of(x, offsets, probes, metric), len(probes), offsets, S, radius, radius, low)
    print("long sequences", D, metric, "results", int((ref[1] >= 0).sum()), "of", ref[1].size)
    assert (ref[1] >= 0).sum() >= 20
    for splits in (0, 1, 2, 3, 4, 5, 6, S, N):                # N: a cut at every sequence start
        _assert_same(idx.search_repeats(probes, S, radius, gap=radius, min_score=low, splits=splits), ref[:3], splits)


def test_invariance_is_bitwise(tmp_path):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(8)
    D = 64
    lens = rng.integers(1, 300, 60)
    offsets = _offsets(lens)
    N, grp = int(offsets[-1]), _groups_of(offsets)
    x = np.round(rng.standard_normal((N, D)) * 2).astype(np.float32) / 2
    probes = [x[a:a + m] + np.float32(0.5) * rng.integers(-1, 2, (m, D)).astype(np.float32)
              for m, a in zip(rng.integers(1, 65, 70), rng.integers(0, N - 64, 70))]
    idx = SyllableIndex(x, metric="l2", groups=grp, device=DEV)
    k, radius, low = 12, F(90), F(1)                          # unrelated rows: d about 2 D = 128 +- 23
    base = idx.search_repeats(probes, k, radius, min_score=low)
    assert (base[1] >= 0).float().mean() > 0.9
    for kw in ({"splits": 1}, {"splits": 3}, {"splits": 17}, {"splits": N}, {"phrase_chunk": 1}, {"phrase_chunk": 7}, {"phrase_chunk": 69},
               {"block_phrases": 1}, {"block_phrases": 2}, {"block_phrases": 5, "splits": 4, "phrase_chunk": 33},
               {"_workspace_fill": 0x00}, {"_workspace_fill": 0xFF}, {"_workspace_fill": 0xFF, "splits": 9}):
        got = idx.search_repeats(probes, k, radius, min_score=low, **kw)
        for a, b in zip(base, got):
            assert torch.equal(a, b), kw
    for p in (0, 13, 69):                                     # alone against in a batch of others
        got = idx.search_repeats([probes[p]], k, radius, min_score=low)
        for a, b in zip(base, got):
            assert torch.equal(a[p:p + 1], b)
    many = SyllableIndex(metric="l2", device=DEV)             # one add against many
    for s in range(len(lens)):
        many.add(x[offsets[s]:offsets[s + 1]], groups=grp[offsets[s]:offsets[s + 1]])
    for a, b in zip(base, many.search_repeats(probes, k, radius, min_score=low)):
        assert torch.equal(a, b)
    idx.save(str(tmp_path / "idx.npz"))                       # save / load
    back = SyllableIndex.load(str(tmp_path / "idx.npz"), device=DEV)
    for a, b in zip(base, back.search_repeats(probes, k, radius, min_score=low)):
        assert torch.equal(a, b)
    ref = R.search_repeats(_d_of(x, offsets, probes[:6], "l2"), 6, offsets, k, radius, F(2) * radius, low)
    _assert_same([t[:6] for t in base], ref[:3])


def test_exclusion_short_lists_nan_and_zero_rows_and_explicit_sequences():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(9)
    D = 16
    lens = [5, 9, 130, 4, 7, 3]
    offsets = _offsets(lens)
    N = int(offsets[-1])
    x = rng.standard_normal((N, D)).astype(np.float32)
    x[offsets[1] + 4] = np.nan                                # a NaN row inside sequence 1
    x[offsets[4]:offsets[5]] = np.nan                         # sequence 4 is NaN throughout
    x[offsets[2] + 100] = 0.0                                 # a zero row
    grp = np.array([0] * 5 + [1] * 9 + [0] * 130 + [2] * 4 + [3] * 7 + [1] * 3, np.int32)
    probes = [rng.standard_normal((m, D)).astype(np.float32) for m in (3, 1, 10, 2)]
    probes[3][1] = np.nan                                     # a NaN probe row: its cells are +inf, the other row still matches
    probes.append(np.zeros((2, D), np.float32))
    probes.append(x[offsets[1] + 2:offsets[1] + 7].copy())    # a copy with the NaN row in its middle: two runs of two rows
    pgrp = np.array([0, 1, 2, 0, 3, 2], np.int32)
    for metric, radius in (("l2", F(24)), ("cosine", F(0.875))):
        idx = SyllableIndex(x, metric=metric, groups=grp, device=DEV)
        assert np.array_equal(idx.sequence_offsets(), offsets)
        sgrp = grp[offsets[:-1]]
        k, low = 8, F(radius / 8)                             # more than the 6 sequences: short lists
        d_of = _d_of(x, offsets, probes, metric)
        for gap in (F(0), F(2) * radius):
            ref = R.search_repeats(d_of, len(probes), offsets, k, radius, gap, low)
            got = idx.search_repeats(probes, k, radius, gap=gap, min_score=low)
            _assert_same(got, ref[:3], (metric, gap))
            c, q, sp = (_np(t) for t in got)
            assert (q[:, 6:] == -1).all() and (c[:, 6:] == 0).all() and (sp[:, 6:] == -1).all()
            if metric == "l2":
                assert 4 not in q                             # a NaN sequence is never returned
                assert (q[4] == -1).all() or (c[4][q[4] >= 0] > 0).all()
            ref = R.search_repeats(d_of, len(probes), offsets, k, radius, gap, low, probe_groups=pgrp, seq_groups=sgrp)
            got = idx.search_repeats(probes, k, radius, gap=gap, min_score=low, groups=pgrp, exclude_same_group=True)
            _assert_same(got, ref[:3], (metric, gap, "groups"))
            q = _np(got[1])
            assert not np.isin(q[0], [0, 2]).any() and not np.isin(q[1], [1, 5]).any() and not np.isin(q[2], [3]).any()
        # explicit sequences: cut the long one, join the short ones
        seqs = np.array([0, 14, 80, 144, N], np.int64)
        d_of = _d_of(x, seqs, probes, metric)
        ref = R.search_repeats(d_of, len(probes), seqs, 3, radius, radius, low, probe_groups=pgrp, seq_groups=grp[seqs[:-1]])
        _assert_same(idx.search_repeats(probes, 3, radius, gap=radius, min_score=low, sequences=seqs, groups=pgrp, exclude_same_group=True), ref[:3])
        ref = R.search_repeats(d_of, len(probes), seqs, 3, radius, radius, low)
        _assert_same(idx.search_repeats(probes, 3, radius, gap=radius, min_score=low, sequences=torch.from_numpy(seqs)), ref[:3])


def _spy(monkeypatch, name="sylber_dtw_local"):
    from sylber_amd import _lib
    lib = _lib.load()
    launched = []
    real = getattr(lib, name)

    class Spy:
        def __call__(self, *a):
            launched.append(1)
            return real(*a)
    monkeypatch.setattr(_lib, "_LIB", type("L", (), {"__getattr__": lambda self, n: Spy() if n == name else getattr(lib, n)})())
    return launched


def test_every_refusal_comes_before_a_launch(monkeypatch):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(10)
    x = rng.standard_normal((40, 16)).astype(np.float32)
    idx = SyllableIndex(x, groups=np.repeat(np.arange(4), 10), device=DEV)
    launched = _spy(monkeypatch)
    p = [x[:3]]
    bad = [dict(probes=p, k=0), dict(probes=p, k=129), dict(probes=p, k=1.5), dict(probes=[x[:0]], k=1), dict(probes=[np.zeros((65, 16), np.float32)], k=1),
           dict(probes=[np.zeros((3, 32), np.float32)], k=1), dict(probes=p, k=1, exclude_same_group=True),
           dict(probes=p, k=1, groups=[0, 1], exclude_same_group=True), dict(probes=x[:5], k=1), dict(probes=x[:5], k=1, lengths=[2, 2]),
           dict(probes=x[:5], k=1, lengths=[5, 0]), dict(probes=x[:5], k=1, lengths=[[5]]), dict(probes=x[:5], k=1, lengths=[2.5, 2.5]),
           dict(probes=p, k=1, sequences=[0, 10, 10, 40]), dict(probes=p, k=1, sequences=[1, 40]), dict(probes=p, k=1, sequences=[0, 30]),
           dict(probes=p, k=1, sequences=[0, 25, 20, 40]), dict(probes=p, k=1, sequences=[40]), dict(probes=p, k=1, splits=-1),
           dict(probes=p, k=1, phrase_chunk=0), dict(probes=p, k=1, block_phrases=-1)]
    for r in (0, -1.0, float("nan"), float("inf"), 1e39, 1e-46, None, "1", True):
        bad.append(dict(probes=p, k=1, radius=r))
    for g in (-0.5, float("nan"), float("inf"), 1e39, "0"):
        bad.append(dict(probes=p, k=1, gap=g))
    for m in (0, -1.0, float("nan"), float("inf"), 1e-46, "3"):
        bad.append(dict(probes=p, k=1, min_score=m))
    bad.append(dict(probes=p, k=1, radius=2e38))              # the default min_score = 3 radius is not finite
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(ValueError):
            idx.search_repeats(kw.pop("probes"), kw.pop("k"), kw.pop("radius", 1.0), **kw)
    with pytest.raises(ValueError):
        SyllableIndex(device=DEV).search_repeats(p, 1, 1.0)
    with pytest.raises(ValueError):
        SyllableIndex(device=DEV).find_repeats(1, 1.0)
    for kw in (dict(k=0), dict(k=129), dict(radius=0), dict(radius=float("nan")), dict(gap=-1), dict(min_score=0), dict(window=65), dict(window=0),
               dict(hop=0), dict(hop=33, window=32), dict(hop=1.5), dict(window=True), dict(splits=-1), dict(phrase_chunk=0),
               dict(sequences=[0, 30])):
        kw = dict(kw)
        with pytest.raises(ValueError):
            idx.find_repeats(kw.pop("k", 2), kw.pop("radius", 1.0), **kw)
    big = SyllableIndex(np.zeros((65537, 16), np.float32), device=DEV)
    with pytest.raises(ValueError, match="sequences="):
        big.search_repeats(p, 1, 1.0)
    with pytest.raises(ValueError, match="sequences="):
        big.find_repeats(1, 1.0)
    assert not launched
    c, s, sp = big.search_repeats(p, 1, 1.0, sequences=[0, 65536, 65537])
    assert launched and s.shape == (1, 1) and sp.shape == (1, 1, 2, 2)
    launched.clear()
    c, s, sp = idx.search_repeats([], 4, 1.0)
    assert c.shape == (0, 4) and s.shape == (0, 4) and sp.shape == (0, 4, 2, 2) and not launched
    assert c.dtype == torch.float32 and s.dtype == torch.int64 and sp.dtype == torch.int64 and c.device.type == "cuda"


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_against_float64_within_the_derived_bound(metric):
    from sylber_amd import SyllableIndex
    x, offsets, probes, radii = R.float64_case()
    S, radius = len(offsets) - 1, radii[metric]
    idx = SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)
    xs = _np(idx.features).astype(np.float64)                # the rows as the index holds them (unit rows for cosine)
    qs = [_np(idx._prep(torch.from_numpy(p))).astype(np.float64) for p in probes]
    low = F(radius / 4)
    for gap in (F(0), F(2) * radius):
        c, q, sp = (_np(t) for t in idx.search_repeats(probes, S, radius, gap=gap, min_score=low))
        for p in range(len(probes)):
            s64, bound = np.empty(S), np.empty(S)
            for s in range(S):
                xr = xs[offsets[s]:offsets[s + 1]]
                s64[s] = R.local(dtw_ref.local_costs(qs[p], xr, metric), radius, gap, np.float64)[0]
                bound[s] = R.score_error_bound(qs[p], xr, s64[s], radius, gap, metric)
            got = q[p][q[p] >= 0]
            assert got.size >= 1 and len(set(got.tolist())) == got.size
            err = np.abs(c[p][:got.size].astype(np.float64) - s64[got])
            print("float64 check", metric, "gap", float(gap), "m", len(probes[p]), "max err / bound", float((err / bound[got]).max()))
            assert (err <= bound[got]).all()
            out = np.setdiff1d(np.arange(S), got)
            assert (s64[out] < float(low) + bound[out]).all()             # what is missing was below min_score
            assert (c[p][:got.size] >= low).all() and (np.diff(c[p]) <= 0).all()


# ---- find_repeats -------------------------------------------------------------------------------------------------------------------
def _repeat_corpus(seed=31, D=16):
    """12 sequences, sequence 8 of 150 rows (four windows of 64 at hop 32, the last one clipped), with planted repeats: rows
    100 .. 129 of sequence 8 again in sequence 10 (30 rows: inside one window at hop 32), 12 rows of sequence 0 in sequence 3, the
    whole of sequence 5 (9 rows) inside sequence 11, and 40 rows of sequence 8 again in sequence 9 (more than window - hop + 1)"""
    rng = np.random.default_rng(seed)
    lens = [25, 40, 3, 30, 1, 9, 64, 33, 150, 70, 45, 28]
    offsets = _offsets(lens)
    N = int(offsets[-1])
    x = rng.standard_normal((N, D)).astype(np.float32)

    def copy(dst, src, n, noise=0.15):
        x[dst:dst + n] = x[src:src + n] + noise * rng.standard_normal((n, D)).astype(np.float32)
    copy(offsets[10] + 5, offsets[8] + 100, 30)
    copy(offsets[3] + 10, offsets[0] + 4, 12)
    copy(offsets[11] + 15, offsets[5], 9)
    copy(offsets[9] + 20, offsets[8] + 20, 40)
    return x, offsets


@pytest.fixture(scope="module")
def repeat_case():
    from sylber_amd import SyllableIndex
    x, offsets = _repeat_corpus()
    # the probes are the rows as the index holds them, prepared like any probe: under "cosine" the unit rows, normalised once more
    return x, offsets, {m: _local_costs(x, offsets, _np(SyllableIndex(x, metric=m, device=DEV).features), m) for m in ("l2", "cosine")}


def _assert_repeats(got, ref, what=""):
    sc, pairs, spans = (_np(t) for t in got)
    assert np.array_equal(pairs, ref[1]), what
    assert np.array_equal(sc.view(np.uint32), ref[0].view(np.uint32)), what
    assert np.array_equal(spans, ref[2]), what


@pytest.mark.parametrize("metric,radius", [("l2", 12.0), ("cosine", 0.5)])
def test_find_repeats_against_the_contract(repeat_case, metric, radius):
    from sylber_amd import SyllableIndex
    x, offsets, dd = repeat_case
    d, radius = dd[metric], F(radius)
    idx = SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)
    # the defaults: only the planted repeats are three perfect matches long
    ref = R.find_repeats(d, offsets, 6, radius, F(2) * radius, F(3) * radius)
    got = idx.find_repeats(6, radius)
    _assert_repeats(got, ref, "defaults")
    assert ref[1][:4].tolist() == [[8, 9], [8, 10], [0, 3], [5, 11]] and (ref[1][4:] == -1).all(), ref[1]
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[2].shape == (6, 2, 2) and got[0].device.type == "cuda"
    # a low min_score lets chance pairs in: the per-pair reduction and the order among many
    low = F(radius / 4)
    for k, gap, kw in ((128, F(0), {}), (20, radius, {"phrase_chunk": 3}), (7, F(2) * radius, {"splits": 5, "_workspace_fill": 0xFF})):
        ref = R.find_repeats(d, offsets, k, radius, gap, low)
        assert (ref[1][:, 0] >= 0).sum() >= min(k, 30)
        _assert_repeats(idx.find_repeats(k, radius, gap=gap, min_score=low, **kw), ref, (k, gap))
    # the window theorem on the planted pair (8, 10): 30 rows <= 64 - 32 + 1, so the windows find what the whole sequence finds
    s8 = slice(offsets[8], offsets[9])
    full = R.local(d[s8, offsets[10]:offsets[11]], radius, F(2) * radius)
    assert full[1][1] - full[1][0] <= 33
    r = [i for i, pr in enumerate(_np(got[1]).tolist()) if pr == [8, 10]][0]
    assert _np(got[0])[r].view(np.uint32) == F(full[0]).view(np.uint32)
    assert _np(got[2])[r].tolist() == [[full[1][0] + offsets[8], full[1][1] + offsets[8]], [full[2][0] + offsets[10], full[2][1] + offsets[10]]]
    # (8, 9) is 40 rows long: no window holds it, its score is not larger than the whole sequence's
    full = R.local(d[s8, offsets[9]:offsets[10]], radius, F(2) * radius)
    assert 0 < _np(got[0])[0] <= full[0]


@pytest.mark.parametrize("window,hop", [(64, 64), (16, 1), (33, 20)])
def test_find_repeats_windows(repeat_case, window, hop):
    from sylber_amd import SyllableIndex
    x, offsets, dd = repeat_case
    radius = F(12)
    idx = SyllableIndex(x, metric="l2", groups=_groups_of(offsets), device=DEV)
    ref = R.find_repeats(dd["l2"], offsets, 10, radius, F(2) * radius, radius, window, hop)
    assert (ref[1][:, 0] >= 0).sum() >= 4
    _assert_repeats(idx.find_repeats(10, radius, min_score=radius, window=window, hop=hop), ref, (window, hop))
    _assert_repeats(idx.find_repeats(10, radius, min_score=radius, window=window, hop=hop, phrase_chunk=5, splits=2), ref, (window, hop, "chunks"))


def test_find_repeats_groups_sequences_and_too_few(repeat_case, monkeypatch):
    from sylber_amd import SyllableIndex
    x, offsets, dd = repeat_case
    radius = F(12)
    grp = np.repeat(np.array([0, 1, 2, 0, 3, 4, 5, 6, 7, 7, 8, 4], np.int32), np.diff(offsets))     # 0 ~ 3, 8 ~ 9 and 5 ~ 11 share a group
    idx = SyllableIndex(x, metric="l2", groups=grp, device=DEV)
    assert len(idx.sequence_offsets()) == 12                  # 8 and 9 run together by default: pass the sequences
    ref = R.find_repeats(dd["l2"], offsets, 6, radius, F(2) * radius, F(3) * radius, groups=grp)
    assert ref[1].tolist()[:2] == [[8, 10], [-1, -1]]
    _assert_repeats(idx.find_repeats(6, radius, sequences=offsets, exclude_same_group=True), ref)
    ref = R.find_repeats(dd["l2"], offsets, 6, radius, F(2) * radius, F(3) * radius)
    _assert_repeats(idx.find_repeats(6, radius, sequences=offsets), ref)
    # one add against many, save / load: covered for search_repeats; here: fewer than two sequences is padding without a launch
    launched = _spy(monkeypatch)
    one = SyllableIndex(x[:50], metric="l2", device=DEV)
    sc, pairs, spans = one.find_repeats(3, radius)
    assert not launched and sc.tolist() == [0, 0, 0] and (pairs == -1).all() and (spans == -1).all()
    assert sc.shape == (3,) and pairs.shape == (3, 2) and spans.shape == (3, 2, 2)
    sc, pairs, spans = idx.find_repeats(3, F(1e-3), sequences=offsets)       # nothing is that close: padding after the launches
    assert launched and (pairs == -1).all() and (sc == 0).all()


def test_segmenter_outputs_end_to_end():
    from sylber_amd import Segmenter, SyllableIndex
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_state_dict
    seg = Segmenter(model_ckpt=synthetic_state_dict(0), device=DEV)
    wavs = [syllable_wave(int(m), s) for s, m in enumerate([40000, 24000, 32000], start=70)]
    wavs = [wavs[0], wavs[1], wavs[0], wavs[2]]               # clip 0 is in the batch twice
    outs = seg(wav=wavs, in_second=False)
    counts = [len(o["segments"]) for o in outs]
    assert counts[0] == counts[2] and counts[0] >= 3, counts
    nonempty = [ci for ci, c in enumerate(counts) if c]
    idx = SyllableIndex.from_outputs(outs, metric="cosine")
    off = idx.sequence_offsets()
    a, b = nonempty.index(0), nonempty.index(2)
    sc, pairs, spans = (_np(t) for t in idx.find_repeats(3, 0.05))
    print("end to end", counts, sc.tolist(), pairs.tolist(), spans.tolist())
    assert pairs[0].tolist() == [a, b] and sc[0] > 0
    assert spans[0, 0, 1] - spans[0, 0, 0] == spans[0, 1, 1] - spans[0, 1, 0] >= 3
    assert off[a] <= spans[0, 0, 0] < spans[0, 0, 1] <= off[a + 1] and off[b] <= spans[0, 1, 0] < spans[0, 1, 1] <= off[b + 1]
    prov = idx.provenance(spans[0, :, 0])
    assert prov[0][0] == 0 and prov[1][0] == 2 and prov[0][1] == prov[1][1]

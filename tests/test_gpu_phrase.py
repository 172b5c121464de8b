"""GPU tier, phrase search (csrc/dtw.hip behind ``SyllableIndex.search_phrases``): subsequence DTW of syllable sequences.

* bitwise against the contract: the local costs are taken from the library itself (``SyllableIndex.search`` over pieces of at most
  128 rows of one sequence with k = the piece's length gives every d[i][j]), the fp32 DP of tests/dtw_ref.py runs over them, and
  ``search_phrases`` must return exactly those costs, spans and that order;
* long sequences crossing many tiles, under every admissible cut of the database;
* against float64 within the derived bound of ``dtw_ref.cost_error_bound``;
* m = 1 against ``search``, a planted phrase, invariance under the split / chunk / packing hooks, batching, how the index was built
  and stale workspace contents, group exclusion, short lists, NaN and zero rows, explicit sequences, the refusals, and end to end
  from ``Segmenter`` outputs."""
import numpy as np
import pytest
import torch

import dtw_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INF = np.float32(np.inf)


def _np(t):
    return t.cpu().numpy()


def _local_costs(x, offsets, rows, metric):
    """d [R, N] fp32 of the phrase rows against every database row, from ``search`` on pieces of one sequence (<= 128 rows)"""
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


def _reference(x, offsets, phrases, metric, k, phrase_groups=None, seq_groups=None):
    rows = np.concatenate(phrases)
    d = _local_costs(x, offsets, rows, metric)
    r0 = np.concatenate([[0], np.cumsum([len(p) for p in phrases])])
    return R.search_phrases(lambda p, s: d[r0[p]:r0[p + 1], offsets[s]:offsets[s + 1]], len(phrases), offsets, k, np.float32,
                            phrase_groups, seq_groups)


def _assert_same(got, ref):
    c, q, sp = (_np(t) for t in got)
    assert np.array_equal(q, ref[1])
    assert np.array_equal(c.view(np.uint32), ref[0].astype(np.float32).view(np.uint32))
    assert np.array_equal(sp, ref[2])


def _groups_of(offsets):
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets)).astype(np.int32)


SEQ_LENS = [128, 1, 127, 5, 123, 128, 2, 60, 66, 100, 28, 128, 37, 1, 1, 90, 126, 3, 64, 64, 128, 128, 17, 111]


def _corpus(D, integer, seed):
    """sequences of 1 .. 128 rows whose boundaries fall inside and on 128-row tile edges; with ``integer`` small integer rows (exact
    ties in every sum), duplicated rows inside sequences and whole duplicated sequences"""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(SEQ_LENS)]).astype(np.int64)
    N = int(offsets[-1])
    x = rng.integers(-2, 3, (N, D)).astype(np.float32) if integer else rng.standard_normal((N, D)).astype(np.float32)
    x[offsets[5]:offsets[6]] = x[offsets[0]:offsets[1]]       # sequence 5 = sequence 0; 20 and 21 = 11
    x[offsets[20]:offsets[21]] = x[offsets[11]:offsets[12]]
    x[offsets[21]:offsets[22]] = x[offsets[11]:offsets[12]]
    x[offsets[9] + 10:offsets[9] + 20] = x[offsets[9] + 9]    # a run of equal rows
    phrases = []
    for m in (1, 2, 7, 63, 64):
        a = int(rng.integers(0, N - m))
        p = x[a:a + m].copy()
        if not integer:
            p += 0.3 * rng.standard_normal(p.shape).astype(np.float32)
        phrases.append(p)
    phrases.append(x[offsets[11] + 3:offsets[11] + 10].copy())  # exact copies: equal costs in sequences 11, 20, 21
    phrases.append(np.repeat(x[offsets[9] + 9][None], 5, 0))
    return x, offsets, phrases


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,integer", [(16, True), (16, False), (768, False), (768, True)])
def test_bitwise_against_the_contract(D, integer, metric):
    from sylber_amd import SyllableIndex
    x, offsets, phrases = _corpus(D, integer, D + integer)
    S = len(offsets) - 1
    idx = SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)
    assert np.array_equal(idx.sequence_offsets(), offsets)
    got = idx.search_phrases(phrases, S)
    ref128 = _reference(x, offsets, phrases, metric, 128)
    ref = [r[:, :S] for r in ref128]
    assert (ref[1] >= 0).all()                               # every sequence is returned for every phrase: nothing is left out
    _assert_same(got, ref)
    _assert_same(idx.search_phrases(phrases, 128), ref128)   # the largest k: lists end in (+inf, -1, (-1, -1))
    # one [sum m, D] array with lengths= is the same call
    got2 = idx.search_phrases(np.concatenate(phrases), S, lengths=[len(p) for p in phrases])
    for a, b in zip(got, got2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("D,metric", [(16, "l2"), (768, "cosine")])
def test_long_sequences_under_every_cut(D, metric):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(D)
    lens = [3000, 70, 1500, 128, 2049, 1, 700]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N, S = int(offsets[-1]), len(lens)
    x = rng.standard_normal((N, D)).astype(np.float32)
    phrases = []
    for m, a in ((1, 5), (7, 2990), (64, 4000), (33, 7000), (12, 3060)):
        p = x[a:a + m] + 0.2 * rng.standard_normal((m, D)).astype(np.float32)
        phrases.append(np.delete(p, m // 2, 0) if m > 2 else p)
    idx = SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)
    ref = _reference(x, offsets, phrases, metric, S)
    for splits in (0, 1, 2, 3, 4, 5, 6, S, N):                # N: a cut at every sequence start
        _assert_same(idx.search_phrases(phrases, S, splits=splits), ref)


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_against_float64_within_the_derived_bound(metric):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(11)
    D = 768
    lens = rng.integers(5, 200, 40)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N, S, k = int(offsets[-1]), len(lens), 10
    x = rng.standard_normal((N, D)).astype(np.float32)
    phrases = []
    for m in (1, 3, 8, 20, 64):
        a = int(rng.integers(0, N - m))
        phrases.append((x[a:a + m] + 0.5 * rng.standard_normal((m, D))).astype(np.float32))
    idx = SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)
    c, q, sp = (_np(t) for t in idx.search_phrases(phrases, k))
    xs = _np(idx.features).astype(np.float64)                # the rows as the index holds them (unit rows for cosine)
    for p, ph in enumerate(phrases):
        qs = _np(idx._prep(torch.from_numpy(ph))).astype(np.float64)
        c64 = np.empty(S)
        bound = np.empty(S)
        for s in range(S):
            xr = xs[offsets[s]:offsets[s + 1]]
            c64[s] = R.dtw(R.local_costs(qs, xr, metric), np.float64)[0]
            bound[s] = R.cost_error_bound(qs, xr, c64[s], metric)
        assert (q[p] >= 0).all() and len(set(q[p].tolist())) == k
        err = np.abs(c[p].astype(np.float64) - c64[q[p]])
        print("float64 check", metric, "m", len(ph), "max err / bound", float((err / bound[q[p]]).max()))
        assert (err <= bound[q[p]]).all()
        out = np.setdiff1d(np.arange(S), q[p])
        assert (c64[out] >= c64[q[p, -1]] - (bound[out] + bound[q[p, -1]])).all()
        assert (np.diff(c[p]) >= 0).all()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_one_row_phrases_are_search(metric):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3000, 32)).astype(np.float32)
    grp = np.sort(rng.integers(0, 90, 3000)).astype(np.int32)
    idx = SyllableIndex(x, metric=metric, groups=grp, device=DEV)
    q = rng.standard_normal((150, 32)).astype(np.float32)
    c, s, sp = idx.search_phrases(q, 3, lengths=[1] * 150)
    sc, ids = idx.search(q, 1)
    assert torch.equal(sp[:, 0, 0], ids[:, 0]) and torch.equal(sp[:, 0, 1], ids[:, 0] + 1)
    want = sc[:, 0] if metric == "l2" else torch.clamp(1.0 - sc[:, 0], min=0.0)
    assert torch.equal(c[:, 0], want)
    off = idx.sequence_offsets()
    assert np.array_equal(_np(s[:, 0]), np.searchsorted(off, _np(ids[:, 0]), side="right") - 1)


def test_planted_phrase_ranks_its_clip_first():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(4)
    D = 768
    lens = rng.integers(20, 61, 300)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = rng.standard_normal((int(offsets[-1]), D)).astype(np.float32)
    idx = SyllableIndex(x, metric="cosine", groups=_groups_of(offsets), device=DEV)
    for clip, a0, m in ((17, 3, 8), (250, 10, 12), (0, 0, 6)):
        a = int(offsets[clip]) + a0
        p = x[a:a + m] + 0.3 * rng.standard_normal((m, D)).astype(np.float32)
        p = np.insert(np.delete(p, m - 2, 0), 2, p[2], 0)     # one syllable dropped, one duplicated
        c, s, sp = (_np(t) for t in idx.search_phrases([p], 5))
        assert s[0, 0] == clip and sp[0, 0, 0] < a + m and sp[0, 0, 1] > a
        assert offsets[clip] <= sp[0, 0, 0] < sp[0, 0, 1] <= offsets[clip + 1]


def test_invariance_is_bitwise():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(8)
    D = 64
    lens = rng.integers(1, 300, 60)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N, grp = int(offsets[-1]), _groups_of(offsets)
    x = np.round(rng.standard_normal((N, D)) * 2).astype(np.float32) / 2
    phrases = [x[a:a + m] + np.float32(0.5) * rng.integers(-1, 2, (m, D)).astype(np.float32)
               for m, a in zip(rng.integers(1, 65, 70), rng.integers(0, N - 64, 70))]
    idx = SyllableIndex(x, metric="l2", groups=grp, device=DEV)
    k = 12
    base = idx.search_phrases(phrases, k)
    for kw in ({"splits": 1}, {"splits": 3}, {"splits": 17}, {"splits": N}, {"phrase_chunk": 1}, {"phrase_chunk": 7}, {"phrase_chunk": 69},
               {"block_phrases": 1}, {"block_phrases": 2}, {"block_phrases": 5, "splits": 4, "phrase_chunk": 33},
               {"_workspace_fill": 0xFF}, {"_workspace_fill": 0xFF, "splits": 9}):
        got = idx.search_phrases(phrases, k, **kw)
        for a, b in zip(base, got):
            assert torch.equal(a, b), kw
    for p in (0, 13, 69):                                     # alone against in a batch of others
        got = idx.search_phrases([phrases[p]], k)
        for a, b in zip(base, got):
            assert torch.equal(a[p:p + 1], b)
    many = SyllableIndex(metric="l2", device=DEV)             # one add against many
    for s in range(len(lens)):
        many.add(x[offsets[s]:offsets[s + 1]], groups=grp[offsets[s]:offsets[s + 1]])
    for a, b in zip(base, many.search_phrases(phrases, k)):
        assert torch.equal(a, b)
    ref = _reference(x, offsets, phrases[:6], "l2", k)
    _assert_same([t[:6] for t in base], ref)


def test_exclusion_short_lists_nan_and_zero_rows_and_explicit_sequences():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(9)
    D = 16
    lens = [5, 9, 130, 4, 7, 3]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(offsets[-1])
    x = rng.standard_normal((N, D)).astype(np.float32)
    x[offsets[1] + 4] = np.nan                                # a NaN row inside sequence 1
    x[offsets[4]:offsets[5]] = np.nan                         # sequence 4 is NaN throughout: never returned
    x[offsets[2] + 100] = 0.0                                 # a zero row: similarity 0, d = 1 under cosine
    grp = np.array([0] * 5 + [1] * 9 + [0] * 130 + [2] * 4 + [3] * 7 + [1] * 3, np.int32)     # groups 0 and 1 occur twice: separate sequences
    phrases = [rng.standard_normal((m, D)).astype(np.float32) for m in (3, 1, 10, 2)]
    phrases[3][1] = np.nan                                    # a NaN phrase row: no result
    phrases.append(np.zeros((2, D), np.float32))
    pgrp = np.array([0, 1, 2, 0, 3], np.int32)
    for metric in ("l2", "cosine"):
        idx = SyllableIndex(x, metric=metric, groups=grp, device=DEV)
        assert np.array_equal(idx.sequence_offsets(), offsets)
        sgrp = grp[offsets[:-1]]
        k = 8                                                 # more than the 6 sequences
        ref = _reference(x, offsets, phrases, metric, k)
        got = idx.search_phrases(phrases, k)
        _assert_same(got, ref)
        c, q, sp = (_np(t) for t in got)
        if metric == "l2":
            assert (q[3] == -1).all() and np.isinf(c[3]).all() and (sp[3] == -1).all()
            assert 4 not in q and (q[0, 5:] == -1).all() and (q[0, :5] >= 0).all()
        else:                                                 # the unit-row step stores a row with a NaN as a zero row (as for ``search``): d = 1
            assert (q[:, 6:] == -1).all() and (q[:, :6] >= 0).all() and np.isfinite(c[:, :6]).all()
        if metric == "cosine":
            assert (c[4][q[4] >= 0] == 2.0).all()             # a zero phrase row costs 1 per cell: two rows, diagonal or vertical
        ref = _reference(x, offsets, phrases, metric, k, pgrp, sgrp)
        got = idx.search_phrases(phrases, k, groups=pgrp, exclude_same_group=True)
        _assert_same(got, ref)
        q = _np(got[1])
        assert not np.isin(q[0], [0, 2]).any() and not np.isin(q[1], [1, 5]).any() and not np.isin(q[2], [3]).any()
        # explicit sequences: cut the long one, join the short ones
        seqs = np.array([0, 14, 80, 144, N], np.int64)
        ref = _reference(x, seqs, phrases, metric, 3, pgrp, grp[seqs[:-1]])
        _assert_same(idx.search_phrases(phrases, 3, sequences=seqs, groups=pgrp, exclude_same_group=True), ref)
        _assert_same(idx.search_phrases(phrases, 3, sequences=torch.from_numpy(seqs)), _reference(x, seqs, phrases, metric, 3))


def test_every_refusal_comes_before_a_launch(monkeypatch):
    from sylber_amd import SyllableIndex, _lib
    rng = np.random.default_rng(10)
    x = rng.standard_normal((40, 16)).astype(np.float32)
    idx = SyllableIndex(x, groups=np.repeat(np.arange(4), 10), device=DEV)
    lib = _lib.load()
    launched = []
    real = lib.sylber_dtw_search

    class Spy:
        def __call__(self, *a):
            launched.append(1)
            return real(*a)
    monkeypatch.setattr(_lib, "_LIB", type("L", (), {"__getattr__": lambda self, n: Spy() if n == "sylber_dtw_search" else getattr(lib, n)})())
    p = [x[:3]]
    bad = [dict(phrases=p, k=0), dict(phrases=p, k=129), dict(phrases=p, k=1.5), dict(phrases=[x[:0]], k=1), dict(phrases=[np.zeros((65, 16), np.float32)], k=1),
           dict(phrases=[np.zeros((3, 32), np.float32)], k=1), dict(phrases=p, k=1, exclude_same_group=True),
           dict(phrases=p, k=1, groups=[0, 1], exclude_same_group=True), dict(phrases=x[:5], k=1), dict(phrases=x[:5], k=1, lengths=[2, 2]),
           dict(phrases=x[:5], k=1, lengths=[5, 0]), dict(phrases=x[:5], k=1, lengths=[[5]]), dict(phrases=x[:5], k=1, lengths=[2.5, 2.5]),
           dict(phrases=p, k=1, sequences=[0, 10, 10, 40]), dict(phrases=p, k=1, sequences=[1, 40]), dict(phrases=p, k=1, sequences=[0, 30]),
           dict(phrases=p, k=1, sequences=[0, 25, 20, 40]), dict(phrases=p, k=1, sequences=[40]), dict(phrases=p, k=1, splits=-1),
           dict(phrases=p, k=1, phrase_chunk=0)]
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(ValueError):
            idx.search_phrases(kw.pop("phrases"), kw.pop("k"), **kw)
    with pytest.raises(ValueError):
        SyllableIndex(device=DEV).search_phrases(p, 1)
    big = SyllableIndex(np.zeros((65537, 16), np.float32), device=DEV)
    with pytest.raises(ValueError, match="sequences="):
        big.search_phrases(p, 1)
    assert not launched
    c, s, sp = big.search_phrases(p, 1, sequences=[0, 65536, 65537])
    assert launched and s.shape == (1, 1)
    launched.clear()
    c, s, sp = idx.search_phrases([], 4)
    assert c.shape == (0, 4) and s.shape == (0, 4) and sp.shape == (0, 4, 2) and not launched
    assert c.dtype == torch.float32 and s.dtype == torch.int64 and sp.dtype == torch.int64 and c.device.type == "cuda"


def test_segmenter_outputs_end_to_end():
    from sylber_amd import Segmenter, SyllableIndex
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_state_dict
    seg = Segmenter(model_ckpt=synthetic_state_dict(0), device=DEV)
    wavs = [syllable_wave(int(m), s) for s, m in enumerate([32000, 24000, 40000, 28000], start=70)]
    outs = seg(wav=wavs, in_second=False)
    counts = [len(o["segments"]) for o in outs]
    assert sum(c > 0 for c in counts) >= 3, counts
    for metric in ("l2", "cosine"):
        idx = SyllableIndex.from_outputs(outs, metric=metric)
        off = idx.sequence_offsets()
        nonempty = [ci for ci, c in enumerate(counts) if c]
        assert np.array_equal(np.diff(off), [counts[ci] for ci in nonempty])
        si = int(np.argmax(np.diff(off)))
        ci, L = nonempty[si], int(off[si + 1] - off[si])
        a, m = (1, L - 2) if L >= 4 else (0, L)
        phrase = np.asarray(outs[ci]["segment_features"])[a:a + m]
        c, s, sp = (_np(t) for t in idx.search_phrases([phrase], 3, groups=[ci], exclude_same_group=False))
        assert s[0, 0] == si and sp[0, 0].tolist() == [off[si] + a, off[si] + a + m]
        assert c[0, 0] <= 1e-3 * max(1.0, float((phrase.astype(np.float64) ** 2).sum()))       # rounding residue, not == 0
        prov = idx.provenance(sp[0, 0])
        assert prov[0][0] == ci and prov[0][1] == a
        assert idx.provenance([sp[0, 0, 1] - 1])[0][:2] == (ci, a + m - 1)

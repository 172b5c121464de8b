"""GPU tier of the unit search (sylber_amd.UnitIndex, csrc/unit_search.hip) against tests/unit_search_ref.py: costs, sequences and
spans equal bit for bit -- the costs are small integers, no tolerance is involved.  Shapes are the smallest at which the kernel
can go wrong: phrases of 1, 2, 63 and 64 units, full and ragged waves and blocks, sequences around the column tile, a sequence
start on a tile's first and last column, one sequence of 65 536 units, widths that fill their padded row and widths that do not,
alphabets of 2 (ties everywhere) and 20 000 symbols, lists that overflow k and lists that end in padding."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unit_search_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

from sylber_amd import UnitIndex  # noqa: E402
from sylber_amd.units import TILE_COLS  # noqa: E402

T = TILE_COLS


def _np(out):
    return tuple(o.cpu().numpy() for o in out)


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def _index(corpus, off):
    """an index whose default sequences are ``off``: one group per sequence"""
    g = np.repeat(np.arange(len(off) - 1), np.diff(off)).astype(np.int32)
    return UnitIndex(corpus, groups=g), g


def _check(idx, corpus, off, phrases, k, rows=None, **kw):
    """both searches on the GPU equal the reference; returns the reference's (phrases, occurrences) with their counts"""
    if rows is None:
        corpus2 = ref.as_units(corpus)
        rows = ref.last_rows(phrases, [corpus2[off[s]:off[s + 1]] for s in range(len(off) - 1)])
    rkw = {a: b for a, b in kw.items() if a == "max_cost"}
    want_p = ref.search_phrases(corpus, off, phrases, k, rows=rows, **rkw)
    want_o = ref.search_occurrences(corpus, off, phrases, k, rows=rows, **rkw)
    got_p, got_o = _np(idx.search_phrases(phrases, k, **kw)), _np(idx.search_occurrences(phrases, k, **kw))
    assert _same(got_p, want_p[:3])
    assert _same(got_o, want_o[:3])
    return want_p, want_o


def _corrupt(rng, piece, A):
    """a copy of a corpus substring with one substitution (two units or more) and one deletion (four or more)"""
    p = np.array(piece, copy=True)
    if len(p) < 2:
        return p
    p[rng.integers(len(p))] = rng.integers(0, A, p.shape[1:])
    return np.delete(p, rng.integers(len(p)), 0) if len(p) > 3 else p


# ---- sequence lengths against the tile, phrase lengths and packing -------------------------------------------------------------------
# sequence starts at rows 0 and T (a tile's first column) and at 2 T - 1 (its last); lengths 1, 2, T - 1, T, T + 1, 3 T + 5
TILE_LENGTHS = [T, T - 1, 1, 2, T - 1, T + 1, 3 * T + 5, 1, 40]


@pytest.fixture(scope="module")
def tiles():
    rng = np.random.default_rng(10)
    off = np.concatenate([[0], np.cumsum(TILE_LENGTHS)])
    assert off[1] % T == 0 and off[2] % T == T - 1
    corpus = rng.integers(0, 2, int(off[-1]))              # two symbols: ties everywhere
    return corpus, off, _index(corpus, off)[0]


@pytest.mark.parametrize("lens", [[1, 2, 63, 64, 5, 17, 64], [1] * 70, [64] * 5, [2] * 33 + [63]],
                         ids=["mixed", "one-unit-waves", "full-blocks", "pairs"])
def test_phrase_lengths_and_packing_against_the_tile(tiles, lens):
    corpus, off, idx = tiles
    rng = np.random.default_rng(len(lens))
    phrases = [rng.integers(0, 2, m) for m in lens]        # includes m > L against the sequences of 1 and 2 units
    want_p, want_o = _check(idx, corpus, off, phrases, 10, splits=1)
    assert want_p[3].min() >= 1 and want_o[3].max() > 10   # more occurrences than k


def test_one_sequence_of_65536_units():
    rng = np.random.default_rng(11)
    corpus = rng.integers(0, 3, 65536)
    p = rng.integers(0, 3, 7)
    E, ST = ref.last_row_scan(p, corpus)
    idx = UnitIndex(corpus)
    want_p, want_o = _check(idx, corpus, np.array([0, 65536]), [p], 10, rows=(E[None, None], ST[None, None]), max_cost=1)
    assert want_o[3][0] > 10 and want_p[2][0, 0, 1] <= 65536
    with pytest.raises(ValueError, match="65537"):
        UnitIndex(np.zeros(65537, np.int64)).search_phrases([p], 1)


# ---- widths and alphabets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, A", [(1, 20000), (2, 2), (2, 20000), (3, 2), (8, 2), (8, 20000)])
def test_widths_and_alphabets(W, A):
    rng = np.random.default_rng(100 * W + A % 7)
    lens = rng.integers(20, 61, 14)
    off = np.concatenate([[0], np.cumsum(lens)])
    corpus = rng.integers(0, A, (int(off[-1]), W))
    if W == 1:
        corpus = corpus[:, 0]
    phrases = []
    for m in (1, 2, 5, 9, 16, 33, 64, 3, 7):
        a = int(rng.integers(0, len(corpus) - m))
        phrases.append(_corrupt(rng, ref.as_units(corpus)[a:a + m], A) if W > 1 else _corrupt(rng, corpus[a:a + m], A))
    idx, _ = _index(corpus, off)
    assert idx.width == W and idx.nbytes == len(corpus) * (4 * W + 4) and idx.units.dtype == torch.int32
    want_p, want_o = _check(idx, corpus, off, phrases, 10)
    assert want_p[3].min() >= 1                            # every phrase finds the substring it was cut from
    if A > 2:
        assert (want_p[0] == ref.PAD).any()                # ... and with 20 000 symbols little else: the lists end in padding


# ---- k ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many():
    """200 short sequences over two symbols: far more admissible sequences and occurrences than any k"""
    rng = np.random.default_rng(12)
    lens = rng.integers(3, 11, 200)
    off = np.concatenate([[0], np.cumsum(lens)])
    corpus = rng.integers(0, 2, (int(off[-1]), 2))
    phrases = [rng.integers(0, 2, (m, 2)) for m in rng.integers(1, 7, 40)]          # k = 128 packs 32 phrases per block: two blocks
    seqs = [corpus[off[s]:off[s + 1]] for s in range(200)]
    idx, g = _index(corpus, off)
    return corpus, off, phrases, idx, g, ref.last_rows(phrases, seqs)


@pytest.mark.parametrize("k", [1, 10, 128])
def test_k_overflows_and_pads(many, k):
    corpus, off, phrases, idx, g, rows = many
    want_p, want_o = _check(idx, corpus, off, phrases, k, rows=rows)
    assert want_p[3].max() > 128 and want_o[3].max() > 128
    want_p, want_o = _check(idx, corpus, off, phrases, k, rows=rows, max_cost=0)     # exact matches only
    if k == 128:
        assert (want_p[0] == ref.PAD).any() and (want_o[0] == ref.PAD).any() and (want_p[0] == 0).any()


# ---- invariance -------------------------------------------------------------------------------------------------------------------
def test_nothing_depends_on_splits_chunks_workspace_or_adds(many):
    corpus, off, phrases, idx, g, rows = many
    base = [_np(idx.search_phrases(phrases, 10)), _np(idx.search_occurrences(phrases, 10))]
    assert _same(base[0], ref.search_phrases(corpus, off, phrases, 10, rows=rows)[:3])
    runs = [dict(splits=1), dict(splits=2), dict(splits=7), dict(phrase_chunk=1), dict(phrase_chunk=3), dict(_workspace_fill=0xA5),
            dict(splits=7, phrase_chunk=3, _workspace_fill=0xFF)]
    for kw in runs:
        assert _same(_np(idx.search_phrases(phrases, 10, **kw)), base[0]), kw
        assert _same(_np(idx.search_occurrences(phrases, 10, **kw)), base[1]), kw
    parts = UnitIndex(width=2)
    for a in range(0, 200, 37):                            # many adds against one
        lo, hi = off[a], off[min(a + 37, 200)]
        assert parts.add(torch.from_numpy(corpus[lo:hi]), groups=g[lo:hi]) == range(lo, hi)
    assert np.array_equal(parts.sequence_offsets(), off)
    assert _same(_np(parts.search_phrases(phrases, 10)), base[0]) and _same(_np(parts.search_occurrences(phrases, 10)), base[1])
    # packed phrases with lengths= are the list
    packed, lens = np.concatenate(phrases), [len(p) for p in phrases]
    assert _same(_np(idx.search_phrases(packed, 10, lengths=lens)), base[0])


# ---- filters ----------------------------------------------------------------------------------------------------------------------
def test_groups_max_cost_and_explicit_sequences(many):
    corpus, off, phrases, idx, g, rows = many
    P = len(phrases)
    pg = np.arange(P) % 5                                  # phrase p may not match the sequences of group p % 5
    sg = np.arange(200) % 5
    gidx = UnitIndex(corpus, groups=np.repeat(sg, np.diff(off)).astype(np.int32))
    for fn, name in ((ref.search_phrases, "search_phrases"), (ref.search_occurrences, "search_occurrences")):
        want = fn(corpus, off, phrases, 10, rows=rows, phrase_groups=pg, seq_groups=sg)
        got = _np(getattr(gidx, name)(phrases, 10, groups=pg, exclude_same_group=True, sequences=off))
        assert _same(got, want[:3])
        assert not np.any(sg[got[1]][got[1] >= 0] == np.broadcast_to(pg[:, None], got[1].shape)[got[1] >= 0])
    mc = np.arange(P) % 4
    _check(idx, corpus, off, phrases, 10, rows=rows, max_cost=mc)
    _check(idx, corpus, off, phrases, 10, rows=rows, max_cost=torch.from_numpy(mc))
    _check(idx, corpus, off, phrases, 10, rows=rows, max_cost=2)
    # explicit sequences: the same rows cut elsewhere
    off2 = np.arange(0, len(corpus) + 1, 1)[::9]
    off2 = np.concatenate([off2[off2 < len(corpus)], [len(corpus)]])
    _check(idx, corpus, off2, phrases[:8], 10, sequences=off2)


# ---- occurrences ------------------------------------------------------------------------------------------------------------------
def test_a_keyword_planted_five_times_and_the_chain():
    rng = np.random.default_rng(13)
    word = rng.integers(0, 20000, (6, 2))
    corpus = rng.integers(0, 20000, (900, 2))
    off = np.array([0, 200, 700, 900])
    at = [210, 300, 387, 509, 690]                         # five times in sequence 1, once across the edge of a tile (row 512)
    for a in at:
        corpus[a:a + 6] = word
    idx, _ = _index(corpus, off)
    c, s, sp = _np(idx.search_occurrences([word], 8, max_cost=0))
    assert c[0].tolist() == [0] * 5 + [ref.PAD] * 3 and s[0].tolist() == [1] * 5 + [-1] * 3
    assert sp[0, :5].tolist() == [[a, a + 6] for a in at]
    c, s, sp = _np(idx.search_phrases([word], 8, max_cost=0))
    assert c[0].tolist() == [0] + [ref.PAD] * 7 and sp[0, 0].tolist() == [210, 216]
    _check(idx, corpus, off, [word], 8)
    # A - B - C: A and C disjoint, both overlapping B, costs 3 > 2 > 1: only C is emitted
    p, t = [1, 0, 0, 1], [2, 2, 1, 2, 2, 1, 0, 0, 2, 1]
    E, ST = ref.last_row_loop(p, t)
    assert ref.families(E, ST, 3) == [(3, 0, 2), (2, 2, 5), (1, 5, 7)]
    c, s, sp = _np(UnitIndex(t).search_occurrences([p], 4))
    assert c[0].tolist() == [1] + [ref.PAD] * 3 and sp[0, 0].tolist() == [5, 8] and s[0, 0] == 0


# ---- round trips ------------------------------------------------------------------------------------------------------------------
def test_from_tokens_provenance_and_save_load(tmp_path):
    rng = np.random.default_rng(14)
    toks = []
    for n in (12, 0, 30, 7):
        ends = np.cumsum(rng.integers(2, 9, n))
        toks.append({"units": rng.integers(0, 50, (n, 2)), "segments": np.stack([ends - 2, ends], 1).reshape(-1, 2).astype(np.int64),
                     "frames": int(ends[-1]) if n else 1})
    idx = UnitIndex.from_tokens(toks)
    assert len(idx) == 49 and idx.width == 2 and np.array_equal(idx.sequence_offsets(), [0, 12, 42, 49])
    word = toks[2]["units"][10:14]
    c, s, sp = _np(idx.search_phrases([word], 2))
    assert c[0, 0] == 0 and s[0, 0] == 1 and sp[0, 0].tolist() == [22, 26]
    prov = idx.provenance(range(*sp[0, 0]))
    assert prov == [(2, 10 + i, int(toks[2]["segments"][10 + i, 0]), int(toks[2]["segments"][10 + i, 1])) for i in range(4)]
    assert idx.provenance([-1, 49]) == [None, None]
    path = str(tmp_path / "units.npz")
    idx.save(path)
    back = UnitIndex.load(path)
    phrases = [rng.integers(0, 50, (m, 2)) for m in (1, 3, 5)] + [word]
    for name in ("search_phrases", "search_occurrences"):
        assert _same(_np(getattr(back, name)(phrases, 5)), _np(getattr(idx, name)(phrases, 5)))
    assert back.provenance(range(*sp[0, 0])) == prov and len(back) == 49 and back.nbytes == idx.nbytes
    np.savez(str(tmp_path / "other.npz"), units=np.zeros((3, 1), np.int32))
    with pytest.raises(ValueError, match="not a saved UnitIndex"):
        UnitIndex.load(str(tmp_path / "other.npz"))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    idx = UnitIndex(np.arange(20) % 3)
    one = [np.array([1, 2])]
    with pytest.raises(ValueError, match="-1"):
        UnitIndex(np.array([3, -1, 2]))
    with pytest.raises(ValueError, match=str(2 ** 31)):
        idx.add(np.array([2 ** 31]))
    with pytest.raises(ValueError, match="integers"):
        idx.add(np.array([1.5]))
    with pytest.raises(ValueError, match="expected W = 1, got 2"):
        idx.add(np.zeros((4, 2), np.int64))
    with pytest.raises(ValueError, match="expected W = 1, got 2"):
        idx.search_phrases([np.zeros((2, 2), np.int64)], 1)
    with pytest.raises(ValueError, match=r"\[1, 8\], got 9"):
        UnitIndex(np.zeros((4, 9), np.int64))
    with pytest.raises(ValueError, match="from 65 to 65"):
        idx.search_phrases([np.zeros(65, np.int64)], 1)
    with pytest.raises(ValueError, match="129"):
        idx.search_occurrences(one, 129)
    with pytest.raises(ValueError, match="from 0 to 2"):
        idx.search_phrases([np.zeros(0, np.int64), np.array([1, 2])], 1)
    with pytest.raises(ValueError, match="lengths sum to 3"):
        idx.search_phrases(np.array([1, 2]), 1, lengths=[3])
    with pytest.raises(ValueError, match="need lengths"):
        idx.search_phrases(np.array([1, 2]), 1)
    with pytest.raises(ValueError, match="max_cost must be >= 0, got -1"):
        idx.search_phrases(one, 1, max_cost=-1)
    with pytest.raises(ValueError, match="max_cost"):
        idx.search_phrases(one, 1, max_cost=[1, 2])
    with pytest.raises(ValueError, match="exclude_same_group needs"):
        idx.search_phrases(one, 1, exclude_same_group=True)
    with pytest.raises(ValueError, match="empty"):
        UnitIndex(width=1).search_phrases(one, 1)
    assert len(idx) == 20                                  # nothing refused was stored
    c, s, sp = idx.search_phrases([], 3)
    assert c.shape == (0, 3) and c.dtype == torch.int32 and s.shape == (0, 3) and sp.shape == (0, 3, 2)

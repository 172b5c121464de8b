"""GPU tier, warping paths (csrc/dtw_align.hip behind ``SyllableIndex.align_phrases`` and the classes that delegate to it), bitwise
against tests/align_ref.py: the local costs are taken from the library itself (``SyllableIndex.search`` on pieces of at most 128
rows, as tests/test_gpu_phrase.py takes them), the fp32 window DP and the backtrack of align_ref run over them, and the call must
return exactly those rows, steps and cost bits.  On the spans of every phrase search the path must start and end where the span does
and carry the search's cost bits (the theorem of include/sylber_hip.h)."""
import functools

import numpy as np
import pytest
import torch

import align_ref as A
from test_gpu_dtwpq import _decoded_index
from test_gpu_phrase import _groups_of, _local_costs, _np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PIECES = np.array([0, 128, 256, 300], np.int64)             # how _local_costs cuts the 300 rows; no sequence enters an alignment
WIDTHS = (1, 31, 32, 33, 64, 65, 100, 3)                    # the chunk of 32 columns: below, on and above one edge and two; 3 < m = 7, 64


def _rows_and_phrases(D, integer, seed, N=300):
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, (N, D)).astype(np.float32) if integer else rng.standard_normal((N, D)).astype(np.float32)
    x[40:50] = x[39]                                          # a run of equal rows: ties along a row of the DP
    phrases = []
    for m in (1, 2, 7, 64):
        a = int(rng.integers(0, N - m))
        p = x[a:a + m].copy()
        if not integer:
            p += 0.3 * rng.standard_normal(p.shape).astype(np.float32)
        phrases.append(p)
    return x, phrases


def _windows(P, N, seed):
    rng = np.random.default_rng(seed)
    sp = np.empty((P, len(WIDTHS), 2), np.int64)
    for p in range(P):
        for r, w in enumerate(WIDTHS):
            a = int(rng.integers(0, N - w + 1))
            sp[p, r] = (a, a + w)
    sp[0, 0], sp[P - 1, len(WIDTHS) - 1] = (0, 1), (N - 3, N)  # the first and the last row of the index
    return sp


def _reference(x, phrases, spans, metric, pieces=PIECES):
    d = _local_costs(x, pieces, np.concatenate(phrases), metric)
    r0 = np.concatenate([[0], np.cumsum([len(p) for p in phrases])])
    return A.align_phrases(lambda p, a, b: d[r0[p]:r0[p + 1], a:b], [len(p) for p in phrases], _np(spans) if torch.is_tensor(spans) else spans)


def _assert_same(got, ref):
    rows, steps, costs = got
    assert rows.dtype == torch.int64 and steps.dtype == torch.int32 and costs.dtype == torch.float32 and rows.device.type == "cuda"
    assert np.array_equal(_np(rows), ref[0])
    assert np.array_equal(_np(steps), ref[1])
    assert np.array_equal(_np(costs).view(np.uint32), ref[2].astype(np.float32).view(np.uint32))


def _equal(a, b, what=None):
    for s, t in zip(a, b):
        assert torch.equal(s, t), what


def _is_padding(rows, steps, costs, mask):
    return bool((rows[mask] == -1).all() and (steps[mask] == 0).all() and torch.isposinf(costs[mask]).all())


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,integer", [(16, True), (16, False), (768, False)])
def test_bitwise_against_the_contract(D, integer, metric):
    from sylber_amd import SyllableIndex
    x, phrases = _rows_and_phrases(D, integer, D + integer)
    idx = SyllableIndex(x, metric=metric, device=DEV)
    spans = _windows(len(phrases), len(x), 5)
    ref = _reference(x, phrases, spans, metric)
    got = idx.align_phrases(phrases, spans)
    _assert_same(got, ref)
    rows, steps = _np(got[0]), _np(got[1])
    assert rows.shape == (4, len(WIDTHS), 64, 2) and (steps > 0).all()
    assert (rows[0, :, 1:] == -1).all() and (rows[2, :, 7:] == -1).all()         # i >= m_p
    assert steps[3, 0] == 64                                  # m = 64 on one column: nothing but vertical steps
    r = rows[2, 7, :7]                                        # m = 7 on 3 columns: lo[i+1] == hi[i] is a vertical step, at least m - W
    assert (r[1:, 0] == r[:-1, 1] - 1).sum() >= 7 - 3 and steps[2, 7] <= 7 + 3 - 1
    # one [sum m, D] array with lengths= is the same call; the start that the walk tracked is the one the codes lead back to
    again = idx.align_phrases(np.concatenate(phrases), spans, lengths=[len(p) for p in phrases], _tracked_start=True)
    _equal(got, again[:3])
    assert torch.equal(again[3], got[0][:, :, 0, 0])


def _searched_corpus(metric, integer):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(11 + integer)
    lens = [40, 7, 90, 1, 33, 65]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N, D = int(offsets[-1]), 16
    x = rng.integers(-2, 3, (N, D)).astype(np.float32) if integer else rng.standard_normal((N, D)).astype(np.float32)
    phrases = []
    for m in (1, 2, 7, 30):
        a = int(rng.integers(0, N - m))
        p = x[a:a + m].copy()
        phrases.append(np.delete(p, m // 2, 0) if m > 2 else p)           # a row left out: the match has to warp
    phrases.append(np.repeat(x[50][None], 4, 0))
    return x, offsets, phrases, SyllableIndex(x, metric=metric, groups=_groups_of(offsets), device=DEV)


@pytest.mark.parametrize("metric,integer", [("l2", True), ("cosine", False)])
def test_spans_from_each_search_start_end_and_cost(metric, integer):
    x, offsets, phrases, idx = _searched_corpus(metric, integer)
    lens = np.array([len(p) for p in phrases])
    k = 8                                                     # more than the 6 sequences: every list ends in padding
    seeds = idx.search(np.concatenate(phrases), 16)
    searches = {"search_phrases": idx.search_phrases(phrases, k), "search_phrases_refined": idx.search_phrases_refined(phrases, k, 2),
                "search_occurrences": idx.search_occurrences(phrases, k), "search_occurrences_refined": idx.search_occurrences_refined(phrases, k, 2),
                "search_phrases_seeded": idx.search_phrases_seeded(phrases, seeds[0], seeds[1], k, 2)}
    d = _local_costs(x, offsets, np.concatenate(phrases), metric)
    r0 = np.concatenate([[0], np.cumsum(lens)])
    for name, (costs, seqs, spans) in searches.items():
        rows, steps, acost, tracked = idx.align_phrases(phrases, spans, _tracked_start=True)
        assert torch.equal(tracked, rows[:, :, 0, 0]), name
        hit = seqs >= 0
        assert hit.any() and ((~hit).any() or "occurrences" in name), name      # 6 sequences: a list of one match per sequence ends in padding
        assert _is_padding(rows, steps, acost, ~hit), name                # padding in, padding out
        last = torch.from_numpy(lens - 1).to(DEV)[:, None, None, None].expand(-1, k, 1, 2)
        ends = rows.gather(2, last)[:, :, 0, 1]
        assert torch.equal(rows[:, :, 0, 0][hit], spans[:, :, 0][hit]), name      # the path starts where the span does
        assert torch.equal(ends[hit], spans[:, :, 1][hit]), name                  # and ends where it does
        assert torch.equal(acost.view(torch.int32), costs.view(torch.int32)), name       # with the search's cost, bit for bit
        assert (steps[hit] >= torch.from_numpy(lens).to(DEV)[:, None].expand(-1, k)[hit]).all(), name
        _assert_same((rows, steps, acost), A.align_phrases(lambda p, a, b: d[r0[p]:r0[p + 1], a:b], lens.tolist(), _np(spans)))


def test_non_finite_rows_and_windows_that_are_no_span():
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(4)
    N, D, m = 200, 16, 5
    x = rng.standard_normal((N, D)).astype(np.float32)
    phrase = rng.standard_normal((m, D)).astype(np.float32)
    x[100 + 6:100 + 6 + m] = phrase                           # planted in the middle of the window [100, 111)
    x[31] = np.nan                                            # a NaN row near the start of the window [30, 50) ...
    x[79] = np.nan                                            # ... and as the last row of the window [60, 80)
    x[150:153] = np.nan                                       # a window of nothing else
    spans = np.array([[[100, 111], [30, 50], [60, 80], [150, 153], [-1, -1], [25, 32]]], np.int64)
    idx = SyllableIndex(x, metric="l2", device=DEV)
    ref = _reference(x, [phrase], spans, "l2", np.array([0, 128, 200]))
    got = idx.align_phrases([phrase], spans, _tracked_start=True)
    assert torch.equal(got[3], got[0][:, :, 0, 0])
    got = got[:3]
    _assert_same(got, ref)
    rows, steps, costs = got
    assert rows[0, 0, 0].tolist() == [106, 107] and rows[0, 0, m - 1].tolist() == [110, 111] and int(steps[0, 0]) == m
    assert int(rows[0, 1, 0, 0]) > 31 and torch.isfinite(costs[0, 1])      # +inf cells: the path starts behind the NaN row
    pad = torch.tensor([[False, False, True, True, True, True]], device=DEV)
    assert _is_padding(rows, steps, costs, pad)               # (m-1, b-1) is +inf: padding, as for the padding span


def test_invariance_is_bitwise():
    from sylber_amd import SyllableIndex
    x, phrases = _rows_and_phrases(32, True, 8)
    spans = _windows(len(phrases), len(x), 9)
    spans[1, 2] = -1
    idx = SyllableIndex(x, metric="l2", device=DEV)
    base = idx.align_phrases(phrases, spans)
    for kw in ({"pair_chunk": 1}, {"pair_chunk": 5}, {"pair_chunk": 10 ** 6}):
        _equal(base, idx.align_phrases(phrases, spans, **kw), kw)
    _equal(base, idx.align_phrases(phrases, torch.from_numpy(spans)), "a host tensor")
    _equal(base, idx.align_phrases(phrases, torch.from_numpy(spans).to(DEV)), "a device tensor")
    for p in (0, 3):                                          # alone against in a batch of others: Mx differs, the rows do not
        alone = idx.align_phrases([phrases[p]], spans[p:p + 1])
        m = len(phrases[p])
        assert torch.equal(alone[0], base[0][p:p + 1, :, :m]) and torch.equal(alone[1], base[1][p:p + 1]) and torch.equal(alone[2], base[2][p:p + 1])
    many = SyllableIndex(metric="l2", device=DEV)             # one add against three
    for lo, hi in ((0, 90), (90, 91), (91, 300)):
        many.add(x[lo:hi])
    _equal(base, many.align_phrases(phrases, spans))


def test_save_load_round_trip(tmp_path):
    from sylber_amd import SyllableIndex
    x, phrases = _rows_and_phrases(16, False, 2)
    spans = _windows(len(phrases), len(x), 3)
    idx = SyllableIndex(x, metric="cosine", device=DEV)
    idx.save(str(tmp_path / "i.npz"))
    _equal(idx.align_phrases(phrases, spans), SyllableIndex.load(str(tmp_path / "i.npz"), device=DEV).align_phrases(phrases, spans))


def test_the_inverted_file_delegates():
    from sylber_amd import IVFSyllableIndex
    x, offsets, phrases, idx = _searched_corpus("l2", False)
    ivf = IVFSyllableIndex.build(idx, 4, seed=1)
    costs, seqs, spans = ivf.search_phrases(phrases, 3, nprobe=4, seeds=16)
    got = ivf.align_phrases(phrases, spans)
    _equal(got, idx.align_phrases(phrases, spans))
    assert torch.equal(got[2].view(torch.int32), costs.view(torch.int32)) and torch.equal(got[0][:, :, 0, 0], spans[:, :, 0])


def _compressed_corpus():
    """rows in sequences of 1, 33 and 65 rows around the 32-column chunk of csrc/dtw_pair.h, random codebooks (M = 2), four phrases"""
    rng = np.random.default_rng(6)
    lens = [40, 7, 90, 1, 33, 65, 20]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N, D, M = int(offsets[-1]), 32, 2
    x = rng.standard_normal((N, D)).astype(np.float32)
    books = rng.standard_normal((M, 256, D // M)).astype(np.float32)
    phrases = [x[a:a + m] + 0.1 * rng.standard_normal((m, D)).astype(np.float32) for m, a in ((1, 3), (4, 60), (9, 150), (30, 200))]
    return x, offsets, books, phrases


def test_the_compressed_index_with_and_without_its_rows():
    from sylber_amd import PQSyllableIndex, SyllableIndex
    x, offsets, books, phrases = _compressed_corpus()
    N, M = len(x), len(books)
    idx = SyllableIndex(x, metric="l2", groups=_groups_of(offsets), device=DEV)
    pq = PQSyllableIndex.build(idx, M, codebooks=books)
    k = 8
    exact = pq.search_phrases(phrases, 2, 4)                  # rerank=True: spans of the exact rows
    _equal(pq.align_phrases(phrases, exact[2]), idx.align_phrases(phrases, exact[2]))
    costs, seqs, spans = pq.search_phrases(phrases, k, 1, rerank=False)
    held = pq.align_phrases(phrases, spans, rerank=False)     # the decoded rows while the exact ones are still held
    pq.drop_rows()
    with pytest.raises(ValueError, match="rerank"):
        pq.align_phrases(phrases, spans, rerank=True)
    got = pq.align_phrases(phrases, spans, _tracked_start=True)
    assert torch.equal(got[3], got[0][:, :, 0, 0])
    got = got[:3]
    _equal(held, got, "drop_rows")
    hit = seqs >= 0
    assert hit.any() and (~hit).any() and _is_padding(*got, ~hit)
    assert torch.equal(got[2].view(torch.int32), costs.view(torch.int32))        # the costs of the search on the decoded rows
    assert torch.equal(got[0][:, :, 0, 0][hit], spans[:, :, 0][hit])
    xhat = _np(pq.decode(np.arange(N)))
    _assert_same(got, _reference(xhat, phrases, spans, "l2", offsets))
    for kw in ({"pair_chunk": 3}, {"pair_chunk": 1}):
        _equal(got, pq.align_phrases(phrases, spans, **kw), kw)


MASKED = 100                                                # a row inside the 90-row sequence, rows 47 .. 136
CODED_WINDOWS = ((90, 110), (80, MASKED + 1), (3, 4), (40, 55), (-1, -1), (MASKED, MASKED + 1), (137, 236))
#                 holds the masked row | ends on it | one row | crosses the sequence edges 40 and 47 | padding | the masked row alone |
#                 the sequences of 1, 33 and 65 rows: 99 columns, four chunks


@functools.lru_cache(maxsize=None)
def _coded_alignment():
    """the corpus with one masked row, the windows, and what ``SyllableIndex.align_phrases`` returns for them on the decoded rows with
    the masked row as a NaN row: the oracle of ``PQSyllableIndex.align_phrases(rerank=False)``, computed once"""
    from sylber_amd import PQSyllableIndex
    x, offsets, books, phrases = _compressed_corpus()
    x = x.copy()
    x[MASKED, 5] = np.nan
    grp = _groups_of(offsets)
    pq = PQSyllableIndex.build(x, len(books), codebooks=books, groups=grp, metric="l2", device=DEV)
    assert _np(pq._bad).nonzero()[0].tolist() == [MASKED]
    windows = np.array([CODED_WINDOWS] * len(phrases), np.int64)
    windows[1:, 2] = ((50, 51), (136, 137), (len(x) - 1, len(x)))   # other 1-row windows: inside, the last row of the 90, the last of all
    want = _decoded_index(pq, grp, nan_masked=True).align_phrases(phrases, windows, _tracked_start=True)
    return x, grp, books, phrases, windows, want


@pytest.mark.parametrize("dropped", [False, True])
def test_the_compressed_index_aligns_straight_from_its_codes(dropped):
    """``PQSyllableIndex.align_phrases(rerank=False)`` (``sylber_dtw_align_codes`` on plain codes: identity positions, no lists)
    against the fp32 alignment on the materialised rows, bit for bit, with the rows held and after ``drop_rows()``"""
    from sylber_amd import PQSyllableIndex
    x, grp, books, phrases, windows, want = _coded_alignment()
    pq = PQSyllableIndex.build(x, len(books), codebooks=books, groups=grp, metric="l2", device=DEV)
    if dropped:
        pq.drop_rows()
    got = pq.align_phrases(phrases, windows, rerank=False, _tracked_start=True)
    assert len(got) == 4
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
    _equal(got[:2] + got[3:], want[:2] + want[3:])
    assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32))
    rows, steps, costs, start = got
    assert torch.equal(start, rows[:, :, 0, 0])
    pad = torch.zeros(costs.shape, dtype=torch.bool, device=DEV)
    pad[:, [1, 4, 5]] = True                                  # a window that ends on the masked row has no path, nor has the padding
    assert _is_padding(rows, steps, costs, pad) and torch.isfinite(costs[~pad]).all() and (steps[~pad] > 0).all()
    assert (rows[:, 0, 0, 0] > MASKED).all()                  # the path starts behind the masked row
    assert int(steps[3, 2]) == 30                             # 30 phrase rows on one column
    for pair_chunk in (1, 3, None):
        _equal(got, pq.align_phrases(phrases, windows, pair_chunk=pair_chunk, rerank=False, _tracked_start=True), pair_chunk)


def test_every_refusal_comes_before_a_launch(monkeypatch):
    from sylber_amd import PQSyllableIndex, SyllableIndex, _lib
    rng = np.random.default_rng(10)
    x = rng.standard_normal((40, 16)).astype(np.float32)
    idx = SyllableIndex(x, groups=np.repeat(np.arange(4), 10), device=DEV)
    big = SyllableIndex(np.zeros((65600, 16), np.float32), device=DEV)
    pq = PQSyllableIndex.build(idx, 1, codebooks=rng.standard_normal((1, 256, 16)).astype(np.float32))
    pq.drop_rows()
    lib = _lib.load()

    def fail(*a):
        raise AssertionError("launched")
    entries = {"sylber_dtw_align", "sylber_dtw_align_codes"}
    monkeypatch.setattr(_lib, "_LIB", type("L", (), {"__getattr__": lambda self, n: fail if n in entries else getattr(lib, n)})())
    p = [x[:3]]
    ok = np.array([[[0, 5], [-1, -1]]], np.int64)
    bad = [dict(spans=[[[0, 41]]]), dict(spans=[[[-2, 5]]]), dict(spans=[[[-1, 5]]]), dict(spans=[[[5, 5]]]), dict(spans=[[[7, 3]]]),
           dict(spans=[[[3, -1]]]), dict(spans=[[[0, 5]], [[0, 5]]]), dict(spans=[[0, 5]]), dict(spans=np.zeros((1, 2, 3), np.int64)),
           dict(spans=ok.astype(np.int32)), dict(spans=ok.astype(np.float32)), dict(spans=torch.zeros((1, 1, 2), dtype=torch.int32, device=DEV)),
           dict(spans=ok, pair_chunk=0), dict(spans=ok, pair_chunk=1.5),
           dict(spans=ok, phrases=[x[:0]]), dict(spans=ok, phrases=[np.zeros((65, 16), np.float32)]), dict(spans=ok, phrases=[np.zeros((3, 32), np.float32)]),
           dict(spans=ok, phrases=x[:5]), dict(spans=ok, phrases=x[:5], lengths=[2, 2]), dict(spans=ok, phrases=x[:5], lengths=[5, 0]),
           dict(spans=ok, phrases=x[:5], lengths=[[5]]), dict(spans=ok, phrases=x[:5], lengths=[2.5, 2.5])]
    for call in (idx.align_phrases, pq.align_phrases):
        for kw in bad:
            kw = dict(kw)
            with pytest.raises(ValueError):
                call(kw.pop("phrases", p), kw.pop("spans"), **kw)
    with pytest.raises(TypeError):
        pq.align_phrases(p, ok, scratch_rows=0)             # there is no scratch to bound
    with pytest.raises(ValueError):
        SyllableIndex(device=DEV).align_phrases(p, ok)
    with pytest.raises(ValueError, match="65536"):
        big.align_phrases(p, [[[0, 65537]]])
    for P, k in ((0, 4), (1, 0)):                             # no pair: empty outputs without a launch
        rows, steps, costs = idx.align_phrases(p[:P], np.zeros((P, k, 2), np.int64))
        assert rows.shape == (P, k, 3 * P, 2) and steps.shape == (P, k) and costs.shape == (P, k)
        assert rows.dtype == torch.int64 and steps.dtype == torch.int32 and costs.dtype == torch.float32 and rows.device.type == "cuda"
    rows, steps, costs = idx.align_phrases(p, np.full((1, 2, 2), -1, np.int64))      # nothing but padding: no launch either
    assert _is_padding(rows, steps, costs, torch.ones((1, 2), dtype=torch.bool, device=DEV))
    monkeypatch.undo()
    rows, steps, costs = big.align_phrases(p, [[[64, 65600]]])               # the largest window, 65 536 rows, does launch
    assert int(steps[0, 0]) >= 3 and rows[0, 0, 2, 1] == 65600 and torch.isfinite(costs[0, 0])


def test_the_entry_refuses_bad_arguments_and_a_bad_window_comes_back_as_padding():
    """the C ABI by itself: status 1 with ``sylber_last_error`` for what the entry can see; the windows are device data, so a window
    that ``align_phrases`` would have refused is bounds-checked by the kernel before anything is read and reported as padding"""
    from sylber_amd import SyllableIndex, _lib
    from sylber_amd._index import _on_device, _phrase_blocks, _prep, _row_norms
    from sylber_amd.kmeans import _stream, _vp
    rng = np.random.default_rng(12)
    x = rng.standard_normal((40, 16)).astype(np.float32)
    idx = SyllableIndex(x, device=DEV)
    lib, dev = _lib.load(), idx.device
    b = _phrase_blocks(lib, dev, _prep(torch.from_numpy(x[:3]), "l2", dev), np.array([3], np.int64), 0, 1, np.array([0, 1], np.int64), 1, 0, 0, None)
    qn = _row_norms(b.qp)
    place_d, len_d = _on_device(b.place, np.int32, dev), _on_device(b.ln, np.int32, dev)
    # max_cols = 8: none | reversed | past the last row | before the first | too long | legal | empty | legal, but of phrase 1 of 1
    win = torch.tensor([[-1, -1], [5, 3], [33, 41], [-3, 4], [0, 9], [2, 10], [7, 7], [2, 10]], dtype=torch.int32, device=dev)
    pp = torch.tensor([0, 0, 0, 0, 0, 0, 0, 1], dtype=torch.int32, device=dev)
    n = int(win.shape[0])
    rows = torch.full((n, 3, 2), 7, dtype=torch.int32, device=dev)
    steps = torch.full((n,), 7, dtype=torch.int32, device=dev)
    costs = torch.zeros(n, dtype=torch.float32, device=dev)
    assert int(lib.sylber_dtw_align_workspace_bytes(n, 8)) == n * 16 * (8 + 63)
    for bad in ((0, 8), (n, 0), (n, 65537)):
        assert int(lib.sylber_dtw_align_workspace_bytes(*bad)) == -1
    ws = torch.empty(n * 16 * (8 + 63), dtype=torch.uint8, device=dev)
    good = dict(q=_vp(b.qp), nb=b.nb, qn=_vp(qn), place=_vp(place_d), len=_vp(len_d), P=1, x=_vp(idx._x), N=40, D=16, cn=_vp(idx._c), metric=0,
                pp=_vp(pp), win=_vp(win), n=n, max_cols=8, max_rows=3, rows=_vp(rows), steps=_vp(steps), costs=_vp(costs), start=None, ws=_vp(ws))
    with torch.cuda.device(dev):
        st = _stream(dev)
        for over in (dict(q=None), dict(x=None), dict(win=None), dict(ws=None), dict(nb=0), dict(P=0), dict(n=0), dict(N=0), dict(D=8), dict(metric=5),
                     dict(qn=None), dict(cn=None), dict(max_cols=0), dict(max_cols=65537), dict(max_rows=0), dict(max_rows=65)):
            assert lib.sylber_dtw_align(*dict(good, **over).values(), st) == 1, over
            assert lib.sylber_last_error().decode().startswith("sylber_dtw_align"), over
        assert (rows == 7).all() and (steps == 7).all()       # a refused call wrote nothing
        assert lib.sylber_dtw_align(*good.values(), st) == 0
    ok = torch.tensor([False, False, False, False, False, True, False, False], device=dev)
    assert (rows[~ok] == -1).all() and (steps[~ok] == 0).all() and torch.isposinf(costs[~ok]).all()
    want = idx.align_phrases([x[:3]], [[[2, 10]]])
    assert torch.equal(rows[5].to(torch.int64), want[0][0, 0]) and steps[5] == want[1][0, 0] and costs[5] == want[2][0, 0]

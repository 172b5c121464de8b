"""GPU tier, phrase search on the compressed inverted file (``IVFPQSyllableIndex.search_phrases`` / ``align_phrases``; csrc/dtw_codes.hip:
``sylber_dtw_rerank_codes``, ``sylber_dtw_align_codes``).

(1) kernel against kernel through the C ABI: both entries on a coded database equal ``sylber_dtw_rerank`` / ``sylber_dtw_align`` on the
    materialised plane, bit for bit;
(2) ``rerank=True`` is ``ix.index.search_phrases_seeded`` on ``ix.search``'s seeds, ``cand`` / ``bound`` the numpy vote on them;
(3) ``rerank=False``: under "l2" the ``SyllableIndex(ix.decode(...))`` identity; for "cosine" and masked rows the vote on the reported
    seeds followed by the fp32 kernel on the plane;
(4) bitwise invariance: ``drop_rows()``, ``save`` / ``load``, ``build`` against ``build`` + two ``add``s, the chunk hooks, a stale
    workspace;
(5) the planted phrases at the reference's settings; (6) ``align_phrases`` on the spans of (2) and (3); (7) exclusion;
(8) refusals and empty input."""
import functools

import numpy as np
import pytest
import torch

import ivfpq_phrase_ref as Q
import phrase_vote_ref as V

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K, REFINE, NPROBE, SEEDS = 3, 4, 3, 32


def _np(t):
    return t.cpu().numpy()


def _assert_equal(got, want, what=""):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        if a.dtype == torch.float32:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what
        else:
            assert torch.equal(a, b), what


def _lens_rows(phrases):
    lens = np.array([len(p) for p in phrases])
    return lens, np.cumsum(lens) - lens


# ---- (1) the C ABI: a coded database against its materialised plane -----------------------------------------------------------------
SEQ_LENS = (1, 2, 31, 32, 33, 64, 65, 72)                                   # 300 rows: the chunk of 32 from both sides
PHRASE_LENS = (1, 2, 63, 64, 5)


class _Coded:
    """a random coded database of 300 rows in a shuffled position order: one masked row, one row behind the lists (in no list), an
    empty list; ``plane`` is its materialisation in id order"""

    def __init__(self, D, M, residual, identity=False, seed=0):
        g = torch.Generator().manual_seed(seed + D + M)
        N, nlist, dsub = sum(SEQ_LENS), 5, D // M
        self.N, self.D, self.M, self.residual = N, D, M, residual
        self.cb = torch.randn((M, 256, dsub), generator=g).to(DEV)
        self.code = torch.randint(0, 256, (N, M), generator=g, dtype=torch.uint8).to(DEV)          # by position
        perm = torch.arange(N) if identity else torch.randperm(N, generator=g)
        self.pos = perm.to(torch.int32).to(DEV)                                                  # row id -> position
        bad = torch.zeros(N, dtype=torch.uint8)
        self.masked_id, self.unlisted_id = 40, 150                                                # in the sequences of 32 and of 64 rows
        bad[perm[self.masked_id]] = 1
        if residual and not identity:                                                            # the unlisted row lies behind the lists
            last = int(perm[self.unlisted_id])
            other = int((perm == N - 1).nonzero()[0, 0])
            perm[self.unlisted_id], perm[other] = N - 1, last
            self.pos = perm.to(torch.int32).to(DEV)
            bad = torch.zeros(N, dtype=torch.uint8)
            bad[perm[self.masked_id]] = 1
        self.bad = bad.to(DEV)
        listed = N - 1 if residual else N
        self.off = torch.tensor([0, 70, 70, 150, 220, listed], dtype=torch.int32, device=DEV)     # list 1 is empty
        self.cent = torch.randn((nlist, D), generator=g).to(DEV)
        codes_id = self.code[self.pos.long()].long()                                             # [N, M] in id order
        x = torch.cat([self.cb[m][codes_id[:, m]] for m in range(M)], 1)
        nan = self.bad[self.pos.long()] != 0
        if residual:
            lst = torch.bucketize(self.pos, self.off[1:], right=True)                            # the l with off[l] <= p < off[l + 1]
            nan |= lst >= nlist
            x = self.cent[lst.clamp(max=nlist - 1).long()] + x                                   # one fp32 addition per element
        self.plane = torch.where(nan[:, None], torch.full_like(x, float("nan")), x).contiguous()
        self.nan_ids = set(_np(nan.nonzero().flatten()).tolist())

    def db_args(self, vp, pos=True):
        lists = (vp(self.off), vp(self.cent), 5) if self.residual else (None, None, 0)
        return (vp(self.code), vp(self.bad), vp(self.pos) if pos else None, vp(self.cb), self.M) + lists


def _packed(q, lens, metric, list_size):
    """the phrases as the searches pack them -> (blocks, ||q||^2 or None, place, lengths)"""
    from sylber_amd import _lib
    from sylber_amd._index import _on_device, _phrase_blocks, _prep, _row_norms
    dev = torch.device(DEV)
    lens = np.asarray(lens, np.int64)
    b = _phrase_blocks(_lib.load(), dev, _prep(torch.as_tensor(q), metric, dev), lens, 0, len(lens), np.array([0, 1], np.int64), list_size, 0, 0,
                       None)
    return b, (_row_norms(b.qp) if metric == "l2" else None), _on_device(b.place, np.int32, dev), _on_device(b.ln, np.int32, dev)


def _rerank_pair(db, metric, q, lens, cand, off, k, fill=None, pos=True):
    """(costs, seqs, spans) of ``sylber_dtw_rerank`` on the plane and of ``sylber_dtw_rerank_codes`` on the codes"""
    from sylber_amd import _lib
    from sylber_amd._index import METRICS, _row_norms
    from sylber_amd.kmeans import _stream, _vp
    lib, dev = _lib.load(), torch.device(DEV)
    P, m = cand.shape
    b, qn, place_d, len_d = _packed(q, lens, metric, m)
    cn = _row_norms(db.plane) if metric == "l2" else None
    cand_d = torch.as_tensor(cand, dtype=torch.int32).to(dev)
    off_d = torch.as_tensor(off, dtype=torch.int32).to(dev)
    out = []
    with torch.cuda.device(dev):
        st = _stream(dev)
        for coded in (False, True):
            costs = torch.full((P, k), 7.0, dtype=torch.float32, device=dev)
            seqs = torch.full((P, k), 7, dtype=torch.int64, device=dev)
            spans = torch.full((P, k, 2), 7, dtype=torch.int64, device=dev)
            ws = torch.empty(int(lib.sylber_dtw16_workspace_bytes(P, m, 1)), dtype=torch.uint8, device=dev)
            if fill is not None:
                ws.fill_(fill)
            head = (_vp(b.qp), b.nb, _vp(qn), _vp(place_d), _vp(len_d), P)
            tail = (db.N, db.D, _vp(cn), METRICS[metric], _vp(cand_d), m, _vp(off_d), len(off) - 1, k, _vp(costs), _vp(seqs), _vp(spans), _vp(ws), st)
            if coded:
                _lib.check(lib.sylber_dtw_rerank_codes(*head, *db.db_args(_vp, pos), *tail), "sylber_dtw_rerank_codes")
            else:
                _lib.check(lib.sylber_dtw_rerank(*head, _vp(db.plane), *tail), "sylber_dtw_rerank")
            out.append((costs, seqs, spans))
    return out


def _phrases_for(db, seed=1):
    """phrases of 1, 2, 63, 64 and 5 rows near rows of the plane (NaN rows replaced), and candidates: every sequence and a -1 for
    each phrase, nothing but -1 for the last"""
    g = torch.Generator().manual_seed(seed)
    plane = torch.nan_to_num(db.plane.cpu(), nan=0.5)
    starts = (3, 34, 160, 228, 100)
    q = torch.cat([plane[a:a + n] + 0.1 * torch.randn((n, db.D), generator=g) for a, n in zip(starts, PHRASE_LENS)])
    q = torch.cat([q, torch.randn((3, db.D), generator=g)])
    lens = list(PHRASE_LENS) + [3]
    S = len(SEQ_LENS)
    cand = np.full((len(lens), S + 2), -1, np.int32)
    for p in range(len(lens) - 1):
        cand[p, :S + 1] = np.roll(np.concatenate([np.arange(S), [-1]]), p)
    return q, lens, cand


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,M", [(32, 2), (32, 1), (64, 4)])
def test_rerank_codes_is_rerank_on_the_plane(D, M, metric, residual):
    db = _Coded(D, M, residual)
    assert db.masked_id in db.nan_ids and (db.unlisted_id in db.nan_ids) == residual
    off = np.concatenate([[0], np.cumsum(SEQ_LENS)])
    q, lens, cand = _phrases_for(db)
    want, got = _rerank_pair(db, metric, q, lens, cand, off, 4, fill=0xFF)
    _assert_equal(got, want, (D, M, metric, residual))
    c, s = _np(got[0]), _np(got[1])
    assert np.isfinite(c[:-1, 0]).all() and (s[:-1, 0] >= 0).all()
    assert np.isposinf(c[-1]).all() and (s[-1] == -1).all() and (_np(got[2])[-1] == -1).all()      # nothing but -1 candidates
    assert np.isfinite(c[:-1]).all()                                          # a path may start behind a NaN row: every sequence matches


def test_rerank_codes_at_the_widest_geometry_and_with_identity_positions():
    off = np.concatenate([[0], np.cumsum(SEQ_LENS)])
    db = _Coded(1024, 64, True)
    q, lens, cand = _phrases_for(db)
    want, got = _rerank_pair(db, "l2", q, lens, cand, off, 4)
    _assert_equal(got, want, "D = 1024, M = 64")
    assert np.isfinite(_np(got[0])[:-1, 0]).all()
    for residual in (False, True):
        db = _Coded(32, 2, residual, identity=True)
        q, lens, cand = _phrases_for(db)
        want, got = _rerank_pair(db, "l2", q, lens, cand, off, 4, pos=False)
        _assert_equal(got, want, "pos_dev = null")
        assert np.isfinite(_np(got[0])[:-1, 0]).all()


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,M", [(32, 2), (64, 4)])
def test_align_codes_is_align_on_the_plane(D, M, metric, residual):
    from sylber_amd import _lib
    from sylber_amd._index import METRICS, _row_norms
    from sylber_amd.kmeans import _stream, _vp
    db = _Coded(D, M, residual)
    lib, dev = _lib.load(), torch.device(DEV)
    q, lens, _ = _phrases_for(db)
    b, qn, place_d, len_d = _packed(q, lens, metric, 1)
    cn = _row_norms(db.plane) if metric == "l2" else None
    # (phrase, window): whole sequences, windows that start mid-sequence and cross sequence ends, one that ends on the masked row (id
    # 40: the forced end costs +inf), one that ends on the row in no list (id 150), one row, 65 and 72 rows, padding (none, reversed,
    # past the end, too long, a phrase too many), the last row alone, and two windows that cross those rows: the path starts behind them
    pairs = [(0, 0, 1), (0, 10, 43), (1, 35, 37), (1, 41, 74), (4, 96, 161), (4, 20, 41), (4, 140, 151), (2, 164, 229), (3, 228, 300),
             (3, 100, 133), (2, 151, 215), (0, -1, -1), (1, 9, 3), (4, 290, 301), (4, 0, 73), (6, 0, 8), (4, 299, 300), (4, 20, 60),
             (4, 140, 160)]
    pp = torch.tensor([p for p, _, _ in pairs], dtype=torch.int32, device=dev)
    win = torch.tensor([[a, e] for _, a, e in pairs], dtype=torch.int32, device=dev)
    n, max_cols, Mx = len(pairs), 72, 64
    out = []
    with torch.cuda.device(dev):
        st = _stream(dev)
        for coded in (False, True):
            rows = torch.full((n, Mx, 2), 7, dtype=torch.int32, device=dev)
            steps = torch.full((n,), 7, dtype=torch.int32, device=dev)
            costs = torch.zeros(n, dtype=torch.float32, device=dev)
            start = torch.full((n,), 7, dtype=torch.int32, device=dev)
            ws = torch.full((int(lib.sylber_dtw_align_workspace_bytes(n, max_cols)),), 0xFF, dtype=torch.uint8, device=dev)
            head = (_vp(b.qp), b.nb, _vp(qn), _vp(place_d), _vp(len_d), len(lens))
            tail = (db.N, db.D, _vp(cn), METRICS[metric], _vp(pp), _vp(win), n, max_cols, Mx, _vp(rows), _vp(steps), _vp(costs), _vp(start),
                    _vp(ws), st)
            if coded:
                _lib.check(lib.sylber_dtw_align_codes(*head, *db.db_args(_vp), *tail), "sylber_dtw_align_codes")
            else:
                _lib.check(lib.sylber_dtw_align(*head, _vp(db.plane), *tail), "sylber_dtw_align")
            out.append((rows, steps, costs, start))
    want, got = out
    _assert_equal(got, want, (D, M, metric, residual))
    rows, steps, costs, start = (_np(t) for t in got)
    pad = np.array([False] * 11 + [True] * 5 + [False] * 3)
    pad[5] = True                                                              # the window that ends on the masked row: +inf
    if residual:
        pad[6] = True                                                          # and the one that ends on the row in no list
    assert (steps[pad] == 0).all() and np.isposinf(costs[pad]).all() and (rows[pad] == -1).all() and (start[pad] == -1).all()
    assert (steps[~pad] > 0).all() and np.isfinite(costs[~pad]).all() and np.array_equal(start[~pad], rows[~pad, 0, 0])
    assert rows[1, 0, 0] == 42 and rows[8, 63, 1] == 300 and rows[16, 4, 1] == 300 and rows[17, 0, 0] > 40
    assert not residual or rows[18, 0, 0] > 150


# ---- the index level: the planted case ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case():
    c = V.planted_case()
    rng = np.random.default_rng(11)
    x, D = c["x"], c["x"].shape[1]
    extra = [rng.standard_normal((1, D)).astype(np.float32), (x[200:264] + 0.2 * rng.standard_normal((64, D))).astype(np.float32),
             (x[900:933] * 1.1).astype(np.float32)]
    c["all_phrases"] = list(c["phrases"]) + extra
    t = int(c["truth"][0])
    c["nan_row"] = int(c["offsets"][t]) + 1
    xm = x.copy()
    xm[c["nan_row"], 5] = np.nan                                              # inside the first planted phrase's sequence
    c["x_masked"] = xm
    return c


@functools.lru_cache(maxsize=None)
def _codebooks(residual):
    return Q.planted_index(residual)["codebooks"]


def _build(metric, residual, x=None, groups=None, **kw):
    from sylber_amd import IVFPQSyllableIndex, SyllableIndex
    c = _case()
    idx = SyllableIndex(c["x"] if x is None else x, metric=metric, groups=c["groups"] if groups is None else groups, device=DEV)
    return IVFPQSyllableIndex.build(idx, M=Q.M, centroids=c["centroids"], codebooks=_codebooks(residual), residual=residual, **kw)


@functools.lru_cache(maxsize=None)
def _ix(metric, residual, masked=False):
    return _build(metric, residual, _case()["x_masked"] if masked else None)


def _plane(ix):
    """what ``rerank=False`` runs on: ``ix.decode`` of every row, a masked row a NaN row; and its c"""
    x = ix.decode(torch.arange(len(ix)))
    bad = ix._by_id(ix._rbad) != 0
    return torch.where(bad[:, None], torch.full_like(x, float("nan")), x).contiguous()


def _vote_then_fp32(ix, ph, k, refine, sc, ids, off, metric, pg=None, sg=None):
    """the numpy vote on reported seeds, then ``sylber_dtw_rerank`` on the materialised plane with ``ix``'s own c"""
    from sylber_amd import _lib
    from sylber_amd._index import METRICS
    from sylber_amd.kmeans import _stream, _vp
    lib, dev = _lib.load(), torch.device(DEV)
    lens, rows = _lens_rows(ph)
    m = k * refine
    cand, bound = V.vote(_np(sc), _np(ids), rows, lens, off, metric, m, pg, sg)
    plane, P = _plane(ix), len(ph)
    b, qn, place_d, len_d = _packed(np.concatenate(ph), lens, metric, m)
    cn = ix._phrase_state()[1]
    costs, seqs, spans = (torch.empty((P, k), dtype=torch.float32, device=dev), torch.empty((P, k), dtype=torch.int64, device=dev),
                          torch.empty((P, k, 2), dtype=torch.int64, device=dev))
    cand_d, off_d = torch.from_numpy(cand).to(dev), torch.as_tensor(off, dtype=torch.int32).to(dev)
    ws = torch.empty(int(lib.sylber_dtw16_workspace_bytes(P, m, 1)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.sylber_dtw_rerank(_vp(b.qp), b.nb, _vp(qn), _vp(place_d), _vp(len_d), P, _vp(plane), len(ix), ix.dim, _vp(cn),
                                         METRICS[metric], _vp(cand_d), m, _vp(off_d), len(off) - 1, k, _vp(costs), _vp(seqs), _vp(spans), _vp(ws),
                                         _stream(dev)), "sylber_dtw_rerank")
    return costs, seqs, spans, torch.from_numpy(cand.astype(np.int64)).to(dev), torch.from_numpy(bound).to(dev)


# ---- (2) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,residual", [("l2", False), ("l2", True), ("cosine", True)])
def test_rows_held_is_the_seeded_search_of_the_rows(metric, residual):
    c, ix = _case(), _ix(metric, residual)
    ph = c["all_phrases"]
    got = ix.search_phrases(ph, K, NPROBE, seeds=SEEDS, refine=REFINE, return_candidates=True)
    stats = ix.last_search
    sc, ids = ix.search(np.concatenate(ph), SEEDS, NPROBE, refine=1, rerank=True)
    _assert_equal(got, ix.index.search_phrases_seeded(ph, sc, ids, K, REFINE, return_candidates=True), (metric, residual))
    lens, rows = _lens_rows(ph)
    cand, bound, seen = V.vote(_np(sc), _np(ids), rows, lens, c["offsets"], metric, K * REFINE, return_seen=True)
    assert np.array_equal(_np(got[3]), cand.astype(np.int64)) and np.array_equal(_np(got[4]).view(np.uint32), bound.view(np.uint32))
    assert stats["seen"] == pytest.approx(seen.mean()) and stats["pairs"] > 0 and "seen" not in ix.last_search
    assert np.array_equal(ix.sequence_offsets(), c["offsets"])
    # (6) the paths behind these spans
    rows_, steps, costs = ix.align_phrases(ph, got[2])
    hit = _np(got[1]) >= 0
    assert np.array_equal(_np(costs).view(np.uint32), _np(got[0]).view(np.uint32))
    assert np.array_equal(_np(rows_)[:, :, 0, 0][hit], _np(got[2])[:, :, 0][hit]) and (_np(steps)[hit] > 0).all()


# ---- (3) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
def test_codes_only_l2_is_the_index_of_the_decoded_rows(residual):
    from sylber_amd import SyllableIndex
    c, ix = _case(), _ix("l2", residual)
    ph = c["all_phrases"]
    before = ix.nbytes if ix._pos is None else None
    got = ix.search_phrases(ph, K, NPROBE, seeds=SEEDS, refine=REFINE, rerank=False, return_candidates=True)
    if before is not None:
        assert ix.nbytes == before + 8 * len(ix)                              # pos and c, once they exist
    dec = SyllableIndex(ix.decode(torch.arange(len(ix))), metric="l2", groups=c["groups"], device=DEV)
    assert torch.equal(dec._c.view(torch.int32), ix._phrase_state()[1].view(torch.int32))
    seeds = ix.search(np.concatenate(ph), SEEDS, NPROBE, rerank=False)
    _assert_equal(got, dec.search_phrases_seeded(ph, *seeds, K, REFINE, return_candidates=True), residual)
    assert (_np(got[1])[:12, 0] == c["truth"]).all()
    # (6): the paths, with the search's bits, the same after drop_rows()
    al = ix.align_phrases(ph, got[2], rerank=False, _tracked_start=True)
    _assert_equal(al[:3], dec.align_phrases(ph, got[2]), "align")
    hit = _np(got[1]) >= 0
    assert np.array_equal(_np(al[2]).view(np.uint32), _np(got[0]).view(np.uint32))
    assert np.array_equal(_np(al[0])[:, :, 0, 0][hit], _np(got[2])[:, :, 0][hit]) and torch.equal(al[3], al[0][:, :, 0, 0])
    held = ix.align_phrases(ph, got[2])                                       # rerank=True: on the rows, other costs
    assert not torch.equal(held[2], al[2])


@pytest.mark.parametrize("metric,residual,masked", [("cosine", False, False), ("cosine", True, False), ("l2", False, True), ("l2", True, True)])
def test_codes_only_is_the_vote_and_the_fp32_kernel_on_the_plane(metric, residual, masked):
    c, ix = _case(), _ix(metric, residual, masked)
    ph = c["all_phrases"]
    got = ix.search_phrases(ph, K, NPROBE, seeds=SEEDS, refine=REFINE, rerank=False, return_candidates=True)
    sc, ids = ix.search(np.concatenate(ph), SEEDS, NPROBE, rerank=False)
    _assert_equal(got, _vote_then_fp32(ix, ph, K, REFINE, sc, ids, c["offsets"], metric), (metric, residual, masked))
    assert np.isfinite(_np(got[0])[1:12, 0]).all()
    if masked:
        bad = c["nan_row"]
        assert int(ix.labels[bad]) == -1 and not (_np(ids) == bad).any()
        sp = _np(got[2]).reshape(-1, 2)
        assert not ((sp[:, 0] <= bad) & (bad < sp[:, 1])).any()                 # no span crosses the NaN row
        al = ix.align_phrases(ph, got[2], rerank=False)
        assert np.array_equal(_np(al[2]).view(np.uint32), _np(got[0]).view(np.uint32))
        # a window that ends on it is padding (the end is forced); one across it starts behind it
        r, s, a = ix.align_phrases(ph[:1], [[[bad - 1, bad + 1], [bad - 1, bad + 3]]], rerank=False)
        assert (r[0, 0] == -1).all() and int(s[0, 0]) == 0 and bool(torch.isposinf(a[0, 0]))
        assert int(r[0, 1, 0, 0]) > bad and int(s[0, 1]) > 0 and bool(torch.isfinite(a[0, 1]))


# ---- (4) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
def test_invariance(tmp_path, residual):
    from sylber_amd import IVFPQSyllableIndex
    c = _case()
    ph = c["all_phrases"]
    ix = _build("l2", residual)
    args = dict(seeds=SEEDS, refine=REFINE, rerank=False, return_candidates=True)
    base = ix.search_phrases(ph, K, NPROBE, **args)
    held = ix.search_phrases(ph, K, NPROBE, seeds=SEEDS, refine=REFINE, return_candidates=True)
    for hook in (dict(query_chunk=1), dict(phrase_chunk=1), dict(splits=3), dict(_workspace_fill=0xFF), dict(query_chunk=5, phrase_chunk=4)):
        _assert_equal(ix.search_phrases(ph, K, NPROBE, **args, **hook), base, str(hook))
    lens, _ = _lens_rows(ph)
    _assert_equal(ix.search_phrases(np.concatenate(ph), K, NPROBE, lengths=lens, **args), base, "lengths=")
    path = str(tmp_path / "ix.npz")
    ix.save(path)
    loaded = IVFPQSyllableIndex.load(path, device=DEV)
    _assert_equal(loaded.search_phrases(ph, K, NPROBE, **args), base, "save / load")
    _assert_equal(loaded.search_phrases(ph, K, NPROBE, seeds=SEEDS, refine=REFINE, return_candidates=True), held, "save / load, rows held")
    # build + two adds: the lists are laid out again, so pos changes
    n0, n1 = int(c["offsets"][20]), int(c["offsets"][41])
    part = _build("l2", residual, c["x"][:n0], c["groups"][:n0])
    part.search_phrases(ph[:2], K, NPROBE, **args)                            # the lazy state exists before the adds
    first = part._pos
    part.add(c["x"][n0:n1], groups=c["groups"][n0:n1])
    assert part._pos is None
    part.add(c["x"][n1:], groups=c["groups"][n1:])
    _assert_equal(part.search_phrases(ph, K, NPROBE, **args), base, "build + add + add")
    assert part._pos.shape[0] == len(ix) and first.shape[0] == n0 and torch.equal(part._pos, ix._pos)
    # drop_rows: the same bits from the codes alone, for the search and the paths
    al = ix.align_phrases(ph, base[2], rerank=False)
    ix.drop_rows()
    _assert_equal(ix.search_phrases(ph, K, NPROBE, **dict(args, rerank=None)), base, "drop_rows")
    _assert_equal(ix.align_phrases(ph, base[2]), al, "drop_rows, align")
    assert np.array_equal(ix.sequence_offsets(), c["offsets"])
    ix.save(path)
    _assert_equal(IVFPQSyllableIndex.load(path, device=DEV).search_phrases(ph, K, NPROBE, **dict(args, rerank=None)), base, "dropped, save / load")
    with pytest.raises(ValueError):
        ix.search_phrases(ph, K, NPROBE, rerank=True)
    with pytest.raises(ValueError):
        ix.align_phrases(ph, base[2], rerank=True)


# ---- (5) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
def test_planted_phrases_are_recovered(residual):
    c = _case()
    t, off = c["truth"], c["offsets"]
    ix = _build("l2", residual)
    for dropped in (False, True):
        if dropped:
            ix.drop_rows()
        for nprobe, seeds in Q.SETTINGS:
            costs, seqs, spans = ix.search_phrases(c["phrases"], Q.K, nprobe, seeds=seeds, refine=Q.REFINE)
            assert np.array_equal(_np(seqs)[:, 0], t), (residual, dropped, nprobe, seeds)
            sp = _np(spans)[:, 0]
            assert ((sp[:, 0] >= off[t]) & (sp[:, 1] <= off[t + 1])).all()


# ---- (7) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rerank", [True, False])
def test_exclusion(rerank):
    c, ix = _case(), _ix("l2", True)
    ph, off = c["phrases"], c["offsets"]
    pg = c["truth"].astype(np.int32)                                          # group = sequence number: each phrase's own clip is excluded
    lens, rows = _lens_rows(ph)
    args = dict(seeds=SEEDS, refine=REFINE, rerank=rerank, groups=pg, exclude_same_group=True, return_candidates=True)
    # default sequences: stage 1a spends no seed on the phrase's own clip
    got = ix.search_phrases(ph, K, NPROBE, **args)
    sc, ids = ix.search(np.concatenate(ph), SEEDS, NPROBE, 1, rerank=rerank, groups=np.repeat(pg, lens), exclude_same_group=True)
    assert not (c["groups"][np.maximum(_np(ids), 0)] == np.repeat(pg, lens)[:, None])[_np(ids) >= 0].any()
    cand, bound = V.vote(_np(sc), _np(ids), rows, lens, off, "l2", K * REFINE, pg, np.arange(off.size - 1))
    assert np.array_equal(_np(got[3]), cand.astype(np.int64)) and np.array_equal(_np(got[4]).view(np.uint32), bound.view(np.uint32))
    assert not (_np(got[1]) == c["truth"][:, None]).any() and (_np(got[1])[:, 0] >= 0).all()
    if rerank:
        _assert_equal(got, ix.index.search_phrases_seeded(ph, sc, ids, K, REFINE, groups=pg, exclude_same_group=True, return_candidates=True))
    else:
        _assert_equal(got, _vote_then_fp32(ix, ph, K, REFINE, sc, ids, off, "l2", pg, np.arange(off.size - 1)), "default sequences")
    # explicit sequences: stage 1a excludes nothing, the vote does
    mid = (off[:-1] + off[1:]) // 2
    cut = np.unique(np.concatenate([off, mid[::2]]))
    got = ix.search_phrases(ph, K, NPROBE, sequences=cut, **args)
    sc, ids = ix.search(np.concatenate(ph), SEEDS, NPROBE, 1, rerank=rerank)
    sg = c["groups"][cut[:-1]]
    cand, bound = V.vote(_np(sc), _np(ids), rows, lens, cut, "l2", K * REFINE, pg, sg)
    assert np.array_equal(_np(got[3]), cand.astype(np.int64)) and np.array_equal(_np(got[4]).view(np.uint32), bound.view(np.uint32))
    assert not (sg[np.maximum(_np(got[1]), 0)] == pg[:, None])[_np(got[1]) >= 0].any()
    if rerank:
        _assert_equal(got, ix.index.search_phrases_seeded(ph, sc, ids, K, REFINE, groups=pg, exclude_same_group=True, sequences=cut,
                                                          return_candidates=True))
    else:
        _assert_equal(got, _vote_then_fp32(ix, ph, K, REFINE, sc, ids, cut, "l2", pg, sg), "explicit sequences")


# ---- (8) ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_input():
    from sylber_amd import _lib
    c, ix = _case(), _ix("l2", False)
    ph = c["phrases"][:2]
    for rerank in (True, False):
        for kw in (dict(seeds=0), dict(seeds=129), dict(seeds=2.5), dict(refine=0), dict(refine=64), dict(phrase_chunk=0), dict(query_chunk=0),
                   dict(splits=-1), dict(exclude_same_group=True), dict(sequences=[0, 5]), dict(groups=[1])):
            with pytest.raises(ValueError):
                ix.search_phrases(ph, K, NPROBE, rerank=rerank, **kw)
        for k, nprobe in ((0, 3), (129, 3), (K, 0), (K, 9)):
            with pytest.raises(ValueError):
                ix.search_phrases(ph, k, nprobe, rerank=rerank)
        for bad in ([np.zeros((65, 32), np.float32)], [np.zeros((3, 16), np.float32)], np.zeros((3, 32), np.float32)):
            with pytest.raises(ValueError):
                ix.search_phrases(bad, K, NPROBE, rerank=rerank)
        for spans in (np.zeros((2, 1, 2), np.int32), np.zeros((3, 1, 2), np.int64), np.array([[[5, 5]], [[0, 1]]]), np.array([[[0, len(ix) + 1]], [[0, 1]]])):
            with pytest.raises(ValueError):
                ix.align_phrases(ph, spans, rerank=rerank)
        # P = 0
        got = ix.search_phrases([], K, NPROBE, rerank=rerank, return_candidates=True)
        assert [tuple(t.shape) for t in got] == [(0, K), (0, K), (0, K, 2), (0, K * 4), (0, K * 4)]
        assert [t.dtype for t in got] == [torch.float32, torch.int64, torch.int64, torch.int64, torch.float32]
        assert ix.last_search["seen"] == 0.0
        rows, steps, costs = ix.align_phrases(ph, np.full((2, 2, 2), -1, np.int64), rerank=rerank)       # nothing but padding: no launch
        assert (rows == -1).all() and (steps == 0).all() and torch.isposinf(costs).all()
    # rows of another length than the codes
    other = _build("l2", False)
    other.index.add(c["x"][:3], groups=c["groups"][:3])
    for rerank in (True, False):
        with pytest.raises(ValueError):
            other.search_phrases(ph, K, NPROBE, rerank=rerank)
        with pytest.raises(ValueError):
            other.align_phrases(ph, np.zeros((2, 1, 2), np.int64) - 1, rerank=rerank)
    # the C entries by themselves: status 1 before any launch
    lib = _lib.load()
    for name, good, cases in Q.abi_refusals():
        for case in cases:
            assert getattr(lib, name)(*dict(good, **case).values()) == 1, (name, case)
            assert lib.sylber_last_error().decode().startswith(name + ": "), (name, case)
    torch.cuda.synchronize()                                                  # and nothing above left an error behind

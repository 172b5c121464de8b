"""GPU tier, every occurrence of a phrase on the approximate indexes (``SyllableIndex.search_occurrences_seeded``,
``IVFSyllableIndex.search_occurrences``, ``PQSyllableIndex.search_occurrences``, ``IVFPQSyllableIndex.search_occurrences``;
csrc/dtw_codes.hip: ``sylber_dtw_rerank_occurrences_codes``).

(1) the C ABI: the entry on a coded database equals ``sylber_dtw_rerank_occurrences`` on the materialised plane, bit for bit, and for
    one configuration tests/occ_ref.py on local costs taken from the library;
(2) the seeded and the inverted-file search against their siblings' candidates and occ_ref restricted to them;
(3) the product-quantized index, rows held and codes only; (4) the compressed inverted file, plain and residual;
(5) consequences; (6) bitwise invariance; (7) ``align_phrases`` on the new spans; (8) refusals and empty input."""
import functools

import numpy as np
import pytest
import torch

import occ_ref as O
import phrase_vote_ref as V
from test_gpu_phrase import _local_costs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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


def _assert_ref(got, ref, what=""):
    """the (costs, seqs, spans) of a call against occ_ref's, bit for bit"""
    c, q, sp = (_np(t) for t in got[:3])
    assert np.array_equal(sp, ref[2]), what
    assert np.array_equal(q, ref[1]), what
    assert np.array_equal(c.view(np.uint32), ref[0].astype(np.float32).view(np.uint32)), what


def _reference(x, offsets, phrases, metric, k, only, phrase_groups=None, seq_groups=None):
    """occ_ref on the library's own local costs, restricted to the candidates ``only``"""
    d = _local_costs(x, offsets, np.concatenate(phrases), metric)
    r0 = np.concatenate([[0], np.cumsum([len(p) for p in phrases])])
    return O.search_occurrences(lambda p, s: d[r0[p]:r0[p + 1], offsets[s]:offsets[s + 1]], len(phrases), offsets, k, np.float32,
                                phrase_groups, seq_groups, only)


def _packed(q, lens, metric, list_size):
    """the phrases as the searches pack them -> (blocks, ||q||^2 or None, place, lengths)"""
    from sylber_amd import _lib
    from sylber_amd._index import _on_device, _phrase_blocks, _prep, _row_norms
    dev = torch.device(DEV)
    lens = np.asarray(lens, np.int64)
    b = _phrase_blocks(_lib.load(), dev, _prep(torch.as_tensor(q), metric, dev), lens, 0, len(lens), np.array([0, 1], np.int64), list_size, 0, 0,
                       None)
    return b, (_row_norms(b.qp) if metric == "l2" else None), _on_device(b.place, np.int32, dev), _on_device(b.ln, np.int32, dev)


def _entry(q, lens, metric, cand, off, k, N, D, cn, plane=None, coded=None, fill=0xA5):
    """(costs, seqs, spans) of ``sylber_dtw_rerank_occurrences`` on ``plane``, or of ``sylber_dtw_rerank_occurrences_codes`` on the
    coded-database group ``coded``; outputs and workspace hold garbage before the call"""
    from sylber_amd import _lib
    from sylber_amd._index import METRICS
    from sylber_amd.kmeans import _stream, _vp
    lib, dev = _lib.load(), torch.device(DEV)
    cand = np.asarray(cand)
    P, m = cand.shape
    b, qn, place_d, len_d = _packed(q, lens, metric, m)
    cand_d = torch.as_tensor(cand.astype(np.int32)).to(dev)
    off_d = torch.as_tensor(np.asarray(off), dtype=torch.int32).to(dev)
    costs = torch.full((P, k), 7.0, dtype=torch.float32, device=dev)
    seqs = torch.full((P, k), 7, dtype=torch.int64, device=dev)
    spans = torch.full((P, k, 2), 7, dtype=torch.int64, device=dev)
    ws = torch.full((int(lib.sylber_dtw_occ_workspace_bytes(P, m, k)),), fill, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        head = (_vp(b.qp), b.nb, _vp(qn), _vp(place_d), _vp(len_d), P)
        tail = (N, D, _vp(cn), METRICS[metric], _vp(cand_d), m, _vp(off_d), len(off) - 1, k, _vp(costs), _vp(seqs), _vp(spans), _vp(ws), _stream(dev))
        if coded is not None:
            _lib.check(lib.sylber_dtw_rerank_occurrences_codes(*head, *coded, *tail), "sylber_dtw_rerank_occurrences_codes")
        else:
            _lib.check(lib.sylber_dtw_rerank_occurrences(*head, _vp(plane), *tail), "sylber_dtw_rerank_occurrences")
    return costs, seqs, spans


# ---- (1) the C ABI: a coded database against its materialised plane -----------------------------------------------------------------
SEQ_LENS = (1, 2, 31, 32, 33, 64, 65, 72)                                   # 300 rows: the chunk of 32 from both sides
PHRASE_LENS = (1, 2, 63, 64, 5)
OFF1 = np.concatenate([[0], np.cumsum(SEQ_LENS)])


class _Coded:
    """a random coded database of 300 rows in a shuffled position order (``identity``: in id order, for ``pos_dev = null``): one masked
    row, with residual codes one row behind the lists (in no list) and an empty list; ``plane`` is its materialisation in id order"""

    def __init__(self, D, M, residual, identity=False, seed=0):
        g = torch.Generator().manual_seed(seed + D + M)
        N, nlist, dsub = sum(SEQ_LENS), 5, D // M
        self.N, self.D, self.M, self.residual = N, D, M, residual
        self.cb = torch.randn((M, 256, dsub), generator=g).to(DEV)
        self.code = torch.randint(0, 256, (N, M), generator=g, dtype=torch.uint8).to(DEV)          # by position
        perm = torch.arange(N) if identity else torch.randperm(N, generator=g)
        self.masked_id = 40                                                                      # in the sequence of 32 rows
        self.unlisted_id = N - 1 if identity else 150                                            # in the sequence of 72 / of 64 rows
        if residual and not identity:                                                            # the unlisted row lies behind the lists
            last = int(perm[self.unlisted_id])
            other = int((perm == N - 1).nonzero()[0, 0])
            perm[self.unlisted_id], perm[other] = N - 1, last
        self.pos = perm.to(torch.int32).to(DEV)                                                  # row id -> position
        bad = torch.zeros(N, dtype=torch.uint8)
        bad[perm[self.masked_id]] = 1
        self.bad = bad.to(DEV)
        self.off = torch.tensor([0, 70, 70, 150, 220, N - 1 if residual else N], dtype=torch.int32, device=DEV)      # list 1 is empty
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

    def group(self, pos=True):
        from sylber_amd.kmeans import _vp
        lists = (_vp(self.off), _vp(self.cent), 5) if self.residual else (None, None, 0)
        return (_vp(self.code), _vp(self.bad), _vp(self.pos) if pos else None, _vp(self.cb), self.M) + lists


def _phrases_for(db, seed=1):
    """phrases of 1, 2, 63, 64 and 5 rows near rows of the plane (NaN rows replaced) and one of 3 random rows; candidates: every
    sequence (distinct, in another order for each phrase) around a -1 hole, and nothing but -1 for the last phrase"""
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


def _non_vacuous(full, k, finite_rows):
    """on the reference result ``full`` at k = 128: some (phrase, sequence) pair has two occurrences or more, some phrase's list is
    cut at k, some list ends in padding"""
    c, s = _np(full[0]), _np(full[1])
    twice = any(np.unique(s[p][s[p] >= 0], return_counts=True)[1].max(initial=0) >= 2 for p in range(len(s)))
    have = np.isfinite(c).sum(1)
    have[0] = max(have[0], finite_rows)                        # the one-row phrase: every finite row is an occurrence
    return twice and (have > k).any() and (have < k).any()


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("D,M", [(64, 4), (768, 48)])
def test_occurrences_codes_is_the_fp32_entry_on_the_plane(D, M, metric, residual):
    from sylber_amd._index import _row_norms
    for identity in (False, True):                             # pos_dev given (a shuffled order), and null
        db = _Coded(D, M, residual, identity)
        assert db.masked_id in db.nan_ids and (db.unlisted_id in db.nan_ids) == residual and len(db.nan_ids) == 1 + residual
        q, lens, cand = _phrases_for(db)
        cn = _row_norms(db.plane) if metric == "l2" else None
        want = {}
        for k in (1, 5, 128):
            want[k] = _entry(q, lens, metric, cand, OFF1, k, db.N, D, cn, plane=db.plane)
            got = _entry(q, lens, metric, cand, OFF1, k, db.N, D, cn, coded=db.group(pos=not identity), fill=0xFF)
            _assert_equal(got, want[k], (D, M, metric, residual, identity, k))
        for k in (1, 5, 128):
            assert _non_vacuous(want[128], k, db.N - len(db.nan_ids)), (D, M, metric, residual, identity, k)
            _assert_equal([t[:, :k] for t in want[128]], want[k], "the first k of the 128")
        c, s, sp = (_np(t) for t in want[128])
        assert np.isposinf(c[-1]).all() and (s[-1] == -1).all() and (sp[-1] == -1).all()           # nothing but -1 candidates
        live = sp[..., 0] >= 0
        for bad in db.nan_ids:                                 # no occurrence crosses a NaN row
            assert not ((sp[..., 0] <= bad) & (bad < sp[..., 1]) & live).any()


def test_occurrences_codes_against_the_contract():
    """one configuration against occ_ref on local costs from the library (``search`` on pieces of the plane), every k"""
    from sylber_amd._index import _row_norms
    D, M = 64, 4
    db = _Coded(D, M, True)
    q, lens, cand = _phrases_for(db)
    plane = _np(db.plane)
    phrases = np.split(q.numpy(), np.cumsum(lens)[:-1])
    ref = _reference(plane, OFF1, phrases, "l2", 128, cand)
    counts = ref[3]
    S = len(SEQ_LENS)
    per_pair = [len(O.occurrences(_local_costs(plane, OFF1, phrases[1], "l2")[:, OFF1[s]:OFF1[s + 1]])) for s in range(S)]
    assert max(per_pair) >= 2                                  # a (phrase, sequence) pair with two occurrences or more
    for k in (1, 5, 128):
        assert (counts > k).any() and (counts < k).any()       # a list cut at k, a list that ends in padding
        got = _entry(q, lens, "l2", cand, OFF1, k, db.N, D, _row_norms(db.plane), coded=db.group(), fill=0xFF)
        _assert_ref(got, [r[:, :k] for r in ref[:3]], k)


# ---- the index level ----------------------------------------------------------------------------------------------------------------
LENS = (20, 35, 1, 64, 33, 90, 12, 40, 31, 2, 50, 25)                       # 403 rows in 12 sequences
D2, M2, NLIST, NPROBE, SEEDS = 64, 4, 4, 2, 32
PLANTED_SEQ, PLANTED_AT, PLANTED_ROWS = 5, (4, 40, 80), 6


@functools.lru_cache(maxsize=None)
def _case():
    rng = np.random.default_rng(17)
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    N = int(off[-1])
    x = rng.standard_normal((N, D2)).astype(np.float32)
    phrase = rng.standard_normal((PLANTED_ROWS, D2)).astype(np.float32)
    planted = [int(off[PLANTED_SEQ]) + a for a in PLANTED_AT]
    for a in planted:
        x[a:a + PLANTED_ROWS] = phrase

    def near(a, n):
        return (x[a:a + n] + 0.3 * rng.standard_normal((n, D2))).astype(np.float32)

    phrases = [phrase, near(int(off[1]) + 3, 1), near(int(off[3]) + 10, 9), near(int(off[7]) + 5, 20), rng.standard_normal((12, D2)).astype(np.float32)]
    owner = np.array([PLANTED_SEQ, 1, 3, 7, 10], np.int32)                  # the sequence each phrase is excluded from in (5)
    xm = x.copy()
    nan_row = int(off[3]) + 30
    xm[nan_row, 7] = np.nan
    sel = rng.choice(N, 256, replace=False)
    unit = x / np.linalg.norm(x, axis=1, keepdims=True)
    cb = {"l2": np.stack([x[sel, m * 16:(m + 1) * 16] for m in range(M2)]).astype(np.float32),      # sub-rows of real rows as codebooks
          "cosine": np.stack([unit[sel, m * 16:(m + 1) * 16] for m in range(M2)]).astype(np.float32)}
    return dict(x=x, x_masked=xm, nan_row=nan_row, off=off, N=N, phrases=phrases, owner=owner, planted=sorted((a, a + PLANTED_ROWS) for a in planted),
                groups=np.repeat(np.arange(len(LENS)), LENS).astype(np.int32), centroids=x[rng.choice(N, NLIST, replace=False)].copy(), cb=cb)


def _index(metric="l2", masked=False, rows=slice(None)):
    from sylber_amd import SyllableIndex
    c = _case()
    return SyllableIndex((c["x_masked"] if masked else c["x"])[rows], metric=metric, groups=c["groups"][rows], device=DEV)


def _build(kind, metric="l2", masked=False, rows=slice(None)):
    """a fresh index of one of the four kinds over (a prefix of) the case's rows, with the case's centroids and codebooks"""
    from sylber_amd import IVFPQSyllableIndex, IVFSyllableIndex, PQSyllableIndex
    c, idx = _case(), _index(metric, masked, rows)
    if kind == "flat":
        return idx
    if kind == "ivf":
        return IVFSyllableIndex.build(idx, centroids=c["centroids"])
    if kind == "pq":
        return PQSyllableIndex.build(idx, M=M2, codebooks=c["cb"][metric])
    return IVFPQSyllableIndex.build(idx, M=M2, centroids=c["centroids"], codebooks=c["cb"][metric], residual=kind == "ivfpq-res")


@functools.lru_cache(maxsize=None)
def _ix(kind, metric="l2", masked=False):
    return _build(kind, metric, masked)


def _load(kind, path):
    from sylber_amd import IVFPQSyllableIndex, IVFSyllableIndex, PQSyllableIndex, SyllableIndex
    cls = {"flat": SyllableIndex, "ivf": IVFSyllableIndex, "pq": PQSyllableIndex}.get(kind, IVFPQSyllableIndex)
    return cls.load(path, device=DEV)


def _rows_of(ph):
    return ph if isinstance(ph, np.ndarray) else np.concatenate(ph)


def _lens_rows(ph):
    lens = np.array([len(p) for p in ph])
    return lens, np.cumsum(lens) - lens


def _occ(ix, kind, mode, ph, k, refine, **kw):
    """the new search of an index of ``kind`` (``mode``: its ``rerank``, None where it has none), with its candidates"""
    kw = dict(kw, return_candidates=True)
    if kind == "flat":
        seed_kw = {key: kw.pop(key) for key in ("query_chunk",) if key in kw}
        return ix.search_occurrences_seeded(ph, *ix.search(_rows_of(ph), SEEDS, **seed_kw), k, refine, **kw)
    if kind == "ivf":
        return ix.search_occurrences(ph, k, NPROBE, SEEDS, refine, **kw)
    if kind == "pq":
        return ix.search_occurrences(ph, k, refine, rerank=mode, **kw)
    return ix.search_occurrences(ph, k, NPROBE, SEEDS, refine, rerank=mode, **kw)


def _sibling(ix, kind, mode, ph, k, refine, **kw):
    """the per-sequence search with the same stage 1"""
    kw = dict(kw, return_candidates=True)
    if kind == "flat":
        return ix.search_phrases_seeded(ph, *ix.search(_rows_of(ph), SEEDS), k, refine, **kw)
    if kind == "ivf":
        return ix.search_phrases(ph, k, NPROBE, SEEDS, refine, **kw)
    if kind == "pq":
        return ix.search_phrases(ph, k, refine, rerank=mode, **kw)
    return ix.search_phrases(ph, k, NPROBE, SEEDS, refine, rerank=mode, **kw)


def _align(ix, kind, mode, ph, spans):
    return ix.align_phrases(ph, spans) if kind in ("flat", "ivf") else ix.align_phrases(ph, spans, rerank=mode)


def _plane(ix, kind):
    """the rows that ``rerank=False`` runs on: ``decode`` of every row, a masked row a NaN row"""
    x = ix.decode(torch.arange(len(ix)))
    bad = (ix._bad if kind == "pq" else ix._by_id(ix._rbad)) != 0
    return torch.where(bad[:, None], torch.full_like(x, float("nan")), x).contiguous()


def _norms(ix, kind):
    return ix._recon_norms() if kind == "pq" else ix._phrase_state()[1]


METHODS = [("flat", None), ("ivf", None), ("pq", True), ("pq", False), ("ivfpq", True), ("ivfpq", False), ("ivfpq-res", True), ("ivfpq-res", False)]
IDS = ["seeded", "ivf", "pq-rows", "pq-codes", "ivfpq-rows", "ivfpq-codes", "ivfpq-res-rows", "ivfpq-res-codes"]


# ---- (2) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("kind", ["flat", "ivf"])
def test_seeded_and_ivf_are_the_contract_on_the_siblings_candidates(kind, metric):
    c, ix = _case(), _ix(kind, metric)
    ph, K, R = c["phrases"], 4, 2
    got = _occ(ix, kind, None, ph, K, R)
    if kind == "ivf":
        seen = ix.last_search["seen"]
        assert seen > 0 and ix.last_search["pairs"] > 0
    sib = _sibling(ix, kind, None, ph, K, R)
    _assert_equal(got[3:], sib[3:], "cand and bound are the sibling's")
    if kind == "ivf":
        assert ix.last_search["seen"] == seen
    cand = _np(got[3])
    ref = _reference(c["x"], c["off"], ph, metric, K, cand)
    _assert_ref(got, ref, (kind, metric))
    assert (ref[3] > K).any() and (cand >= 0).any(1).all()
    # the three planted spans come first
    assert PLANTED_SEQ in cand[0]
    assert sorted(map(tuple, _np(got[2])[0, :3].tolist())) == c["planted"] and (_np(got[1])[0, :3] == PLANTED_SEQ).all()
    assert _np(got[0])[0, 3] > 100 * max(float(_np(got[0])[0, 2]), 1e-6)


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_with_everything_seeded_it_is_search_occurrences(metric):
    """nprobe == nlist, seeds covering every row, m covering every sequence: ``index.search_occurrences``, bit for bit"""
    from sylber_amd import IVFSyllableIndex
    c = _case()
    rows = slice(0, int(c["off"][4]) + 5)                      # 125 rows <= 128 seeds: sequences 0 .. 3 and the start of the next
    idx = _index(metric, rows=rows)
    n, S = len(idx), idx.sequence_offsets().size - 1
    assert n <= 128 and S == 5
    ivf = IVFSyllableIndex.build(idx, centroids=c["centroids"])
    ph = c["phrases"][1:]
    want = idx.search_occurrences(ph, 8)
    _assert_equal(ivf.search_occurrences(ph, 8, NLIST, seeds=n, refine=1), want, "ivf")
    _assert_equal(idx.search_occurrences_seeded(ph, *idx.search(_rows_of(ph), n), 8, 1), want, "seeded")
    assert (_np(want[1])[:, 0] >= 0).all()


# ---- (3) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_pq_rows_held_is_the_contract_on_the_scans_candidates(metric):
    c, pq = _case(), _ix("pq", metric)
    ph, K, R = c["phrases"], 4, 2
    got = pq.search_occurrences(ph, K, R, return_candidates=True)
    _assert_equal(got[3:], pq.search_phrases(ph, K, R, return_candidates=True)[3:], "cand and coarse are search_phrases'")
    cand = _np(got[3])
    _assert_ref(got, _reference(c["x"], c["off"], ph, metric, K, cand), metric)
    want = _entry(_rows_of(ph), _lens_rows(ph)[0], metric, cand, c["off"], K, c["N"], D2, pq.index._c, plane=pq.index._x)
    _assert_equal(got[:3], want, "search_occurrences_refined's stage 2 on the same candidates")


def test_pq_codes_only_l2_is_the_index_of_the_decoded_rows():
    from sylber_amd import SyllableIndex
    c, pq = _case(), _ix("pq")
    ph, K, R = c["phrases"], 4, 2
    dec = SyllableIndex(pq.decode(torch.arange(len(pq))), metric="l2", groups=c["groups"], device=DEV)
    for storage in ("fp16", "bf16"):
        got = pq.search_occurrences(ph, K, R, storage, rerank=False, return_candidates=True)
        _assert_equal(got, dec.search_occurrences_refined(ph, K, R, storage, return_candidates=True), storage)
    assert np.isfinite(_np(got[0])).all()
    assert not torch.equal(got[0], pq.search_occurrences(ph, K, R)[0])         # the rows' own costs are other costs


def test_pq_codes_only_cosine_with_a_masked_row_is_the_fp32_entry_on_the_plane():
    c, pq = _case(), _build("pq", "cosine")
    ph, K, R = c["phrases"], 4, 2
    # a NaN row has no direction: under "cosine" it is stored as a zero row, so no add() masks a row.  The mask is set by hand.
    assert not pq._bad.any()
    pq._bad[c["nan_row"]] = 1
    got = pq.search_occurrences(ph, K, R, rerank=False, return_candidates=True)
    _assert_equal(got[3:], pq.search_phrases(ph, K, R, rerank=False, return_candidates=True)[3:], "cand, coarse")
    cand = _np(got[3])
    want = _entry(_rows_of(ph), _lens_rows(ph)[0], "cosine", cand, c["off"], K, c["N"], D2, None, plane=_plane(pq, "pq"))
    _assert_equal(got[:3], want, "the NaN-masked plane")
    sp = _np(got[2]).reshape(-1, 2)
    assert (3 == cand).any() and not ((sp[:, 0] <= c["nan_row"]) & (c["nan_row"] < sp[:, 1])).any()


# ---- (4) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("kind", ["ivfpq", "ivfpq-res"])
def test_ivfpq_rows_held_is_the_seeded_search_of_the_rows(kind, metric):
    c, ix = _case(), _ix(kind, metric)
    ph, K, R = c["phrases"], 4, 2
    got = ix.search_occurrences(ph, K, NPROBE, SEEDS, R, return_candidates=True)
    sc, ids = ix.search(_rows_of(ph), SEEDS, NPROBE, refine=1, rerank=True)
    _assert_equal(got, ix.index.search_occurrences_seeded(ph, sc, ids, K, R, return_candidates=True), (kind, metric))
    _assert_equal(got[3:], ix.search_phrases(ph, K, NPROBE, SEEDS, R, return_candidates=True)[3:], "cand, bound")
    _assert_ref(got, _reference(c["x"], c["off"], ph, metric, K, _np(got[3])), (kind, metric))


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("kind", ["ivfpq", "ivfpq-res"])
def test_ivfpq_codes_only_is_the_vote_and_the_fp32_entry_on_the_plane(kind, metric):
    c = _case()
    masked = metric == "l2"                                    # under "cosine" a NaN row is stored as a zero row: nothing is masked
    ix = _build(kind, metric, masked=masked)
    ph, K, R = c["phrases"], 4, 2
    got = ix.search_occurrences(ph, K, NPROBE, SEEDS, R, rerank=False, return_candidates=True)
    sc, ids = ix.search(_rows_of(ph), SEEDS, NPROBE, rerank=False)
    lens, rows = _lens_rows(ph)
    cand, bound = V.vote(_np(sc), _np(ids), rows, lens, c["off"], metric, K * R)
    assert np.array_equal(_np(got[3]), cand.astype(np.int64)) and np.array_equal(_np(got[4]).view(np.uint32), bound.view(np.uint32))
    want = _entry(_rows_of(ph), lens, metric, cand, c["off"], K, c["N"], D2, _norms(ix, kind), plane=_plane(ix, kind))
    _assert_equal(got[:3], want, (kind, metric))
    assert np.isfinite(_np(got[0])[:, 0]).all()
    if masked:
        sp = _np(got[2]).reshape(-1, 2)
        assert int(ix.labels[c["nan_row"]]) == -1 and not ((sp[:, 0] <= c["nan_row"]) & (c["nan_row"] < sp[:, 1])).any()
    # identical from the codes alone
    al = ix.align_phrases(ph, got[2], rerank=False)
    ix.drop_rows()
    _assert_equal(ix.search_occurrences(ph, K, NPROBE, SEEDS, R, return_candidates=True), got, "drop_rows")
    _assert_equal(ix.align_phrases(ph, got[2]), al, "drop_rows, align")
    assert np.array_equal(_np(al[2]).view(np.uint32), _np(got[0]).view(np.uint32))
    with pytest.raises(ValueError):
        ix.search_occurrences(ph, K, NPROBE, SEEDS, R, rerank=True)


# ---- (5) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", METHODS, ids=IDS)
def test_consequence_the_first_entry_of_each_sequence_is_the_siblings(kind, mode):
    c, ix = _case(), _ix(kind)
    ph = c["phrases"][2:]
    got = _occ(ix, kind, mode, ph, 128, 1)
    sib = _sibling(ix, kind, mode, ph, 128, 1)
    _assert_equal(got[3:], sib[3:], "the same candidates")
    cc, q, sp = (_np(t) for t in got[:3])
    pc, pq_, psp = (_np(t) for t in sib[:3])
    assert np.isposinf(cc[:, -1]).all()                        # nothing was cut at k
    for p in range(len(ph)):
        live = np.nonzero(q[p] >= 0)[0]
        first = np.sort(live[np.unique(q[p, live], return_index=True)[1]])      # each sequence's first entry, in list order
        n = int((pq_[p] >= 0).sum())
        assert n == first.size and n > 1 and live.size > n
        assert np.array_equal(q[p, first], pq_[p, :n]) and np.array_equal(sp[p, first], psp[p, :n])
        assert np.array_equal(cc[p, first].view(np.uint32), pc[p, :n].view(np.uint32))


@pytest.mark.parametrize("kind,mode", METHODS, ids=IDS)
def test_consequence_one_row_phrases_find_every_finite_row(kind, mode):
    c = _case()
    ix = _ix(kind, "l2", True)
    ph = [c["phrases"][1], c["x"][int(c["off"][3]) + 29:int(c["off"][3]) + 30] * np.float32(1.01)]      # the second beside the NaN row
    K = 128
    got = _occ(ix, kind, mode, ph, K, 1)
    cc, q, sp, cand = (_np(t) for t in got[:4])
    rows = _np(_plane(ix, kind)) if mode is False else c["x_masked"]
    d = _local_costs(rows, c["off"], _rows_of(ph), "l2")
    off = c["off"]
    for p in range(2):
        ids = np.concatenate([np.arange(off[s], off[s + 1]) for s in cand[p][cand[p] >= 0]])
        ids = ids[np.isfinite(d[p, ids])]
        order = ids[np.lexsort((ids, d[p, ids]))][:K]
        n = order.size
        assert n > 1 and np.array_equal(sp[p, :n, 0], order) and np.array_equal(sp[p, :n, 1], order + 1) and (q[p, n:] == -1).all()
        assert np.array_equal(cc[p, :n].view(np.uint32), d[p, order].view(np.uint32))
        assert np.array_equal(q[p, :n], np.searchsorted(off, order, side="right") - 1)
        assert c["nan_row"] not in sp[p, :, 0]
    assert 3 in cand[1]                                        # the sequence with the NaN row was searched


@pytest.mark.parametrize("kind,mode", METHODS, ids=IDS)
def test_consequence_exclusion_removes_the_phrases_own_sequence(kind, mode):
    c, ix = _case(), _ix(kind)
    ph, pg = c["phrases"], c["owner"]
    got = _occ(ix, kind, mode, ph, 6, 2, groups=pg, exclude_same_group=True)
    free = _occ(ix, kind, mode, ph, 6, 2)
    assert not (_np(got[1]) == pg[:, None]).any() and not (_np(got[3]) == pg[:, None]).any()
    assert (_np(got[1])[:, 0] >= 0).all()
    if mode is not False:                                      # on the rows themselves the three planted copies come first
        assert (_np(free[1])[0, :3] == pg[0]).all()
    _assert_equal(got[3:], _sibling(ix, kind, mode, ph, 6, 2, groups=pg, exclude_same_group=True)[3:], "the sibling's candidates")


# ---- (6) ----------------------------------------------------------------------------------------------------------------------------
HOOKS = {"flat": [dict(phrase_chunk=1), dict(_workspace_fill=0xFF), dict(query_chunk=3)],
         "ivf": [dict(phrase_chunk=1), dict(query_chunk=1), dict(item_tiles=1), dict(_workspace_fill=0xFF), dict(query_chunk=5, phrase_chunk=2)],
         "pq": [dict(phrase_chunk=1), dict(splits=3), dict(block_phrases=1), dict(_workspace_fill=0xFF), dict(splits=len(LENS), phrase_chunk=2)],
         "ivfpq": [dict(phrase_chunk=1), dict(query_chunk=1), dict(splits=3), dict(_workspace_fill=0xFF), dict(query_chunk=5, phrase_chunk=2)]}


@pytest.mark.parametrize("kind,mode", METHODS, ids=IDS)
def test_invariance(tmp_path, kind, mode):
    c = _case()
    ph, K, R = c["phrases"], 4, 2
    ix = _build(kind)
    base = _occ(ix, kind, mode, ph, K, R)
    assert (_np(base[1])[:, 0] >= 0).all()
    for hook in HOOKS[kind.split("-")[0]]:
        _assert_equal(_occ(ix, kind, mode, ph, K, R, **hook), base, str(hook))
    lens, _ = _lens_rows(ph)
    _assert_equal(_occ(ix, kind, mode, _rows_of(ph), K, R, lengths=lens), base, "lengths=")
    path = str(tmp_path / "ix.npz")
    ix.save(path)
    _assert_equal(_occ(_load(kind, path), kind, mode, ph, K, R), base, "save / load")
    n0, n1 = int(c["off"][4]), int(c["off"][8])
    part = _build(kind, rows=slice(0, n0))
    if mode is False:
        _occ(part, kind, mode, ph[:2], K, R)                   # the lazy state exists before the adds
    part.add(c["x"][n0:n1], groups=c["groups"][n0:n1])
    part.add(c["x"][n1:], groups=c["groups"][n1:])
    _assert_equal(_occ(part, kind, mode, ph, K, R), base, "build + add + add")
    if mode is False:                                          # whether the rows are still held
        ix.drop_rows()
        _assert_equal(_occ(ix, kind, None, ph, K, R), base, "drop_rows")
        ix.save(path)
        _assert_equal(_occ(_load(kind, path), kind, None, ph, K, R), base, "dropped, save / load")


# ---- (7) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", METHODS, ids=IDS)
def test_align_phrases_on_the_new_spans(kind, mode):
    c, ix = _case(), _ix(kind)
    ph = c["phrases"]
    got = _occ(ix, kind, mode, ph, 6, 2)
    rows, steps, costs = _align(ix, kind, mode, ph, got[2])
    hit = _np(got[1]) >= 0
    assert hit.any(1).all()
    assert np.array_equal(_np(costs).view(np.uint32), _np(got[0]).view(np.uint32))
    assert np.array_equal(_np(rows)[:, :, 0, 0][hit], _np(got[2])[:, :, 0][hit]) and (_np(steps)[hit] > 0).all()
    assert (_np(rows)[~hit] == -1).all() and (_np(steps)[~hit] == 0).all()


# ---- (8) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", METHODS, ids=IDS)
def test_refusals_and_empty_input(kind, mode):
    c, ix = _case(), _ix(kind)
    ph, K = c["phrases"][:2], 3
    bad = [dict(k=0), dict(k=129), dict(k=2.5), dict(refine=0), dict(refine=64), dict(phrase_chunk=0), dict(exclude_same_group=True),
           dict(sequences=[0, 5]), dict(groups=[1])]
    for kw in bad:
        kw = dict(kw)
        k, refine = kw.pop("k", K), kw.pop("refine", 2)
        with pytest.raises(ValueError):
            _occ(ix, kind, mode, ph, k, refine, **kw)
    for wrong in ([np.zeros((65, D2), np.float32)], [np.zeros((3, 16), np.float32)], np.zeros((3, D2), np.float32)):
        with pytest.raises(ValueError):
            if kind == "flat":
                ix.search_occurrences_seeded(wrong, torch.zeros((3, 4)), torch.zeros((3, 4), dtype=torch.int64), K)
            else:
                _occ(ix, kind, mode, wrong, K, 2)
    if kind == "flat":
        n = sum(len(p) for p in ph)
        sc, si = torch.zeros((n, 4)), torch.zeros((n, 4), dtype=torch.int64)
        for a, b in ((sc[:-1], si[:-1]), (sc, si[:, :3]), (sc.double(), si), (sc, si.int()), (sc, si + len(ix)), (sc, si - 2),
                     (torch.zeros((n, 129)), torch.zeros((n, 129), dtype=torch.int64))):
            with pytest.raises(ValueError):
                ix.search_occurrences_seeded(ph, a, b, K)
        empty = ix.search_occurrences_seeded([], torch.zeros((0, 4)), torch.zeros((0, 4), dtype=torch.int64), K, 2, return_candidates=True)
    else:
        more = [dict(query_chunk=0)] if kind != "pq" else [dict(splits=-1), dict(storage="fp8"), dict(block_phrases=-1)]
        if kind == "ivf":
            more.append(dict(item_tiles=-1))
        if kind.startswith("ivfpq"):
            more.append(dict(splits=-1))
        for kw in more:
            with pytest.raises(ValueError):
                _occ(ix, kind, mode, ph, K, 2, **kw)
        if kind != "pq":
            for nprobe, seeds in ((0, SEEDS), (NLIST + 1, SEEDS), (NPROBE, 0), (NPROBE, 129), (NPROBE, 2.5)):
                with pytest.raises(ValueError):
                    ix.search_occurrences(ph, K, nprobe, seeds, 2)
        empty = _occ(ix, kind, mode, [], K, 2)
    assert [tuple(t.shape) for t in empty] == [(0, K), (0, K), (0, K, 2), (0, K * 2), (0, K * 2)]
    assert [t.dtype for t in empty] == [torch.float32, torch.int64, torch.int64, torch.int64, torch.float32]
    if mode is not None:                                       # rerank=True without the rows; rows of another length than the codes
        gone = _build(kind)
        gone.drop_rows()
        with pytest.raises(ValueError):
            _occ(gone, kind, True, ph, K, 2)
        other = _build(kind)
        other.index.add(c["x"][:3], groups=c["groups"][:3])
        with pytest.raises(ValueError):
            _occ(other, kind, mode, ph, K, 2)
    torch.cuda.synchronize()                                   # and nothing above left an error behind

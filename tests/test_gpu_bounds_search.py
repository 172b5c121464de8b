"""GPU tier, guard bands (tests/guarded_alloc.py) around the search and unit entry points, through the wrappers: sylber_knn_row_norms /
_unit_rows / _search, sylber_knn16_pack / _scan and sylber_knn_rerank; sylber_pq_encode / _lut / _scan / _decode; sylber_ivf_search;
sylber_ivfpq_scan, _scan_residual, _list_terms, _recon_norms and _decode; the phrase searches (sylber_dtw_search, sylber_dtw16_scan +
sylber_dtw_rerank, sylber_dtwpq_scan, sylber_dtw_occurrences, sylber_dtw_rerank_occurrences, the *_codes forms, sylber_phrase_vote)
and sylber_dtw_align; sylber_unit_search, _occurrences and _align; sylber_unit_strings_align.

Every case builds its index from device rows and runs once plainly and once per fill byte (0xFF, 0x00) with every allocation of the
wrappers -- the stored rows, norms, 16-bit planes and codes, the ``[n, k]`` result lists, the per-chunk workspaces -- and the
device-resident inputs between guards.  ``check()`` finds any byte written outside them; the result lists lie in guarded buffers;
for every ``sylber_*_workspace_bytes`` function a wrapper asked, a guarded buffer of exactly a returned size was handed out; and
the results (whole lists: padding is defined as +inf / -1) are bit-identical across the three runs.  No tolerances.

Shapes: N in {1, 129} rows (one row past a 128-row tile), n = 3 queries one at a time (``query_chunk = 1``), k in {1, 128}; phrase
corpora of four sequences of 3, 60, 1 and 65 rows with phrases of 5 (longer than two of the sequences), 1 and 17 rows,
``phrase_chunk`` / ``pair_chunk`` = 1.

Findings: none -- no guard was dirty and no result moved with the fill on an MI355X."""
import numpy as np
import pytest
import torch

from guarded_alloc import FILLS, Guards, recorded_sizes
from sylber_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, M, NLIST = 32, 2, 3
SEQ = [3, 60, 1, 65]                                    # 129 rows in four sequences
PHRASES = [5, 1, 17]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tier needs the MI355X"
    return _lib.load()


def _flat(r):
    if torch.is_tensor(r):
        return [r]
    out = []
    for t in r:
        out += _flat(t) if (torch.is_tensor(t) or isinstance(t, (tuple, list))) else []
    return out


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _three(lib, call, lists=1, sized=True):
    """``call(g)`` plainly and under both fills (the wrappers' allocations guarded, the size functions recorded); at least ``lists``
    tensors of every result tuple must lie in guarded buffers (an int64 id list that torch widened from the kernel's guarded int32
    list does not); everything returned must be bit-identical"""
    plain = _flat(call(None))
    assert plain
    torch.cuda.synchronize()
    for fill in FILLS:
        g = Guards(fill)
        with g.patched(), recorded_sizes(lib) as sizes:
            r = call(g)
        g.check()
        for res in (r if isinstance(r, list) else [r]):
            head = [t for t in _flat(res) if g.covers(t)]
            assert len(head) >= lists, (len(head), g.names())
        if sized:
            assert sizes, "no size function was asked"
        for name, got in sizes.items():
            assert any(g.handed_out(b) for b in got), (name, got, g.names())
        got = _flat(r)
        assert len(got) == len(plain)
        for x, y in zip(got, plain):
            assert x.shape == y.shape and x.dtype == y.dtype
            assert torch.equal(_bits(x), _bits(y)), "fill 0x%02X" % fill


class Data:
    def __init__(self, N, dim=D):
        rng = np.random.default_rng(N + dim)
        self.N = N
        self.x = torch.from_numpy(rng.standard_normal((N, dim)).astype(np.float32)).to(DEV)
        self.groups = np.repeat(np.arange(len(SEQ), dtype=np.int32), SEQ)[:N] if N > 1 else np.zeros(1, np.int32)
        self.q = torch.from_numpy(rng.standard_normal((3, dim)).astype(np.float32)).to(DEV)
        self.qg = np.array([0, 1, 3], np.int32)
        self.centroids = rng.standard_normal((NLIST, dim)).astype(np.float32)
        self.codebooks = rng.standard_normal((M, 256, dim // M)).astype(np.float32)
        # phrases: noisy copies of stored runs, so that matches are real
        xs = self.x.cpu().numpy()
        self.phrases = []
        for m, a in zip(PHRASES, (70, 10, 30)):
            rows = xs[np.arange(a, a + m) % N] + 0.1 * rng.standard_normal((m, dim)).astype(np.float32)
            self.phrases.append(torch.from_numpy(rows.astype(np.float32)).to(DEV))
        self.pg = np.array([1, 3, 0], np.int32)

    def index(self, g, kind="flat", metric="l2", **kw):
        """the index of this kind over the rows, built from a guarded copy of them under guards"""
        from sylber_amd import IVFPQSyllableIndex, IVFSyllableIndex, PQSyllableIndex, SyllableIndex
        x = self.x if g is None else g.guarded_copy(self.x, "rows")
        ix = SyllableIndex(x, metric=metric, groups=self.groups, device=DEV)
        if kind == "ivf":
            ix = IVFSyllableIndex.build(ix, centroids=self.centroids)
        elif kind == "pq":
            ix = PQSyllableIndex.build(ix, M, codebooks=self.codebooks)
        elif kind == "ivfpq":
            ix = IVFPQSyllableIndex.build(ix, M=M, centroids=self.centroids, codebooks=self.codebooks, **kw)
        return ix

    def queries(self, g):
        return self.q if g is None else g.guarded_copy(self.q, "queries")

    def phr(self, g):
        return self.phrases if g is None else [g.guarded_copy(p, "phrase") for p in self.phrases]


_DATA = {}


def _data(N, dim=D):
    if (N, dim) not in _DATA:
        _DATA[(N, dim)] = Data(N, dim)
    return _DATA[(N, dim)]


# ---- exact and two-stage k-NN --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("k", [1, 128])
@pytest.mark.parametrize("N,dim", [(1, 16), (129, 16), (129, 32)])
def test_flat_search(lib, N, dim, k, metric):
    d = _data(N, dim)

    def call(g):
        ix, q = d.index(g, metric=metric), d.queries(g)
        out = [ix.search(q, k, splits=s, query_chunk=1) for s in (0, 3)]
        out.append(ix.search(q, k))
        if N > 1:
            out.append(ix.search(q, k, groups=d.qg, exclude_same_group=True, query_chunk=1))
        return out
    _three(lib, call)


@pytest.mark.parametrize("storage", ["fp16", "bf16"])
@pytest.mark.parametrize("k,refine", [(1, 1), (1, 4), (128, 1)])
@pytest.mark.parametrize("N", [1, 129])
def test_search_refined(lib, N, k, refine, storage):
    d = _data(N)

    def call(g):
        ix, q = d.index(g), d.queries(g)
        out = [ix.search_refined(q, k, refine, storage, splits=s, query_chunk=1) for s in (0, 3)]
        if N > 1:
            out.append(ix.search_refined(q, k, refine, storage, groups=d.qg, exclude_same_group=True, return_candidates=True))
        return out
    _three(lib, call)


# ---- compressed and inverted-file indexes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,refine", [(1, 4), (128, 1)])
def test_pq(lib, k, refine):
    d = _data(129)

    def call(g):
        ix, q = d.index(g, "pq"), d.queries(g)
        codes, bad = ix.encode(q)
        out = [(codes, bad), (ix.decode([0, 5, 128]),)]
        for rerank in (True, False):
            out += [ix.search(q, k, refine, rerank=rerank, splits=s, query_chunk=1) for s in (0, 3)]
        out.append(ix.search(q, k, refine, groups=d.qg, exclude_same_group=True, return_candidates=True))
        return out
    _three(lib, call)


@pytest.mark.parametrize("k", [1, 128])
def test_ivf(lib, k):
    d = _data(129)

    def call(g):
        ix, q = d.index(g, "ivf"), d.queries(g)
        out = [ix.search(q, k, nprobe, query_chunk=1) for nprobe in (1, NLIST)]
        out.append(ix.search(q, k, 2, groups=d.qg, exclude_same_group=True, item_tiles=1))
        return out
    _three(lib, call)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("k,refine", [(1, 4), (128, 1)])
def test_ivfpq(lib, k, refine, residual):
    d = _data(129)

    def call(g):
        ix, q = d.index(g, "ivfpq", residual=residual), d.queries(g)
        out = [(ix.decode([0, 5, 128]),)]
        for rerank in (True, False):
            out += [ix.search(q, k, nprobe, refine, rerank=rerank, splits=s, query_chunk=1) for nprobe, s in ((1, 0), (NLIST, 3))]
        out.append(ix.search(q, k, 2, refine, groups=d.qg, exclude_same_group=True, return_candidates=True))
        return out
    _three(lib, call)


# ---- phrase search -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 6])
def test_phrases_flat(lib, k):
    """fp32 and 16-bit two-stage scans, every occurrence, and the warping paths of what they returned"""
    d = _data(129)

    def call(g):
        ix, ph = d.index(g), d.phr(g)
        one = ix.search_phrases(ph, k, phrase_chunk=1)
        out = [one, ix.search_phrases(ph, k, splits=3, groups=d.pg, exclude_same_group=True)]
        out.append(ix.search_phrases_refined(ph, k, 2, "fp16", phrase_chunk=1, return_candidates=True))
        out.append(ix.search_phrases_refined(ph, k, 1, "bf16", splits=3))
        occ = ix.search_occurrences(ph, k, phrase_chunk=1)
        out += [occ, ix.search_occurrences_refined(ph, k, 2, "fp16", phrase_chunk=1)]
        out += [ix.align_phrases(ph, one[2], pair_chunk=1), ix.align_phrases(ph, occ[2])]
        return out
    _three(lib, call, lists=2)


@pytest.mark.parametrize("k", [1, 6])
def test_phrases_pq(lib, k):
    d = _data(129)

    def call(g):
        ix, ph = d.index(g, "pq"), d.phr(g)
        out = []
        for rerank in (True, False):
            one = ix.search_phrases(ph, k, 2, "fp16", rerank=rerank, phrase_chunk=1)
            occ = ix.search_occurrences(ph, k, 2, "bf16", rerank=rerank, phrase_chunk=1)
            out += [one, occ, ix.align_phrases(ph, one[2], pair_chunk=1, rerank=rerank), ix.align_phrases(ph, occ[2], rerank=rerank)]
        return out
    _three(lib, call, lists=2)


@pytest.mark.parametrize("kind", ["ivf", "ivfpq", "ivfpq_residual"])
def test_phrases_through_the_lists(lib, kind):
    d = _data(129)
    k = 2

    def call(g):
        ix, ph = d.index(g, kind.split("_")[0], **({"residual": True} if kind.endswith("residual") else {})), d.phr(g)
        out = []
        for kw in ([{}] if kind == "ivf" else [{"rerank": True}, {"rerank": False}]):
            one = ix.search_phrases(ph, k, 2, 8, 2, phrase_chunk=1, query_chunk=1, **kw)
            occ = ix.search_occurrences(ph, k, NLIST, 8, 2, phrase_chunk=1, **kw)
            out += [one, occ, ix.align_phrases(ph, one[2], pair_chunk=1, **kw)]
        return out
    _three(lib, call, lists=2)


# ---- unit strings --------------------------------------------------------------------------------------------------------------------
def _units(W):
    rng = np.random.default_rng(W)
    u = rng.integers(0, 6, (129, W)).astype(np.int32)
    groups = np.repeat(np.arange(len(SEQ), dtype=np.int32), SEQ)
    phrases = []
    for m, a in zip(PHRASES, (70, 10, 30)):
        p = u[a:a + m].copy()
        p[m // 2] = (p[m // 2] + 1) % 6
        phrases.append(torch.from_numpy(p).to(DEV))
    return torch.from_numpy(u).to(DEV), groups, phrases


@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("k", [1, 6])
def test_unit_index(lib, W, k):
    from sylber_amd.units import UnitIndex
    u, groups, phrases = _units(W)

    def call(g):
        ix = UnitIndex(u if g is None else g.guarded_copy(u, "units"), groups=groups, device=DEV)
        ph = phrases if g is None else [g.guarded_copy(p, "phrase") for p in phrases]
        one = ix.search_phrases(ph, k, phrase_chunk=1)
        occ = ix.search_occurrences(ph, k, splits=3, groups=np.array([1, 3, 0], np.int32), exclude_same_group=True)
        out = [one, occ, ix.search_phrases(ph, k, max_cost=1, splits=3)]
        out += [ix.align_phrases(ph, one[2], pair_chunk=1), ix.align_phrases(ph, occ[2], free_start=False)]
        return out
    _three(lib, call, lists=2)


@pytest.mark.parametrize("W", [1, 2])
def test_unit_strings(lib, W):
    """whole strings of 0, 1, 33 and 300 units against hypotheses of 5, 0, 40 and 257, one pair at a time and all at once"""
    from sylber_amd.units import align_unit_strings
    rng = np.random.default_rng(40 + W)
    refs = [rng.integers(0, 5, (m, W)).astype(np.int32) for m in (0, 1, 33, 300)]
    hyps = [rng.integers(0, 5, (m, W)).astype(np.int32) for m in (5, 0, 40, 257)]

    def call(g):
        out = []
        for pairing in (False, True):
            for chunk in (1, None):
                r = align_unit_strings(refs, hyps, pairing=pairing, device=DEV, pair_chunk=chunk)
                out.append(tuple(t for t in r if torch.is_tensor(t)))
        return out
    _three(lib, call, lists=2)

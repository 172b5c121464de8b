"""GPU tier, guard bands (tests/guarded_alloc.py) around ``sylber_dtw_local`` through its two wrappers,
``SyllableIndex.search_repeats`` and ``SyllableIndex.find_repeats``: every allocation of the wrappers -- the packed probe rows, the
tables of the plan, scores, sequences and spans, the workspace of exactly ``sylber_dtw_workspace_bytes`` -- and the device-resident
rows of the index lie between guards of one fill byte (0xFF, 0x00).  ``check()`` finds any byte written outside them; what the
kernels wrote into lies in guarded buffers; a guarded buffer of exactly a size the size function returned was handed out; and the
results are bit-identical to the plain run's.

Shapes: sequences of 3, 70, 1, 65, 130 and 150 rows (tile edges inside and at the end of sequences, the last tile of a cut short);
probes of 1, 2, 7, 63 and 64 rows and three sharing a half; one cut, automatic cuts, a cut at every sequence; one probe per block;
k = 1, 6 and 128."""
import numpy as np
import pytest
import torch

from guarded_alloc import FILLS, Guards, recorded_sizes
from sylber_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = ["sylber_dtw_workspace_bytes"]
LENS = (3, 70, 1, 65, 130, 150)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tier needs the MI355X"
    return _lib.load()


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _three(lib, call, written):
    """``call(g)`` plainly and under both fills; ``written(result)``: the tensors that must lie in guarded buffers"""
    plain = call(None)
    torch.cuda.synchronize()
    for fill in FILLS:
        g = Guards(fill)
        with g.patched(), recorded_sizes(lib, names=SIZE) as sizes:
            r = call(g)
        g.check()
        assert g.checked > 0
        assert sizes[SIZE[0]] and all(g.handed_out(b) for b in sizes[SIZE[0]]), (sizes, g.names())
        assert all(g.covers(t) for t in written(r)), g.names()
        flat_r, flat_p = [t for res in r for t in res], [t for res in plain for t in res]
        assert len(flat_r) == len(flat_p)
        for x, y in zip(flat_r, flat_p):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)), "fill 0x%02X" % fill
    return plain


def _corpus(D, seed):
    rng = np.random.default_rng(seed)
    N = sum(LENS)
    x = rng.standard_normal((N, D)).astype(np.float32)
    x[269 + 40:269 + 70] = x[139 + 95:139 + 125] + 0.1 * rng.standard_normal((30, D)).astype(np.float32)   # sequence 4's rows 95 .. 124 again in 5
    x[3 + 20:3 + 30] = x[74 + 50:74 + 60]                     # sequence 3's rows 50 .. 59 in sequence 1
    groups = np.repeat(np.array([0, 1, 2, 3, 4, 1], np.int32), LENS)
    return x, groups


@pytest.mark.parametrize("metric,D", [("l2", 16), ("cosine", 48)])
def test_search_repeats(lib, metric, D):
    from sylber_amd import SyllableIndex
    x, groups = _corpus(D, 70 + D)
    rng = np.random.default_rng(D)
    probes = [x[a:a + m] + 0.1 * rng.standard_normal((m, D)).astype(np.float32) for m, a in ((1, 2), (2, 73), (7, 100), (63, 150), (64, 300), (20, 5), (30, 240), (9, 400))]
    radius = {"l2": 0.5 * D, "cosine": 0.6}[metric]
    xd = torch.from_numpy(x).to(DEV)

    def call(g):
        ix = SyllableIndex(xd if g is None else g.guarded_copy(xd, "rows"), metric=metric, groups=groups, device=DEV)
        return [ix.search_repeats(probes, 6, radius, min_score=radius / 4),
                ix.search_repeats(probes, 128, radius, gap=0.0, min_score=radius / 4, splits=1),
                ix.search_repeats(probes, 1, radius, splits=len(x), block_phrases=1, phrase_chunk=3),
                ix.search_repeats(probes, 6, radius, min_score=radius / 4, groups=[0, 1, 2, 3, 4, 0, 1, 2], exclude_same_group=True)]
    # scores, sequences and spans are the kernels' own output buffers
    plain = _three(lib, call, lambda r: [t for res in r for t in res])
    assert (plain[0][1][:, 0] >= 0).all()                     # every probe was cut from the corpus: it finds itself


@pytest.mark.parametrize("metric,D", [("l2", 16), ("cosine", 48)])
def test_find_repeats(lib, metric, D):
    from sylber_amd import SyllableIndex
    x, groups = _corpus(D, 80 + D)
    radius = {"l2": 0.5 * D, "cosine": 0.6}[metric]
    xd = torch.from_numpy(x).to(DEV)
    offsets = np.concatenate([[0], np.cumsum(LENS)])

    def call(g):
        ix = SyllableIndex(xd if g is None else g.guarded_copy(xd, "rows"), metric=metric, groups=groups, device=DEV)
        return [ix.find_repeats(4, radius), ix.find_repeats(128, radius, min_score=radius / 4, gap=0.0, window=16, hop=5, phrase_chunk=4),
                ix.find_repeats(3, radius, exclude_same_group=True, splits=len(x), sequences=offsets), ix.find_repeats(2, radius, window=7, hop=7)]
    # the padded result lists are allocated by the wrapper
    plain = _three(lib, call, lambda r: [t for res in r for t in res])
    scores, pairs, spans = plain[0]
    assert pairs[:2].tolist() == [[4, 5], [1, 3]] and scores[0] > scores[1] > 0

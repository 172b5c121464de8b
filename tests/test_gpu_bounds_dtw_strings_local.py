"""GPU tier, guard bands (tests/guarded_alloc.py) around ``sylber_dtw_strings_local`` through its two wrappers,
``local_align_sequences`` and ``SyllableIndex.local_align_sequences``: every allocation of the wrappers -- the flat rows and their
norms, the scores and spans, a workspace of exactly ``sylber_dtw_strings_local_workspace_bytes`` per launch -- and the
device-resident inputs lie between guards of one fill byte (0xFF, 0x00).  ``check()`` finds any byte written outside them; what the
kernel wrote into lies in guarded buffers; a guarded buffer of exactly every size the size function returned was handed out; and the
results are bit-identical to the plain run's.

Shapes (m, L): (0, 5), (1, 0), (33, 40), (65, 257), (300, 129) -- the empty sides, one strip and tile, two strips on three tiles,
three super-strips with their carried rows -- and a sequence against itself, with n_best 1 and 4, one pair at a time and all at
once."""
import numpy as np
import pytest
import torch

from guarded_alloc import FILLS, Guards, recorded_sizes
from sylber_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = ["sylber_dtw_strings_local_workspace_bytes"]
SHAPES = ((0, 5), (1, 0), (33, 40), (65, 257), (300, 129))
RADIUS = 48.0                                                      # integer rows in -2 .. 2, D = 32: unrelated rows are about 128 apart


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tier needs the MI355X"
    return _lib.load()


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _three(lib, call):
    """``call(g)`` plainly and under both fills; the scores of every result are the kernel's own output buffer"""
    plain = call(None)
    torch.cuda.synchronize()
    for fill in FILLS:
        g = Guards(fill)
        with g.patched(), recorded_sizes(lib, names=SIZE) as sizes:
            r = call(g)
        g.check()
        assert g.checked > 0
        assert sizes[SIZE[0]] and all(g.handed_out(b) for b in sizes[SIZE[0]]), (sizes, g.names())
        assert all(g.covers(res[0]) for res in r), g.names()
        flat_r, flat_p = [t for res in r for t in res], [t for res in plain for t in res]
        assert len(flat_r) == len(flat_p)
        for x, y in zip(flat_r, flat_p):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)), "fill 0x%02X" % fill
    return plain


def _rows(rng, n):
    return rng.integers(-2, 3, (n, 32)).astype(np.float32)


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_local_align_sequences(lib, metric):
    from sylber_amd import local_align_sequences
    rng = np.random.default_rng(72)
    xs = [_rows(rng, m) for m, _ in SHAPES]
    ys = [_rows(rng, L) for _, L in SHAPES]
    ys[3][100:140], ys[4][60:100] = xs[3][10:50], xs[4][200:240]  # repeats across a tile edge and across a super-strip edge
    own = _rows(rng, 300)
    own[200:230] = own[20:50]                                      # and one inside a sequence
    xd = [torch.from_numpy(x).to(DEV) for x in xs]
    radius = RADIUS if metric == "l2" else 0.5

    def call(g):
        a = xs if g is None else [g.guarded_copy(x, "x") for x in xd]
        out = [local_align_sequences(a, ys, radius=radius, n_best=n_best, metric=metric, device=DEV, pair_chunk=chunk)
               for chunk in (1, None) for n_best in (1, 4)]
        return out + [local_align_sequences([own, xs[2]], radius=radius, n_best=n_best, metric=metric, device=DEV) for n_best in (1, 4)]
    plain = _three(lib, call)
    scores, spans = plain[1]                                       # all pairs at once, n_best = 4
    assert (scores[:3] == 0).all() and (spans[:3] == -1).all() and (scores[3:, 0] > 20 * radius).all()
    assert float(plain[-1][0][0, 0]) > 20 * radius and float(plain[-1][0][1, 0]) == 0


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_index_local_align_sequences(lib, metric):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(73)
    lens = (5, 1, 33, 40, 65, 257, 300, 129)
    off = np.concatenate([[0], np.cumsum(lens)])
    rows = _rows(rng, sum(lens))
    rows[off[5] + 100:off[5] + 140] = rows[off[4] + 10:off[4] + 50]
    rows[off[6] + 200:off[6] + 230] = rows[off[6] + 20:off[6] + 50]
    x = torch.from_numpy(rows).to(DEV)
    groups = np.repeat(np.arange(len(lens), dtype=np.int32), lens)
    pairs = np.array([[1, 0], [2, 3], [4, 5], [6, 7], [6, 6]], np.int64)
    radius = RADIUS if metric == "l2" else 0.5

    def call(g):
        ix = SyllableIndex(x if g is None else g.guarded_copy(x, "rows"), metric=metric, groups=groups, device=DEV)
        return [ix.local_align_sequences(pairs, radius, n_best=n_best, pair_chunk=chunk) for chunk in (1, None) for n_best in (1, 4)]
    plain = _three(lib, call)
    scores, spans = plain[3]
    assert float(scores[2, 0]) > 20 * radius and float(scores[4, 0]) > 20 * radius
    assert spans[4, 0, 0].tolist() == [off[6] + 20, off[6] + 50] and spans[4, 0, 1].tolist() == [off[6] + 200, off[6] + 230]

"""GPU tier, guard bands (tests/guarded_alloc.py) around ``sylber_dtw_strings_align_split`` through ``align_sequences(split=(128,
128))`` and ``SyllableIndex.align_sequences``: every allocation of the wrappers -- the flat rows and their norms, the costs, steps and
runs, a workspace of exactly ``sylber_dtw_strings_split_workspace_bytes`` per call -- and the device-resident inputs lie between guards
of one fill byte (0xFF, 0x00).  ``check()`` finds any byte written outside them; what the kernels wrote into lies in guarded buffers; a
guarded buffer of exactly every size the size function returned was handed out; and the results are bit-identical to the plain run's.

Shapes (m, L): (300, 400), 3 x 4 blocks ragged both ways, and (129, 129), whose last band is one row and whose last chunk is one
column; with and without the path, one pair per call and both at once."""
import numpy as np
import pytest
import torch

from guarded_alloc import FILLS, Guards, recorded_sizes
from sylber_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = ["sylber_dtw_strings_split_workspace_bytes"]
SHAPES = ((300, 400), (129, 129))


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


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_align_sequences_split(lib, metric):
    from sylber_amd import align_sequences
    rng = np.random.default_rng(72)
    xs = [rng.standard_normal((m, 16)).astype(np.float32) for m, _ in SHAPES]
    ys = [rng.standard_normal((L, 16)).astype(np.float32) for _, L in SHAPES]
    xd = [torch.from_numpy(x).to(DEV) for x in xs]

    def call(g):
        a = xs if g is None else [g.guarded_copy(x, "x") for x in xd]
        return [align_sequences(a, ys, metric=metric, path=path, device=DEV, pair_chunk=chunk, split=(128, 128)) for chunk in (1, None) for path in (False, True)]
    # costs and steps are the kernels' own output buffers; the int64 runs are widened from a guarded int32 buffer
    _three(lib, call, lambda r: [t for res in r for t in (res[:2] if len(res) == 2 else res[1:3])])
    plain = call(None)
    base = [align_sequences(xs, ys, metric=metric, path=path, device=DEV, split=False) for path in (False, True)]
    for got, want in zip(plain, base + base):
        for x, y in zip(got, want):
            assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_index_align_sequences_split(lib, metric):
    from sylber_amd import SyllableIndex
    rng = np.random.default_rng(73)
    lens = (300, 400, 129, 129)
    x = torch.from_numpy(rng.standard_normal((sum(lens), 16)).astype(np.float32)).to(DEV)
    groups = np.repeat(np.arange(len(lens), dtype=np.int32), lens)
    pairs = np.array([[0, 1], [2, 3]], np.int64)

    def call(g):
        ix = SyllableIndex(x if g is None else g.guarded_copy(x, "rows"), metric=metric, groups=groups, device=DEV)
        return [ix.align_sequences(pairs, path=path, pair_chunk=chunk, split=(128, 128)) for chunk in (1, None) for path in (False, True)]
    _three(lib, call, lambda r: [t for res in r for t in (res[:2] if len(res) == 2 else res[1:3])])

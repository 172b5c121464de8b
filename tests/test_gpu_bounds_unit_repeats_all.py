"""GPU tier, guard bands (tests/guarded_alloc.py) around ``sylber_unit_local_align_all`` through its two wrappers,
``local_align_unit_strings_all`` and ``UnitIndex.find_repeats`` with ``per_pair`` / ``within``: every allocation of the wrappers --
the flat strings, the scores and spans of every round, the workspace of exactly ``sylber_unit_local_all_workspace_bytes`` -- and the
device-resident inputs lie between guards of one fill byte (0xFF, 0x00).  ``check()`` finds any byte written outside them; what the
kernel wrote into lies in guarded buffers; a guarded buffer of exactly a size the size function returned was handed out; and the
results are bit-identical to the plain run's.

Shapes: strings of 0, 1, 33, 65 and 300 units against 5, 0, 40, 257 and 129 -- no strip, one strip, two with their carried rows, five
-- one pair at a time and all at once, 1, 7 and 32 rounds, and the same strings against themselves; a corpus of six sequences of 3,
70, 1, 65, 130 and 200 rows."""
import numpy as np
import pytest
import torch

from guarded_alloc import FILLS, Guards, recorded_sizes
from sylber_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = ["sylber_unit_local_all_workspace_bytes"]


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


@pytest.mark.parametrize("W", [1, 2, 3])
def test_local_align_unit_strings_all(lib, W):
    from sylber_amd.units import local_align_unit_strings_all
    rng = np.random.default_rng(50 + W)
    xs = [rng.integers(0, 3, (m, W)).astype(np.int32) for m in (0, 1, 33, 65, 300)]
    ys = [rng.integers(0, 3, (m, W)).astype(np.int32) for m in (5, 0, 40, 257, 129)]
    xd = [torch.from_numpy(x).to(DEV) for x in xs]

    def call(g):
        a = xs if g is None else [g.guarded_copy(x, "x") for x in xd]
        out = []
        for chunk, R in ((1, 7), (None, 1), (None, 32)):
            for par in ((2, 3, 4), (1, 1, 1)):
                out.append(local_align_unit_strings_all(a, ys, n_best=R, min_score=1, match=par[0], mismatch=par[1], gap=par[2],
                                                        device=DEV, pair_chunk=chunk))
        out.append(local_align_unit_strings_all(a, n_best=5, device=DEV))
        out.append(local_align_unit_strings_all(a, n_best=3, min_sep=4, device=DEV, pair_chunk=2))
        return out
    # the int32 scores are the kernel's own output buffer; the int64 spans are widened from a guarded int32 buffer
    _three(lib, call, lambda r: [res[0] for res in r])
    assert (call(None)[2][0][2:] > 0).all()                # 32 rounds of every pair with two sides


@pytest.mark.parametrize("W", [1, 2])
def test_find_repeats_every_repeat(lib, W):
    from sylber_amd.units import UnitIndex
    rng = np.random.default_rng(60 + W)
    lens = (3, 70, 1, 65, 130, 200)
    u = rng.integers(0, 4, (sum(lens), W)).astype(np.int32)
    u[150:170] = u[10:30]                                  # sequence 1's units 7 .. 26 again in sequence 4
    u[400:420] = u[300:320]                                # and 20 units of sequence 5 twice
    groups = np.repeat(np.array([0, 1, 2, 1, 3, 4], np.int32), lens)
    ud = torch.from_numpy(u).to(DEV)

    def call(g):
        ix = UnitIndex(ud if g is None else g.guarded_copy(ud, "units"), groups=groups, device=DEV)
        return [ix.find_repeats(6, per_pair=4, within=True), ix.find_repeats(20, per_pair=2, pair_chunk=1, exclude_same_group=True),
                ix.find_repeats(3, within=True, min_sep=3, min_score=1, pair_chunk=3)]
    # the padded result lists are allocated by the wrapper
    _three(lib, call, lambda r: [t for res in r for t in res])
    scores, pairs, spans = call(None)[0]
    assert scores[1] >= 2 * W * 20 and sorted(pairs[:2].tolist()) == [[1, 4], [5, 5]]

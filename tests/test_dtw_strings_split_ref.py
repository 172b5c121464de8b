"""CPU tier: the blocked recurrence of ``sylber_dtw_strings_align_split`` (tests/dtw_strings_split_ref.py: blocks in diagonal order,
explicit boundary rows, columns and corner, two-parity storage reuse) against the global DP of tests/dtw_strings_ref.py, bit for bit
in A, n, the codes and the runs; the two planted defects are rejected by the same comparison; the host's diagonal schedule and the
workspace arithmetic.

Block sizes here are a few cells, not 128: the reference is written for any size, and the storage scheme does not know the number."""
import ctypes

import numpy as np
import pytest

import dtw_strings_ref as G
import dtw_strings_split_ref as B

# (m, L, BR, BC, SR): 1 x 1 blocks; 1 x N; N x 1; 3 x 4 with ragged last blocks; 5 x 5; super-strips inside a block, ragged
CASES = ((3, 4, 4, 4, None), (5, 5, 5, 5, None), (3, 17, 4, 5, None), (17, 3, 5, 4, None), (11, 17, 4, 5, None), (15, 15, 3, 3, None),
         (14, 11, 6, 4, 2), (9, 7, 4, 2, 2), (13, 9, 8, 3, 4))


def _same(d, BR, BC, SR, order="up", defect=None):
    """is the blocked recurrence the global one, bit for bit in A, n, the codes and the runs"""
    A, n, code = G.global_loop(d)
    bA, bn, bcode = B.blocked(d, BR, BC, SR, order, defect)
    ok = np.array_equal(A.view(np.uint32), bA.view(np.uint32)) and np.array_equal(n, bn) and np.array_equal(code, bcode)
    m, L = A.shape
    ref, got = G.align(d), B.align(d, BR, BC, SR, order, defect)
    if ref is None or got is None:
        return ok and ref is None and got is None
    return ok and np.float32(ref[0]).view(np.uint32) == np.float32(got[0]).view(np.uint32) and ref[1] == got[1] and np.array_equal(ref[2], got[2])


@pytest.mark.parametrize("m,L,BR,BC,SR", CASES)
@pytest.mark.parametrize("order", ["up", "down"])
def test_blocked_is_global_bit_for_bit(m, L, BR, BC, SR, order):
    rng = np.random.default_rng(1000 * m + L)
    for d in G.tied_matrices(rng, m, L):                          # random, tied, constant, +inf-holed
        assert _same(d, BR, BC, SR, order), (m, L, BR, BC, SR, order)


def test_an_inf_row_or_column_on_a_block_edge_is_padding():
    rng = np.random.default_rng(3)
    for i, j in ((3, None), (4, None), (None, 4), (None, 5), (7, 9)):
        d = rng.random((11, 17)).astype(np.float32)
        if i is not None:
            d[i, :] = np.inf
        if j is not None:
            d[:, j] = np.nan                                      # a NaN cost counts as +inf
        assert G.align(d) is None and B.align(d, 4, 5) is None and _same(d, 4, 5, None, "down")


def _diagonal(m):
    """0 on the diagonal, 1 elsewhere: the path goes through every block corner of square blocks"""
    return (1 - np.eye(m)).astype(np.float32)


def test_the_planted_defects_are_rejected():
    """the same comparison sees the corner taken from the boundary row after its rewrite, and the swapped column parity"""
    d = _diagonal(15)
    assert _same(d, 3, 3, None, "up") and _same(d, 3, 3, None, "down")
    # block (b+1, c-1) of the same launch rewrites the boundary row: whoever runs after it reads the wrong corner
    assert not _same(d, 3, 3, None, "down", "corner_from_row")
    assert not (_same(d, 3, 3, None, "up", "corner_from_row") and _same(d, 3, 3, None, "down", "corner_from_row"))
    for order in ("up", "down"):
        assert not _same(d, 3, 3, None, order, "column_parity")
    rng = np.random.default_rng(8)
    r = rng.integers(0, 3, (11, 17)).astype(np.float32)
    assert not _same(r, 4, 5, None, "down", "column_parity")


def test_the_schedule_runs_every_block_once_after_its_inputs():
    from sylber_amd.search import split_schedule
    for nbr, nbc in ((1, 1), (1, 6), (6, 1), (3, 4), (4, 3), (5, 5), (512, 2)):
        launches = split_schedule(nbr, nbc)
        assert launches == B.schedule(nbr, nbc)
        assert len(launches) == nbr + nbc - 1
        when = {}
        for d, blocks in enumerate(launches):
            assert blocks and len(blocks) <= min(nbr, nbc)
            for b, c in blocks:
                assert (b, c) not in when and 0 <= b < nbr and 0 <= c < nbc and b + c == d
                when[(b, c)] = d
            assert len({c for _, c in blocks}) == len(blocks)    # one block per chunk: the inner rows of a chunk have one user
        assert len(when) == nbr * nbc
        for (b, c), d in when.items():
            for src in ((b - 1, c), (b, c - 1)):
                if src in when:
                    assert when[src] == d - 1                     # inputs from the launch before
            if (b - 1, c - 1) in when:
                assert when[(b - 1, c - 1)] == d - 2              # the corner's cell is two launches old:
            if (b + 1, c - 1) in when:
                assert when[(b + 1, c - 1)] == d                  # ... and its row is rewritten in this one
    assert split_schedule(0, 3) == [] and split_schedule(3, 0) == []


SIZES = ((0, 5), (5, 0), (1, 1), (128, 128), (129, 129), (1, 300), (300, 1), (64, 257), (300, 400), (385, 257), (8192, 8192), (65536, 8192))
BLOCKS = ((128, 128), (256, 128), (128, 384), (256, 256), (1024, 1024), (0, 0))


def test_workspace_arithmetic():
    from sylber_amd import search as S
    for BR, BC in BLOCKS:
        br, bc = BR or S.SPLIT_BLOCK[0], BC or S.SPLIT_BLOCK[1]
        for path in (False, True):
            got = S.dtw_strings_split_workspace_bytes([m for m, _ in SIZES], [L for _, L in SIZES], path, BR, BC)
            assert got.dtype == np.int64 and got.tolist() == [B.workspace_bytes(m, L, path, br, bc) for m, L in SIZES]
    # what a split adds to a pair: the boundary state, never more than 256 + 16 (2 L + m + bands) + 3 x 255 bytes
    m, L = np.array([65536]), np.array([65536])
    assert int(S.dtw_strings_split_workspace_bytes(m, L, False, 256, 128)[0]) <= 256 + 16 * (2 * 65536 + 65536 + 256) + 765
    # the checks use it: the need of a split pair is its own, the others keep theirs
    ml, Ll = np.array([300, 40, 0]), np.array([400, 50, 7])
    plan = (np.array([True, False, False]), 128, 128)
    need = S._check_sequence_pairs(ml, Ll, True, None, plan)
    assert need.tolist() == [B.workspace_bytes(300, 400, True, 128, 128) + 64, G.workspace_bytes(40, 50, True) + 64, 64]


def test_the_library_agrees_with_the_arithmetic():
    from sylber_amd import _lib
    from sylber_amd import search as S
    lib = _lib.load()
    i32p = ctypes.POINTER(ctypes.c_int32)
    xw = np.array([[0, m] for m, _ in SIZES], np.int32)
    yw = np.array([[0, L] for _, L in SIZES], np.int32)
    fn = lib.sylber_dtw_strings_split_workspace_bytes
    for BR, BC in BLOCKS:
        for path in (0, 1):
            want = 256 * -(-len(SIZES) * 64 // 256) + int(S.dtw_strings_split_workspace_bytes(xw[:, 1], yw[:, 1], bool(path), BR, BC).sum())
            assert int(fn(xw.ctypes.data_as(i32p), yw.ctypes.data_as(i32p), len(SIZES), path, BR, BC)) == want
    for BR, BC in ((100, 128), (128, 100), (-128, 128), (128, -128), (65536 + 128, 128)):
        assert int(fn(xw.ctypes.data_as(i32p), yw.ctypes.data_as(i32p), len(SIZES), 0, BR, BC)) == -1
    assert int(fn(None, yw.ctypes.data_as(i32p), 1, 0, 128, 128)) == -1 and int(fn(xw.ctypes.data_as(i32p), yw.ctypes.data_as(i32p), 0, 0, 128, 128)) == -1


def test_the_split_argument_is_checked_on_the_host():
    from sylber_amd import search as S
    ml, Ll = np.array([300, 40, 0, 128]), np.array([400, 50, 7, 128])
    assert S._split_plan(ml, Ll, False, None) is None
    mask, BR, BC = S._split_plan(ml, Ll, True, None)
    assert mask.tolist() == [True, False, False, False] and (BR, BC) == S.SPLIT_BLOCK
    mask, BR, BC = S._split_plan(ml, Ll, (256, 384), None)
    assert mask.tolist() == [True, True, False, True] and (BR, BC) == (256, 384)
    assert S._split_plan(np.array([0]), np.array([9]), (128, 128), None) is None and S._split_plan(np.array([100]), np.array([90]), True, None) is None
    for bad in ((100, 128), (128, 0), (0, 128), (-128, 128), (128, -128), (128,), (128, 128, 128), (128.0, 128), (True, 128), "yes", 1, (65664, 128)):
        with pytest.raises(ValueError):
            S._split_plan(ml, Ll, bad, None)

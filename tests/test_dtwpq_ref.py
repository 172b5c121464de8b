"""CPU tier, compressed phrase search: tests/dtwpq_ref.py is consistent with the restatements it is built on, and the C entry
``sylber_dtwpq_scan`` is declared, exported and refuses bad arguments by itself (no GPU call)."""
import ctypes
import os
import re

import numpy as np
import pytest

import dtw16_ref as R16
import dtw_ref as DR
import dtwpq_ref as R
import pq_ref as PQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small(seed=3, D=32, M=2):
    """rows that are exactly code words: 9 sequences of 3 .. 12 rows, 5 phrases"""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((M, PQ.KSUB, D // M)).astype(np.float32)
    lens = rng.integers(3, 13, 9)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(offsets[-1])
    x = PQ.decode(rng.integers(0, PQ.KSUB, (N, M)), C).astype(np.float32)
    phrases = [(x[a:a + m] + 0.2 * rng.standard_normal((m, D))).astype(np.float32) for m, a in ((1, 4), (3, 10), (5, 20), (2, 31), (4, 40))]
    return x, C, offsets, phrases


@pytest.mark.parametrize("storage", R.STORAGES)
@pytest.mark.parametrize("rerank", (True, False))
def test_rows_that_are_code_words_give_the_two_stage_search_on_the_rows(storage, rerank):
    x, C, offsets, phrases = _small()
    xh, codes, bad = R.decoded(x, C)
    assert not bad.any() and np.array_equal(xh, x)            # every row decodes to itself, so both stages see the rows
    want = R16.two_stage(phrases, x, offsets, 2, 2, storage, "l2")
    got = R.two_stage(phrases, x, C, offsets, 2, 2, storage, "l2", rerank=rerank)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    grp = np.arange(len(offsets) - 1) % 3
    pgrp = np.array([0, 1, 2, 0, 1])
    want = R16.two_stage(phrases, x, offsets, 2, 2, storage, "l2", pgrp, grp)
    got = R.two_stage(phrases, x, C, offsets, 2, 2, storage, "l2", rerank, pgrp, grp)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_a_masked_row_never_lies_on_a_finite_path(metric):
    x, C, offsets, phrases = _small(seed=4)
    S = len(offsets) - 1
    s_cut, s_all = 2, 5
    codes, bad = PQ.encode(R16.stored(phrases, x, metric)[1], C)
    assert not bad.any()
    bad[int(offsets[s_cut]) + 1] = True                       # a masked row inside sequence 2: a path stays on one side of it
    bad[offsets[s_all]:offsets[s_all + 1]] = True             # sequence 5 is masked throughout
    qs, xh, cc, exact = R.references(phrases, x, C, offsets, "fp16", metric, rerank=False, codes=codes, bad=bad)
    assert np.isnan(xh[bad]).all() and not np.isnan(xh[~bad]).any()
    assert np.isinf(cc[:, s_all]).all() and np.isinf(exact[0][:, s_all]).all()
    for p, q in enumerate(qs):
        d = R16.coarse_local_costs(q, xh[offsets[s_cut]:offsets[s_cut + 1]], "fp16", metric)
        assert np.isinf(d[:, 1]).all() and np.isfinite(np.delete(d, 1, 1)).all()
        sides = [DR.dtw(part, np.float64)[0] for part in (d[:, :1], d[:, 2:]) if part.shape[1]]
        assert cc[p, s_cut] == min(sides)                     # the best path of the two pieces: none crosses the masked column
    got = R.two_stage(phrases, x, C, offsets, S, 1, "fp16", metric, rerank=False, codes=codes, bad=bad)
    assert s_all not in got[1] and s_all not in got[3]
    assert (got[3][:, S - 1] == -1).all() and np.isinf(got[4][:, S - 1]).all()


def test_the_entry_is_declared_exported_and_refuses_by_itself():
    from sylber_amd import build, _lib
    build.build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "sylber_hip.h")).read()
    assert re.search(r"\bint\s+sylber_dtwpq_scan\s*\(", hdr)
    assert "sylber_dtwpq_scan" in _lib.EXPORTS and hasattr(lib, "sylber_dtwpq_scan")
    null = [None if t is ctypes.c_void_p else 1 for t in _lib.EXPORTS["sylber_dtwpq_scan"][1]]
    assert lib.sylber_dtwpq_scan(*null) == 1
    msg = lib.sylber_last_error().decode()
    assert "sylber_dtwpq_scan" in msg and "null" in msg

"""CPU tier, ``sylber_dtw_rerank_occurrences_codes`` (csrc/dtw_codes.hip) as a C entry: it is exported, ``_lib.EXPORTS`` gives it the
argument list of ``sylber_dtw_rerank_codes``, and every class of bad argument returns 1 with a ``sylber_last_error`` that names the
entry BEFORE any device call -- the pointers below are never dereferenced and no device is needed."""
import ctypes

import pytest

NAME = "sylber_dtw_rerank_occurrences_codes"


def _good():
    p = 4096
    return dict(q=p, nb=1, qn=p, prow=p, plen=p, P=3, code=p, bad=p, pos=p, cb=p, M=4, off=p, cent=p, nlist=5, N=100, D=64, cn=p, metric=0,
                cand=p, m=12, soff=p, S=7, k=20, cost=p, seq=p, span=p, ws=p, stream=None)


# the fp32 entry's own: null arguments, counts, D, the ranges of m and k (k is not bounded by m: k = 20 > m = 12 above is legal),
# the metric and its norms
FP32 = [dict(q=None), dict(prow=None), dict(plen=None), dict(cand=None), dict(soff=None), dict(cost=None), dict(seq=None), dict(span=None),
        dict(ws=None), dict(nb=0), dict(P=0), dict(N=0), dict(S=0), dict(D=8), dict(D=72), dict(m=0), dict(m=129), dict(k=0), dict(k=129),
        dict(metric=2), dict(cn=None), dict(qn=None)]
GEOMETRY = [dict(M=0), dict(M=65), dict(M=3), dict(M=8), dict(D=1024, M=128)]
PARTIAL_LISTS = [dict(off=None), dict(cent=None), dict(nlist=0), dict(nlist=-1), dict(off=None, cent=None), dict(off=None, nlist=0),
                 dict(cent=None, nlist=0)]
NO_CODES = [dict(code=None), dict(cb=None)]
TOO_LARGE = [dict(P=70000, nb=547, m=128, k=128), dict(P=1 << 20, nb=1 << 13, m=32, k=33)]      # beyond 2^30 list entries


def test_the_entry_is_exported_with_the_arguments_of_its_sibling():
    from sylber_amd import _lib
    assert NAME in _lib.EXPORTS
    assert _lib.EXPORTS[NAME] == _lib.EXPORTS["sylber_dtw_rerank_codes"]      # the coded-database group unchanged, in the same order
    assert len(_lib.EXPORTS[NAME][1]) == len(_good())
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, NAME)
    assert getattr(_lib.load(), NAME).argtypes == _lib.EXPORTS[NAME][1]


@pytest.mark.parametrize("cases", [FP32, GEOMETRY, PARTIAL_LISTS, NO_CODES, TOO_LARGE], ids=["fp32", "geometry", "lists", "codes", "large"])
def test_bad_arguments_are_refused_before_any_device_call(cases):
    from sylber_amd import _lib
    lib = _lib.load()
    for case in cases:
        args = dict(_good(), **case)
        assert getattr(lib, NAME)(*args.values()) != 0, case
        assert lib.sylber_last_error().decode().startswith(NAME + ": "), case

"""CPU tier: the numpy restatement of the residual codes (tests/ivfpq_residual_ref.py) is itself checked -- its t is the distance to
the reconstruction, with one list at the origin its codes are pq_ref's, and on lists that lie far apart the residual codes
reconstruct better than the codes of the rows themselves -- the fixture the GPU tests use keeps away from fp32 near-ties, and the new
C entry points refuse bad arguments before they touch a device."""
import ctypes

import numpy as np
import pytest

import ivfpq_ref as F
import ivfpq_residual_ref as Q
import pq_ref as P

FIXTURES = [(2000, 32, 2, 8), (2000, 64, 4, 8), (2000, 256, 16, 8), (3000, 768, 48, 8), (4096, 64, 4, 512)]      # N, D, M, nlist


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_t_is_the_distance_to_the_reconstruction(metric):
    """float64 throughout (the reconstruction too): t = ||q - xhat||^2 - ||q||^2 ("l2"), -2 q . xhat ("cosine"), to 1e-9 of the
    magnitudes that cancel in it (||q||^2 + ||xhat||^2)"""
    q, x, cent, _ = Q.clustered_lists(3, 2000, 64, 4, 8, 25)
    qs, xs = P.stored(q, metric), P.stored(x, metric)
    cent = P.stored(cent, metric)
    labels = F.assign(xs, cent)
    C = Q.sampled_codebooks(Q.residuals(xs, cent, labels), 4, 1)
    codes, bad = Q.encode(xs, cent, labels, C)
    assert not bad.any() and labels.min() >= 0
    xhat = Q.reconstruct(codes, labels, cent, C, np.float64)
    probe = F.probe_lists(qs, cent, 3)
    t = Q.scan_t(Q.lut(qs, C), codes, Q.list_terms(qs, cent, probe), Q.recon_norms(xhat) if metric == "l2" else None, labels, probe)
    assert t.dtype == np.float64
    q64 = qs.astype(np.float64)
    inner = -2.0 * q64 @ xhat.T
    want = inner + (xhat * xhat).sum(1)[None] if metric == "l2" else inner
    if metric == "l2":
        direct = ((q64[:, None, :] - xhat[None]) ** 2).sum(2) - (q64 * q64).sum(1)[:, None]
        assert np.abs(direct - want).max() <= 1e-9 * ((q64 * q64).sum(1).max() + (xhat * xhat).sum(1).max())
        want = direct
    member = F.member(labels, probe)
    assert member.any(1).all() and not member.all() and np.isnan(t[~member]).all() and not np.isnan(t[member]).any()
    scale = (q64 * q64).sum(1)[:, None] + (xhat * xhat).sum(1)[None]
    assert (np.abs(t - want)[member] <= 1e-9 * scale[member]).all()
    # the search of the contract returns rows of the probed lists only, best first
    s, i, cand = Q.search(q, x, cent, C, 5, labels, probe, metric=metric, rerank=False)
    for r in range(len(q)):
        assert (i[r] >= 0).all() and member[r, i[r]].all() and np.array_equal(i[r], cand[r])
        key = s[r] if metric == "l2" else -s[r]
        assert (np.diff(key) >= 0).all()


def test_one_list_at_the_origin_gives_the_pq_codes():
    q, x, C = P.clustered(5, 1500, 64, 4, 4, noise=0.3)
    x[[7, 90], 3] = np.nan                                               # in no list: code 0 in every sub-space, masked
    cent = np.zeros((1, 64), np.float32)
    labels = F.assign(x, cent)
    assert labels[7] == -1 and labels[90] == -1 and (np.delete(labels, [7, 90]) == 0).all()
    codes, bad = Q.encode(x, cent, labels, C)
    pc, pb = P.encode(x, C)
    keep = np.delete(np.arange(1500), [7, 90])
    assert np.array_equal(codes[keep], pc[keep]) and not bad[keep].any() and not pb[keep].any()
    assert (codes[[7, 90]] == 0).all() and bad[[7, 90]].all() and pb[[7, 90]].all()
    assert np.array_equal(Q.reconstruct(codes, labels, cent, C)[keep].view(np.uint32), P.decode(pc, C)[keep].view(np.uint32))


def test_residual_codes_reconstruct_better_where_the_lists_lie_far_apart():
    """512 lists, 256 sampled rows as codebooks in both modes, the lists the true centres: the codes of the rows themselves have to say
    where the list lies, the residual codes do not"""
    N, D, M, nlist = FIXTURES[-1]
    q, x, cent, lists = Q.clustered_lists(11, N, D, M, nlist, 8)
    labels = F.assign(x, cent)
    assert np.array_equal(labels, lists)
    r = Q.residuals(x, cent, labels)
    Cr, Cx = Q.sampled_codebooks(r, M, 2), Q.sampled_codebooks(x, M, 2)
    res = Q.recon_error(x, Q.reconstruct(Q.encode(x, cent, labels, Cr)[0], labels, cent, Cr))
    plain = Q.recon_error(x, P.decode(P.encode(x, Cx)[0], Cx))
    assert res < plain, (res, plain)
    assert res < 0.5 * plain, (res, plain)                               # far below: the lists lie 4 / 0.5 spreads apart


@pytest.mark.parametrize("N,D,M,nlist", FIXTURES)
def test_the_fixture_keeps_away_from_fp32_near_ties(N, D, M, nlist):
    """what lets the GPU tests compare codes and lists with float64: no list assignment near a tie (smallest coarse gap above 500)
    and at most 0.025 % of the (row, sub-space) code decisions within the fp32 chain bound of one"""
    q, x, cent, lists = Q.clustered_lists(D + M + N, N, D, M, nlist, 40)
    gap = Q.coarse_gap(x, cent)
    assert gap.min() > 500, gap.min()
    labels = F.assign(x, cent)
    assert np.array_equal(labels, lists)
    r = Q.residuals(x, cent, labels)
    und = 1.0 - P.decided(r, Q.sampled_codebooks(r, M, 1)).mean()
    assert und <= 0.00025, und


def test_entry_points_refuse_bad_arguments_without_a_device():
    from sylber_amd import build, _lib
    build.build()
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()                                       # never read: every call below is refused before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)

    def refused(name, good, cases):
        for c in cases:
            a = dict(good, **c)
            assert getattr(lib, name)(*a.values()) == 1, (name, c)
            assert lib.sylber_last_error().decode().startswith(name + ": "), (name, c)

    refused("sylber_ivfpq_scan_residual",
            dict(lut=p, n=1, probe=p, nprobe=1, off=p, nlist=1, code=p, bad=p, rid=p, NL=1, M=2, m=1, qg=None, xg=None, splits=0, a=p,
                 nrm=p, t=p, cand=p, ws=p, stream=None),
            [dict(lut=None), dict(probe=None), dict(off=None), dict(code=None), dict(rid=None), dict(a=None), dict(t=None), dict(cand=None),
             dict(ws=None), dict(n=0), dict(n=-3), dict(M=0), dict(M=65), dict(m=0), dict(m=129), dict(nprobe=0), dict(nprobe=129),
             dict(nlist=0), dict(NL=-1), dict(qg=p), dict(xg=p), dict(splits=-1)])
    refused("sylber_ivfpq_list_terms", dict(q=p, n=1, D=32, cent=p, nlist=1, probe=p, nprobe=1, a=p, stream=None),
            [dict(q=None), dict(cent=None), dict(probe=None), dict(a=None), dict(n=0), dict(D=0), dict(D=30), dict(nlist=0), dict(nprobe=0),
             dict(nprobe=129)])
    for name in ("sylber_ivfpq_recon_norms", "sylber_ivfpq_decode"):
        refused(name, dict(code=p, n=1, lists=p, cent=p, nlist=1, cb=p, M=2, D=32, out=p, stream=None),
                [dict(code=None), dict(lists=None), dict(cent=None), dict(cb=None), dict(out=None), dict(n=0), dict(nlist=0), dict(M=0),
                 dict(M=65), dict(M=3), dict(M=4), dict(D=0)])

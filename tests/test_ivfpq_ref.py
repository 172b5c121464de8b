"""CPU tier: the numpy restatement of the compressed inverted-file search (tests/ivfpq_ref.py) is itself checked -- with every list
probed it is pq_ref.search, with fewer it is an explicit loop over the rows of the probed lists -- and the C entry points refuse bad
arguments before they touch a device."""
import ctypes

import numpy as np
import pytest

import ivfpq_ref as F
import knn_ref as R
import pq_ref as P


def _case(seed, N, D, M, n, nlist, metric):
    rng = np.random.default_rng(seed)
    q, x, C = P.clustered(seed, N, D, M, n, noise=0.4)
    xs, qs = P.stored(x, metric), P.stored(q, metric)
    cent = xs[rng.permutation(N)[:nlist]] * (1 + 0.01 * rng.standard_normal((nlist, D)).astype(np.float32))      # near stored rows
    return q, x, C, cent, F.assign(xs, cent), qs, rng.integers(0, 3, N), rng.integers(0, 3, n)


@pytest.mark.parametrize("rerank", [True, False])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_every_list_probed_is_the_pq_reference(metric, rerank):
    """with nprobe == nlist the composition is the product-quantized search itself (D = 64, M = 4, N = 6 000, 12 lists, 40 queries)"""
    q, x, C, cent, labels, qs, xg, qg = _case(11, 6000, 64, 4, 40, 12, metric)
    assert labels.min() >= 0 and len(np.unique(labels)) == 12
    probe = F.probe_lists(qs, cent, 12)
    assert np.array_equal(np.sort(probe, 1), np.tile(np.arange(12), (40, 1)))
    for kw in ({}, dict(q_group=qg, x_group=xg)):
        got = F.search(q, x, C, 10, labels, probe, 4, metric, rerank, **kw)
        want = P.search(q, x, C, 10, 4, metric, rerank, **kw)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    if metric == "l2":                      # a NaN row is in no list and is masked by the PQ rule as well; a NaN query probes nothing
        xb, qb = x.copy(), q.copy()
        xb[[5, 77]] = np.nan
        qb[3] = np.nan
        lab = F.assign(xb, cent)
        assert lab[5] == -1 and lab[77] == -1
        probe = F.probe_lists(qb, cent, 12)
        assert (probe[3] == -1).all()
        got = F.search(qb, xb, C, 10, lab, probe, 4, metric, rerank)
        want = P.search(qb, xb, C, 10, 4, metric, rerank)
        for a, b in zip(got, want):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        assert (got[1][3] == -1).all() and np.isinf(got[0][3]).all() and not np.isin([5, 77], got[2]).any()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_fewer_lists_is_brute_force_over_their_rows(metric):
    q, x, C, cent, labels, qs, xg, qg = _case(12, 700, 32, 2, 15, 9, metric)
    labels[labels == 4] = 3                                              # list 4 is empty
    codes, bad = P.encode(P.stored(x, metric), C)
    table = P.lut(qs, C, metric)
    full = R.scores(q, x, metric)
    for nprobe in (1, 3):
        probe = F.probe_lists(qs, cent, nprobe)
        probe[2, 0] = -1                                                 # a slot without a list
        for grouped in (False, True):
            kw = dict(q_group=qg, x_group=xg) if grouped else {}
            s, i, cand = F.search(q, x, C, 5, labels, probe, 4, metric, True, **kw)
            ss, si, scand = F.search(q, x, C, 5, labels, probe, metric=metric, rerank=False, **kw)
            assert cand.shape == (15, 20) and scand.shape == (15, 5) and np.array_equal(si, scand)
            for r in range(15):
                rows = [j for j in range(700) if labels[j] in set(probe[r][probe[r] >= 0].tolist()) and not (grouped and xg[j] == qg[r])]
                tt = []
                for j in rows:
                    acc = table[r, 0, codes[j, 0]]
                    for m in range(1, 2):
                        acc = acc + table[r, m, codes[j, m]]
                    tt.append(acc)
                by_t = [j for _, j in sorted(zip(tt, rows))]
                want = by_t[:20] + [-1] * (20 - len(by_t[:20]))
                assert cand[r].tolist() == want and scand[r].tolist() == want[:5]
                # the re-ranked list is the exact order over the candidate set
                c = np.array(by_t[:20], np.int64)
                top = c[np.lexsort((c, full[r, c]))][:5].tolist()
                assert i[r].tolist() == top + [-1] * (5 - len(top))
                assert np.isinf(s[r][len(top):]).all() and np.isinf(ss[r][len(by_t[:5]):]).all()
    # the order is (t, original id) whatever list a row is in: a copy of query 0's best row, with the largest id and in another list,
    # ties with it
    every = np.tile(np.arange(9), (15, 1))
    b = int(F.search(q, x, C, 1, labels, every, metric=metric, rerank=False)[2][0, 0])
    lab2 = np.concatenate([labels, [(labels[b] + 1) % 9]])
    x2 = np.concatenate([x, x[b:b + 1]])
    t = P.scan_t(table, np.concatenate([codes, codes[b:b + 1]]))
    _, _, cand = F.search(q, x2, C, 128, lab2, every, 1, metric)
    for r in range(15):
        c = cand[r]
        assert (c >= 0).all() and c.tolist() == c[np.lexsort((c, t[r, c]))].tolist()
    c = cand[0]
    assert c[0] == b and np.isin(700, c) and t[0, b] == t[0, 700] and (t[0, c[:np.nonzero(c == 700)[0][0]]] == t[0, b]).all()


def test_entry_points_refuse_bad_arguments_without_a_device():
    from sylber_amd import build, _lib
    build.build()
    lib = _lib.load()
    wb = lib.sylber_ivfpq_workspace_bytes
    assert wb(70, 8, 40, 0) > 0 and wb(70, 8, 40, 3) > 0 and wb(1, 128, 128, 0) > 0
    for bad in ((0, 8, 40, 0), (70, 0, 40, 0), (70, 129, 40, 0), (70, 8, 0, 0), (70, 8, 129, 0), (70, 8, 40, -1)):
        assert wb(*bad) == -1, bad
    # automatic splits: about 512 workgroups, never more than nprobe; the bytes are those of the lists [n][S][m] and [n][ceil(S/2)][m]
    al = lambda b: (b + 255) // 256 * 256
    for n, nprobe, m, splits, S in ((1, 128, 40, 0, 128), (100, 32, 10, 0, 6), (512, 8, 10, 0, 1), (9000, 8, 10, 0, 1), (70, 8, 40, 3, 3),
                                    (70, 2, 40, 7, 2), (3, 8, 128, 0, 8)):
        assert wb(n, nprobe, m, splits) == 2 * al(n * S * m * 4) + 2 * al(n * ((S + 1) // 2) * m * 4), (n, nprobe, m, splits)
    buf = (ctypes.c_char * 4096)()                                       # never read: every call below is refused before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(lut=p, n=1, probe=p, nprobe=1, off=p, nlist=1, code=p, bad=p, rid=p, NL=1, M=2, m=1, qg=None, xg=None, splits=0, t=p,
                cand=p, ws=p, stream=None)
    cases = [dict(lut=None), dict(probe=None), dict(off=None), dict(code=None), dict(rid=None), dict(t=None), dict(cand=None),
             dict(ws=None), dict(n=0), dict(n=-3), dict(M=0), dict(M=65), dict(m=0), dict(m=129), dict(nprobe=0), dict(nprobe=129),
             dict(nlist=0), dict(qg=p), dict(xg=p), dict(splits=-1)]
    for c in cases:
        a = dict(good, **c)
        assert lib.sylber_ivfpq_scan(*a.values()) == 1, c
        assert lib.sylber_last_error().decode().startswith("sylber_ivfpq_scan: "), c

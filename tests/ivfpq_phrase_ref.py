"""numpy restatement of phrase search on the compressed inverted file (``sylber_amd.pq.IVFPQSyllableIndex.search_phrases``): seed,
vote, exact DTW.  It adds no arithmetic of its own; it composes

* stage 1a: tests/ivfpq_ref.py (codes of the rows) or tests/ivfpq_residual_ref.py (codes of the residuals to the list centroids):
  ``search(all phrase rows, k=seeds, refine=1, rerank=rerank)`` over each row's ``nprobe`` nearest lists, scores as reported;
* stage 1b: tests/phrase_vote_ref.py ``vote`` on those seeds, ``m = k * refine`` candidates per phrase;
* stage 2: tests/dtw_ref.py ``dtw`` in fp32 of every candidate, on the stored rows (``rerank=True``) or on the reconstruction
  ``xhat`` that ``ix.decode`` returns (``rerank=False``: pq_ref ``decode``, for residual codes ivfpq_residual_ref ``reconstruct``; a
  masked row is a NaN row, ``+inf`` against every phrase row), ranked by ``dtw_ref.rank``;
* ``align``: tests/align_ref.py on the same local costs.

``bound`` ranks candidates and certifies nothing: with ``rerank=False`` the seeds' scores are sums of table entries, not the ``d`` of
the DTW, and with ``rerank=True`` the seeds are not each row's nearest rows.

The planted settings are fixed here: ``phrase_vote_ref.planted_case()``, ``M = 2``, the case's own 8 centroids, ``k = 2``,
``refine = 4``, codebooks sampled from the rows (or from their residuals)."""
import numpy as np

import align_ref as A
import dtw_ref as T
import ivfpq_ref as F
import ivfpq_residual_ref as RR
import phrase_vote_ref as V
import pq_ref as P

M, K, REFINE = 2, 2, 4
SETTINGS = ((1, 8), (3, 8), (3, 32), (8, 32))          # (nprobe, seeds) at which the planted phrases come first


def planted_index(residual, seed=3, case=None):
    """the planted case as an index: dict(case..., labels, codebooks, codes, bad, xhat (masked rows NaN), residual)"""
    c = dict(case if case is not None else V.planted_case())
    x, cent = c["x"], c["centroids"]
    labels = F.assign(x, cent)
    if residual:
        C = RR.sampled_codebooks(RR.residuals(x, cent, labels), M, seed)
        codes, bad = RR.encode(x, cent, labels, C)
        xhat = RR.reconstruct(codes, labels, cent, C)
    else:
        C = RR.sampled_codebooks(x, M, seed)
        codes, bad = P.encode(x, C)
        xhat = P.decode(codes, C).astype(np.float32)
    xhat = np.where(np.asarray(bad, bool)[:, None], np.float32(np.nan), xhat).astype(np.float32)
    c.update(labels=labels, codebooks=C, codes=codes, bad=bad, xhat=xhat, residual=residual)
    return c


def seeds_of(ix, q, nprobe, seeds, rerank, metric="l2", q_group=None):
    """stage 1a -> (scores fp32 [R, seeds], ids int64 [R, seeds]) as ``ix.search(q, seeds, nprobe, refine=1, rerank=rerank)`` reports them"""
    probe = F.probe_lists(P.stored(q, metric), ix["centroids"], nprobe)
    kw = dict(refine=1, metric=metric, rerank=rerank, q_group=q_group, x_group=ix["groups"] if q_group is not None else None)
    if ix["residual"]:
        sc, ids, _ = RR.search(q, ix["x"], ix["centroids"], ix["codebooks"], seeds, ix["labels"], probe, **kw)
    else:
        sc, ids, _ = F.search(q, ix["x"], ix["codebooks"], seeds, ix["labels"], probe, **kw)
    return np.asarray(sc, np.float32), np.asarray(ids, np.int64)


def rerank_rows(ix, rerank, metric="l2"):
    """the rows stage 2 runs on, as the index holds them"""
    return P.stored(ix["x"], metric) if rerank else ix["xhat"]


def exact(rows, phrases, cand, offsets, k, metric="l2"):
    """stage 2: the fp32 DTW of every candidate on ``rows`` -> (costs [P, k], seqs [P, k], spans [P, k, 2])"""
    off = np.asarray(offsets, np.int64)
    S = off.size - 1
    out = []
    for p, ph in enumerate(phrases):
        q = P.stored(ph, metric)
        costs, starts, ends = np.full(S, np.inf, np.float32), np.zeros(S, np.int64), np.zeros(S, np.int64)
        for s in cand[p][cand[p] >= 0]:
            costs[s], starts[s], ends[s] = T.dtw(T.local_costs(q, rows[off[s]:off[s + 1]], metric), np.float32)
        out.append(T.rank(costs, starts, ends, off[:-1], k))
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def search_phrases(ix, phrases, k, nprobe, seeds, refine, rerank, metric="l2", offsets=None, phrase_group=None):
    """the whole call -> (costs, seqs, spans, cand int32 [P, m], bound fp32 [P, m]); default sequences: the case's own, whose groups
    are the sequence numbers"""
    off = ix["offsets"] if offsets is None else np.asarray(offsets, np.int64)
    lens = np.array([len(p) for p in phrases])
    rows = np.cumsum(lens) - lens
    own = phrase_group is not None and offsets is None
    sc, ids = seeds_of(ix, np.concatenate(phrases), nprobe, seeds, rerank, metric, np.repeat(phrase_group, lens) if own else None)
    sg = ix["groups"][off[:-1]] if phrase_group is not None else None
    cand, bound = V.vote(sc, ids, rows, lens, off, metric, k * refine, phrase_group, sg)
    return exact(rerank_rows(ix, rerank, metric), phrases, cand, off, k, metric) + (cand, bound)


def align(ix, phrases, spans, rerank, metric="l2"):
    """align_ref.align_phrases on the rows stage 2 ran on"""
    rows = rerank_rows(ix, rerank, metric)
    lens = np.array([len(p) for p in phrases])
    qs = [P.stored(ph, metric) for ph in phrases]
    return A.align_phrases(lambda p, a, b: T.local_costs(qs[p], rows[a:b], metric), lens, spans)


def abi_refusals():
    """(entry, a good argument list by name, the overrides that each make it return 1) for ``sylber_dtw_rerank_codes`` and
    ``sylber_dtw_align_codes``: every refusal comes before a launch, so the pointers (4096) are never dereferenced"""
    p = 4096
    db = dict(code=p, bad=p, pos=p, cb=p, M=4, off=p, cent=p, nlist=5)
    head = dict(q=p, nb=1, qn=p, prow=p, plen=p, P=3)
    rerank = dict(head, **db, N=100, D=64, cn=p, metric=0, cand=p, m=12, soff=p, S=7, k=3, cost=p, seq=p, span=p, ws=p, stream=None)
    align = dict(head, **db, N=100, D=64, cn=p, metric=0, pp=p, win=p, n=5, max_cols=8, max_rows=3, rows=p, steps=p, costs=p, start=None,
                 ws=p, stream=None)
    shared = [dict(q=None), dict(prow=None), dict(plen=None), dict(code=None), dict(cb=None), dict(ws=None), dict(nb=0), dict(P=0), dict(N=0),
              dict(D=8), dict(D=72), dict(metric=2), dict(cn=None), dict(qn=None), dict(M=0), dict(M=65), dict(M=3), dict(M=8), dict(D=1024, M=128),
              dict(off=None), dict(cent=None), dict(nlist=0), dict(nlist=-1), dict(off=None, cent=None), dict(off=None, nlist=0),
              dict(cent=None, nlist=0)]
    return (("sylber_dtw_rerank_codes", rerank, shared + [dict(cand=None), dict(soff=None), dict(cost=None), dict(seq=None), dict(span=None),
                                                          dict(S=0), dict(m=0), dict(m=129), dict(k=0), dict(k=13)]),
            ("sylber_dtw_align_codes", align, shared + [dict(pp=None), dict(win=None), dict(rows=None), dict(steps=None), dict(costs=None),
                                                        dict(n=0), dict(max_cols=0), dict(max_cols=65537), dict(max_rows=0), dict(max_rows=65)]))

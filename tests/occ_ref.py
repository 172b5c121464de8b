"""numpy restatement of "Every occurrence of a phrase" (include/sylber_hip.h; sylber_amd.SyllableIndex.search_occurrences /
search_occurrences_refined, csrc/dtw.hip and csrc/dtw16.hip), on top of tests/dtw_ref.py: local costs, the recurrence, the
predecessor order on ties, ``start[i][j]`` and the NaN -> ``+inf`` rule are ``dtw_ref``'s.

For one phrase (m rows) and one sequence (columns 0 .. L - 1), ``E[j] = A[m-1][j]`` and ``st[j] = start[m-1][j]``:

1. Families: only columns with ``E[j] < +inf`` count; columns with equal ``st[j]`` form a family with ``start = st[j]``,
   ``cost = min E[j]``, ``end`` = the smallest such j.  ``st`` does not decrease over the finite columns, so a family is a run of
   neighbouring finite columns (``families`` groups neighbours; ``test_occ_ref`` checks that no family is split by it).
2. One left-to-right pass: the first family becomes pending; a later family ``F`` with ``F.start <= pending.end`` competes with
   it (the cheaper stays, the pending one on equal cost), otherwise the pending one is emitted and ``F`` becomes pending; at the
   sequence end the pending one is emitted.
3. Per phrase: the k best emitted occurrences over the admissible sequences by (cost, first row id), padded with
   ``(+inf, -1, (-1, -1))``.

This is not global greedy suppression by cost (``greedy``): see ``test_occ_ref.test_one_pass_is_not_greedy_suppression``."""
import numpy as np

import dtw_ref


def last_row(d, dtype=np.float32):
    """``(E [L], st [L])`` of the recurrence, one anti-diagonal at a time as ``dtw_ref.dtw`` evaluates it (the same additions);
    ``st`` of a column with ``E = +inf`` means nothing"""
    d = dtw_ref._clean(d, dtype)
    m, L = d.shape
    inf = dtype(np.inf)
    ii = np.arange(m)
    p1, p2 = np.full(m, inf, dtype), np.full(m, inf, dtype)        # A[i][t - 1 - i], A[i][t - 2 - i]
    s1, s2 = np.zeros(m, np.int64), np.zeros(m, np.int64)
    last, lstart = np.full(L, inf, dtype), np.zeros(L, np.int64)
    for t in range(m + L - 1):
        j = t - ii
        ok = (j >= 0) & (j < L)
        dv = d[ii, np.clip(j, 0, L - 1)]
        best = np.concatenate([[inf], p2[:-1]]).astype(dtype)      # diagonal
        bs = np.concatenate([[0], s2[:-1]])
        up, su = np.concatenate([[inf], p1[:-1]]).astype(dtype), np.concatenate([[0], s1[:-1]])
        mk = up < best
        best[mk], bs[mk] = up[mk], su[mk]
        mk = p1 < best                                             # left
        best[mk], bs[mk] = p1[mk], s1[mk]
        cur = (dv + best).astype(dtype)
        cur[0], bs[0] = dv[0], j[0]
        cur[~ok] = inf
        if ok[m - 1]:
            last[j[m - 1]], lstart[j[m - 1]] = cur[m - 1], bs[m - 1]
        p2, s2, p1, s1 = p1, s1, cur, bs
    return last, lstart


def last_row_loop(d, dtype=np.float32):
    """the same cell by cell, as the contract writes it"""
    d = dtw_ref._clean(d, dtype)
    m, L = d.shape
    inf = dtype(np.inf)
    A = np.full((m, L), inf, dtype)
    S = np.zeros((m, L), np.int64)
    for i in range(m):
        for j in range(L):
            if i == 0:
                A[i, j], S[i, j] = d[i, j], j
                continue
            best, bs = (A[i - 1, j - 1], S[i - 1, j - 1]) if j > 0 else (inf, 0)
            if A[i - 1, j] < best:
                best, bs = A[i - 1, j], S[i - 1, j]
            if j > 0 and A[i, j - 1] < best:
                best, bs = A[i, j - 1], S[i, j - 1]
            A[i, j], S[i, j] = dtype(d[i, j] + best), bs
    return A[m - 1], S[m - 1]


def families(E, st):
    """rule 1 -> [(cost, start, end)] in column order: neighbouring finite columns of equal start"""
    out = []
    for j in np.nonzero(E < np.inf)[0]:
        if out and out[-1][1] == st[j]:
            if E[j] < out[-1][0]:
                out[-1] = (E[j], int(st[j]), int(j))
        else:
            out.append((E[j], int(st[j]), int(j)))
    return out


def one_pass(fams):
    """rule 2 -> the emitted occurrences [(cost, start, end)], in column order"""
    out, pending = [], None
    for f in fams:
        if pending is None:
            pending = f
        elif f[1] <= pending[2]:
            if f[0] < pending[0]:
                pending = f
        else:
            out.append(pending)
            pending = f
    if pending is not None:
        out.append(pending)
    return out


def one_pass_columns(E, st):
    """rule 2 with every finite column offered by itself as (E[j], st[j], j), families never formed: the form with one pending
    occurrence as the only state, which the kernels run.  Equal to ``one_pass(families(E, st))``."""
    out, pending = [], None
    for j in np.nonzero(E < np.inf)[0]:
        f = (E[j], int(st[j]), int(j))
        if pending is not None and f[1] > pending[2]:
            out.append(pending)
            pending = f
        elif pending is None or f[0] < pending[0]:
            pending = f
    if pending is not None:
        out.append(pending)
    return out


def greedy(fams):
    """what the contract is NOT: global suppression, families taken by (cost, start) ascending, one kept when it shares no row
    with any kept before"""
    kept = []
    for f in sorted(fams, key=lambda f: (f[0], f[1])):
        if all(f[2] < g[1] or g[2] < f[1] for g in kept):
            kept.append(f)
    return sorted(kept, key=lambda f: f[1])


def occurrences(d, dtype=np.float32):
    """one phrase against one sequence -> [(cost, start column, end column)]"""
    return one_pass(families(*last_row(d, dtype)))


def rank(occ, offsets, k, admissible=None, dtype=np.float32):
    """one phrase's list from ``occ[s]`` = the occurrences of sequence s (columns relative to it) -> (costs [k], seqs [k],
    spans [k, 2]) by (cost, first row id)"""
    S = len(offsets) - 1
    adm = np.ones(S, bool) if admissible is None else np.asarray(admissible, bool)
    ent = [(c, int(offsets[s]) + a, int(offsets[s]) + e + 1, s) for s in range(S) if adm[s] for c, a, e in occ[s]]
    ent.sort(key=lambda t: (t[0], t[1]))
    ent = ent[:k]
    oc = np.full(k, np.inf, dtype)
    os_ = np.full(k, -1, np.int64)
    sp = np.full((k, 2), -1, np.int64)
    for i, (c, a, e, s) in enumerate(ent):
        oc[i], os_[i], sp[i] = c, s, (a, e)
    return oc, os_, sp


def search_occurrences(d_of, phrase_count, offsets, k, dtype=np.float32, phrase_groups=None, seq_groups=None, only=None):
    """the whole contract from ``d_of(p, s) -> d [m_p, L_s]`` -> (costs [P, k], seqs [P, k], spans [P, k, 2], counts [P]);
    ``only[p]``: the sequences searched for phrase p (the refined call's candidates; negative entries are padding);
    ``counts[p]``: how many occurrences phrase p has before the cut at k"""
    S = len(offsets) - 1
    C, Q, SP, n = [], [], [], []
    for p in range(phrase_count):
        adm = np.ones(S, bool) if phrase_groups is None else np.asarray(seq_groups) != phrase_groups[p]
        if only is not None:
            o = np.asarray(only[p])
            adm &= np.isin(np.arange(S), o[o >= 0])
        occ = [occurrences(d_of(p, s), dtype) if adm[s] else [] for s in range(S)]
        n.append(sum(len(o) for o in occ))
        c, q, sp = rank(occ, offsets, k, adm, dtype)
        C.append(c); Q.append(q); SP.append(sp)
    return np.stack(C), np.stack(Q), np.stack(SP), np.array(n)

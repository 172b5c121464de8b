"""numpy restatement of "Unit search" (include/sylber_hip.h; sylber_amd.UnitIndex.search_phrases / search_occurrences,
csrc/unit_search.hip): semi-global edit distance of phrases of syllable unit ids against sequences of them.

A unit is a row of ``W`` non-negative ids.  For phrase unit ``p_i`` (i = 0 .. m-1) and sequence unit ``t_j`` (j = 0 .. L-1), int32::

    sub(i, j) = number of columns c with p_i[c] != t_j[c];   an insertion or a deletion costs W
    E[-1][j] = 0,           start[-1][j] = j + 1     (j = -1 .. L-1)
    E[i][-1] = (i + 1) W,   start[i][-1] = 0
    E[i][j]  = min(E[i-1][j-1] + sub(i, j), E[i-1][j] + W, E[i][j-1] + W), the first smallest in that order;
               start[i][j] = start of the predecessor taken

A column of the last row is admissible when ``E[m-1][j] <= thr = min(max_cost, m W - 1)``.  ``search_phrases``: per pair the
smallest admissible cost, the smallest such column, its start; per phrase the k best sequences by (cost, sequence).
``search_occurrences``: families of admissible columns with equal start, the one-pass rule of tests/occ_ref.py, per phrase the k
best by (cost, first row id).  Padding ``(2**31 - 1, -1, (-1, -1))``.

``last_rows`` evaluates all (phrase, sequence) pairs at once, one anti-diagonal per step (vector over pairs and phrase rows, each
cell with the contract's order of comparisons); ``last_row_loop`` is the same cell by cell, as the contract writes it."""
import numpy as np

PAD = 2 ** 31 - 1


def as_units(a):
    """[n] or [n, W] -> int64 [n, W]"""
    a = np.asarray(a, np.int64)
    return a[:, None] if a.ndim == 1 else a


def last_row_loop(p, t):
    """one phrase [m, W] against one sequence [L, W], cell by cell -> (E [L], start [L]) of the last row"""
    p, t = as_units(p), as_units(t)
    m, L, W = p.shape[0], t.shape[0], p.shape[1]
    E = np.zeros((m + 1, L + 1), np.int64)                 # E[i + 1][j + 1] = the contract's E[i][j]
    S = np.zeros((m + 1, L + 1), np.int64)
    S[0] = np.arange(L + 1)                                # start[-1][j] = j + 1
    E[1:, 0] = (np.arange(m) + 1) * W
    for i in range(1, m + 1):
        for j in range(1, L + 1):
            best, bs = E[i - 1, j - 1] + int((p[i - 1] != t[j - 1]).sum()), S[i - 1, j - 1]
            if E[i - 1, j] + W < best:
                best, bs = E[i - 1, j] + W, S[i - 1, j]
            if E[i, j - 1] + W < best:
                best, bs = E[i, j - 1] + W, S[i, j - 1]
            E[i, j], S[i, j] = best, bs
    return E[m, 1:], S[m, 1:]


def last_row_scan(p, t):
    """``last_row_loop`` one phrase row at a time, for one long sequence: along a row ``E[j] = min(c[j], E[j-1] + W)`` with
    ``c[j]`` the better of the diagonal and the upper term (the diagonal on ties), so ``E[j] = min over j' <= j of
    c[j'] + (j - j') W``, a running minimum; the left term loses ties, which makes the origin the LATEST ``j'`` that attains it"""
    p, t = as_units(p), as_units(t)
    m, L, W = p.shape[0], t.shape[0], p.shape[1]
    E, S = np.zeros(L + 1, np.int64), np.arange(L + 1)     # index j + 1; row -1: 0 with start j + 1
    jj, pos = np.arange(-1, L), np.arange(L + 1)
    for i in range(m):
        cd, cu = E[:-1] + (p[i][None, :] != t).sum(1), E[1:] + W
        up = cu < cd
        c, sc = np.where(up, cu, cd), np.where(up, S[1:], S[:-1])
        key = np.concatenate([[(i + 1) * W], c]) - jj * W  # column -1 is (i + 1) W with start 0
        cm = np.minimum.accumulate(key)
        org = np.maximum.accumulate(np.where(key == cm, pos, -1))
        E, S = cm + jj * W, np.concatenate([[0], sc])[org]
    return E[1:], S[1:]


def last_rows(phrases, seqs):
    """every phrase (list of [m_p, W]) against every sequence (list of [L_s, W]) -> (E, ST) int64 [P, S, Lmax]; the columns at or
    past a sequence's length mean nothing"""
    phrases, seqs = [as_units(p) for p in phrases], [as_units(t) for t in seqs]
    P, S, W = len(phrases), len(seqs), phrases[0].shape[1]
    plen, tlen = np.array([p.shape[0] for p in phrases]), np.array([t.shape[0] for t in seqs])
    M, Lm = int(plen.max()), int(tlen.max())
    pu = np.full((P, M, W), -1, np.int64)
    tu = np.full((S, Lm, W), -2, np.int64)
    for a, p in enumerate(phrases):
        pu[a, :p.shape[0]] = p
    for a, t in enumerate(seqs):
        tu[a, :t.shape[0]] = t
    ii = np.arange(M)
    # lane i = phrase row i; before its first column it holds column -1: E[i][-1] = (i + 1) W, start 0
    p1 = np.broadcast_to(((ii + 1) * W)[None, None, :], (P, S, M)).copy()
    s1 = np.zeros((P, S, M), np.int64)
    p2, s2 = p1.copy(), s1.copy()
    E = np.zeros((P, S, Lm), np.int64)
    ST = np.zeros((P, S, Lm), np.int64)
    ar = np.arange(P)
    zero = np.zeros((P, S, 1), np.int64)
    for t in range(Lm + M - 1):
        j = t - ii
        ok = (j >= 0) & (j < Lm)
        sub = (pu[:, None, :, :] != tu[None, :, np.clip(j, 0, Lm - 1), :]).sum(-1)          # [P, S, M]
        best = np.concatenate([zero, p2[:, :, :-1]], 2) + sub                              # diagonal; row -1: 0 with start j = t
        bs = np.concatenate([zero + t, s2[:, :, :-1]], 2)
        up = np.concatenate([zero, p1[:, :, :-1]], 2) + W                                  # (i-1, j); row -1: 0 with start j + 1
        su = np.concatenate([zero + t + 1, s1[:, :, :-1]], 2)
        mk = up < best
        best[mk], bs[mk] = up[mk], su[mk]
        left = p1 + W                                                                      # (i, j-1)
        mk = left < best
        best[mk], bs[mk] = left[mk], s1[mk]
        p2, s2 = p1, s1
        p1, s1 = np.where(ok, best, p1), np.where(ok, bs, s1)
        jl = t - (plen - 1)                                                                # the column of each phrase's last row
        w = (jl >= 0) & (jl < Lm)
        E[ar[w], :, jl[w]] = p1[ar[w], :, plen[w] - 1]
        ST[ar[w], :, jl[w]] = s1[ar[w], :, plen[w] - 1]
    return E, ST


def thresholds(phrases, W, max_cost=None):
    m = np.array([as_units(p).shape[0] for p in phrases])
    cap = m * W - 1
    return cap if max_cost is None else np.minimum(np.broadcast_to(np.asarray(max_cost, np.int64), m.shape), cap)


def best_match(E, st, thr):
    """search_phrases for one pair -> (cost, start, end) or None"""
    c = int(E.min())
    if c > thr:
        return None
    e = int(np.argmax(E == c))
    return c, int(st[e]), e


def families(E, st, thr):
    """[(cost, start, end)] in column order: the admissible columns grouped by start"""
    out = []
    for j in np.nonzero(E <= thr)[0]:
        if out and out[-1][1] == st[j]:
            if E[j] < out[-1][0]:
                out[-1] = (int(E[j]), int(st[j]), int(j))
        else:
            out.append((int(E[j]), int(st[j]), int(j)))
    return out


def one_pass(fams):
    """the emitted occurrences [(cost, start, end)], in column order"""
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


def one_pass_columns(E, st, thr):
    """the one-pass rule with every admissible column offered by itself as (E[j], start[j], j): the form the kernel runs"""
    out, pending = [], None
    for j in np.nonzero(E <= thr)[0]:
        f = (int(E[j]), int(st[j]), int(j))
        if pending is not None and f[1] > pending[2]:
            out.append(pending)
            pending = f
        elif pending is None or f[0] < pending[0]:
            pending = f
    if pending is not None:
        out.append(pending)
    return out


def _pad(ent, k):
    c = np.full(k, PAD, np.int32)
    q = np.full(k, -1, np.int64)
    sp = np.full((k, 2), -1, np.int64)
    for i, (cost, a, e, s) in enumerate(ent[:k]):
        c[i], q[i], sp[i] = cost, s, (a, e)
    return c, q, sp


def _search(corpus, offsets, phrases, k, occurrences, max_cost=None, phrase_groups=None, seq_groups=None, rows=None):
    corpus = as_units(corpus)
    offsets = np.asarray(offsets, np.int64)
    W, S = corpus.shape[1], len(offsets) - 1
    seqs = [corpus[offsets[s]:offsets[s + 1]] for s in range(S)]
    thr = thresholds(phrases, W, max_cost)
    E, ST = rows if rows is not None else last_rows(phrases, seqs)
    C, Q, SP, counts = [], [], [], []
    for p in range(len(phrases)):
        ent = []
        for s in range(S):
            if phrase_groups is not None and seq_groups[s] == phrase_groups[p]:
                continue
            L, o = int(offsets[s + 1] - offsets[s]), int(offsets[s])
            e, st = E[p, s, :L], ST[p, s, :L]
            if occurrences:
                ent += [(c, o + a, o + b + 1, s) for c, a, b in one_pass(families(e, st, thr[p]))]
            else:
                b = best_match(e, st, thr[p])
                if b is not None:
                    ent.append((b[0], o + b[1], o + b[2] + 1, s))
        ent.sort(key=(lambda x: (x[0], x[1])) if occurrences else (lambda x: (x[0], x[3])))
        counts.append(len(ent))
        c, q, sp = _pad(ent, k)
        C.append(c); Q.append(q); SP.append(sp)
    return np.stack(C), np.stack(Q), np.stack(SP), np.array(counts)


def search_phrases(corpus, offsets, phrases, k, **kw):
    """-> (costs int32 [P, k], seqs int64 [P, k], spans int64 [P, k, 2], counts [P]: the entries before the cut at k)"""
    return _search(corpus, offsets, phrases, k, False, **kw)


def search_occurrences(corpus, offsets, phrases, k, **kw):
    return _search(corpus, offsets, phrases, k, True, **kw)

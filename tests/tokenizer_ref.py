"""Test-only float64 restatement, fp32 numpy restatement and error bounds of the code between segmentation and the decoder
(csrc/downstream.hip: k-means tokens, the learned quantizer's FFEncoder / unit norms / residual VQ, the conditioner's silence
decisions) and of the 64x64 ``gemm_f32_kernel`` (csrc/fp32_path.hip) underneath it.  Never imported by the product.

Bounds (u = 2^-24, gamma_k = k u / (1 - k u)):

* Linear ``y = x W^T + b`` as an ascending fp32 fmaf chain plus one add:
  ``|err| <= gamma_K (|x| |W|^T) + u (|x W^T| + |b|)``  (``linear_bound``).
* FFEncoder: a layer fed with inputs that are already off by ``e_in`` gives ``e_out = |W| e_in + (own bound at |x| + e_in)``; ReLU is
  1-Lipschitz, so the error passes through it unchanged -- an element whose float64 pre-activation lies inside its bound may thereby
  come out as 0 or as the value (``ffenc64`` returns the bound with the float64 output).
* Arg-min (one rule, ``judge_ids``): with ``bnd`` the row's largest ``knn_ref.dot_error_bound`` over the codebook (D = the padded
  width) and ``gap`` the second-best minus the best float64 score, ``gap > 2 bnd`` demands the float64 id; otherwise the chosen
  id's float64 score must lie within ``2 bnd`` of the best.  Ids outside ``[0, K)`` are always wrong.  Every row is judged.
* Unit norms ``x / sqrt(sum x^2 + c)``: relative error at most ``(D + 4) u`` per element (``NORM_REL``)."""
import numpy as np

import knn_ref

U = 2.0 ** -24
INT_MAX = 2 ** 31 - 1
EPS_LQ = float(np.float32(1e-5))       # the constants as the device holds them
EPS_KM = float(np.float32(1e-8))


def gamma(k):
    return k * U / (1 - k * U)


def NORM_REL(D):
    return (D + 4) * U


# ---- Linear / FFEncoder --------------------------------------------------------------------------------------------------------
def linear64(x, W, b):
    return np.asarray(x, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)


def linear_bound(x, W, b, e_in=None):
    """the Linear bound per element ``[M, N]``; with ``e_in`` (``[M, K]``, the error already in x) the propagated one"""
    ax, aW = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(W, np.float64))
    K = ax.shape[1]
    y = np.abs(linear64(x, W, np.zeros(len(aW))))
    if e_in is None:
        return gamma(K) * (ax @ aW.T) + U * (y + np.abs(np.asarray(b, np.float64)))
    prop = e_in @ aW.T
    return prop + gamma(K) * ((ax + e_in) @ aW.T) + U * (y + prop + np.abs(np.asarray(b, np.float64)))


def fma_chain32(x, W):
    """``x W^T`` as the device contracts it: one fp32 accumulator per output, k ascending, one rounding per step (the product of two
    fp32 values is exact in float64)"""
    x, W = np.asarray(x, np.float32), np.asarray(W, np.float32)
    acc = np.zeros((x.shape[0], W.shape[0]), np.float32)
    for k in range(x.shape[1]):
        acc = (x[:, k, None].astype(np.float64) * W[None, :, k].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def linear32(x, W, b, relu=False, steps=None):
    """fp32 restatement of one GEMM launch; ``steps`` < K drops the tail of the contraction (a planted defect)"""
    K = np.asarray(x).shape[1] if steps is None else steps
    y = (fma_chain32(np.asarray(x)[:, :K], np.asarray(W)[:, :K]) + np.asarray(b, np.float32)[None, :]).astype(np.float32)
    return np.maximum(y, np.float32(0)) if relu else y


def ffenc_layers(dims, weights):
    """[(W, b, relu)] in launch order for ``sylber_ffenc(num_hidden = len(dims) - 2)``: per hidden width Linear, Linear + ReLU,
    Linear; then the output Linear.  ``weights``: the flat [W0, b0, W1, b1, ...] list the C entry takes."""
    H = len(dims) - 2
    relus = [False, True, False] * H + [False]
    assert len(weights) == 2 * len(relus)
    return [(weights[2 * i], weights[2 * i + 1], relus[i]) for i in range(len(relus))]


def ffenc64(x, layers):
    """-> (float64 output, propagated bound) of the chain"""
    y = np.asarray(x, np.float64)
    e = np.zeros_like(y)
    for W, b, relu in layers:
        e = linear_bound(y, W, b, e)
        y = linear64(y, W, b)
        if relu:
            y = np.maximum(y, 0.0)
    return y, e


def ffenc32(x, layers):
    y = np.asarray(x, np.float32)
    for W, b, relu in layers:
        y = linear32(y, W, b, relu)
    return y


def judge_elements(got, ref, bound):
    """indices ``[m, 2]`` of the elements of ``got`` farther from ``ref`` than ``bound`` (or not finite)"""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - ref) <= bound)
    return np.argwhere(bad)


# ---- arg-min -------------------------------------------------------------------------------------------------------------------
def km_normalize64(x):
    x = np.asarray(x, np.float64)
    return x / np.sqrt((x * x).sum(1, keepdims=True) + EPS_KM) * 6.0


def km_normalize32(x, eps=1e-8):
    x = np.asarray(x, np.float32)
    s = (x.astype(np.float64) ** 2).sum(1, keepdims=True).astype(np.float32)
    return (x / np.sqrt(s + np.float32(eps)) * np.float32(6)).astype(np.float32)


def scores64(x, c):
    """``||c||^2 - 2 x.c`` in float64: the score every arg-min of the library ranks by"""
    return knn_ref.scores(x, c, "l2")


def row_bounds(x, c, D=None, norm_rel=0.0):
    """one bound per row: the largest ``dot_error_bound`` over the codebook; ``norm_rel`` adds the relative error the rows carry from
    a device normalisation in front (it scales ``2 x.c``)"""
    b = knn_ref.dot_error_bound(x, c, D)
    if norm_rel:
        b = b + 2.0 * norm_rel * (np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(c, np.float64)).T)
    return b.max(1)


def gaps(s):
    """(float64 arg-min with ties to the smallest index, second-best minus best) per row"""
    best = s.argmin(1)
    if s.shape[1] == 1:
        return best, np.full(len(s), np.inf)
    part = np.partition(s, 1, axis=1)
    return best, part[:, 1] - part[:, 0]


def judge_ids(s, bnd, ids, exact=False):
    """the id rule; -> list of (row, message), empty when every row passes.  ``exact``: the table is exact in fp32, the device must
    return the float64 arg-min with ties to the smallest index.  Rows whose float64 scores hold a NaN are the caller's."""
    n, K = s.shape
    ids = np.asarray(ids).astype(np.int64)
    bnd = np.broadcast_to(np.asarray(bnd, np.float64), (n,))
    best, gap = gaps(s)
    bad = []
    for r in range(n):
        if np.isnan(s[r]).any():
            continue
        i = int(ids[r])
        if not 0 <= i < K:
            bad.append((r, "id %d outside [0, %d)" % (i, K)))
        elif exact:
            if i != best[r]:
                bad.append((r, "id %d, exact arg-min %d (scores %r, %r)" % (i, best[r], s[r, i], s[r, best[r]])))
        elif gap[r] > 2 * bnd[r]:
            if i != best[r]:
                bad.append((r, "id %d, float64 id %d with gap %.3e > 2 x %.3e" % (i, best[r], gap[r], bnd[r])))
        elif s[r, i] - s[r, best[r]] > 2 * bnd[r]:
            bad.append((r, "id %d scores %.3e above the best, bound %.3e" % (i, s[r, i] - s[r, best[r]], bnd[r])))
    return bad


def argmin32(x, c, K=None, steps=None, larger_on_tie=False):
    """fp32 restatement of ``km_nearest``: dots on the fmaf chain, ``fmaf(-2, dot, ||c||^2)``, ties to the smallest index over the
    first K rows.  ``steps`` / ``larger_on_tie``: planted defects."""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    K = len(c) if K is None else K
    D = x.shape[1] if steps is None else steps
    dots = fma_chain32(x[:, :D], c[:, :D])
    cn = (c.astype(np.float64) ** 2).sum(1).astype(np.float32)
    d = (-2.0 * dots.astype(np.float64) + cn[None, :].astype(np.float64)).astype(np.float32)[:, :K]
    if larger_on_tie:
        return K - 1 - d[:, ::-1].argmin(1)
    return d.argmin(1)


def near_tie_rows(c, a, b, bound_of, score_of=None, target=8.0, iters=3):
    """rows ``x = (c_a + c_b) / 2 + eps (c_a - c_b)`` in fp32 with eps set per row so that the float64 gap between the scores of a and
    b is ``target`` times the row's bound.  ``bound_of(x) -> [n]``; ``score_of(x) -> [n, K]`` (default ``scores64(x, c)``).  The
    score difference is linear in eps up to the rounding of x, so a few secant steps on the rounded rows settle it."""
    c64 = np.asarray(c, np.float64)
    score_of = score_of or (lambda x: scores64(x, c))
    mid, dif = (c64[a] + c64[b]) / 2, c64[a] - c64[b]
    r = np.arange(len(a))

    def make(eps):
        return (mid + eps[:, None] * dif).astype(np.float32)

    def diff(x):
        s = score_of(x)
        return s[r, b] - s[r, a]
    e0, e1 = np.zeros(len(a)), np.full(len(a), 1e-3)
    d0, d1 = diff(make(e0)), diff(make(e1))
    for _ in range(iters):
        x = make(e1)
        want = target * bound_of(x)
        slope = np.where(d1 != d0, (d1 - d0) / np.where(e1 != e0, e1 - e0, 1.0), 1.0)
        e2 = e1 + (want - d1) / np.where(slope != 0, slope, 1.0)
        e0, d0, e1 = e1, d1, e2
        d1 = diff(make(e1))
    return make(e1)


def int_table(rng, n, K, D, lim=8):
    """tokens and codebook of integers |v| <= lim: with D <= 64 every dot product and norm is exact in fp32"""
    assert D <= 64 and lim <= 8
    return (rng.integers(-lim, lim + 1, (n, D)).astype(np.float32), rng.integers(-lim, lim + 1, (K, D)).astype(np.float32))


def random_tokens(rng, c, n, noise=0.7):
    c = np.asarray(c, np.float32)
    return (c[rng.integers(0, len(c), n)] + noise * rng.standard_normal((n, c.shape[1]))).astype(np.float32)


def km_bounds(x, c, normalize):
    """(float64 scores, one bound per row) of ``sylber_km_assign(normalize)`` for fp32 tokens x"""
    D = np.asarray(x).shape[1]
    xs = km_normalize64(x) if normalize else x
    return scores64(xs, c), row_bounds(xs, c, D, NORM_REL(D) if normalize else 0.0)


def near_ties(c, n, rng, normalize=False, exclude=()):
    """n near-tie rows between a random centroid (none of ``exclude``) and its nearest other one"""
    c64 = np.asarray(c, np.float64)
    ok = np.array([i for i in range(len(c)) if i not in set(exclude)])
    a = ok[rng.integers(0, len(ok), n)]
    d2 = ((c64[a][:, None, :] - c64[None, :, :]) ** 2).sum(-1)
    d2[np.arange(n), a] = np.inf
    d2[:, np.array(list(exclude), np.int64)] = np.inf
    b = d2.argmin(1)                                               # the nearest other centroid: the pair is then the row's two best
    if normalize:
        return near_tie_rows(c, a, b, lambda x: km_bounds(x, c, True)[1], lambda x: km_bounds(x, c, True)[0])
    return near_tie_rows(c, a, b, lambda x: km_bounds(x, c, False)[1])


KM_D, KM_K, KM_N = (16, 64, 768), (4, 5, 7, 8, 65, 257, 1002), (1, 63, 64, 65, 130)
KM_TIES = slice(2, 42)            # rows of km_pool that are near ties; rows 42.. are random tokens


def km_pool(D, K, normalize=False):
    """the k-means case of one (D, K): codebook ``c`` (rows of norm 6 under ``normalize``, where the tokens are scaled to that norm
    before the look-up) with duplicated rows planted -- 259 = 3 across the arg-min's 256-thread stride, K-1 = K-5 across the ragged
    K % 4 tail --, and 130 tokens: row 0 is the last centroid, row 1 is centroid 3, rows 2..41 are near ties, the rest
    ``c[pick] + 0.7 noise``.  -> (c, x, [(smaller, larger)] duplicated pairs).  The first n rows are the case of n tokens."""
    rng = np.random.default_rng(1000 * D + 2 * K + int(normalize))
    c = rng.standard_normal((K, D))
    if normalize:
        c = c / np.sqrt((c * c).sum(1, keepdims=True)) * 6.0
    c = c.astype(np.float32)
    dups = []
    if K > 259:
        c[259] = c[3]; dups.append((3, 259))
    if K % 4 and K >= 5:
        c[K - 1] = c[K - 5]; dups.append((K - 5, K - 1))
    x = random_tokens(rng, c, 130, 0.7 if not normalize else 0.7 * 6.0 / np.sqrt(D))
    x[0], x[1] = c[K - 1], c[3]
    x[KM_TIES] = near_ties(c, 40, rng, normalize, [i for p in dups for i in p])
    return c, x, dups


def km_second_book(D, K):
    """stage 2 of the residual form: the same K (so its ragged tail runs too) at the scale of the residuals"""
    return (0.6 * np.random.default_rng(77 * D + K).standard_normal((K, D))).astype(np.float32)


def linear_case(M, N, K, seed=0):
    """rows at scales 1e-3, 1 and 1e3; a bias that outweighs the dot product on every third column"""
    rng = np.random.default_rng(seed + 10000 * M + 100 * N + K)
    x = (rng.standard_normal((M, K)) * rng.choice([1e-3, 1.0, 1e3], (M, 1))).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = (rng.standard_normal(N) * np.where(np.arange(N) % 3 == 0, 1e4, 0.1)).astype(np.float32)
    return x, W, b


def ffenc_case(M, dims=(48, 80, 32), seed=4):
    """one hidden width: Linear(48, 80), Linear(80, 80) + ReLU, Linear(80, 80), Linear(80, 32) -> (x, flat weight list)"""
    rng = np.random.default_rng(seed)
    i, h, o = dims
    weights = []
    for a, b in ((h, i), (h, h), (h, h), (o, h)):
        weights += [(rng.standard_normal((a, b)) / np.sqrt(b)).astype(np.float32), (0.3 * rng.standard_normal(a)).astype(np.float32)]
    x = (rng.standard_normal((M, i)) * rng.choice([1e-3, 1.0, 1e3], (M, 1))).astype(np.float32)
    return x, weights


# ---- residual stacks -----------------------------------------------------------------------------------------------------------
def pad_books(books):
    """[Q][K, d] -> fp32 [Q, Kp, Dp], zero-padded the way ``sylber_rvq_*`` take them"""
    Q, (K, d) = len(books), books[0].shape
    out = np.zeros((Q, (K + 3) & ~3, (d + 15) & ~15), np.float32)
    for q, E in enumerate(books):
        out[q, :K, :d] = E
    return out


def rvq_sum32(ids, books, K):
    """z of ``sylber_rvq_assign`` / ``sylber_rvq_decode``: ``((0 + E_0[i_0]) + E_1[i_1]) + ...`` in fp32, ids clamped to [0, K)"""
    ids = np.clip(np.asarray(ids, np.int64), 0, K - 1)
    z = np.zeros((len(ids), books[0].shape[1]), np.float32)
    for q, E in enumerate(books):
        z = (z + np.asarray(E, np.float32)[ids[:, q]]).astype(np.float32)
    return z


def rvq_judge(x, books, ids):
    """the id rule stage by stage on the residual formed (in fp32, one subtract per element, as the device forms it) from the ids
    under test; -> (failures [(row, stage, message)], share of (row, stage) pairs with gap > 2 bnd)"""
    r = np.asarray(x, np.float32).copy()
    Dp = (r.shape[1] + 15) & ~15
    ids = np.asarray(ids, np.int64)
    bad, clear, total = [], 0, 0
    for q, E in enumerate(books):
        E = np.asarray(E, np.float32)
        s, bnd = scores64(r, E), row_bounds(r, E, Dp)
        bad += [(row, q, m) for row, m in judge_ids(s, bnd, ids[:, q])]
        clear += int((gaps(s)[1] > 2 * bnd).sum()); total += len(r)
        r = (r - E[np.clip(ids[:, q], 0, len(E) - 1)]).astype(np.float32)
    return bad, clear / max(total, 1)


def rvq_assign32(x, books):
    """fp32 restatement of ``sylber_rvq_assign``'s ids"""
    r = np.asarray(x, np.float32).copy()
    ids = np.zeros((len(r), len(books)), np.int64)
    for q, E in enumerate(books):
        E = np.asarray(E, np.float32)
        ids[:, q] = argmin32(r, E)
        r = (r - E[ids[:, q]]).astype(np.float32)
    return ids


def unit_rows32(rng, n, d):
    x = rng.standard_normal((n, d))
    return (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float32)


def rvq_books(rng, d, K, Q):
    """stage q at scale 0.5^q / sqrt(d): the residual of unit-norm rows shrinks stage by stage"""
    return [(rng.standard_normal((K, d)) * 0.5 ** q / np.sqrt(d)).astype(np.float32) for q in range(Q)]


def rvq_case(d, K, Q, n=500):
    """the residual-VQ case of one (d, K, Q): books with row K - 1 a copy of row 1 at every stage (K >= 64), unit-norm rows, row 7 a
    zero token (it scores the zero-padded rows K..Kp-1 lowest of all), row 8 an exact hit on the duplicated row"""
    rng = np.random.default_rng(d * K + Q)
    books, x = rvq_books(rng, d, K, Q), unit_rows32(rng, n, d)
    if K >= 64:
        for E in books:
            E[K - 1] = E[1]
    x[7] = 0.0
    x[8] = books[0][1]
    return books, x


# ---- unit norms ----------------------------------------------------------------------------------------------------------------
def lq_norm64(x, split=0, eps=EPS_LQ):
    """``sylber_lq_norm`` with ``normalize = 1`` in float64: the ranges [0, split) and [split, D) for 0 < split < D, else [0, D)"""
    x = np.asarray(x, np.float64)
    D = x.shape[1]
    sp = split if 0 < split < D else D
    out = np.empty_like(x)
    for lo, hi in ((0, sp), (sp, D)):
        if hi > lo:
            out[:, lo:hi] = x[:, lo:hi] / np.sqrt((x[:, lo:hi] ** 2).sum(1, keepdims=True) + eps)
    return out


def lq_norm32(x, split=0, eps=1e-5):
    x = np.asarray(x, np.float32)
    D = x.shape[1]
    sp = split if 0 < split < D else D
    out = np.empty_like(x)
    for lo, hi in ((0, sp), (sp, D)):
        if hi > lo:
            s = (x[:, lo:hi].astype(np.float64) ** 2).sum(1, keepdims=True).astype(np.float32)
            out[:, lo:hi] = x[:, lo:hi] / np.sqrt(s + np.float32(eps))
    return out


def blank_rows32(x):
    """the blank mask of ``Quantizer.forward`` as fp32 evaluates it: ``!(sum fl(x^2) > 0)`` -- NaN rows and rows whose every square
    underflows are blank"""
    x = np.asarray(x, np.float32)
    with np.errstate(under="ignore", invalid="ignore"):
        return ~((x * x).sum(1) > 0)


# ---- the conditioner's silence decisions on rows with one non-zero element (no summation order involved) --------------------------
def silent_features32(v):
    """``sqrtf(fl(v v)) < 1e-4f``"""
    v = np.asarray(v, np.float32)
    return np.sqrt(v * v) < np.float32(1e-4)


def silent_hidden32(v, thr, eps=1e-8):
    """``sqrtf(fl(v v) + 1e-8f) < thr``"""
    v = np.asarray(v, np.float32)
    return np.sqrt(v * v + np.float32(eps)) < np.float32(thr)


def ulp_neighbours(v, k):
    """the 2k + 1 fp32 values from k ulps below v to k ulps above"""
    v = np.float32(v)
    out = [v]
    lo = hi = v
    for _ in range(k):
        lo = np.nextafter(lo, np.float32(-np.inf)); hi = np.nextafter(hi, np.float32(np.inf))
        out = [lo] + out + [hi]
    return np.array(out, np.float32)


def features_crossing():
    """the smallest positive fp32 v with ``sqrtf(fl(v v)) >= 1e-4f``"""
    v = np.float32(1e-4)
    while not silent_features32(v):
        v = np.nextafter(v, np.float32(0))
    while silent_features32(v):
        v = np.nextafter(v, np.float32(1))
    return v

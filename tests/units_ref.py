"""Test-only numpy / float64 restatement of the syllable-unit path (like tests/cfm_ref.py, never imported by the product):

* residual k-means, ``ResidualKMQuantizer.get_indices`` / ``decode`` (sylber/model/quantizer.py:137-180): stage 1 is the nearest
  centroid of ``c1``, stage 2 the nearest centroid of ``c2`` to the fp32 residual ``x - c1[i1]``; ``decode`` = ``c1[i1] + c2[i2]``;
* ``expand_feature(avg_fts, durations)`` (sylber/model/flowmatching.py:873-882) and the span form the project's API uses
  (unit j of row b covers frames ``[start, end)``), with the conversion between the two."""
import numpy as np


def km_assign(x, c):
    """nearest centroid in float64 (first index on ties) and the full squared-distance table ``[n, K]``"""
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    d2 = (x64 ** 2).sum(1)[:, None] - 2 * x64 @ c64.T + (c64 ** 2).sum(1)[None, :]
    return d2.argmin(1), d2


def residual_assign(x, c1, c2):
    """-> ids ``[n, 2]`` and the two distance tables; the residual is formed in fp32, one subtract per element"""
    x = np.asarray(x, np.float32)
    i1, d1 = km_assign(x, c1)
    r = (x - np.asarray(c1, np.float32)[i1]).astype(np.float32)
    i2, d2 = km_assign(r, c2)
    return np.stack([i1, i2], 1), d1, d2


def decode(ids, books):
    """``KMQuantizer`` / ``ResidualKMQuantizer.decode``: the sum of the codebook rows in fp32 (negative ids read as 0)"""
    ids = np.maximum(np.asarray(ids), 0)
    out = np.asarray(books[0], np.float32)[ids[..., 0]]
    for k in range(1, len(books)):
        out = (out + np.asarray(books[k], np.float32)[ids[..., k]]).astype(np.float32)
    return out


def expand_feature(avg_fts, durations):
    """flowmatching.py:873-882: every unit row followed by a zero row, each repeated by its duration; rows must sum to one T"""
    avg_fts, durations = np.asarray(avg_fts), np.asarray(durations)
    B, S, D = avg_fts.shape
    rows = []
    for b in range(B):
        parts = []
        for j in range(S):
            parts.append(np.repeat(avg_fts[b, j][None], int(durations[b, j, 0]), 0))
            parts.append(np.zeros((int(durations[b, j, 1]), D), avg_fts.dtype))
        rows.append(np.concatenate(parts, 0))
    if len({len(r) for r in rows}) != 1:
        raise ValueError("ragged rows")
    return np.stack(rows)


def expand_spans(feats, spans, nunits, T):
    """the span form: frame t of row b takes the row of the last unit whose [start, end) holds it, else zeros"""
    feats = np.asarray(feats)
    B, _, D = feats.shape
    out = np.zeros((B, T, D), feats.dtype)
    for b in range(B):
        for j in range(int(nunits[b])):
            s, e = spans[b, j]
            out[b, s:e] = feats[b, j]
    return out


def spans_to_durations(feats, spans, nunits, T):
    """span tables -> upstream's (avg_fts, durations): a leading gap becomes a first pair with an all-zero feature (expand_feature
    has no slot for one), each unit's gap after it runs to the next start (the last one to T); rows padded with (0, 0) pairs"""
    feats = np.asarray(feats)
    B, _, D = feats.shape
    rows_f, rows_d = [], []
    for b in range(B):
        n = int(nunits[b])
        f, d = [], []
        first = int(spans[b, 0, 0]) if n else T
        if first > 0:
            f.append(np.zeros(D, feats.dtype)); d.append((first, 0))
        for j in range(n):
            s, e = int(spans[b, j, 0]), int(spans[b, j, 1])
            nxt = int(spans[b, j + 1, 0]) if j + 1 < n else T
            f.append(feats[b, j]); d.append((e - s, nxt - e))
        rows_f.append(f); rows_d.append(d)
    S = max(len(d) for d in rows_d)
    avg = np.zeros((B, S, D), feats.dtype)
    dur = np.zeros((B, S, 2), np.int64)
    for b in range(B):
        avg[b, :len(rows_f[b])] = np.stack(rows_f[b])
        dur[b, :len(rows_d[b])] = rows_d[b]
    return avg, dur

"""numpy restatement of the inverted-file search of sylber_amd.search.IVFSyllableIndex / csrc/knn.hip on top of tests/knn_ref.py.

    query i scans the rows j with labels[j] in probe[i] (probe entries < 0 name no list; rows with label < 0 are in no list);
    its result is knn_ref.search over exactly those rows, in ascending id order, with the ids mapped back.

The list assignment ``labels [N]`` and the probe table ``probe [n, nprobe]`` are inputs, so an fp32 near-tie of the coarse step never
has to be reproduced here.  ``work_items`` restates the host-only work-item table (``sylber_ivf_work_items``)."""
import numpy as np

import knn_ref as R

TILE, ITEM_TILES, TARGET_ITEMS, MIN_TILES, MAX_CUTS = 128, 16, 512, 2, 16


def candidates(labels, probe_row):
    """ascending ids of the rows in the lists of one probe row"""
    lists = np.asarray(probe_row)
    return np.nonzero(np.isin(np.asarray(labels), lists[lists >= 0]) & (np.asarray(labels) >= 0))[0]


def search(q, x, k, labels, probe, metric="l2", q_group=None, x_group=None):
    """(reported scores [n, k] float64, ids [n, k] int64) of the contract"""
    q, x = np.asarray(q), np.asarray(x)
    n = q.shape[0]
    S = R.scores(q, x, metric)             # once for all rows: a score does not depend on which rows are scanned beside it
    out_s = np.full((n, k), np.inf)
    out_i = np.full((n, k), -1, np.int64)
    for i in range(n):
        cand = candidates(labels, probe[i])
        if len(cand) == 0:
            continue
        s, j = R.search(q[i:i + 1], x[cand], k, metric, None if q_group is None else np.asarray(q_group)[i:i + 1],
                        None if x_group is None else np.asarray(x_group)[cand], s=S[i:i + 1, cand])
        out_s[i] = s[0]
        out_i[i] = np.where(j[0] >= 0, cand[np.maximum(j[0], 0)], -1)
    return out_s, out_i


def work_items(pair_counts, list_offsets, item_tiles=0):
    """(items [W, 8] int32, cuts): {list, pair_begin, pair_count, row_lo, row_hi, cut, last, tile_begin} per work item"""
    pc = np.asarray(pair_counts, np.int64)
    off = np.asarray(list_offsets, np.int64)
    tiles = (np.diff(off) + TILE - 1) // TILE
    qb = (pc + TILE - 1) // TILE
    probed = pc > 0
    T = int(item_tiles)
    if T <= 0:
        T = ITEM_TILES
        if qb[probed].sum() < TARGET_ITEMS:
            t = int(-(-(qb[probed] * np.maximum(tiles[probed], 1)).sum() // TARGET_ITEMS))
            T = max(MIN_TILES, min(t, ITEM_TILES))
    maxt = int(tiles[probed].max()) if probed.any() else 0
    T = max(T, -(-maxt // MAX_CUTS))
    items, C, pb = [], 1, 0
    for l in np.nonzero(probed)[0]:
        cuts = max(1, -(-int(tiles[l]) // T))
        C = max(C, cuts)
        for b in range(0, int(pc[l]), TILE):
            for c in range(cuts):
                t0, t1 = c * T, min((c + 1) * T, int(tiles[l]))
                r0 = int(off[l]) + t0 * TILE
                r1 = max(r0, min(int(off[l]) + t1 * TILE, int(off[l + 1])))
                items.append([l, pb + b, min(TILE, int(pc[l]) - b), r0, r1, c, int(c == cuts - 1), t0])
        pb += int(pc[l])
    return np.asarray(items, np.int32).reshape(-1, 8), C

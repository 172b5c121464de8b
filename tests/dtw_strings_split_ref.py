"""numpy restatement of the BLOCKED recurrence of ``sylber_dtw_strings_align_split`` (include/sylber_hip.h "Embedding strings";
csrc/dtw_strings_split.hip), on top of tests/dtw_strings_ref.py, whose global DP it must equal bit for bit.

The matrix of a pair is cut into blocks of ``BR`` rows by ``BC`` columns.  Block ``(b, c)`` takes three inputs -- the last row of block
``(b-1, c)``, the last column of block ``(b, c-1)`` and the corner cell above and left of it -- and launch ``d`` runs the blocks with
``b + c = d``.  What is modelled here is the STORAGE those inputs travel through, with its reuse, because that is where the scheme
can go wrong:

* ``brow [2, L]``: band b writes its last row to row ``b & 1``, the columns of its chunk;
* ``inner [2, L]``: the rows between the super-strips of ``SR`` rows inside one block, by the parity of the super-strip;
* ``bcol [2, m + bands]``: chunk c writes each row's last cell to column ``c & 1``; band b's cells lie at ``b (BR + 1) + 1 ..``, and
  the cell before them, ``b (BR + 1)``, is the corner of the block to the RIGHT, which the writer knows as the last cell of its own
  upper row.

Every buffer starts as poison (-1e30, -7: it wins every comparison), so a read of a cell that no earlier launch wrote shows.  The blocks of one launch run in
any ``order`` ("up": ascending b, "down": descending b): a block reads all its inputs when it starts and writes when it ends, as a
workgroup whose launch-mates may be anywhere, so a scheme is race-free only if both orders give the same cells.  ``defect`` plants
one of the two mistakes the kernel's header argues against:

* ``"corner_from_row"``: take the corner from the boundary row, ``brow[(b-1) & 1][c0 - 1]`` -- block ``(b+1, c-1)`` of the same
  launch rewrites it;
* ``"column_parity"``: read the left column from parity ``c & 1`` instead of ``(c-1) & 1``."""
import numpy as np

import dtw_ref as R
import dtw_strings_ref as G

POISON_A, POISON_N = np.float32(-1e30), -7           # a poisoned cell wins every comparison it enters


def schedule(nbr, nbc):
    """launch d -> its blocks (b, c), b + c = d; written out here, held against ``sylber_amd.search.split_schedule``"""
    out = []
    for d in range(nbr + nbc - 1 if nbr and nbc else 0):
        out.append([(b, d - b) for b in range(nbr) if 0 <= d - b < nbc])
    return out


def workspace_bytes(m, L, path, BR, BC, SR=128):
    """what a pair adds to ``sylber_dtw_strings_split_workspace_bytes`` beyond its 64 B of table, written out from the header's formula"""
    al = lambda b: (b + 255) // 256 * 256
    if m <= 0 or L <= 0:
        return 0
    nbr, nbc = -(-m // BR), -(-L // BC)
    total = 256
    total += al(16 * L) if nbr > 1 else 0
    total += al(16 * L) if BR > SR and m > SR else 0
    total += al(16 * (m + nbr)) if nbc > 1 else 0
    return total + (G.workspace_bytes(m, L, True) - G.workspace_bytes(m, L, False) if path else 0)


def blocked(d, BR, BC, SR=None, order="up", defect=None, dtype=np.float32):
    """the blocked recurrence over the local costs ``d [m, L]`` -> (A [m, L], n int64 [m, L], code int8 [m, L]) assembled from what each
    block computed.  ``SR``: the rows of a super-strip inside a block (divides BR; default BR: one per block)."""
    d = R._clean(d, dtype)
    m, L = d.shape
    SR = SR or BR
    assert BR % SR == 0
    inf = dtype(np.inf)
    nbr, nbc = -(-m // BR), -(-L // BC)
    A = np.full((m, L), POISON_A, dtype)
    n = np.full((m, L), POISON_N, np.int64)
    code = np.full((m, L), -1, np.int8)
    brow_a, brow_n = np.full((2, L), POISON_A, dtype), np.full((2, L), POISON_N, np.int64)
    inner_a, inner_n = np.full((2, L), POISON_A, dtype), np.full((2, L), POISON_N, np.int64)
    bcol_a, bcol_n = np.full((2, m + nbr), POISON_A, dtype), np.full((2, m + nbr), POISON_N, np.int64)
    for blocks in schedule(nbr, nbc):
        for b, c in (blocks if order == "up" else blocks[::-1]):
            i0, i1, c0, c1 = b * BR, min(m, (b + 1) * BR), c * BC, min(L, (c + 1) * BC)
            band = b * (BR + 1)
            # ---- the block's inputs, read when it starts
            top_a, top_n = (brow_a[(b + 1) & 1, c0:c1].copy(), brow_n[(b + 1) & 1, c0:c1].copy()) if b > 0 else (np.full(c1 - c0, inf, dtype), np.zeros(c1 - c0, np.int64))
            if c > 0:
                par = (c & 1) if defect == "column_parity" else ((c + 1) & 1)
                left_a, left_n = bcol_a[par, band:band + 1 + i1 - i0].copy(), bcol_n[par, band:band + 1 + i1 - i0].copy()
                if defect == "corner_from_row" and b > 0:
                    left_a[0], left_n[0] = brow_a[(b + 1) & 1, c0 - 1], brow_n[(b + 1) & 1, c0 - 1]
            else:
                left_a, left_n = np.full(1 + i1 - i0, inf, dtype), np.zeros(1 + i1 - i0, np.int64)
            corner = (top_a[-1], top_n[-1])                      # the last cell of its upper row: the corner of the block to the right
            # ---- its cells, super-strip by super-strip; wa / wn: a padded window with the row above and the column to the left
            for s0 in range(i0, i1, SR):
                s1, ss = min(i1, s0 + SR), s0 // SR
                if s0 > i0:                                      # the row the super-strip before left in the inner rows
                    top_a, top_n = inner_a[(ss + 1) & 1, c0:c1].copy(), inner_n[(ss + 1) & 1, c0:c1].copy()
                wa, wn = np.full((s1 - s0 + 1, c1 - c0 + 1), inf, dtype), np.zeros((s1 - s0 + 1, c1 - c0 + 1), np.int64)
                wa[0, 1:], wn[0, 1:] = top_a, top_n
                wa[:, 0], wn[:, 0] = left_a[s0 - i0:s1 - i0 + 1], left_n[s0 - i0:s1 - i0 + 1]
                for i in range(s0, s1):
                    for j in range(c0, c1):
                        p, q = i - s0 + 1, j - c0 + 1
                        if i == 0 and j == 0:
                            wa[p, q], wn[p, q], code[i, j] = d[0, 0], 1, G.DIAG
                            continue
                        best, nb, cd = wa[p - 1, q - 1], wn[p - 1, q - 1], G.DIAG
                        if wa[p - 1, q] < best:
                            best, nb, cd = wa[p - 1, q], wn[p - 1, q], G.UP
                        if wa[p, q - 1] < best:
                            best, nb, cd = wa[p, q - 1], wn[p, q - 1], G.LEFT
                        wa[p, q], wn[p, q], code[i, j] = dtype(d[i, j] + best), nb + 1, cd
                A[s0:s1, c0:c1], n[s0:s1, c0:c1] = wa[1:, 1:], wn[1:, 1:]
                if s1 < i1:                                      # to the block's own next super-strip: the columns of its chunk only
                    inner_a[ss & 1, c0:c1], inner_n[ss & 1, c0:c1] = wa[-1, 1:], wn[-1, 1:]
            # ---- what it leaves, written when it ends
            if b + 1 < nbr:
                brow_a[b & 1, c0:c1], brow_n[b & 1, c0:c1] = A[i1 - 1, c0:c1], n[i1 - 1, c0:c1]
            if c + 1 < nbc:
                bcol_a[c & 1, band], bcol_n[c & 1, band] = corner
                bcol_a[c & 1, band + 1:band + 1 + i1 - i0], bcol_n[c & 1, band + 1:band + 1 + i1 - i0] = A[i0:i1, c1 - 1], n[i0:i1, c1 - 1]
    return A, n, code


def align(d, BR, BC, SR=None, order="up", defect=None, dtype=np.float32):
    """one pair through the blocked recurrence -> (cost, steps, runs int64 [m, 2]) or None for padding, as ``dtw_strings_ref.align``"""
    d = np.asarray(d)
    if d.ndim != 2 or d.shape[0] == 0 or d.shape[1] == 0:
        return None
    A, n, code = blocked(d, BR, BC, SR, order, defect, dtype)
    m, L = A.shape
    if not A[m - 1, L - 1] < np.inf:
        return None
    return A[m - 1, L - 1], int(n[m - 1, L - 1]), G.runs_of(G.walk(code, m, L), m)

// What the subsequence-DTW kernels share: the geometry (the cost tile that the dynamic programme reads, the limits of a phrase and
// of a sequence, how many phrases sylber_dtw_plan packs into a query block) and the device pieces -- a workgroup's LDS carve, the
// per-tile column data, the epilogue that turns the contraction into local costs, the lane state with the wavefront over a tile,
// the write-out of a block's lists.  Who uses what:
//   * dtw.hip's dtw_scan_body<OCC> (dtw_search_kernel and dtw_occ_kernel; fp32, spans tracked: SPAN = true) and dtwpq.hip's
//     dtwpq_scan_kernel (SPAN = false) are built from all of them;
//   * dtw16.hip's dtw16_scan_kernel uses the column data and keeps the rest written out (its header says why);
//   * the wave-per-pair kernels (dtw16.hip's dtw_rerank_kernel and dtw_occ_rerank_kernel, dtw_align.hip's dtw_align_kernel) use the
//     local cost, the lane state and the cell (dt_cost, dt_up, dt_cell) through dtw_pair.h, which holds their chunk walk.
// The occurrence scans (dtw_occ_kernel, dtw_occ_rerank_kernel) add a pending occurrence to the lane state and hand over at any
// column: DtOcc, dt_occ_cell, dt_occ_wavefront below, siblings that leave the pieces above as they were.  The order of the
// predecessor comparisons and the NaN -> +inf rule are the contract's (include/sylber_hip.h).  Every piece is forced inline; the
// contraction (fp32: knn_tile.h, 16-bit: knn16_tile.h) and the K loop around it stay with the kernels.
#pragma once
#include "knn_tile.h"

constexpr int DT_LD = 132;                                // row stride of the cost tile: lane i reads d[i][t - i], bank (3 i + t) % 32
constexpr int DT_MAX_M = 64;                              // rows of a phrase: one wave
constexpr int DT_MAX_SEQ = 65536;                         // rows of a sequence (the DP along a sequence is serial)
constexpr int DT_FIXED = KN_BM * DT_LD + KN_BN + 132 + KN_BN;   // floats: cost tile (aliases the staging) | c_j | sequence ids | groups
constexpr int DT_LIST_BYTES = 65536;                      // LDS of a workgroup's lists, 16 B per entry: 32 phrases at k = 128

static_assert(DT_FIXED * 4 % 16 == 0, "the lists start 16-byte aligned");
static inline int dt_block_phrases(int k, int block_phrases) {
    int ph = DT_LIST_BYTES / (16 * k);
    ph = ph < KN_BM ? ph : KN_BM;
    return block_phrases > 0 && block_phrases < ph ? block_phrases : ph;
}

// A workgroup's dynamic LDS: the DT_FIXED floats, then the sorted lists of its ph phrases, m entries each; with SPAN the spans
// (8 B entries) come first.
template <bool SPAN>
struct DtLds {
    float* dm;                                             // [128][DT_LD] local costs of the tile, aliasing the operand staging
    float* cns;                                            // [128] c_j of the tile's columns
    int* sq;                                               // [130] sequence of columns n0 - 1 .. n0 + 128 (-1 outside the cut)
    int* sgs;                                              // [128] group of each column's sequence
    int2* lp;                                              // [ph][m] (first row, last row) of each entry (SPAN)
    float* ls;                                             // [ph][m] sorted costs
    int* li;                                               // [ph][m] their sequences
    __device__ __forceinline__ DtLds(float* smem, int ph, int m) {
        dm = smem;
        cns = smem + KN_BM * DT_LD;
        sq = (int*)(cns + KN_BN);
        sgs = sq + 132;
        lp = (int2*)(sgs + KN_BN);
        ls = SPAN ? (float*)(lp + ph * m) : (float*)lp;
        li = (int*)(ls + ph * m);
    }
    // every thread of the 256: all lists empty
    __device__ __forceinline__ void clear(int tid, int ph, int m) const {
        for (int e = tid; e < ph * m; e += 256) {
            ls[e] = INFINITY; li[e] = INT_MAX;
            if constexpr (SPAN) lp[e] = make_int2(-1, -1);
        }
    }
};

// The column data of the tile at row n0 of the cut [rlo, rhi), filled at the tile's first K step between the two barriers of the
// staging.  masked(j): row j counts as a NaN row (its c_j is read in both metrics, so its local cost is +inf against every phrase row).
template <bool SPAN, class Masked>
__device__ __forceinline__ void dt_tile_meta(const DtLds<SPAN>& L, int tid, int n0, int rlo, int rhi, const float* __restrict__ cn,
                                             const int32_t* __restrict__ seqid, const int32_t* __restrict__ sgrp, Masked masked) {
    if (tid < KN_BN) {
        const int j = n0 + tid;
        const float c = (cn && j < rhi) ? cn[j] : 0.f;
        L.cns[tid] = (j < rhi && masked(j)) ? NAN : c;
        L.sgs[tid] = (sgrp && j < rhi) ? sgrp[seqid[j]] : 0;
    }
    if (tid < KN_BN + 2) {
        const int j = n0 - 1 + tid;
        L.sq[tid] = (j >= rlo && j < rhi) ? seqid[j] : -1;
    }
}

// One local cost from a dot product: s = fmaf(-2, dot, c_j) as sylber_knn_search; d = max(0, ||q||^2 + s) (L2) or
// max(0, 1 - (-s / 2)) (cosine); a NaN d counts as +inf.
__device__ __forceinline__ float dt_cost(float dot, float cj, bool l2, float qn) {
    const float s = __builtin_fmaf(-2.0f, dot, cj);
    const float v = l2 ? qn + s : 1.0f - (0.f - 0.5f * s);
    return v != v ? INFINITY : fmaxf(0.f, v);
}

// The epilogue of a tile's contraction, behind a barrier that puts every wave past its fragment reads (the cost tile aliases the
// staging): the lane holds phrase row wm*64 + fm*32 + frow against columns wn*64 + fn*32 + 8g + 4fh + e (the C layout of the fp32 and
// of the 16-bit 32x32 MFMA).
__device__ __forceinline__ void dt_cost_tile(float* dm, const float* cns, const f32x16_t (&acc)[2][2], bool l2, const float (&qn)[2],
                                             const bool (&live)[2], int wm, int wn, int frow, int fh) {
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
        if (!live[fm]) continue;
        const int rl = wm * 64 + fm * 32 + frow;
#pragma unroll
        for (int fn = 0; fn < 2; ++fn)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float d[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = dt_cost(acc[fm][fn][4 * g + e], cns[wn * 64 + fn * 32 + 8 * g + 4 * fh + e], l2, qn[fm]);
                *(float4*)(dm + rl * DT_LD + wn * 64 + fn * 32 + 8 * g + 4 * fh) = make_float4(d[0], d[1], d[2], d[3]);
            }
    }
}

// The DP's state of one lane = one phrase row i: A[i][last column done], A[i][the one before] and, of a phrase's last row, the best
// cost of the current sequence; with SPAN also the start rows of those paths and the best one's (start, end).  (bst, be) mean
// something only while bc < +inf, so their initial value is never reported.
struct DtLane {
    float a_cur = INFINITY, a_prev = INFINITY, bc = INFINITY;
    int s_cur = 0, s_prev = 0, bst = 0, be = 0;
};

// the last two results of the lane below: A[i-1][j] and A[i-1][j-1] when this lane works on column j
struct DtUp { float a_cur, a_prev; int s_cur, s_prev; };

template <bool SPAN>
__device__ __forceinline__ DtUp dt_up(const DtLane& s) {
    DtUp u;
    u.a_cur = __shfl_up(s.a_cur, 1); u.a_prev = __shfl_up(s.a_prev, 1);
    u.s_cur = 0; u.s_prev = 0;
    if constexpr (SPAN) { u.s_cur = __shfl_up(s.s_cur, 1); u.s_prev = __shfl_up(s.s_prev, 1); }
    return u;
}

// One cell: local cost d of the lane's row against database row `col`.  first / lastrow: the row is its phrase's first / last;
// isstart: col begins a sequence, which masks the predecessors of the previous column.
template <bool SPAN>
__device__ __forceinline__ void dt_cell(DtLane& s, const DtUp& u, bool first, bool lastrow, bool isstart, float d, int col) {
    float A;
    int sa = col;
    if (first) A = d;
    else {
        float best = isstart ? INFINITY : u.a_prev;        // (i-1, j-1), then (i-1, j), then (i, j-1): the first smallest
        int bs = u.s_prev;
        if (u.a_cur < best) { best = u.a_cur; bs = u.s_cur; }
        const float left = isstart ? INFINITY : s.a_cur;
        if (left < best) { best = left; bs = s.s_cur; }
        A = d + best; sa = bs;
    }
    s.a_prev = s.a_cur; s.a_cur = A;
    if constexpr (SPAN) { s.s_prev = s.s_cur; s.s_cur = sa; }
    if (lastrow) {
        if (isstart) s.bc = INFINITY;                      // a new sequence; no-op where the caller walks one sequence (the re-rank)
        if (A < s.bc) {                                    // the smallest end column on ties
            s.bc = A;
            if constexpr (SPAN) { s.bst = sa; s.be = col; }
        }
    }
}

// What a lane of waves 0 and 1 knows of its packed query row wave * 64 + lane (meta[r]: -1 = padding, else (row of its phrase) |
// (is the phrase's last row) << 7 | (phrase slot in the block) << 8).  Waves 2 and 3 hold no row.
struct DtRow {
    int drow, pi, lastrow, slot, maxi, pg;                 // maxi: the wave's largest phrase row (-1: none), pg: the phrase's group
    bool valid;
    __device__ __forceinline__ DtRow(const int32_t* __restrict__ meta, const int32_t* __restrict__ slot_phrase,
                                     const int32_t* __restrict__ pgrp, int b, int P, int ph, int wave, int lane) {
        drow = (wave & 1) * 64 + lane;
        const int mt = wave < 2 ? meta[(size_t)b * KN_BM + drow] : -1;
        pi = mt & 127; lastrow = (mt >> 7) & 1; slot = (mt >> 8) & 255;
        valid = mt >= 0 && slot < ph;
        maxi = valid ? pi : -1;
#pragma unroll
        for (int o = 32; o; o >>= 1) { const int v = __shfl_xor(maxi, o); maxi = v > maxi ? v : maxi; }
        pg = 0;
        if (pgrp && valid && lastrow) { const int pid = slot_phrase[(size_t)b * KN_BM + slot]; pg = pid >= 0 && pid < P ? pgrp[pid] : 0; }
    }
};

// Waves 0 and 1, behind the barrier after dt_cost_tile: the anti-diagonal wavefront over the tile's ncol columns (lane l works on
// column st - (its phrase row) at step st; a lane that is through the tile keeps its state for the next one).  At a sequence end the
// lane of a phrase's last row hands (cost, sequence [, start, end]) to the phrase's list, unless the groups exclude the sequence.
template <bool SPAN>
__device__ __forceinline__ void dt_wavefront(const DtLds<SPAN>& L, const DtRow& r, DtLane& s, int lane, int n0, int ncol, bool grouped, int m) {
    const float* dr = L.dm + r.drow * DT_LD;
    for (int st = 0; st < ncol + r.maxi; ++st) {
        const DtUp u = dt_up<SPAN>(s);
        const int j = st - r.pi;
        bool fin = false;
        int fseq = 0;
        if (r.valid && j >= 0 && j < ncol) {
            const int sj = L.sq[j + 1];
            dt_cell<SPAN>(s, u, r.pi == 0, r.lastrow, L.sq[j] != sj, dr[j], n0 + j);
            if (r.lastrow && L.sq[j + 2] != sj && s.bc < INFINITY && !(grouped && L.sgs[j] == r.pg)) {
                fseq = sj;
                fin = kn_better(s.bc, sj, L.ls[r.slot * m + m - 1], L.li[r.slot * m + m - 1]);
            }
        }
        uint64_t fb = __ballot(fin);
        while (fb) {
            const int c = __ffsll((unsigned long long)fb) - 1;
            fb &= fb - 1;
            const float v = __shfl(s.bc, c);
            const int vs = __shfl(fseq, c), sl = __shfl(r.slot, c);
            int2 span = make_int2(0, 0);
            if constexpr (SPAN) span = make_int2(__shfl(s.bst, c), __shfl(s.be, c));
            kn_insert_t<SPAN>(L.ls + sl * m, L.li + sl * m, L.lp + sl * m, m, lane, v, vs, span);
        }
    }
}

// ---- every occurrence (sylber_dtw_occurrences, sylber_dtw_rerank_occurrences; "Every occurrence of a phrase" in
// include/sylber_hip.h).  Siblings of dt_cell / dt_wavefront: those two and DtLane are untouched, the kernels built from them
// compile from the text they had.
// What the lane of a phrase's last row keeps of the current sequence beside its DtLane: the pending occurrence (cost, start row,
// end row); pc = +inf: none, and then (ps, pe) mean nothing.  The contract's one-pass rule is stated over families (the finite
// columns of the last row with one start); here every finite column is taken by itself as (E[j], st[j], j).  That is the same
// pass: a family's columns are neighbours and all of them overlap the pending occurrence or none does, so offering them one by
// one against "the cheaper stays, the pending one on ties" leaves what offering their (min, smallest such j) once leaves; a
// column that finds its own family pending overlaps it (start <= end).  tests/test_occ_ref.py holds the two forms equal.
struct DtOcc { float pc = INFINITY; int ps = 0, pe = 0; };

// One cell of the occurrence scan: dt_cell's recurrence (taken with lastrow = false: the best-of-sequence fields of DtLane stay
// unused), then on a phrase's last row the one-pass rule on column `col`.  Returns true when the pending occurrence is pushed out
// by a disjoint one: the caller hands over (ec, es, ee).
__device__ __forceinline__ bool dt_occ_cell(DtLane& s, DtOcc& o, const DtUp& u, bool first, bool lastrow, bool isstart, float d, int col,
                                            float& ec, int& es, int& ee) {
    dt_cell<true>(s, u, first, false, isstart, d, col);
    if (!lastrow) return false;
    if (isstart) o.pc = INFINITY;                          // a new sequence: nothing is pending
    const float A = s.a_cur;
    if (!(A < INFINITY)) return false;                     // the start of an infinite cell carries no meaning
    const int sa = s.s_cur;
    if (o.pc < INFINITY && sa > o.pe) {                    // disjoint from the pending one: that one is an occurrence
        ec = o.pc; es = o.ps; ee = o.pe;
        o.pc = A; o.ps = sa; o.pe = col;
        return true;
    }
    if (A < o.pc) { o.pc = A; o.ps = sa; o.pe = col; }     // the spans share a row: the cheaper stays, the pending one on ties
    return false;
}

// one hand-off per set bit of fb: lane c's (v, start row, (start row, end row)) into the list of its phrase.  Distinct occurrences
// have distinct start rows, so the lists stay strictly ordered by (cost, start row).
__device__ __forceinline__ void dt_occ_hand(const DtLds<true>& L, uint64_t fb, int lane, int m, float v, int vs, int ve, int slot) {
    while (fb) {
        const int c = __ffsll((unsigned long long)fb) - 1;
        fb &= fb - 1;
        const float cv = __shfl(v, c);
        const int cs = __shfl(vs, c), ce = __shfl(ve, c), sl = __shfl(slot, c);
        kn_insert_t<true>(L.ls + sl * m, L.li + sl * m, L.lp + sl * m, m, lane, cv, cs, make_int2(cs, ce));
    }
}

// dt_wavefront for occurrences.  A hand-off can happen at any column, gated by the list's tail exactly as dt_wavefront's; at a
// sequence's last column a lane may owe two: the pending occurrence that a disjoint column has just pushed out, and that column
// itself, pending at the sequence end.  The pending state survives tile edges with DtLane and is cleared at a sequence start;
// cuts fall on sequence starts, so none crosses workgroups.
__device__ __forceinline__ void dt_occ_wavefront(const DtLds<true>& L, const DtRow& r, DtLane& s, DtOcc& o, int lane, int n0, int ncol,
                                                 bool grouped, int m) {
    const float* dr = L.dm + r.drow * DT_LD;
    for (int st = 0; st < ncol + r.maxi; ++st) {
        const DtUp u = dt_up<true>(s);
        const int j = st - r.pi;
        bool fin = false, fin2 = false;
        float ec = INFINITY;
        int es = 0, ee = 0;
        if (r.valid && j >= 0 && j < ncol) {
            const int sj = L.sq[j + 1];
            const bool out = dt_occ_cell(s, o, u, r.pi == 0, r.lastrow, L.sq[j] != sj, dr[j], n0 + j, ec, es, ee);
            const bool adm = r.lastrow && !(grouped && L.sgs[j] == r.pg);
            const float tv = L.ls[r.slot * m + m - 1];
            const int ti = L.li[r.slot * m + m - 1];
            fin = out && adm && kn_better(ec, es, tv, ti);
            fin2 = adm && L.sq[j + 2] != sj && o.pc < INFINITY && kn_better(o.pc, o.ps, tv, ti);
        }
        dt_occ_hand(L, __ballot(fin), lane, m, ec, es, ee, r.slot);
        dt_occ_hand(L, __ballot(fin2), lane, m, o.pc, o.ps, o.pe, r.slot);       // kn_insert_t tests the tail again: the first hand-off may have moved it
    }
}

// behind a barrier after the last tile: the block's lists to ps / pi (/ pp) [P][C][m]; entries that did not fill stay
// (+inf, INT_MAX (, (-1, -1)))
template <bool SPAN>
__device__ __forceinline__ void dt_write_lists(const DtLds<SPAN>& L, const int32_t* __restrict__ slot_phrase, int b, int P, int ph, int C,
                                               int cut, int m, int wave, int lane, float* __restrict__ ps, int32_t* __restrict__ pi,
                                               int2* __restrict__ pp) {
    for (int sl = wave; sl < ph; sl += 4) {
        const int pid = slot_phrase[(size_t)b * KN_BM + sl];
        if (pid < 0 || pid >= P) break;
        const size_t o = ((size_t)pid * C + cut) * m;
        for (int e = lane; e < m; e += 64) {
            ps[o + e] = L.ls[sl * m + e]; pi[o + e] = L.li[sl * m + e];
            if constexpr (SPAN) pp[o + e] = L.lp[sl * m + e];
        }
    }
}

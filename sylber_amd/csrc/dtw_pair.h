// What the wave-per-pair DTW kernels share: dtw16.hip's dtw_rerank_kernel and dtw_occ_rerank_kernel and dtw_align.hip's
// dtw_align_kernel.  One wave owns a (phrase, run of rows) pair, lane l owns phrase row l, and the run is walked in chunks of DP_CH
// columns.  Each piece is here once and forced inline:
//   * the chunk geometry (DP_CH, DP_LD);
//   * DpLane: what a lane knows of its phrase row;
//   * dp_chunk_costs: the local costs of one chunk.  Every lane forms its row's dots with the explicit ascending __builtin_fmaf chain
//     from 0 over D -- what v_mfma_f32_32x32x2_f32 performs in dtw_search_kernel, as knn_rerank_kernel relies on -- the database row
//     being the same address in every lane, and dt_cost (dtw_tile.h) turns them into d in the lane's LDS row between two barriers.
//     This chain is the bitwise contract "every A[i][j] has the bits dtw_search_kernel gives it", and it is stated here only;
//   * dp_walk: the anti-diagonal walk over a chunk, the lane state (DtLane, dtw_tile.h) carried across chunks.  The run is one
//     sequence that starts at its first row.  What happens in a cell is the kernel's: cell(j, col, isstart, u) runs in the lanes
//     that have a cell at this step, step() in every lane after it (the occurrence re-rank's ballots);
//   * dt_pair_check: the host checks of sylber_dtw_rerank, sylber_dtw_rerank_occurrences and sylber_dtw_align, and the norms by metric.
#pragma once
#include "../../include/sylber_hip.h"
#include "dtw_tile.h"

constexpr int DP_CH = 32;                                 // columns of a chunk (RERANK_CHUNK of search.py)
constexpr int DP_LD = 36;                                 // row stride of the chunk's costs: lane i reads d[i][t - i], bank (3 i + t) % 32

// The lane's phrase row for phrase p: rows prow[p] .. + plen[p] of the packed fp32 blocks q [qrows, D], qsq their ||q_i||^2 (L2) or
// null.  max_rows: the most rows the kernel has room for (DT_MAX_M, or the align kernel's Mx).
struct DpLane {
    int mp;                                                // rows of the phrase, clamped to [1, max_rows]
    const float* qr;                                       // the lane's row; lanes behind the phrase read its last row and keep nothing
    float qn;
    bool valid, lastrow;
    __device__ __forceinline__ DpLane(const float* __restrict__ q, const float* __restrict__ qsq, int qrows, const int32_t* __restrict__ prow,
                                      const int32_t* __restrict__ plen, int p, int D, int lane, int max_rows) {
        mp = plen[p];
        mp = mp < 1 ? 1 : (mp > DT_MAX_M ? DT_MAX_M : mp);
        mp = mp > max_rows ? max_rows : mp;
        int r = prow[p] + (lane < mp ? lane : mp - 1);
        r = r < 0 ? 0 : (r < qrows ? r : qrows - 1);
        qr = q + (size_t)r * D;
        qn = qsq ? qsq[r] : 0.f;
        valid = lane < mp; lastrow = lane == mp - 1;
    }
};

// The local costs of columns n0 .. n0 + ncol - 1 of a run that ends before row j1, into the lane's LDS row dr [DP_CH].
// dot[jj] = the fmaf chain over ascending c from 0 of q_lane . x_(n0 + jj): explicit __builtin_fmaf calls, nothing for the compiler
// to contract or reassociate; columns past the run repeat its last row and are not read by the DP.
__device__ __forceinline__ void dp_chunk_costs(float* dr, const DpLane& L, const float* __restrict__ x, int D, const float* __restrict__ cn,
                                               bool l2, int n0, int ncol, int j1) {
    float dot[DP_CH];
#pragma unroll
    for (int jj = 0; jj < DP_CH; ++jj) dot[jj] = 0.f;
    for (int c = 0; c < D; c += 4) {
        const float4 a = *(const float4*)(L.qr + c);
#pragma unroll
        for (int jj = 0; jj < DP_CH; ++jj) {
            const int j = jj < ncol ? n0 + jj : j1 - 1;
            const float4 bv = *(const float4*)(x + (size_t)j * D + c);
            dot[jj] = __builtin_fmaf(bv.x, a.x, dot[jj]);
            dot[jj] = __builtin_fmaf(bv.y, a.y, dot[jj]);
            dot[jj] = __builtin_fmaf(bv.z, a.z, dot[jj]);
            dot[jj] = __builtin_fmaf(bv.w, a.w, dot[jj]);
        }
    }
    __syncthreads();                                       // the previous chunk's costs are read
#pragma unroll
    for (int jj = 0; jj < DP_CH; ++jj) {
        const int j = jj < ncol ? n0 + jj : j1 - 1;
        dr[jj] = dt_cost(dot[jj], cn ? cn[j] : 0.f, l2, L.qn);
    }
    __syncthreads();
}

struct DpNoStep { __device__ __forceinline__ void operator()() const {} };

// Behind dp_chunk_costs: dtw_tile.h's wavefront over the chunk at row n0 of a run that starts at row j0.  st: the lane state that
// the kernel's cell moves on (dt_cell, dt_occ_cell); u: the last two results of the lane below.
template <class Cell, class Step = DpNoStep>
__device__ __forceinline__ void dp_walk(DtLane& st, const DpLane& L, int lane, int n0, int ncol, int j0, Cell cell, Step step = Step()) {
    for (int t = 0; t < ncol + L.mp - 1; ++t) {
        const DtUp u = dt_up<true>(st);
        const int j = t - lane;
        if (L.valid && j >= 0 && j < ncol) cell(j, n0 + j, n0 + j == j0, u);
        step();
    }
}

// Host: what the three entries check alike, in one order, behind an entry's own null check.  count_error: the entry's
// wording for "a count below 1 or a bad D" (n_other: its n_seq or n_pairs); own_error: its verdict on the arguments only it has, or
// null; large / large_error: its own overflow condition beside the packed rows', and its wording.  Sets qn / cn to the norms the
// metric reads, or null.
static inline int dt_pair_check(const char* what, const char* count_error, const char* own_error, const char* large_error, int32_t n_blocks,
                                int32_t n_phrases, int32_t n_other, int32_t N, int32_t D, const float* q_norm_dev, const float* db_norm_dev,
                                int32_t metric, bool large, const float*& qn, const float*& cn) {
    if (n_blocks < 1 || n_phrases < 1 || n_other < 1 || N < 1 || D < 16 || D % 16) { syl_set_error(what, count_error); return 1; }
    if (own_error) { syl_set_error(what, own_error); return 1; }
    if (metric != SYLBER_KNN_L2 && metric != SYLBER_KNN_IP) { syl_set_error(what, "unknown metric"); return 1; }
    if (metric == SYLBER_KNN_L2 && (!db_norm_dev || !q_norm_dev)) { syl_set_error(what, "the L2 metric needs db_norm_dev and q_norm_dev"); return 1; }
    if ((int64_t)n_blocks * KN_BM > INT32_MAX || large) { syl_set_error(what, large_error); return 1; }
    qn = metric == SYLBER_KNN_L2 ? q_norm_dev : nullptr;
    cn = metric == SYLBER_KNN_L2 ? db_norm_dev : nullptr;
    return 0;
}

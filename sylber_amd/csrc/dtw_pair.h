// What the wave-per-pair DTW kernels share: dtw16.hip's dtw_rerank_kernel and dtw_occ_rerank_kernel, dtw_align.hip's dtw_align_kernel
// and dtw_codes.hip's three kernels on a coded database.  One wave owns a (phrase, run of rows) pair, lane l owns phrase row l, and the
// run is walked in chunks of DP_CH columns.  Each piece is here once and forced inline:
//   * the chunk geometry (DP_CH, DP_LD);
//   * DpLane: what a lane knows of its phrase row;
//   * the rows of a chunk, a parameter: rows(jj, j, c) is the float4 at elements c .. c + 3 of the chunk's column jj = database row j,
//     the same in every lane.  The chain asks in segments of rows.seg() elements, a multiple of 4, and calls rows.begin(c0) in front
//     of each, so that a source may look something up once per segment.  DpRows / DpRowsSrc: the rows behind a plain pointer (one
//     segment); dtw_codes.hip's source rebuilds them from code bytes;
//   * dp_chunk_costs: the local costs of one chunk.  Every lane forms its row's dots with the explicit ascending __builtin_fmaf chain
//     from 0 over D -- what v_mfma_f32_32x32x2_f32 performs in dtw_search_kernel, as knn_rerank_kernel relies on -- and dt_cost
//     (dtw_tile.h) turns them into d in the lane's LDS row between two barriers.
//     This chain is the bitwise contract "every A[i][j] has the bits dtw_search_kernel gives it", and it is stated here only;
//   * dp_walk: the anti-diagonal walk over a chunk, the lane state (DtLane, dtw_tile.h) carried across chunks.  The run is one
//     sequence that starts at its first row.  What happens in a cell is the kernel's: cell(j, col, isstart, u) runs in the lanes
//     that have a cell at this step, step() in every lane after it (the occurrence re-rank's ballots);
//   * dp_rerank_pair and dtw_rank_kernel: the body of a re-rank kernel over any source of rows, and the ranking launch behind it
//     (sylber_dtw_rerank, sylber_dtw_rerank_codes);
//   * dp_occ_rerank_pair: the body of an occurrence re-rank kernel over any source of rows: dt_occ_cell for the cell, the two
//     hand-off ballots after it and the pair's list in LDS (sylber_dtw_rerank_occurrences, sylber_dtw_rerank_occurrences_codes);
//   * dt_pair_check: the host checks of sylber_dtw_rerank, sylber_dtw_rerank_occurrences, sylber_dtw_align and the three _codes
//     entries, and the norms by metric.
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

// The rows behind a plain pointer x [N, D]: one segment, nothing to look up.
struct DpRows {
    const float* x;
    int D;
    __device__ __forceinline__ int seg() const { return D; }
    __device__ __forceinline__ void begin(int) {}
    __device__ __forceinline__ float4 operator()(int, int j, int c) const { return *(const float4*)(x + (size_t)j * D + c); }
};
// A source hands out the rows of one chunk: columns n0 .. n0 + ncol - 1 of a run that ends before row j1 (every lane calls).
struct DpRowsSrc {
    const float* x;
    int D;
    __device__ __forceinline__ DpRows chunk(int, int, int, int) const { return DpRows{x, D}; }
};

// The local costs of columns n0 .. n0 + ncol - 1 of a run that ends before row j1, into the lane's LDS row dr [DP_CH].
// dot[jj] = the fmaf chain over ascending c from 0 of q_lane . x_(n0 + jj): explicit __builtin_fmaf calls, nothing for the compiler
// to contract or reassociate; columns past the run repeat its last row and are not read by the DP.
template <class Rows>
__device__ __forceinline__ void dp_chunk_costs(float* dr, const DpLane& L, Rows rows, int D, const float* __restrict__ cn, bool l2, int n0,
                                               int ncol, int j1) {
    float dot[DP_CH];
#pragma unroll
    for (int jj = 0; jj < DP_CH; ++jj) dot[jj] = 0.f;
    const int seg = rows.seg();
    for (int c0 = 0; c0 < D; c0 += seg) {
        rows.begin(c0);
        for (int c = c0; c < c0 + seg; c += 4) {
            const float4 a = *(const float4*)(L.qr + c);
#pragma unroll
            for (int jj = 0; jj < DP_CH; ++jj) {
                const int j = jj < ncol ? n0 + jj : j1 - 1;
                const float4 bv = rows(jj, j, c);
                dot[jj] = __builtin_fmaf(bv.x, a.x, dot[jj]);
                dot[jj] = __builtin_fmaf(bv.y, a.y, dot[jj]);
                dot[jj] = __builtin_fmaf(bv.z, a.z, dot[jj]);
                dot[jj] = __builtin_fmaf(bv.w, a.w, dot[jj]);
            }
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

// The body of a re-rank kernel: workgroup (one wave) e of phrase p = blockIdx.x / m runs the exact subsequence DTW of phrase p (rows
// prow[p] .. + plen[p] of the packed fp32 blocks q, qsq their ||q_i||^2 (L2) or null) against sequence cand[p][e] (rows soff[s] ..
// soff[s + 1] of the N rows that src hands out).  dsm: DT_MAX_M * DP_LD floats of LDS.  Writes (cost, (start row, end row)) to pc /
// pspan [P][m]; (+inf, (-1, -1)) for a candidate of -1.
template <class Src>
__device__ __forceinline__ void dp_rerank_pair(float* dsm, const Src& src, const float* __restrict__ q, const float* __restrict__ qsq, int qrows,
                                               const int32_t* __restrict__ prow, const int32_t* __restrict__ plen, int N, int D,
                                               const float* __restrict__ cn, const int32_t* __restrict__ cand,
                                               const int32_t* __restrict__ soff, int S, int m, float* __restrict__ pc,
                                               int2* __restrict__ pspan) {
    const int lane = threadIdx.x;
    const size_t pair = blockIdx.x;
    const int p = (int)(pair / m);
    const int sidx = cand[pair];
    int j0 = 0, j1 = 0;
    if (sidx >= 0 && sidx < S) {
        j0 = soff[sidx]; j1 = soff[sidx + 1];
        j0 = j0 < 0 ? 0 : j0; j1 = j1 > N ? N : j1;
    }
    if (j1 <= j0) {                                        // workgroup-uniform
        if (lane == 0) { pc[pair] = INFINITY; pspan[pair] = make_int2(-1, -1); }
        return;
    }
    const DpLane L(q, qsq, qrows, prow, plen, p, D, lane, DT_MAX_M);
    DtLane st;
    float* dr = dsm + lane * DP_LD;
    for (int n0 = j0; n0 < j1; n0 += DP_CH) {
        const int ncol = j1 - n0 < DP_CH ? j1 - n0 : DP_CH;
        dp_chunk_costs(dr, L, src.chunk(lane, n0, ncol, j1), D, cn, qsq != nullptr, n0, ncol, j1);
        dp_walk(st, L, lane, n0, ncol, j0, [&](int j, int col, bool isstart, const DtUp& u) {
            dt_cell<true>(st, u, lane == 0, L.lastrow, isstart, dr[j], col);
        });
    }
    if (L.lastrow) {
        pc[pair] = st.bc;
        pspan[pair] = st.bc < INFINITY ? make_int2(st.bst, st.be) : make_int2(-1, -1);
    }
}

// The body of an occurrence re-rank kernel (sylber_dtw_rerank_occurrences, sylber_dtw_rerank_occurrences_codes): dp_rerank_pair's
// pair, walk and pieces, so every A[m-1][j] and start has the bits of dtw_occ_kernel's, with every non-overlapping occurrence of
// the candidate kept.  The lane of the last row runs dt_occ_cell's one-pass rule and the wave keeps the pair's k best occurrences
// as a sorted list of (cost, start row, (start row, end row)) in LDS (ols / oli / olp [KN_KMAX]: 16 B x 128 = 2 KiB, k of them
// used); it goes to ps / pi / pp [P][m][k], a list of fillers for a candidate of -1.  Candidate sequences of a phrase are distinct (stage 1's are),
// so the start rows of its m lists are: knn_merge_kernel<true> reduces them and dtw_occ_finish_kernel reports (dtw_occ.h).
template <class Src>
__device__ __forceinline__ void dp_occ_rerank_pair(float* dsm, float* ols, int* oli, int2* olp, const Src& src, const float* __restrict__ q,
                                                   const float* __restrict__ qsq, int qrows, const int32_t* __restrict__ prow,
                                                   const int32_t* __restrict__ plen, int N, int D, const float* __restrict__ cn,
                                                   const int32_t* __restrict__ cand, const int32_t* __restrict__ soff, int S, int m, int k,
                                                   float* __restrict__ ps, int32_t* __restrict__ pi, int2* __restrict__ pp) {
    const int lane = threadIdx.x;
    const size_t pair = blockIdx.x;
    const int p = (int)(pair / m);
    const int sidx = cand[pair];
    int j0 = 0, j1 = 0;
    if (sidx >= 0 && sidx < S) {
        j0 = soff[sidx]; j1 = soff[sidx + 1];
        j0 = j0 < 0 ? 0 : j0; j1 = j1 > N ? N : j1;
    }
    for (int e = lane; e < k; e += 64) { ols[e] = INFINITY; oli[e] = INT_MAX; olp[e] = make_int2(-1, -1); }
    const DpLane L(q, qsq, qrows, prow, plen, p, D, lane, DT_MAX_M);
    DtLane st;
    DtOcc oc;
    float* dr = dsm + lane * DP_LD;
    for (int n0 = j0; n0 < j1; n0 += DP_CH) {              // no chunk for a candidate of -1: its list stays fillers
        const int ncol = j1 - n0 < DP_CH ? j1 - n0 : DP_CH;
        // a barrier of the source or dp_chunk_costs' first, the first time: the list is cleared
        dp_chunk_costs(dr, L, src.chunk(lane, n0, ncol, j1), D, cn, qsq != nullptr, n0, ncol, j1);
        bool out = false, end = false;                     // what the lane's cell of this step owes the list
        float ec = INFINITY;
        int es = 0, ee = 0;
        dp_walk(st, L, lane, n0, ncol, j0, [&](int j, int col, bool isstart, const DtUp& u) {
            out = dt_occ_cell(st, oc, u, lane == 0, L.lastrow, isstart, dr[j], col, ec, es, ee);
            end = L.lastrow && col == j1 - 1 && oc.pc < INFINITY;
        }, [&] {
            // only lane mp - 1 can owe a hand-off; at the sequence's last column it may owe both
            if (__ballot(out)) {
                const int vs = __shfl(es, L.mp - 1);
                kn_insert_t<true>(ols, oli, olp, k, lane, __shfl(ec, L.mp - 1), vs, make_int2(vs, __shfl(ee, L.mp - 1)));
            }
            if (__ballot(end)) {
                const int vs = __shfl(oc.ps, L.mp - 1);
                kn_insert_t<true>(ols, oli, olp, k, lane, __shfl(oc.pc, L.mp - 1), vs, make_int2(vs, __shfl(oc.pe, L.mp - 1)));
            }
            out = false; end = false;
        });
    }
    __syncthreads();
    for (int e = lane; e < k; e += 64) { ps[pair * k + e] = ols[e]; pi[pair * k + e] = oli[e]; pp[pair * k + e] = olp[e]; }
}

// One wave per phrase i (4 per workgroup).  Lane e (and e + 64) owns pair (i, cand[i][e]); a candidate of -1 or a cost that is not
// below +inf becomes a (+inf, INT_MAX) filler.  Rank = entries strictly before it under (cost, sequence, position) (the position
// only orders the fillers); ranks < k are reported as dtw_finish_kernel reports them: spans as (first row, one past the last row),
// fillers (+inf, -1, (-1, -1)).
static __global__ __launch_bounds__(256) void dtw_rank_kernel(const float* __restrict__ pc, const int2* __restrict__ pspan,
                                                       const int32_t* __restrict__ cand, int P, int m, int k, float* __restrict__ cost,
                                                       int64_t* __restrict__ seq, int64_t* __restrict__ span) {
    __shared__ float ss[4][KN_KMAX];
    __shared__ int si[4][KN_KMAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int i = blockIdx.x * 4 + wave;
    const bool live = i < P;
    i = live ? i : P - 1;
    float sv[KN_KMAX / 64];
    int sj[KN_KMAX / 64];
#pragma unroll
    for (int h = 0; h < KN_KMAX / 64; ++h) {
        const int e = lane + 64 * h;
        sv[h] = INFINITY; sj[h] = INT_MAX;
        if (e < m) {
            const float v = pc[(size_t)i * m + e];
            const int j = cand[(size_t)i * m + e];
            if (j >= 0 && v < INFINITY) { sv[h] = v; sj[h] = j; }
            ss[wave][e] = sv[h]; si[wave][e] = sj[h];
        }
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int h = 0; h < KN_KMAX / 64; ++h) {
        const int e = lane + 64 * h;
        if (e >= m) continue;
        int rank = 0;
        for (int f = 0; f < m; ++f) {
            const float ev = ss[wave][f];
            const int ej = si[wave][f];
            rank += (kn_better(ev, ej, sv[h], sj[h]) || (ev == sv[h] && ej == sj[h] && f < e)) ? 1 : 0;
        }
        if (rank < k) {
            const size_t o = (size_t)i * k + rank;
            if (sj[h] == INT_MAX) { cost[o] = INFINITY; seq[o] = -1; span[2 * o] = -1; span[2 * o + 1] = -1; }
            else {
                const int2 sp = pspan[(size_t)i * m + e];
                cost[o] = sv[h]; seq[o] = sj[h]; span[2 * o] = sp.x; span[2 * o + 1] = (int64_t)sp.y + 1;
            }
        }
    }
}

// Host: the pair results of a re-rank in its workspace (sylber_dtw16_workspace_bytes covers them), and the ranking launch
static inline int64_t dp_rerank_bytes(int64_t P, int64_t m) { return kn_al(P * m * 4) + kn_al(P * m * 8); }
struct DpPairResults {
    float* pc;
    int2* pspan;
    DpPairResults(void* workspace_dev, int64_t P, int64_t m) : pc((float*)workspace_dev), pspan((int2*)((char*)workspace_dev + kn_al(P * m * 4))) {}
};
static inline int dp_rank_launch(const DpPairResults& r, const int32_t* cand_dev, int32_t n_phrases, int32_t m, int32_t k, float* cost_dev,
                                 int64_t* seq_dev, int64_t* span_dev, hipStream_t s) {
    hipLaunchKernelGGL(dtw_rank_kernel, dim3((unsigned)((n_phrases + 3) / 4)), dim3(256), 0, s, r.pc, r.pspan, cand_dev, n_phrases, m, k, cost_dev,
                       seq_dev, span_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Host: what the entries check alike, in one order, behind an entry's own null check.  count_error: the entry's
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

// Phrase search: subsequence DTW of syllable sequences against every sequence of a SyllableIndex (sylber_amd/search.py:
// SyllableIndex.search_phrases; contract in include/sylber_hip.h, restated in tests/dtw_ref.py).
//   * dtw_search_kernel: grid (query blocks) x C database cuts.  A query block holds whole phrases (at most 128 rows; a phrase lies
//     inside one 64-row half, so that one wave owns it); a cut is a run of whole sequences.  The workgroup walks the 128-row tiles of
//     its cut with knn_search_kernel's contraction (knn_tile.h: same operand roles, same k-pair order, so the local costs have the
//     bits of SyllableIndex.search's scores).  After each tile the local costs d go to LDS and waves 0 and 1 advance the dynamic
//     programme over the tile's columns on an anti-diagonal wavefront: lane l holds one phrase row i and works on column t - i at
//     step t; A[i-1][j] and A[i-1][j-1] (and their starts) are the last two results of lane l - 1.  A lane that is through the tile
//     keeps its last two results for the next tile, so the wavefront drains at every tile edge and no cost column is kept.
//     The additions are the contract's, one per cell in a fixed order: nothing is re-associated.
//     A sequence start masks the predecessors of the previous column; at a sequence end the lane of the phrase's last row hands
//     (cost, sequence, start, end) to the phrase's sorted top-k list in LDS (kn_insert's scheme with a payload).
//     Only the fp32 staging and K loop are written here: the column data, the epilogue, the wavefront and the write-out are
//     dtw_tile.h's with SPAN = true, the text that the 16-bit scans (dtw16_scan.h) compile with SPAN = false.
//   * knn_merge_kernel<true> (knn_lists.h) / dtw_finish_kernel: the C partial lists of a phrase merged pairwise, as the k-NN merge
//     does, with the span.  Sequences of different cuts differ, so only the (+inf, INT_MAX) fillers can be equal.
// Lists are ordered by (cost, sequence): strict and total over the admissible sequences, so the result is unique.
//   * dtw_occ_kernel (SyllableIndex.search_occurrences, tests/occ_ref.py): the same scan handing every non-overlapping occurrence
//     of a sequence to the list, ordered by (cost, start row); sylber_dtw_occurrences.
// The two kernels are dtw_scan_body<OCC> and differ in the wavefront alone; the two entry points share dt_scan_check.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "dtw_tile.h"
#include "knn_lists.h"
#include "dtw_occ.h"
#include <climits>

constexpr int DT_TARGET_BLOCKS = 512;                     // automatic cuts: (query blocks) x C >= 2 workgroups per CU
constexpr int DT_MIN_TILES = 4;                           // ... of no less than 4 database tiles on average

static size_t dt_lds_bytes(int ph, int k) { return (size_t)DT_FIXED * 4 + (size_t)ph * k * 16; }

// The fp32 scan of a workgroup, for both kernels below; OCC: the wavefront hands every non-overlapping occurrence of a sequence to
// the phrase's list (dt_occ_wavefront) instead of the sequence's best (dt_wavefront).
// meta[r] of packed query row r: -1 = padding, else (row of its phrase) | (is the phrase's last row) << 7 | (phrase slot in the block) << 8
template <bool OCC>
__device__ __forceinline__ void dtw_scan_body(const float* __restrict__ q, const float* __restrict__ qsq, const int32_t* __restrict__ meta,
                                               const int32_t* __restrict__ slot_phrase, const int32_t* __restrict__ block_rows, int P, int ph,
                                               const float* __restrict__ x, int N, int D, const float* __restrict__ cn, int k,
                                               const int32_t* __restrict__ seqid, const int32_t* __restrict__ cuts,
                                               const int32_t* __restrict__ pgrp, const int32_t* __restrict__ sgrp, int C,
                                               float* __restrict__ ps, int32_t* __restrict__ pi, int2* __restrict__ pp) {
    extern __shared__ __attribute__((aligned(16))) float dt_smem[];
    float* xs = dt_smem;                                   // staging of the query rows
    float* cs = dt_smem + KN_BM * KN_LD;                   // staging of the database rows
    const DtLds<true> L(dt_smem, ph, k);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int b = blockIdx.x, cut = blockIdx.y;
    int rlo = cuts[cut], rhi = cuts[cut + 1];
    rlo = rlo < 0 ? 0 : rlo; rhi = rhi > N ? N : rhi;
    const int nrow = block_rows[b];
    const int tiles = rhi > rlo ? (rhi - rlo + KN_BN - 1) / KN_BN : 0;
    L.clear(tid, ph, k);
    const int sr = tid >> 1, sh = (tid & 1) * 8;
    const float* qrow = q + ((size_t)b * KN_BM + sr) * D + sh;
    float* xdst = xs + sr * KN_LD + (sh >> 1);
    float* cdst = cs + sr * KN_LD + (sh >> 1);
    const int frow = lane & 31, fh = lane >> 5;
    const int ksteps = D / KN_BK, T = ksteps * tiles;
    bool live[2];                                          // wave-uniform: this wave's 32-row half holds phrase rows
    float qn[2] = {0.f, 0.f};
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
        live[fm] = wm * 64 + fm * 32 < nrow;
        if (qsq) qn[fm] = qsq[(size_t)b * KN_BM + wm * 64 + fm * 32 + frow];
    }
    const DtRow row(meta, slot_phrase, pgrp, b, P, ph, wave, lane);
    DtLane st;
    [[maybe_unused]] DtOcc oc;                             // the pending occurrence: OCC only

    f32x16_t acc[2][2];
    float4 xa, xb, ca, cb;
    auto fetch = [&](int t) {
        const int tile = t / ksteps, k0 = (t % ksteps) * KN_BK;
        int cr = rlo + tile * KN_BN + sr; cr = cr < rhi ? cr : rhi - 1;
        const float* crow = x + (size_t)cr * D + sh + k0;
        xa = *(const float4*)(qrow + k0); xb = *(const float4*)(qrow + k0 + 4);
        ca = *(const float4*)crow; cb = *(const float4*)(crow + 4);
    };
    if (T > 0) fetch(0);
    for (int t = 0; t < T; ++t) {
        const int tile = t / ksteps, ks = t % ksteps, n0 = rlo + tile * KN_BN;
        if (ks == 0) kn_zero(acc);
        __syncthreads();                                   // previous fragments, the cost tile, cns / sq / sgs are all read
        kn_stage(xdst, cdst, xa, xb, ca, cb);
        if (ks == 0) dt_tile_meta(L, tid, n0, rlo, rhi, cn, seqid, sgrp, [](int) { return false; });
        __syncthreads();
        if (t + 1 < T) fetch(t + 1);
        kn_mma(xs, cs, wm, wn, frow, fh, acc, live[0], live[1]);
        if (ks != ksteps - 1) continue;
        __syncthreads();                                   // every wave is past its fragment reads: the cost tile aliases the staging
        dt_cost_tile(L.dm, L.cns, acc, qsq != nullptr, qn, live, wm, wn, frow, fh);
        __syncthreads();
        if (wave >= 2 || row.maxi < 0) continue;           // wave-uniform
        const int ncol = rhi - n0 < KN_BN ? rhi - n0 : KN_BN;
        if constexpr (OCC) dt_occ_wavefront(L, row, st, oc, lane, n0, ncol, sgrp != nullptr, k);
        else dt_wavefront(L, row, st, lane, n0, ncol, sgrp != nullptr, k);
    }
    __syncthreads();
    dt_write_lists(L, slot_phrase, b, P, ph, C, cut, k, wave, lane, ps, pi, pp);
}

__global__ __launch_bounds__(256) void dtw_search_kernel(const float* __restrict__ q, const float* __restrict__ qsq,
                                                         const int32_t* __restrict__ meta, const int32_t* __restrict__ slot_phrase,
                                                         const int32_t* __restrict__ block_rows, int P, int ph,
                                                         const float* __restrict__ x, int N, int D, const float* __restrict__ cn, int k,
                                                         const int32_t* __restrict__ seqid, const int32_t* __restrict__ cuts,
                                                         const int32_t* __restrict__ pgrp, const int32_t* __restrict__ sgrp, int C,
                                                         float* __restrict__ ps, int32_t* __restrict__ pi, int2* __restrict__ pp) {
    dtw_scan_body<false>(q, qsq, meta, slot_phrase, block_rows, P, ph, x, N, D, cn, k, seqid, cuts, pgrp, sgrp, C, ps, pi, pp);
}

// dtw_search_kernel's sibling for SyllableIndex.search_occurrences.  A list entry is (cost, start row, (start row, end row)): the
// 16 B of dtw_search_kernel's, ordered by (cost, start row).  Occurrences of different cuts have different start rows, so
// knn_merge_kernel<true> merges the C partial lists as it merges dtw_search_kernel's; dtw_occ_finish_kernel (dtw_occ.h) maps an
// entry to its sequence through seqid.
__global__ __launch_bounds__(256) void dtw_occ_kernel(const float* __restrict__ q, const float* __restrict__ qsq,
                                                      const int32_t* __restrict__ meta, const int32_t* __restrict__ slot_phrase,
                                                      const int32_t* __restrict__ block_rows, int P, int ph,
                                                      const float* __restrict__ x, int N, int D, const float* __restrict__ cn, int k,
                                                      const int32_t* __restrict__ seqid, const int32_t* __restrict__ cuts,
                                                      const int32_t* __restrict__ pgrp, const int32_t* __restrict__ sgrp, int C,
                                                      float* __restrict__ ps, int32_t* __restrict__ pi, int2* __restrict__ pp) {
    dtw_scan_body<true>(q, qsq, meta, slot_phrase, block_rows, P, ph, x, N, D, cn, k, seqid, cuts, pgrp, sgrp, C, ps, pi, pp);
}

// fillers -> (+inf, -1, (-1, -1)); spans as (first row, one past the last row)
__global__ __launch_bounds__(256) void dtw_finish_kernel(const float* __restrict__ ls, const int32_t* __restrict__ li, const int2* __restrict__ lp,
                                                         int64_t tot, float* __restrict__ cost, int64_t* __restrict__ seq, int64_t* __restrict__ span) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tot) return;
    const int j = li[e];
    if (j == INT_MAX) { cost[e] = INFINITY; seq[e] = -1; span[2 * e] = -1; span[2 * e + 1] = -1; return; }
    const int2 p = lp[e];
    cost[e] = ls[e]; seq[e] = j; span[2 * e] = p.x; span[2 * e + 1] = (int64_t)p.y + 1;
}

// Host only.  Packs the phrases, in order, into query blocks of 128 rows and cuts the database at sequence starts.
extern "C" int32_t sylber_dtw_plan(const int32_t* seq_offsets_host, int32_t n_seq, const int32_t* phrase_len_host, int32_t n_phrases,
                                   int32_t k, int32_t splits, int32_t block_phrases, int32_t* cut_rows_host, int32_t cut_capacity,
                                   int32_t* phrase_row_host, int32_t* blocks_out, int32_t* block_phrases_out) {
    if (!seq_offsets_host || !phrase_len_host || n_seq < 1 || n_phrases < 1 || k < 1 || k > KN_KMAX || splits < 0 || block_phrases < 0) return -1;
    if (seq_offsets_host[0] != 0) return -4;
    for (int32_t s = 0; s < n_seq; ++s) {
        const int64_t len = (int64_t)seq_offsets_host[s + 1] - seq_offsets_host[s];
        if (len < 1) return -4;
        if (len > DT_MAX_SEQ) return -3;
    }
    const int ph = dt_block_phrases(k, block_phrases);
    int64_t blk = 0;
    int r = 0, cnt = 0;
    for (int32_t p = 0; p < n_phrases; ++p) {
        const int m = phrase_len_host[p];
        if (m < 1 || m > DT_MAX_M) return -2;
        if ((r & 63) + m > 64) r = (r + 63) & ~63;         // a phrase lies inside one 64-row half: one wave owns it
        if (r + m > KN_BM || cnt == ph) { ++blk; r = 0; cnt = 0; }
        if (phrase_row_host) phrase_row_host[p] = (int32_t)(blk * KN_BM + r);
        r += m; ++cnt;
    }
    const int64_t nb = blk + 1;
    if (nb * KN_BM > INT32_MAX) return -1;
    const int64_t N = seq_offsets_host[n_seq], tiles = (N + KN_BN - 1) / KN_BN;
    int64_t Cw = splits;
    if (Cw <= 0) {
        Cw = (DT_TARGET_BLOCKS + nb - 1) / nb;
        const int64_t cap = tiles / DT_MIN_TILES;
        Cw = Cw < cap ? Cw : cap;
    }
    Cw = Cw < 65535 ? Cw : 65535;
    Cw = Cw < 1 ? 1 : Cw;
    // cut c begins at the first sequence start at or after row c N / Cw; equal boundaries collapse
    int64_t C = 0, last = 0;
    int32_t s = 0;
    if (cut_rows_host) { if (cut_capacity < 2) return -1; cut_rows_host[0] = 0; }
    for (int64_t c = 1; c < Cw; ++c) {
        const int64_t target = c * N / Cw;
        while (s < n_seq && seq_offsets_host[s] < target) ++s;
        if (s >= n_seq) break;
        const int64_t row = seq_offsets_host[s];
        if (row <= last) continue;
        ++C;
        if (cut_rows_host) { if (C + 1 >= cut_capacity) return -1; cut_rows_host[C] = (int32_t)row; }
        last = row;
    }
    ++C;
    if (cut_rows_host) cut_rows_host[C] = (int32_t)N;
    if (blocks_out) *blocks_out = (int32_t)nb;
    if (block_phrases_out) *block_phrases_out = ph;
    return (int32_t)C;
}

extern "C" int64_t sylber_dtw_workspace_bytes(int32_t n_blocks, int32_t n_phrases, int32_t k, int32_t cuts) {
    if (n_blocks < 1 || n_phrases < 1 || k < 1 || k > KN_KMAX || cuts < 1) return -1;
    const int64_t L = (int64_t)n_phrases * cuts * k, L2 = (int64_t)n_phrases * ((cuts + 1) / 2) * k;
    // ||q||^2 [n_blocks * 128] | costs, sequences, spans [P][C][k] | the same [P][ceil(C / 2)][k]
    return kn_al((int64_t)n_blocks * KN_BM * 4) + 2 * kn_al(L * 4) + kn_al(L * 8) + 2 * kn_al(L2 * 4) + kn_al(L2 * 8);
}

// the argument checks of sylber_dtw_search and sylber_dtw_occurrences, which take the same arguments
static int dt_scan_check(const char* what, const float* q_dev, int32_t n_blocks, const int32_t* row_meta_dev, const int32_t* slot_phrase_dev,
                         const int32_t* block_rows_dev, int32_t n_phrases, int32_t block_phrases, const float* db_dev, int32_t N, int32_t D,
                         const float* db_norm_dev, int32_t metric, int32_t k, const int32_t* seq_id_dev, const int32_t* cut_rows_dev,
                         int32_t cuts, const int32_t* phrase_group_dev, const int32_t* seq_group_dev, const float* cost_dev,
                         const int64_t* seq_dev, const int64_t* span_dev, const void* workspace_dev) {
    if (!q_dev || !row_meta_dev || !slot_phrase_dev || !block_rows_dev || !db_dev || !seq_id_dev || !cut_rows_dev || !cost_dev || !seq_dev ||
        !span_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n_blocks < 1 || n_phrases < 1 || N < 1 || D < 16 || D % 16) { syl_set_error(what, "need n_blocks, n_phrases, N >= 1 and D a multiple of 16"); return 1; }
    if (k < 1 || k > KN_KMAX) { syl_set_error(what, "need 1 <= k <= 128"); return 1; }
    if (block_phrases < 1 || block_phrases > dt_block_phrases(k, 0)) { syl_set_error(what, "block_phrases exceeds what sylber_dtw_plan allows for this k"); return 1; }
    if (cuts < 1 || cuts > 65535) { syl_set_error(what, "need 1 <= cuts <= 65535"); return 1; }
    if (metric != SYLBER_KNN_L2 && metric != SYLBER_KNN_IP) { syl_set_error(what, "unknown metric"); return 1; }
    if (metric == SYLBER_KNN_L2 && !db_norm_dev) { syl_set_error(what, "the L2 metric needs db_norm_dev"); return 1; }
    if (!phrase_group_dev != !seq_group_dev) { syl_set_error(what, "phrase_group_dev and seq_group_dev go together"); return 1; }
    if ((int64_t)n_phrases * cuts * k > INT32_MAX / 2) { syl_set_error(what, "n_phrases x cuts x k is too large: use smaller phrase chunks"); return 1; }
    return 0;
}

extern "C" int sylber_dtw_search(const float* q_dev, int32_t n_blocks, const int32_t* row_meta_dev, const int32_t* slot_phrase_dev,
                                 const int32_t* block_rows_dev, int32_t n_phrases, int32_t block_phrases, const float* db_dev, int32_t N,
                                 int32_t D, const float* db_norm_dev, int32_t metric, int32_t k, const int32_t* seq_id_dev,
                                 const int32_t* cut_rows_dev, int32_t cuts, const int32_t* phrase_group_dev, const int32_t* seq_group_dev,
                                 float* cost_dev, int64_t* seq_dev, int64_t* span_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_dtw_search";
    hipStream_t s = (hipStream_t)stream;
    if (dt_scan_check(what, q_dev, n_blocks, row_meta_dev, slot_phrase_dev, block_rows_dev, n_phrases, block_phrases, db_dev, N, D, db_norm_dev,
                      metric, k, seq_id_dev, cut_rows_dev, cuts, phrase_group_dev, seq_group_dev, cost_dev, seq_dev, span_dev, workspace_dev)) return 1;
    const int64_t L = (int64_t)n_phrases * cuts * k, L2 = (int64_t)n_phrases * ((cuts + 1) / 2) * k;
    char* w = (char*)workspace_dev;
    float* qsq = (float*)w; w += kn_al((int64_t)n_blocks * KN_BM * 4);
    float* s0 = (float*)w; w += kn_al(L * 4);
    int32_t* i0 = (int32_t*)w; w += kn_al(L * 4);
    int2* p0 = (int2*)w; w += kn_al(L * 8);
    float* s1 = (float*)w; w += kn_al(L2 * 4);
    int32_t* i1 = (int32_t*)w; w += kn_al(L2 * 4);
    int2* p1 = (int2*)w;
    if (metric == SYLBER_KNN_L2 && launch_km_sqnorm(q_dev, qsq, n_blocks * KN_BM, D, s)) return 1;
    static PerDeviceOnce once;
    if (once.need())
        HIP_TRY(hipFuncSetAttribute((const void*)dtw_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)((size_t)DT_FIXED * 4 + DT_LIST_BYTES)));
    hipLaunchKernelGGL(dtw_search_kernel, dim3((unsigned)n_blocks, (unsigned)cuts), dim3(256), dt_lds_bytes(block_phrases, k), s, q_dev,
                       metric == SYLBER_KNN_L2 ? qsq : nullptr, row_meta_dev, slot_phrase_dev, block_rows_dev, n_phrases, block_phrases, db_dev,
                       N, D, metric == SYLBER_KNN_L2 ? db_norm_dev : nullptr, k, seq_id_dev, cut_rows_dev, phrase_group_dev, seq_group_dev,
                       cuts, s0, i0, p0);
    HIP_TRY(hipGetLastError());
    float* cs = s0; int32_t* ci = i0; int2* cp = p0;
    float* os = s1; int32_t* oi = i1; int2* op = p1;
    for (int m = cuts; m > 1; m = (m + 1) / 2) {
        hipLaunchKernelGGL(knn_merge_kernel<true>, dim3((unsigned)n_phrases, (unsigned)((m + 1) / 2)), dim3(64), 0, s, cs, ci, (const int2*)cp, m, k,
                           os, oi, op);
        HIP_TRY(hipGetLastError());
        float* ts = cs; cs = os; os = ts;
        int32_t* ti = ci; ci = oi; oi = ti;
        int2* tp = cp; cp = op; op = tp;
    }
    const int64_t tot = (int64_t)n_phrases * k;
    hipLaunchKernelGGL(dtw_finish_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, cs, ci, cp, tot, cost_dev, seq_dev, span_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- every occurrence of a phrase (SyllableIndex.search_occurrences): dtw_occ_kernel above ------------------------------------------
extern "C" int sylber_dtw_occurrences(const float* q_dev, int32_t n_blocks, const int32_t* row_meta_dev, const int32_t* slot_phrase_dev,
                                      const int32_t* block_rows_dev, int32_t n_phrases, int32_t block_phrases, const float* db_dev, int32_t N,
                                      int32_t D, const float* db_norm_dev, int32_t metric, int32_t k, const int32_t* seq_id_dev,
                                      const int32_t* cut_rows_dev, int32_t cuts, const int32_t* phrase_group_dev, const int32_t* seq_group_dev,
                                      float* cost_dev, int64_t* seq_dev, int64_t* span_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_dtw_occurrences";
    hipStream_t s = (hipStream_t)stream;
    if (dt_scan_check(what, q_dev, n_blocks, row_meta_dev, slot_phrase_dev, block_rows_dev, n_phrases, block_phrases, db_dev, N, D, db_norm_dev,
                      metric, k, seq_id_dev, cut_rows_dev, cuts, phrase_group_dev, seq_group_dev, cost_dev, seq_dev, span_dev, workspace_dev)) return 1;
    char* w = (char*)workspace_dev;
    float* qsq = (float*)w; w += kn_al((int64_t)n_blocks * KN_BM * 4);
    const DtOccLists lists = dt_occ_lists_carve(w, n_phrases, cuts, k);
    if (metric == SYLBER_KNN_L2 && launch_km_sqnorm(q_dev, qsq, n_blocks * KN_BM, D, s)) return 1;
    static PerDeviceOnce once;
    if (once.need())
        HIP_TRY(hipFuncSetAttribute((const void*)dtw_occ_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)((size_t)DT_FIXED * 4 + DT_LIST_BYTES)));
    hipLaunchKernelGGL(dtw_occ_kernel, dim3((unsigned)n_blocks, (unsigned)cuts), dim3(256), dt_lds_bytes(block_phrases, k), s, q_dev,
                       metric == SYLBER_KNN_L2 ? qsq : nullptr, row_meta_dev, slot_phrase_dev, block_rows_dev, n_phrases, block_phrases, db_dev,
                       N, D, metric == SYLBER_KNN_L2 ? db_norm_dev : nullptr, k, seq_id_dev, cut_rows_dev, phrase_group_dev, seq_group_dev,
                       cuts, lists.s0, lists.i0, lists.p0);
    HIP_TRY(hipGetLastError());
    return dt_occ_merge_finish(lists, n_phrases, cuts, k, seq_id_dev, nullptr, 0, cost_dev, seq_dev, span_dev, s);
}

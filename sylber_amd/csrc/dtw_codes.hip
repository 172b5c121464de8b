// The exact DTW on a coded database (sylber_amd/pq.py: search_phrases / search_occurrences / align_phrases of IVFPQSyllableIndex and of
// PQSyllableIndex with rerank=False; contract in include/sylber_hip.h, restated in tests/ivfpq_phrase_ref.py and
// tests/occ_ref.py): sylber_dtw_rerank, sylber_dtw_rerank_occurrences and sylber_dtw_align on rows that exist only as
// product-quantization codes, in list order, possibly as residuals to a list centroid.  No row is written anywhere: each float4 of
// the dot-product chain is rebuilt from a code byte and the fp32 codebooks (plus the list centroid) where the chain consumes it.
//   * dtw_rerank_codes_kernel / dtw_occ_rerank_codes_kernel / dtw_align_codes_kernel: dtw_pair.h's dp_rerank_pair and
//     dp_occ_rerank_pair and dtw_align.h's da_align_pair, the bodies of dtw_rerank_kernel, dtw_occ_rerank_kernel and
//     dtw_align_kernel, on DcSrc below in place of a plain pointer.  Lane state, chain, cell, the occurrence rule and its hand-off
//     ballots, predecessor bits, walk back, ranking (dtw_rank_kernel) and the merge of the occurrence lists (dtw_occ.h) are those
//     files'; only where a row's elements come from is here.
//   * DcSrc::chunk, once per chunk of DP_CH = 32 columns: lane jj < 32 resolves column jj -- row id -> position (pos, or the id
//     itself), its mask byte, and for residual codes its list, a binary search of the position in list_offsets (uniform trip count:
//     the bits of nlist) -- and the wave stages the chunk's 32 M code bytes in LDS (2 KiB at M = 64, beside the walk's 9 216 B).
//     The lists and the NaN flags go to every lane as wave-uniform values (readlane, ballot).
//   * DcRows, per segment of dsub = D / M elements: the 32 code bytes of sub-space m are read from LDS once, through
//     __builtin_amdgcn_readfirstlane, so that the codebook and centroid addresses are provably wave-uniform and the loads can be
//     scalar; within the segment a float4 is cb[m][code][c - m dsub ..], for residual codes __fadd_rn(centroid[l][c ..], that) per
//     element: one fp32 addition that is rounded before the chain's fmaf and cannot be contracted into it.
//   * A NaN row (mask byte set, position out of range, or residual-coded and in no list) gets a NaN in element x of every float4:
//     its dot is NaN, and dt_cost turns any NaN into +inf, as it does for the NaN row of the materialised plane.
// LDS: dtw_rerank_codes_kernel 9 216 B (the walk's 64 rows x 36 floats) + 2 048 B of code bytes = 11 264 B;
// dtw_occ_rerank_codes_kernel adds the pair's list, 16 B x k, held for k = 128: 9 216 + 2 048 + 2 048 = 13 312 B;
// dtw_align_codes_kernel the walk, dtw_align.h's DaLds and the code bytes.  64 threads each: the wave slots and registers bound the
// occupancy, not LDS (a CU has 160 KiB).
// Every index that comes from device memory is clamped before it is an address: the position into [0, N), the list into
// [0, nlist) by the search's own bounds; a code byte is below 256 by its type, m below M by the loop.
#include "kernels.h"
#include "dtw_align.h"
#include "dtw_occ.h"

constexpr int DC_MAX_M = 64;                              // PQ_MAX_M of pq.hip

// The coded database: the argument group of include/sylber_hip.h.  The kernels take its arrays as __restrict__ parameters of their
// own (DC_DB_PARAMS), so that the compiler knows that nothing they store can change a codebook and may load it with scalar loads.
#define DC_DB_PARAMS                                                                                                                     \
    const uint8_t *__restrict__ code, const uint8_t *__restrict__ bad, const int32_t *__restrict__ pos, const float *__restrict__ cb,    \
        const int32_t *__restrict__ off, const float *__restrict__ cent, int N, int D, int M, int nlist
#define DC_DB_ARGS(db) db.code, db.bad, db.pos, db.cb, db.off, db.cent, db.N, db.D, db.M, db.nlist
struct DcDb {
    const uint8_t* code;                                   // [N, M] in position order
    const uint8_t* bad;                                    // [N] in position order, or null
    const int32_t* pos;                                    // [N] row id -> position, or null: identity
    const float* cb;                                       // [M, 256, dsub]
    const int32_t* off;                                    // [nlist + 1] positions, or null: the codes are the rows' own
    const float* cent;                                     // [nlist, D]
    int N, D, M, dsub, nlist;
};

template <bool RES>
struct DcRows {
    const uint8_t* sc;                                     // LDS: the chunk's code bytes [DP_CH][M]
    const float* cb;
    const float* cent;                                     // RES: the list centroids
    int D, M, dsub;
    unsigned nan;                                          // bit jj: column jj is a NaN row (wave-uniform)
    int lst[DP_CH];                                        // the list of column jj (wave-uniform; residual codes)
    int at[DP_CH];                                         // this segment: element offset of column jj's centroid in its codebook
    const float* cbm;                                      // this segment: codebook m
    int c0;                                                // this segment: its first element
    __device__ __forceinline__ int seg() const { return dsub; }
    __device__ __forceinline__ void begin(int first) {
        c0 = first;
        const int m = __builtin_amdgcn_readfirstlane(c0 / dsub);
        cbm = cb + (size_t)m * 256 * dsub;
#pragma unroll
        for (int jj = 0; jj < DP_CH; ++jj) at[jj] = __builtin_amdgcn_readfirstlane((int)sc[jj * M + m]) * dsub;
    }
    __device__ __forceinline__ float4 operator()(int jj, int, int c) const {
        float4 v = *(const float4*)(cbm + at[jj] + (c - c0));
        if constexpr (RES) {
            const float4 g = *(const float4*)(cent + (size_t)lst[jj] * D + c);
            v = make_float4(__fadd_rn(g.x, v.x), __fadd_rn(g.y, v.y), __fadd_rn(g.z, v.z), __fadd_rn(g.w, v.w));
        }
        if (nan >> jj & 1u) v.x = NAN;
        return v;
    }
};

template <bool RES>
struct DcSrc {
    DcDb db;
    uint8_t* sc;                                           // LDS [DP_CH * DC_MAX_M]
    __device__ __forceinline__ DcRows<RES> chunk(int lane, int n0, int ncol, int j1) const {
        const int jj = lane & (DP_CH - 1);
        const int j = jj < ncol ? n0 + jj : j1 - 1;        // inside [0, N): the kernels clamp their runs
        int p = db.pos ? db.pos[j] : j;
        bool isnan = p < 0 || p >= db.N;
        p = p < 0 ? 0 : (p < db.N ? p : db.N - 1);
        if (db.bad && db.bad[p]) isnan = true;
        int l = 0;
        if constexpr (RES) {                               // the number of offsets at or below p, less one: empty lists are skipped
            int lo = 0, hi = db.nlist + 1;
            for (int w = db.nlist + 1; w > 0; w >>= 1) {   // wave-uniform trip count, enough for any outcome
                const int mid = (lo + hi) >> 1;
                const bool go = lo < hi && db.off[mid < db.nlist ? mid : db.nlist] <= p;
                if (lo < hi) { if (go) lo = mid + 1; else hi = mid; }
            }
            l = lo - 1;
            if (l < 0 || l >= db.nlist) isnan = true;      // before the lists (stale offsets) or behind them: in no list
            l = l < 0 ? 0 : (l < db.nlist ? l : db.nlist - 1);
        }
        // the previous chunk's bytes are read: its chain lies in front of dp_chunk_costs' two barriers
        for (int m = lane >> 5; m < db.M; m += 2) sc[jj * db.M + m] = db.code[(size_t)p * db.M + m];
        DcRows<RES> r;
        r.sc = sc; r.cb = db.cb; r.cent = db.cent;
        r.D = db.D; r.M = db.M; r.dsub = db.dsub;
        r.nan = (unsigned)(__ballot(isnan) & 0xffffffffull);
#pragma unroll
        for (int e = 0; e < DP_CH; ++e) r.lst[e] = __builtin_amdgcn_readlane(l, e);
        __syncthreads();
        return r;
    }
};

template <bool RES>
__global__ __launch_bounds__(64) void dtw_rerank_codes_kernel(const float* __restrict__ q, const float* __restrict__ qsq, int qrows,
                                                              const int32_t* __restrict__ prow, const int32_t* __restrict__ plen,
                                                              DC_DB_PARAMS, const float* __restrict__ cn, const int32_t* __restrict__ cand,
                                                              const int32_t* __restrict__ soff, int S, int m, float* __restrict__ pc,
                                                              int2* __restrict__ pspan) {
    __shared__ float dsm[DT_MAX_M * DP_LD];
    __shared__ uint8_t sc[DP_CH * DC_MAX_M];
    const DcDb db{code, bad, pos, cb, off, cent, N, D, M, D / M, nlist};
    dp_rerank_pair(dsm, DcSrc<RES>{db, sc}, q, qsq, qrows, prow, plen, db.N, db.D, cn, cand, soff, S, m, pc, pspan);
}

template <bool RES>
__global__ __launch_bounds__(64) void dtw_align_codes_kernel(const float* __restrict__ q, const float* __restrict__ qsq, int qrows,
                                                             const int32_t* __restrict__ prow, const int32_t* __restrict__ plen, int P,
                                                             DC_DB_PARAMS, const float* __restrict__ cn, const int32_t* __restrict__ pp,
                                                             const int2* __restrict__ win, int max_cols, int Mx, int2* __restrict__ rows,
                                                             int32_t* __restrict__ steps, float* __restrict__ cost,
                                                             int32_t* __restrict__ tstart, uint64_t* ws) {
    __shared__ float dsm[DT_MAX_M * DP_LD];
    __shared__ DaLds lds;
    __shared__ uint8_t sc[DP_CH * DC_MAX_M];
    const DcDb db{code, bad, pos, cb, off, cent, N, D, M, D / M, nlist};
    da_align_pair(dsm, lds, DcSrc<RES>{db, sc}, q, qsq, qrows, prow, plen, P, db.N, db.D, cn, pp, win, max_cols, Mx, rows, steps, cost, tstart, ws);
}

template <bool RES>
__global__ __launch_bounds__(64) void dtw_occ_rerank_codes_kernel(const float* __restrict__ q, const float* __restrict__ qsq, int qrows,
                                                                  const int32_t* __restrict__ prow, const int32_t* __restrict__ plen,
                                                                  DC_DB_PARAMS, const float* __restrict__ cn, const int32_t* __restrict__ cand,
                                                                  const int32_t* __restrict__ soff, int S, int m, int k, float* __restrict__ ps,
                                                                  int32_t* __restrict__ pi, int2* __restrict__ pp) {
    __shared__ float dsm[DT_MAX_M * DP_LD];
    __shared__ float ols[KN_KMAX];
    __shared__ int oli[KN_KMAX];
    __shared__ int2 olp[KN_KMAX];
    __shared__ uint8_t sc[DP_CH * DC_MAX_M];
    const DcDb db{code, bad, pos, cb, off, cent, N, D, M, D / M, nlist};
    dp_occ_rerank_pair(dsm, ols, oli, olp, DcSrc<RES>{db, sc}, q, qsq, qrows, prow, plen, db.N, db.D, cn, cand, soff, S, m, k, ps, pi, pp);
}

// the entries' verdict on the coded database, reported behind dt_pair_check's count checks
static const char* dc_db_error(int32_t D, int32_t M, const int32_t* list_offsets_dev, const float* centroid_dev, int32_t nlist) {
    if (M < 1 || M > DC_MAX_M || D % M || (D / M) % 16) return "need 1 <= M <= 64, D % M == 0 and (D / M) % 16 == 0";
    const bool any = list_offsets_dev || centroid_dev || nlist != 0, all = list_offsets_dev && centroid_dev && nlist >= 1;
    if (any && !all) return "list_offsets_dev, centroid_dev and nlist >= 1 go together: all of them (residual codes) or none";
    return nullptr;
}

extern "C" int sylber_dtw_rerank_codes(const float* q_dev, int32_t n_blocks, const float* q_norm_dev, const int32_t* phrase_row_dev,
                                       const int32_t* phrase_len_dev, int32_t n_phrases, const uint8_t* code_dev, const uint8_t* bad_dev,
                                       const int32_t* pos_dev, const float* cb_dev, int32_t M, const int32_t* list_offsets_dev,
                                       const float* centroid_dev, int32_t nlist, int32_t N, int32_t D, const float* db_norm_dev,
                                       int32_t metric, const int32_t* cand_dev, int32_t m, const int32_t* seq_offsets_dev, int32_t n_seq,
                                       int32_t k, float* cost_dev, int64_t* seq_dev, int64_t* span_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_dtw_rerank_codes";
    hipStream_t s = (hipStream_t)stream;
    if (!q_dev || !phrase_row_dev || !phrase_len_dev || !code_dev || !cb_dev || !cand_dev || !seq_offsets_dev || !cost_dev || !seq_dev ||
        !span_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    const float *qn, *cn;
    const char* own = m < 1 || m > KN_KMAX || k < 1 || k > m ? "need 1 <= k <= m <= 128" : nullptr;
    if (dt_pair_check(what, "need n_blocks, n_phrases, N, n_seq >= 1 and D a multiple of 16",
                      own ? own : dc_db_error(D, M, list_offsets_dev, centroid_dev, nlist),
                      "n_phrases x m is too large: use smaller phrase chunks", n_blocks, n_phrases, n_seq, N, D, q_norm_dev, db_norm_dev, metric,
                      (int64_t)n_phrases * m > INT32_MAX, qn, cn)) return 1;
    const DcDb db{code_dev, bad_dev, pos_dev, cb_dev, list_offsets_dev, centroid_dev, N, D, M, D / M, nlist};
    const DpPairResults r(workspace_dev, n_phrases, m);
    hipLaunchKernelGGL(list_offsets_dev ? dtw_rerank_codes_kernel<true> : dtw_rerank_codes_kernel<false>, dim3((unsigned)((int64_t)n_phrases * m)),
                       dim3(64), 0, s, q_dev, qn, n_blocks * KN_BM, phrase_row_dev, phrase_len_dev, DC_DB_ARGS(db), cn, cand_dev, seq_offsets_dev, n_seq, m,
                       r.pc, r.pspan);
    HIP_TRY(hipGetLastError());
    return dp_rank_launch(r, cand_dev, n_phrases, m, k, cost_dev, seq_dev, span_dev, s);
}

extern "C" int sylber_dtw_rerank_occurrences_codes(const float* q_dev, int32_t n_blocks, const float* q_norm_dev, const int32_t* phrase_row_dev,
                                                   const int32_t* phrase_len_dev, int32_t n_phrases, const uint8_t* code_dev,
                                                   const uint8_t* bad_dev, const int32_t* pos_dev, const float* cb_dev, int32_t M,
                                                   const int32_t* list_offsets_dev, const float* centroid_dev, int32_t nlist, int32_t N,
                                                   int32_t D, const float* db_norm_dev, int32_t metric, const int32_t* cand_dev, int32_t m,
                                                   const int32_t* seq_offsets_dev, int32_t n_seq, int32_t k, float* cost_dev, int64_t* seq_dev,
                                                   int64_t* span_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_dtw_rerank_occurrences_codes";
    hipStream_t s = (hipStream_t)stream;
    if (!q_dev || !phrase_row_dev || !phrase_len_dev || !code_dev || !cb_dev || !cand_dev || !seq_offsets_dev || !cost_dev || !seq_dev ||
        !span_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    const float *qn, *cn;
    const char* own = m < 1 || m > KN_KMAX || k < 1 || k > KN_KMAX ? "need 1 <= m <= 128 and 1 <= k <= 128" : nullptr;
    if (dt_pair_check(what, "need n_blocks, n_phrases, N, n_seq >= 1 and D a multiple of 16",
                      own ? own : dc_db_error(D, M, list_offsets_dev, centroid_dev, nlist),
                      "n_phrases x m x k is too large: use smaller phrase chunks", n_blocks, n_phrases, n_seq, N, D, q_norm_dev, db_norm_dev, metric,
                      (int64_t)n_phrases * m * k > INT32_MAX / 2, qn, cn)) return 1;
    const DcDb db{code_dev, bad_dev, pos_dev, cb_dev, list_offsets_dev, centroid_dev, N, D, M, D / M, nlist};
    const DtOccLists lists = dt_occ_lists_carve((char*)workspace_dev, n_phrases, m, k);
    hipLaunchKernelGGL(list_offsets_dev ? dtw_occ_rerank_codes_kernel<true> : dtw_occ_rerank_codes_kernel<false>,
                       dim3((unsigned)((int64_t)n_phrases * m)), dim3(64), 0, s, q_dev, qn, n_blocks * KN_BM, phrase_row_dev, phrase_len_dev,
                       DC_DB_ARGS(db), cn, cand_dev, seq_offsets_dev, n_seq, m, k, lists.s0, lists.i0, lists.p0);
    HIP_TRY(hipGetLastError());
    return dt_occ_merge_finish(lists, n_phrases, m, k, nullptr, seq_offsets_dev, n_seq, cost_dev, seq_dev, span_dev, s);
}

extern "C" int sylber_dtw_align_codes(const float* q_dev, int32_t n_blocks, const float* q_norm_dev, const int32_t* phrase_row_dev,
                                      const int32_t* phrase_len_dev, int32_t n_phrases, const uint8_t* code_dev, const uint8_t* bad_dev,
                                      const int32_t* pos_dev, const float* cb_dev, int32_t M, const int32_t* list_offsets_dev,
                                      const float* centroid_dev, int32_t nlist, int32_t N, int32_t D, const float* db_norm_dev,
                                      int32_t metric, const int32_t* pair_phrase_dev, const int32_t* pair_window_dev, int32_t n_pairs,
                                      int32_t max_cols, int32_t max_rows, int32_t* rows_dev, int32_t* steps_dev, float* cost_dev,
                                      int32_t* start_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_dtw_align_codes";
    hipStream_t s = (hipStream_t)stream;
    if (!q_dev || !phrase_row_dev || !phrase_len_dev || !code_dev || !cb_dev || !pair_phrase_dev || !pair_window_dev || !rows_dev ||
        !steps_dev || !cost_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    const float *qn, *cn;
    const char* own = max_cols < 1 || max_cols > DA_MAX_COLS ? "need 1 <= max_cols <= 65536: a window has at most 65536 rows"
                      : max_rows < 1 || max_rows > DT_MAX_M  ? "need 1 <= max_rows <= 64" : nullptr;
    if (dt_pair_check(what, "need n_blocks, n_phrases, n_pairs, N >= 1 and D a multiple of 16",
                      own ? own : dc_db_error(D, M, list_offsets_dev, centroid_dev, nlist),
                      "too many phrase blocks: use smaller phrase chunks", n_blocks, n_phrases, n_pairs, N, D, q_norm_dev, db_norm_dev, metric, false,
                      qn, cn)) return 1;
    const DcDb db{code_dev, bad_dev, pos_dev, cb_dev, list_offsets_dev, centroid_dev, N, D, M, D / M, nlist};
    hipLaunchKernelGGL(list_offsets_dev ? dtw_align_codes_kernel<true> : dtw_align_codes_kernel<false>, dim3((unsigned)n_pairs), dim3(64), 0, s,
                       q_dev, qn, n_blocks * KN_BM, phrase_row_dev, phrase_len_dev, n_phrases, DC_DB_ARGS(db), cn, pair_phrase_dev, (const int2*)pair_window_dev, max_cols, max_rows, (int2*)rows_dev,
                       steps_dev, cost_dev, start_dev, (uint64_t*)workspace_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Repeated phrases on embeddings: LOCAL alignment of probes (1 .. 64 rows) against every sequence of a SyllableIndex
// (sylber_amd/search.py: SyllableIndex.search_repeats / find_repeats; contract "Embedding repeats" in include/sylber_hip.h, restated
// in tests/repeats_ref.py).
//   * dtw_local_kernel: dtw_search_kernel's grid, staging, K loop, column data and epilogue (dtw.hip, dtw_tile.h, knn_tile.h: the
//     local costs have the bits of SyllableIndex.search's scores); the dynamic programme over the cost tile is new.  Where the
//     subsequence DTW consumes the phrase whole and reads its result off the last row, the local alignment may begin and end in any
//     cell: H[i][j] = max(0, H[i-1][j-1] + s, H[i-1][j] + (s - gap), H[i][j-1] + (s - gap)) with s = radius - d[i][j], and the
//     result of (probe, sequence) is the best cell of the whole [m, L] table.  A lane (= one probe row) keeps the best cell of its
//     row in the current sequence; at the sequence's last column it combines that with what the lane above left there one step
//     earlier, so the maximum over rows travels down the probe with the wavefront and reaches the last row exactly when that row
//     finishes the sequence -- where dt_wavefront's hand-off to the probe's list happens, unchanged.
//   * A list entry stays 16 bytes: (-score, sequence, (first row of the sequence span, the three other span ends packed)), so
//     kn_insert_t<true> and knn_merge_kernel<true> order it by (score descending, sequence ascending) as they are; negation is exact.
//   * dtw_local_finish_kernel unpacks to [P, k, 2, 2], negates back and writes the padding (0, -1, -1).
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "dtw_tile.h"
#include "knn_lists.h"
#include <climits>
#include <cmath>

static size_t dl_lds_bytes(int ph, int k) { return (size_t)DT_FIXED * 4 + (size_t)ph * k * 16; }

// The DP's state of one lane = one probe row i.  Columns are counted from the sequence's first row (< 65 536, DT_MAX_SEQ), so a
// path's start (si, sj) is one int: (sj's column) | si << 22, and a best cell with its start is (column) and start | i << 16.
struct DlLane {
    float h_cur = 0.f, h_prev = 0.f;                       // H[i][last column done], H[i][the one before]
    int t_cur = 0, t_prev = 0;                             // the starts of those paths (read only where H > 0)
    float bh = 0.f;                                        // the best H of row i in the current sequence; 0: none, (bt, bj) mean nothing
    int bt = 0, bj = 0;                                    // its start and its column: the smallest column on ties
    float gh = 0.f;                                        // at a sequence's last column: the best of rows 0 .. i, the upper row on ties
    int gt = 0, gj = 0;                                    // its start | row << 16 and its column
    int seq0 = 0;                                          // the index row of the current sequence's first row
};

// what the lane above left: H[i-1][j], H[i-1][j-1], their starts and, where column j ends a sequence, its (gh, gt, gj)
struct DlUp { float h_cur, h_prev, gh; int t_cur, t_prev, gt, gj; };

__device__ __forceinline__ DlUp dl_up(const DlLane& s) {
    DlUp u;
    u.h_cur = __shfl_up(s.h_cur, 1); u.h_prev = __shfl_up(s.h_prev, 1);
    u.t_cur = __shfl_up(s.t_cur, 1); u.t_prev = __shfl_up(s.t_prev, 1);
    u.gh = __shfl_up(s.gh, 1); u.gt = __shfl_up(s.gt, 1); u.gj = __shfl_up(s.gj, 1);
    return u;
}

// One cell: local cost d of probe row i against index row `col`.  first: the row is its probe's first (nothing comes from above);
// isstart / isend: col is its sequence's first / last row.  The three candidates and their order on ties are the contract's.
__device__ __forceinline__ void dl_cell(DlLane& s, const DlUp& u, int i, bool first, bool isstart, bool isend, float d, int col, float radius,
                                        float gap) {
    if (isstart) { s.seq0 = col; s.bh = 0.f; }
    const int c = col - s.seq0;
    const float sc = radius - d, sg = sc - gap;            // d = +inf: both -inf, every candidate -inf, H = 0
    const float hd = (first || isstart) ? 0.f : u.h_prev;
    const float hu = first ? 0.f : u.h_cur;
    const float hl = isstart ? 0.f : s.h_cur;
    float v = hd + sc;
    int t = hd > 0.f ? u.t_prev : (c | i << 22);
    const float cu = hu + sg;
    if (cu > v) { v = cu; t = u.t_cur; }
    const float cl = hl + sg;
    if (cl > v) { v = cl; t = s.t_cur; }
    const float H = v > 0.f ? v : 0.f;
    s.h_prev = s.h_cur; s.t_prev = s.t_cur;
    s.h_cur = H; s.t_cur = t;
    if (H > s.bh) { s.bh = H; s.bt = t; s.bj = c; }        // columns ascend: the smallest column on ties
    if (isend) {                                           // the lane above was here one step ago and left rows 0 .. i-1's best
        if (!first && u.gh >= s.bh) { s.gh = u.gh; s.gt = u.gt; s.gj = u.gj; }
        else { s.gh = s.bh; s.gt = s.bt | i << 16; s.gj = s.bj; }
    }
}

// Waves 0 and 1, behind the barrier after dt_cost_tile: dt_wavefront's walk (lane l works on column st - (its probe row) at step st
// and keeps its state across tiles).  At a sequence end the lane of a probe's last row holds the best cell of the whole table and
// hands (-score, sequence, spans) to the probe's list, unless the score is below min_score, the sequence is numbered <= after
// (find_repeats' s < t) or the groups exclude it.
__device__ __forceinline__ void dl_wavefront(const DtLds<true>& L, const DtRow& r, DlLane& s, int lane, int n0, int ncol, bool grouped, int m,
                                             float radius, float gap, float min_score, int after) {
    const float* dr = L.dm + r.drow * DT_LD;
    for (int st = 0; st < ncol + r.maxi; ++st) {
        const DlUp u = dl_up(s);
        const int j = st - r.pi;
        bool fin = false;
        int fseq = 0;
        if (r.valid && j >= 0 && j < ncol) {
            const int sj = L.sq[j + 1];
            const bool isend = L.sq[j + 2] != sj;
            dl_cell(s, u, r.pi, r.pi == 0, L.sq[j] != sj, isend, dr[j], n0 + j, radius, gap);
            if (r.lastrow && isend && s.gh >= min_score && sj > after && !(grouped && L.sgs[j] == r.pg)) {
                fseq = sj;
                fin = kn_better(-s.gh, sj, L.ls[r.slot * m + m - 1], L.li[r.slot * m + m - 1]);
            }
        }
        uint64_t fb = __ballot(fin);
        if (!fb) continue;
        const int cs = s.gt & 0xffff;                      // (sj row, (j - sj) | i << 16 | si << 22)
        const int ex = s.seq0 + cs, ey = (s.gj - cs) | (s.gt & 0x0fff0000);
        while (fb) {
            const int c = __ffsll((unsigned long long)fb) - 1;
            fb &= fb - 1;
            const float v = __shfl(-s.gh, c);
            const int vs = __shfl(fseq, c), sl = __shfl(r.slot, c);
            const int2 span = make_int2(__shfl(ex, c), __shfl(ey, c));
            kn_insert_t<true>(L.ls + sl * m, L.li + sl * m, L.lp + sl * m, m, lane, v, vs, span);
        }
    }
}

// dtw_scan_body's walk (dtw.hip) around dl_wavefront.  meta[r] of packed query row r: -1 = padding, else (row of its probe) |
// (is the probe's last row) << 7 | (probe slot in the block) << 8
__global__ __launch_bounds__(256) void dtw_local_kernel(const float* __restrict__ q, const float* __restrict__ qsq,
                                                        const int32_t* __restrict__ meta, const int32_t* __restrict__ slot_phrase,
                                                        const int32_t* __restrict__ block_rows, int P, int ph,
                                                        const float* __restrict__ x, int N, int D, const float* __restrict__ cn, int k,
                                                        float radius, float gap, float min_score, const int32_t* __restrict__ seqid,
                                                        const int32_t* __restrict__ cuts, const int32_t* __restrict__ pgrp,
                                                        const int32_t* __restrict__ sgrp, const int32_t* __restrict__ after_seq, int C,
                                                        float* __restrict__ ps, int32_t* __restrict__ pi, int2* __restrict__ pp) {
    extern __shared__ __attribute__((aligned(16))) float dl_smem[];
    float* xs = dl_smem;                                   // staging of the query rows
    float* cs = dl_smem + KN_BM * KN_LD;                   // staging of the database rows
    const DtLds<true> L(dl_smem, ph, k);
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
    bool live[2];                                          // wave-uniform: this wave's 32-row half holds probe rows
    float qn[2] = {0.f, 0.f};
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
        live[fm] = wm * 64 + fm * 32 < nrow;
        if (qsq) qn[fm] = qsq[(size_t)b * KN_BM + wm * 64 + fm * 32 + frow];
    }
    const DtRow row(meta, slot_phrase, pgrp, b, P, ph, wave, lane);
    int after = -1;                                        // of a probe's last row: sequences numbered <= after are not admissible
    if (after_seq && row.valid && row.lastrow) {
        const int pid = slot_phrase[(size_t)b * KN_BM + row.slot];
        after = pid >= 0 && pid < P ? after_seq[pid] : -1;
    }
    DlLane st;

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
        dl_wavefront(L, row, st, lane, n0, ncol, sgrp != nullptr, k, radius, gap, min_score, after);
    }
    __syncthreads();
    dt_write_lists(L, slot_phrase, b, P, ph, C, cut, k, wave, lane, ps, pi, pp);
}

// fillers -> (0, -1, -1); score = -(the list's cost); span[e] = ((si, i + 1), (sj row, j row + 1))
__global__ __launch_bounds__(256) void dtw_local_finish_kernel(const float* __restrict__ ls, const int32_t* __restrict__ li,
                                                               const int2* __restrict__ lp, int64_t tot, float* __restrict__ score,
                                                               int64_t* __restrict__ seq, int64_t* __restrict__ span) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tot) return;
    const int j = li[e];
    if (j == INT_MAX) {
        score[e] = 0.f; seq[e] = -1;
        span[4 * e] = -1; span[4 * e + 1] = -1; span[4 * e + 2] = -1; span[4 * e + 3] = -1;
        return;
    }
    const int2 p = lp[e];
    score[e] = -ls[e]; seq[e] = j;
    span[4 * e] = (p.y >> 22) & 63; span[4 * e + 1] = ((p.y >> 16) & 63) + 1;
    span[4 * e + 2] = p.x; span[4 * e + 3] = (int64_t)p.x + (p.y & 0xffff) + 1;
}

extern "C" int sylber_dtw_local(const float* q_dev, int32_t n_blocks, const int32_t* row_meta_dev, const int32_t* slot_phrase_dev,
                                const int32_t* block_rows_dev, int32_t n_phrases, int32_t block_phrases, const float* db_dev, int32_t N,
                                int32_t D, const float* db_norm_dev, int32_t metric, int32_t k, float radius, float gap, float min_score,
                                const int32_t* seq_id_dev, const int32_t* cut_rows_dev, int32_t cuts, const int32_t* phrase_group_dev,
                                const int32_t* seq_group_dev, const int32_t* after_seq_dev, float* score_dev, int64_t* seq_dev,
                                int64_t* span_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_dtw_local";
    hipStream_t s = (hipStream_t)stream;
    if (!q_dev || !row_meta_dev || !slot_phrase_dev || !block_rows_dev || !db_dev || !seq_id_dev || !cut_rows_dev || !score_dev || !seq_dev ||
        !span_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n_blocks < 1 || n_phrases < 1 || N < 1 || D < 16 || D % 16) { syl_set_error(what, "need n_blocks, n_phrases, N >= 1 and D a multiple of 16"); return 1; }
    if (k < 1 || k > KN_KMAX) { syl_set_error(what, "need 1 <= k <= 128"); return 1; }
    if (block_phrases < 1 || block_phrases > dt_block_phrases(k, 0)) { syl_set_error(what, "block_phrases exceeds what sylber_dtw_plan allows for this k"); return 1; }
    if (cuts < 1 || cuts > 65535) { syl_set_error(what, "need 1 <= cuts <= 65535"); return 1; }
    if (metric != SYLBER_KNN_L2 && metric != SYLBER_KNN_IP) { syl_set_error(what, "unknown metric"); return 1; }
    if (metric == SYLBER_KNN_L2 && !db_norm_dev) { syl_set_error(what, "the L2 metric needs db_norm_dev"); return 1; }
    if (!phrase_group_dev != !seq_group_dev) { syl_set_error(what, "phrase_group_dev and seq_group_dev go together"); return 1; }
    if (!std::isfinite(radius) || !(radius > 0.f)) { syl_set_error(what, "need a finite radius > 0"); return 1; }
    if (!std::isfinite(gap) || !(gap >= 0.f)) { syl_set_error(what, "need a finite gap >= 0"); return 1; }
    if (!std::isfinite(min_score) || !(min_score > 0.f)) { syl_set_error(what, "need a finite min_score > 0"); return 1; }
    if ((int64_t)n_phrases * cuts * k > INT32_MAX / 2) { syl_set_error(what, "n_phrases x cuts x k is too large: use smaller phrase chunks"); return 1; }
    // sylber_dtw_workspace_bytes' layout: ||q||^2 [n_blocks * 128] | costs, sequences, spans [P][C][k] | the same [P][ceil(C / 2)][k]
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
        HIP_TRY(hipFuncSetAttribute((const void*)dtw_local_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)((size_t)DT_FIXED * 4 + DT_LIST_BYTES)));
    hipLaunchKernelGGL(dtw_local_kernel, dim3((unsigned)n_blocks, (unsigned)cuts), dim3(256), dl_lds_bytes(block_phrases, k), s, q_dev,
                       metric == SYLBER_KNN_L2 ? qsq : nullptr, row_meta_dev, slot_phrase_dev, block_rows_dev, n_phrases, block_phrases, db_dev,
                       N, D, metric == SYLBER_KNN_L2 ? db_norm_dev : nullptr, k, radius, gap, min_score, seq_id_dev, cut_rows_dev,
                       phrase_group_dev, seq_group_dev, after_seq_dev, cuts, s0, i0, p0);
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
    hipLaunchKernelGGL(dtw_local_finish_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, cs, ci, cp, tot, score_dev, seq_dev, span_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Two-stage phrase search (sylber_amd/search.py: SyllableIndex.search_phrases_refined; contract in include/sylber_hip.h, restated in
// tests/dtw16_ref.py): a 16-bit MFMA subsequence-DTW scan picks m = k * refine candidate sequences per phrase, the exact fp32
// subsequence DTW of sylber_dtw_search re-ranks only those.
//   * dtw16_scan_kernel<FMT>: dtw_search_kernel's structure -- grid (query blocks of whole phrases) x C database cuts on sequence
//     starts, the 128 x 128 cost tile in LDS aliasing the staging, the anti-diagonal wavefront on waves 0 and 1 with the lane state
//     carried over tile edges -- around knn16_scan_kernel's contraction (knn16_tile.h: 16-bit staging, v_mfma_f32_32x32x16_{f16,bf16},
//     K steps of 32).  dot16 is one MFMA chain over K in ascending 16-wide steps whatever tile, cut or block row computes it, and
//     the DP adds in a fixed cell order, so a coarse cost's bits are a function of (phrase, sequence) alone.  No start is tracked
//     and a list entry is (cost, sequence) without a span: 8 B, half of dtw_search_kernel's.  Of dtw_tile.h's pieces the kernel
//     uses the column data (dt_tile_meta) and keeps the rest written out, as knn16_scan_kernel keeps its K loop: built from the
//     shared epilogue and wavefront (as dtwpq_scan_kernel and dtw_search_kernel are) its register allocation around the
//     accumulators came out different and search_phrases_refined measured 0.5 to 1.4 % slower
//     (profiles/phrase_scan_refactor_ab.md); as written its instructions are those it had before the pieces existed.  The text is
//     dtw_tile.h's, SPAN = false: tests/test_gpu_dtwpq.py holds dtwpq_scan_kernel, which is built from the pieces, bitwise to this
//     kernel on the materialised plane.  The C partial lists of a phrase are merged by knn_lists.h's merge; the host path is
//     dtw16_scan.h's, shared with sylber_dtwpq_scan.
//   * dtw_rerank_kernel: one wave per (phrase, candidate) pair, lane l owns phrase row l.  The wave walks the candidate sequence in
//     chunks; the lane's set-up, a chunk's local costs (the explicit ascending __builtin_fmaf chain that gives every A[i][j] the
//     bits of dtw_search_kernel's) and the wavefront over a chunk are dtw_pair.h's, shared with dtw_occ_rerank_kernel below and
//     dtw_align.hip's dtw_align_kernel; the cell is dtw_tile.h's dt_cell.  The lane of the last row tracks (best cost, start, end),
//     the smallest end on ties.  Only the chunk loop depends on the length.
//     The body is dtw_pair.h's dp_rerank_pair, which dtw_codes.hip runs on a coded database.
//   * dtw_rank_kernel (dtw_pair.h): one wave per phrase ranks its m pair results by (cost, sequence) and writes the best k with
//     spans as row ids.  A second launch: nothing relies on an order between workgroups.
//   * dtw_occ_rerank_kernel (at the end of the file; SyllableIndex.search_occurrences_refined, tests/occ_ref.py): dtw_rerank_kernel's
//     walk (the same pieces of dtw_pair.h, dt_occ_cell for the cell and two ballots after it) with every non-overlapping occurrence
//     of the candidate kept, k per pair in LDS; merged and reported by dtw_occ.h.  The body is dtw_pair.h's dp_occ_rerank_pair.
// LDS and occupancy (a CU has 160 KiB):
//   dtw16_scan_kernel   69 136 B fixed (cost tile 67 584 | c_j, sequence ids, groups) + 8 B x (phrases of the block) x m <= 32 KiB
//                       of lists = at most 101 904 B: one workgroup of 4 waves per CU (dtw_search_kernel: 134 672 B, also one); two
//                       per CU while the lists take at most 12 784 B, e.g. 128 phrases at m <= 12 or 32 phrases at m <= 49.  Two
//                       matter: one workgroup's contraction then hides under the other's wavefront (profiles/phrase_bench.md:
//                       219 ms against 399 ms for the same work).
//   dtw_rerank_kernel   9 216 B (64 rows x 36 floats), 64 threads: LDS allows 17 workgroups per CU, so the wave slots and registers
//                       bound it, not LDS.  dtw_occ_rerank_kernel adds its list (16 B x k, held for k = 128): 11 264 B.
#include "kernels.h"
#include "dtw16_scan.h"
#include "dtw_pair.h"
#include "dtw_occ.h"

// meta / slot_phrase / block_rows / cuts / groups as dtw_search_kernel.  q: the packed phrase blocks' 16-bit rows [n_blocks * 128, D],
// qsq: the fp32 ||q_i||^2 of the unrounded packed rows (L2) or null (cosine); x: the 16-bit plane; cn: the fp32 ||x_j||^2 (L2) or null.
// Writes the sorted best m (cost, sequence) of every phrase over the cut to ps / pi [P][C][m]; entries that did not fill stay
// (+inf, INT_MAX).  Written out: see the file header.
template <int FMT>
__global__ __launch_bounds__(256) void dtw16_scan_kernel(const bf16_t* __restrict__ q, const float* __restrict__ qsq,
                                                         const int32_t* __restrict__ meta, const int32_t* __restrict__ slot_phrase,
                                                         const int32_t* __restrict__ block_rows, int P, int ph,
                                                         const bf16_t* __restrict__ x, int N, int D, const float* __restrict__ cn, int m,
                                                         const int32_t* __restrict__ seqid, const int32_t* __restrict__ cuts,
                                                         const int32_t* __restrict__ pgrp, const int32_t* __restrict__ sgrp, int C,
                                                         float* __restrict__ ps, int32_t* __restrict__ pi) {
    extern __shared__ __attribute__((aligned(16))) float dt_smem[];
    bf16_t* xs = (bf16_t*)dt_smem;                         // staging of the query rows [128][K16_LD]
    bf16_t* cs = xs + KN_BM * K16_LD;                      // staging of the database rows
    float* dm = dt_smem;                                   // [128][DT_LD] local costs of the tile, aliasing the staging
    float* cns = dt_smem + KN_BM * DT_LD;
    int* sq = (int*)(cns + KN_BN);                         // [130] sequence of columns n0 - 1 .. n0 + 128 (-1 outside the cut)
    int* sgs = sq + 132;                                   // [128] group of each column's sequence
    float* ls = (float*)(sgs + KN_BN);                     // [ph][m] sorted coarse costs
    int* li = (int*)(ls + ph * m);                         // [ph][m] their sequences
    const DtLds<false> L(dt_smem, ph, m);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int b = blockIdx.x, cut = blockIdx.y;
    int rlo = cuts[cut], rhi = cuts[cut + 1];
    rlo = rlo < 0 ? 0 : rlo; rhi = rhi > N ? N : rhi;
    const int nrow = block_rows[b];
    const int tiles = rhi > rlo ? (rhi - rlo + KN_BN - 1) / KN_BN : 0;
    for (int e = tid; e < ph * m; e += 256) { ls[e] = INFINITY; li[e] = INT_MAX; }
    // staging: thread -> operand row tid >> 1, halves [16 (tid & 1), 16 (tid & 1) + 16) of the K step, as knn16_scan_kernel
    const int sr = tid >> 1, sh = (tid & 1) * 16;
    const bf16_t* qrow = q + ((size_t)b * KN_BM + sr) * D;
    bf16_t* xdst = xs + sr * K16_LD + sh;
    bf16_t* cdst = cs + sr * K16_LD + sh;
    const int frow = lane & 31, fh = lane >> 5;
    const int ksteps = (D + K16_BK - 1) / K16_BK, T = ksteps * tiles;
    bool live[2];                                          // wave-uniform: this wave's 32-row half holds phrase rows
    float qn[2] = {0.f, 0.f};
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
        live[fm] = wm * 64 + fm * 32 < nrow;
        if (qsq) qn[fm] = qsq[(size_t)b * KN_BM + wm * 64 + fm * 32 + frow];
    }
    // the DP's lane state: waves 0 and 1 own packed rows wave * 64 + lane
    const int drow = (wave & 1) * 64 + lane;
    const int mt = wave < 2 ? meta[(size_t)b * KN_BM + drow] : -1;
    const int pi_ = mt & 127, lastrow = (mt >> 7) & 1, slot = (mt >> 8) & 255;
    const bool valid = mt >= 0 && slot < ph;
    int maxi = valid ? pi_ : -1;
#pragma unroll
    for (int o = 32; o; o >>= 1) { const int v = __shfl_xor(maxi, o); maxi = v > maxi ? v : maxi; }
    int pg = 0;
    if (pgrp && valid && lastrow) { const int pid = slot_phrase[(size_t)b * KN_BM + slot]; pg = pid >= 0 && pid < P ? pgrp[pid] : 0; }
    float a_cur = INFINITY, a_prev = INFINITY, bc = INFINITY;      // A[i][last column done], A[i][the one before], best of the sequence

    f32x16_t acc[2][2];
    uint4 xa, xb, ca, cb;
    auto fetch = [&](int t) {
        const int tile = t / ksteps, k0 = (t % ksteps) * K16_BK;
        int cr = rlo + tile * KN_BN + sr; cr = cr < rhi ? cr : rhi - 1;
        const bool in = k0 + sh < D;                       // D % 16 == 0: a last K step of 16 is completed with zeros on both sides
        const int kc = in ? sh + k0 : 0;                   // the loads stay inside the rows either way
        const bf16_t* crow = x + (size_t)cr * D + kc;
        const uint4 z = make_uint4(0, 0, 0, 0);
        xa = *(const uint4*)(qrow + kc); xb = *(const uint4*)(qrow + kc + 8);
        ca = *(const uint4*)crow; cb = *(const uint4*)(crow + 8);
        if (!in) { xa = z; xb = z; ca = z; cb = z; }
    };
    if (T > 0) fetch(0);
    for (int t = 0; t < T; ++t) {
        const int tile = t / ksteps, ks = t % ksteps, n0 = rlo + tile * KN_BN;
        if (ks == 0) kn_zero(acc);
        __syncthreads();                                   // previous fragments, the cost tile, cns / sq / sgs are all read
        *(uint4*)xdst = xa; *(uint4*)(xdst + 8) = xb;
        *(uint4*)cdst = ca; *(uint4*)(cdst + 8) = cb;
        if (ks == 0) {
            dt_tile_meta(L, tid, n0, rlo, rhi, cn, seqid, sgrp, [](int) { return false; });
        }
        __syncthreads();
        if (t + 1 < T) fetch(t + 1);
        k16_mma<FMT>(xs, cs, wm, wn, frow, fh, acc, live[0], live[1]);
        if (ks != ksteps - 1) continue;
        // epilogue: lane holds phrase row wm*64 + fm*32 + frow against columns wn*64 + fn*32 + 8g + 4fh + e.  t = fmaf(-2, dot16, c_j);
        // d~ = max(0, ||q||^2 + t) (L2) or max(0, 1 - (-t / 2)) (cosine), dtw_search_kernel's expressions; a NaN d~ counts as +inf.
        __syncthreads();                                   // every wave is past its fragment reads: the cost tile aliases the staging
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
                    for (int e = 0; e < 4; ++e) {
                        const int cl = wn * 64 + fn * 32 + 8 * g + 4 * fh + e;
                        const float s = fmaf(-2.0f, acc[fm][fn][4 * g + e], cns[cl]);
                        const float v = qsq ? qn[fm] + s : 1.0f - (0.f - 0.5f * s);
                        d[e] = v != v ? INFINITY : fmaxf(0.f, v);
                    }
                    *(float4*)(dm + rl * DT_LD + wn * 64 + fn * 32 + 8 * g + 4 * fh) = make_float4(d[0], d[1], d[2], d[3]);
                }
        }
        __syncthreads();
        if (wave >= 2 || maxi < 0) continue;               // wave-uniform
        const int ncol = rhi - n0 < KN_BN ? rhi - n0 : KN_BN;
        const float* dr = dm + drow * DT_LD;
        for (int st = 0; st < ncol + maxi; ++st) {
            const float u_cur = __shfl_up(a_cur, 1), u_prev = __shfl_up(a_prev, 1);
            const int j = st - pi_;
            bool fin = false;
            int fseq = 0;
            if (valid && j >= 0 && j < ncol) {
                const float d = dr[j];
                const int sj = sq[j + 1];
                const bool isstart = sq[j] != sj;
                float A;
                if (pi_ == 0) A = d;
                else {
                    float best = isstart ? INFINITY : u_prev;          // (i-1, j-1), then (i-1, j), then (i, j-1): the first smallest
                    if (u_cur < best) best = u_cur;
                    const float left = isstart ? INFINITY : a_cur;
                    if (left < best) best = left;
                    A = d + best;
                }
                a_prev = a_cur; a_cur = A;
                if (lastrow) {
                    if (isstart) bc = INFINITY;
                    if (A < bc) bc = A;
                    if (sq[j + 2] != sj && bc < INFINITY && !(sgrp && sgs[j] == pg)) {
                        fseq = sj;
                        fin = kn_better(bc, sj, ls[slot * m + m - 1], li[slot * m + m - 1]);
                    }
                }
            }
            uint64_t fb = __ballot(fin);
            while (fb) {
                const int c = __ffsll((unsigned long long)fb) - 1;
                fb &= fb - 1;
                const float v = __shfl(bc, c);
                const int vs = __shfl(fseq, c), sl = __shfl(slot, c);
                kn_insert(ls + sl * m, li + sl * m, m, lane, v, vs);
            }
        }
    }
    __syncthreads();
    for (int sl = wave; sl < ph; sl += 4) {
        const int pid = slot_phrase[(size_t)b * KN_BM + sl];
        if (pid < 0 || pid >= P) break;
        const size_t o = ((size_t)pid * C + cut) * m;
        for (int e = lane; e < m; e += 64) { ps[o + e] = ls[sl * m + e]; pi[o + e] = li[sl * m + e]; }
    }
}

// Workgroup (one wave) e of phrase p = blockIdx.x / m: the exact subsequence DTW of phrase p (rows prow[p] .. + plen[p] of the packed
// fp32 blocks q, qsq their ||q_i||^2 (L2) or null) against sequence cand[p][e] (rows soff[s] .. soff[s + 1] of x).  Writes (cost,
// (start row, end row)) to pc / pspan [P][m]; (+inf, (-1, -1)) for a candidate of -1.
__global__ __launch_bounds__(64) void dtw_rerank_kernel(const float* __restrict__ q, const float* __restrict__ qsq, int qrows,
                                                        const int32_t* __restrict__ prow, const int32_t* __restrict__ plen,
                                                        const float* __restrict__ x, int N, int D, const float* __restrict__ cn,
                                                        const int32_t* __restrict__ cand, const int32_t* __restrict__ soff, int S,
                                                        int m, float* __restrict__ pc, int2* __restrict__ pspan) {
    __shared__ float dsm[DT_MAX_M * DP_LD];
    dp_rerank_pair(dsm, DpRowsSrc{x, D}, q, qsq, qrows, prow, plen, N, D, cn, cand, soff, S, m, pc, pspan);
}

extern "C" int64_t sylber_dtw16_workspace_bytes(int32_t n_phrases, int32_t m, int32_t cuts) {
    if (n_phrases < 1 || m < 1 || m > KN_KMAX || cuts < 1) return -1;
    // the C partial lists of the scan and their merge rounds (KnPartials); then, in the same bytes, the pair results of the re-rank
    const int64_t scan = kn_partials_bytes(n_phrases, cuts, m), rr = dp_rerank_bytes(n_phrases, m);
    return scan > rr ? scan : rr;
}

extern "C" int sylber_dtw16_scan(const void* q16_dev, int32_t n_blocks, const int32_t* row_meta_dev, const int32_t* slot_phrase_dev,
                                 const int32_t* block_rows_dev, int32_t n_phrases, int32_t block_phrases, const void* db16_dev, int32_t N,
                                 int32_t D, const float* db_norm_dev, const float* q_norm_dev, int32_t metric, int32_t storage, int32_t m,
                                 const int32_t* seq_id_dev, const int32_t* cut_rows_dev, int32_t cuts, const int32_t* phrase_group_dev,
                                 const int32_t* seq_group_dev, int32_t* cand_dev, float* coarse_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_dtw16_scan";
    hipStream_t s = (hipStream_t)stream;
    if (!q16_dev || !row_meta_dev || !slot_phrase_dev || !block_rows_dev || !db16_dev || !seq_id_dev || !cut_rows_dev || !cand_dev ||
        !coarse_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    return dt16_scan_host(what, nullptr, "the L2 metric needs db_norm_dev and q_norm_dev", n_blocks, n_phrases, block_phrases, N, D, db_norm_dev,
                          q_norm_dev, metric, storage, m, cuts, phrase_group_dev, seq_group_dev, cand_dev, coarse_dev, workspace_dev, s,
                          [&](auto fmt, dim3 grid, size_t lds, int max_lds, const float* qn, const float* cn, float* ps, int32_t* pi) {
        constexpr int FMT = decltype(fmt)::value;
        static PerDeviceOnce once;
        if (once.need()) HIP_TRY(hipFuncSetAttribute((const void*)dtw16_scan_kernel<FMT>, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
        hipLaunchKernelGGL(dtw16_scan_kernel<FMT>, grid, dim3(256), lds, s, (const bf16_t*)q16_dev, qn, row_meta_dev, slot_phrase_dev,
                           block_rows_dev, n_phrases, block_phrases, (const bf16_t*)db16_dev, N, D, cn, m, seq_id_dev, cut_rows_dev,
                           phrase_group_dev, seq_group_dev, cuts, ps, pi);
        return 0;
    });
}

extern "C" int sylber_dtw_rerank(const float* q_dev, int32_t n_blocks, const float* q_norm_dev, const int32_t* phrase_row_dev,
                                 const int32_t* phrase_len_dev, int32_t n_phrases, const float* db_dev, int32_t N, int32_t D,
                                 const float* db_norm_dev, int32_t metric, const int32_t* cand_dev, int32_t m, const int32_t* seq_offsets_dev,
                                 int32_t n_seq, int32_t k, float* cost_dev, int64_t* seq_dev, int64_t* span_dev, void* workspace_dev,
                                 void* stream) {
    static const char* what = "sylber_dtw_rerank";
    hipStream_t s = (hipStream_t)stream;
    if (!q_dev || !phrase_row_dev || !phrase_len_dev || !db_dev || !cand_dev || !seq_offsets_dev || !cost_dev || !seq_dev || !span_dev ||
        !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    const float *qn, *cn;
    if (dt_pair_check(what, "need n_blocks, n_phrases, N, n_seq >= 1 and D a multiple of 16",
                      m < 1 || m > KN_KMAX || k < 1 || k > m ? "need 1 <= k <= m <= 128" : nullptr,
                      "n_phrases x m is too large: use smaller phrase chunks", n_blocks, n_phrases, n_seq, N, D, q_norm_dev, db_norm_dev, metric,
                      (int64_t)n_phrases * m > INT32_MAX, qn, cn)) return 1;
    const DpPairResults r(workspace_dev, n_phrases, m);
    hipLaunchKernelGGL(dtw_rerank_kernel, dim3((unsigned)((int64_t)n_phrases * m)), dim3(64), 0, s, q_dev, qn, n_blocks * KN_BM, phrase_row_dev,
                       phrase_len_dev, db_dev, N, D, cn, cand_dev, seq_offsets_dev, n_seq, m, r.pc, r.pspan);
    HIP_TRY(hipGetLastError());
    return dp_rank_launch(r, cand_dev, n_phrases, m, k, cost_dev, seq_dev, span_dev, s);
}

// ---- every occurrence of a phrase among candidate sequences (SyllableIndex.search_occurrences_refined) ----------------------------
// dtw_rerank_kernel's sibling: the same wave per (phrase, candidate) pair, with every non-overlapping occurrence of the candidate
// kept.  The body is dtw_pair.h's dp_occ_rerank_pair, which dtw_codes.hip runs on a coded database.
__global__ __launch_bounds__(64) void dtw_occ_rerank_kernel(const float* __restrict__ q, const float* __restrict__ qsq, int qrows,
                                                            const int32_t* __restrict__ prow, const int32_t* __restrict__ plen,
                                                            const float* __restrict__ x, int N, int D, const float* __restrict__ cn,
                                                            const int32_t* __restrict__ cand, const int32_t* __restrict__ soff, int S,
                                                            int m, int k, float* __restrict__ ps, int32_t* __restrict__ pi,
                                                            int2* __restrict__ pp) {
    __shared__ float dsm[DT_MAX_M * DP_LD];
    __shared__ float ols[KN_KMAX];
    __shared__ int oli[KN_KMAX];
    __shared__ int2 olp[KN_KMAX];
    dp_occ_rerank_pair(dsm, ols, oli, olp, DpRowsSrc{x, D}, q, qsq, qrows, prow, plen, N, D, cn, cand, soff, S, m, k, ps, pi, pp);
}

extern "C" int64_t sylber_dtw_occ_workspace_bytes(int32_t n_phrases, int32_t m, int32_t k) {
    if (n_phrases < 1 || m < 1 || m > KN_KMAX || k < 1 || k > KN_KMAX) return -1;
    return dt_occ_lists_bytes(n_phrases, m, k);
}

extern "C" int sylber_dtw_rerank_occurrences(const float* q_dev, int32_t n_blocks, const float* q_norm_dev, const int32_t* phrase_row_dev,
                                             const int32_t* phrase_len_dev, int32_t n_phrases, const float* db_dev, int32_t N, int32_t D,
                                             const float* db_norm_dev, int32_t metric, const int32_t* cand_dev, int32_t m,
                                             const int32_t* seq_offsets_dev, int32_t n_seq, int32_t k, float* cost_dev, int64_t* seq_dev,
                                             int64_t* span_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_dtw_rerank_occurrences";
    hipStream_t s = (hipStream_t)stream;
    if (!q_dev || !phrase_row_dev || !phrase_len_dev || !db_dev || !cand_dev || !seq_offsets_dev || !cost_dev || !seq_dev || !span_dev ||
        !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    const float *qn, *cn;
    if (dt_pair_check(what, "need n_blocks, n_phrases, N, n_seq >= 1 and D a multiple of 16",
                      m < 1 || m > KN_KMAX || k < 1 || k > KN_KMAX ? "need 1 <= m <= 128 and 1 <= k <= 128" : nullptr,
                      "n_phrases x m x k is too large: use smaller phrase chunks", n_blocks, n_phrases, n_seq, N, D, q_norm_dev, db_norm_dev, metric,
                      (int64_t)n_phrases * m * k > INT32_MAX / 2, qn, cn)) return 1;
    const DtOccLists lists = dt_occ_lists_carve((char*)workspace_dev, n_phrases, m, k);
    hipLaunchKernelGGL(dtw_occ_rerank_kernel, dim3((unsigned)((int64_t)n_phrases * m)), dim3(64), 0, s, q_dev, qn, n_blocks * KN_BM, phrase_row_dev,
                       phrase_len_dev, db_dev, N, D, cn, cand_dev, seq_offsets_dev, n_seq, m, k, lists.s0, lists.i0, lists.p0);
    HIP_TRY(hipGetLastError());
    return dt_occ_merge_finish(lists, n_phrases, m, k, nullptr, seq_offsets_dev, n_seq, cost_dev, seq_dev, span_dev, s);
}

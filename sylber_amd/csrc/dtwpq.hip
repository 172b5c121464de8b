// Compressed phrase search (sylber_amd/pq.py: PQSyllableIndex.search_phrases; contract in include/sylber_hip.h, restated in
// tests/dtwpq_ref.py): stage 1 of the two-stage phrase search of dtw16.hip, run on the M-byte product-quantization codes instead of
// a 16-bit plane of the rows.  Decode into the MFMA, not table look-ups: a 128-row query block's ADC tables would be 128 M KiB and
// cannot sit in LDS, while decoding a 128-column tile is 128 M gathers of dsub halves from the 16-bit codebooks (512 D bytes,
// L2-resident), amortised over all 128 phrase rows by v_mfma_f32_32x32x16_{f16,bf16}.
//   * dtwpq_scan_kernel<FMT> is dtw16_scan_kernel<FMT> with the database side of `fetch` replaced: thread (sr, sh) needs halves
//     [k0 + sh, k0 + sh + 16) of row cr; (D / M) % 16 == 0, so they lie in one sub-space mm = (k0 + sh) / dsub at offset
//     o = (k0 + sh) % dsub, and the thread loads 32 B from codebooks16 + ((mm * 256 + codes[cr * M + mm]) * dsub + o).  Rounding is
//     element-wise, so that gather IS round16(decode(code)) and the staged bits are those of the materialised plane
//     sylber_knn16_pack(sylber_pq_decode(codes)): with db_norm = recon_norm the candidates and coarse costs equal
//     sylber_dtw16_scan's on that plane bit for bit.  The query side, the `in` test for D % 32 == 16, the row clamp, k16_mma, the
//     epilogue, the wavefront, the list insertion and the write-out are dtw16_scan_kernel's, duplicated here and not shared:
//     dtw16_scan_kernel's instruction stream stays exactly what it was (profiles/phrase_bench.md measures it), and a fetch passed in
//     as a functor would have to carry the LDS code bytes and the mask through that kernel too.
//   * the mask: the epilogue reads cns[cl] in both metrics, so a masked row (bad[j] != 0) needs only cns = NaN where the tile's cns
//     is filled; its local cost is then +inf against every phrase row, as a NaN row's.
//   * the dependent load (code byte, then gather): the tile's 128 x M code bytes are copied to LDS at ks == 0 beside cns / sq / sgs
//     and the fetches of the tile's K steps 1 .. read their byte from there.  The one fetch issued for the NEXT tile's first K step,
//     before the current tile's epilogue and DP, reads its byte from global memory: its latency lies under the DP.
// LDS and occupancy (a CU has 160 KiB): no byte more than dtw16_scan_kernel.
//   dtwpq_scan_kernel   69 136 B fixed (cost tile 67 584 | c_j, sequence ids, groups) + 8 B x (phrases of the block) x m <= 32 KiB of
//                       lists = at most 101 904 B.  The code bytes ([128][M] <= 8 192 B) lie at byte 20 480 of the cost-tile region,
//                       behind the 20 480 B staging that the K loop uses: that part is dead from the end of one tile's DP (the
//                       barrier at the top of the next K step) to the next epilogue's first store (behind the barrier after the last
//                       k16_mma, by which every fetch of the tile has been issued and has returned its byte: the byte feeds an
//                       address).  Two workgroups per CU where dtw16_scan_kernel has two: lists <= 12 784 B.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "dtw_tile.h"
#include "knn16_tile.h"
#include "knn_lists.h"

constexpr int DPQ_MAX_M = 64;                             // PQ_MAX_M of pq.hip
constexpr int DPQ_KSUB = 256;                             // centroids per sub-space
constexpr int DPQ_CODE_OFF = KN_STAGE * 4;                // byte offset of the tile's code bytes in the cost-tile region
static_assert(DPQ_CODE_OFF + KN_BN * DPQ_MAX_M <= KN_BM * DT_LD * 4, "the code bytes fit in the cost tile behind the staging");

static size_t dpq_lds_bytes(int ph, int m) { return (size_t)DT_FIXED * 4 + (size_t)ph * m * 8; }

// As dtw16_scan_kernel, the database given as codes [N][M] (bad [N] or null: 1 = masked row) and cb16 [M][256][D / M], the 16-bit
// codebooks; cn: the fp32 ||decode(code_j)||^2 (L2) or null.
template <int FMT>
__global__ __launch_bounds__(256) void dtwpq_scan_kernel(const bf16_t* __restrict__ q, const float* __restrict__ qsq,
                                                         const int32_t* __restrict__ meta, const int32_t* __restrict__ slot_phrase,
                                                         const int32_t* __restrict__ block_rows, int P, int ph,
                                                         const uint8_t* __restrict__ codes, const uint8_t* __restrict__ bad,
                                                         const bf16_t* __restrict__ cb16, int N, int D, int M,
                                                         const float* __restrict__ cn, int m, const int32_t* __restrict__ seqid,
                                                         const int32_t* __restrict__ cuts, const int32_t* __restrict__ pgrp,
                                                         const int32_t* __restrict__ sgrp, int C, float* __restrict__ ps,
                                                         int32_t* __restrict__ pi) {
    extern __shared__ __attribute__((aligned(16))) float dt_smem[];
    bf16_t* xs = (bf16_t*)dt_smem;                         // staging of the query rows [128][K16_LD]
    bf16_t* cs = xs + KN_BM * K16_LD;                      // staging of the decoded database rows
    uint8_t* cds = (uint8_t*)dt_smem + DPQ_CODE_OFF;       // [128][M] the tile's code bytes, in the cost tile behind the staging
    float* dm = dt_smem;                                   // [128][DT_LD] local costs of the tile, aliasing the staging and the codes
    float* cns = dt_smem + KN_BM * DT_LD;
    int* sq = (int*)(cns + KN_BN);                         // [130] sequence of columns n0 - 1 .. n0 + 128 (-1 outside the cut)
    int* sgs = sq + 132;                                   // [128] group of each column's sequence
    float* ls = (float*)(sgs + KN_BN);                     // [ph][m] sorted coarse costs
    int* li = (int*)(ls + ph * m);                         // [ph][m] their sequences
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
    const int dsub = D / M;
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
        const int tile = t / ksteps, ks = t % ksteps, k0 = ks * K16_BK;
        int cr = rlo + tile * KN_BN + sr; cr = cr < rhi ? cr : rhi - 1;
        const bool in = k0 + sh < D;                       // D % 16 == 0: a last K step of 16 is completed with zeros on both sides
        const int kc = in ? sh + k0 : 0;                   // the loads stay inside the rows and the codebooks either way
        const int mm = kc / dsub, o = kc - mm * dsub;      // (D / M) % 16 == 0: the 16 halves lie in one sub-space
        // a tile's first K step is fetched before its code bytes are in LDS (under the previous tile's DP): from global memory
        const int code = ks == 0 ? codes[(size_t)cr * M + mm] : cds[sr * M + mm];
        const bf16_t* crow = cb16 + ((size_t)(mm * DPQ_KSUB + code) * dsub + o);
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
            if (tid < KN_BN) {
                const int j = n0 + tid;
                const float c = (cn && j < rhi) ? cn[j] : 0.f;
                cns[tid] = (bad && j < rhi && bad[j]) ? NAN : c;
                sgs[tid] = (sgrp && j < rhi) ? sgrp[seqid[j]] : 0;
            }
            if (tid < KN_BN + 2) {
                const int j = n0 - 1 + tid;
                sq[tid] = (j >= rlo && j < rhi) ? seqid[j] : -1;
            }
            if (ksteps > 1) {                              // the two threads of a staging row copy its bytes; a row past the cut
                int cr = n0 + sr; cr = cr < rhi ? cr : rhi - 1;            // repeats the cut's last row, as the fetch clamps it
                for (int mm = tid & 1; mm < M; mm += 2) cds[sr * M + mm] = codes[(size_t)cr * M + mm];
            }
        }
        __syncthreads();
        if (t + 1 < T) fetch(t + 1);
        k16_mma<FMT>(xs, cs, wm, wn, frow, fh, acc, live[0], live[1]);
        if (ks != ksteps - 1) continue;
        // epilogue: lane holds phrase row wm*64 + fm*32 + frow against columns wn*64 + fn*32 + 8g + 4fh + e.  t = fmaf(-2, dot16, c_j);
        // d~ = max(0, ||q||^2 + t) (L2) or max(0, 1 - (-t / 2)) (cosine), dtw16_scan_kernel's expressions; a NaN d~ counts as +inf.
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

// dtw16_cand_kernel's conversion, restated: the merged lists as candidates, the (+inf, INT_MAX) fillers become (+inf, -1)
__global__ __launch_bounds__(256) void dtwpq_cand_kernel(const float* __restrict__ ls, const int32_t* __restrict__ li, int64_t tot,
                                                         int32_t* __restrict__ cand, float* __restrict__ coarse) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tot) return;
    const int j = li[e];
    cand[e] = j == INT_MAX ? -1 : j;
    coarse[e] = j == INT_MAX ? INFINITY : ls[e];
}

extern "C" int sylber_dtwpq_scan(const void* q16_dev, int32_t n_blocks, const int32_t* row_meta_dev, const int32_t* slot_phrase_dev,
                                 const int32_t* block_rows_dev, int32_t n_phrases, int32_t block_phrases, const uint8_t* codes_dev,
                                 const uint8_t* bad_dev, const void* codebooks16_dev, int32_t N, int32_t D, int32_t M,
                                 const float* recon_norm_dev, const float* q_norm_dev, int32_t metric, int32_t storage, int32_t m,
                                 const int32_t* seq_id_dev, const int32_t* cut_rows_dev, int32_t cuts, const int32_t* phrase_group_dev,
                                 const int32_t* seq_group_dev, int32_t* cand_dev, float* coarse_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_dtwpq_scan";
    hipStream_t s = (hipStream_t)stream;
    if (!q16_dev || !row_meta_dev || !slot_phrase_dev || !block_rows_dev || !codes_dev || !codebooks16_dev || !seq_id_dev || !cut_rows_dev ||
        !cand_dev || !coarse_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n_blocks < 1 || n_phrases < 1 || N < 1 || D < 16 || D % 16) { syl_set_error(what, "need n_blocks, n_phrases, N >= 1 and D a multiple of 16"); return 1; }
    if (M < 1 || M > DPQ_MAX_M || D % M || (D / M) % 16) { syl_set_error(what, "need 1 <= M <= 64, D % M == 0 and D / M a multiple of 16"); return 1; }
    if (m < 1 || m > KN_KMAX) { syl_set_error(what, "need 1 <= m <= 128"); return 1; }
    if (block_phrases < 1 || block_phrases > dt_block_phrases(m, 0)) { syl_set_error(what, "block_phrases exceeds what sylber_dtw_plan allows for this m"); return 1; }
    if (cuts < 1 || cuts > 65535) { syl_set_error(what, "need 1 <= cuts <= 65535"); return 1; }
    if (metric != SYLBER_KNN_L2 && metric != SYLBER_KNN_IP) { syl_set_error(what, "unknown metric"); return 1; }
    if (storage != SYLBER_KNN16_FP16 && storage != SYLBER_KNN16_BF16) { syl_set_error(what, "unknown storage"); return 1; }
    if (metric == SYLBER_KNN_L2 && (!recon_norm_dev || !q_norm_dev)) { syl_set_error(what, "the L2 metric needs recon_norm_dev and q_norm_dev"); return 1; }
    if (!phrase_group_dev != !seq_group_dev) { syl_set_error(what, "phrase_group_dev and seq_group_dev go together"); return 1; }
    if ((int64_t)n_phrases * cuts * m > INT32_MAX / 2) { syl_set_error(what, "n_phrases x cuts x m is too large: use smaller phrase chunks"); return 1; }
    char* w = (char*)workspace_dev;
    KnPartials p = kn_partials_carve(w, n_phrases, cuts, m);
    const size_t lds = dpq_lds_bytes(block_phrases, m);
    const int max_lds = (int)((size_t)DT_FIXED * 4 + DT_LIST_BYTES / 2);
    const bf16_t* q16 = (const bf16_t*)q16_dev;
    const bf16_t* cb16 = (const bf16_t*)codebooks16_dev;
    const float* qn = metric == SYLBER_KNN_L2 ? q_norm_dev : nullptr;
    const float* cn = metric == SYLBER_KNN_L2 ? recon_norm_dev : nullptr;
    const dim3 grid((unsigned)n_blocks, (unsigned)cuts);
    if (storage == SYLBER_KNN16_FP16) {
        static PerDeviceOnce once;
        if (once.need()) HIP_TRY(hipFuncSetAttribute((const void*)dtwpq_scan_kernel<FMT_F16>, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
        hipLaunchKernelGGL(dtwpq_scan_kernel<FMT_F16>, grid, dim3(256), lds, s, q16, qn, row_meta_dev, slot_phrase_dev, block_rows_dev, n_phrases,
                           block_phrases, codes_dev, bad_dev, cb16, N, D, M, cn, m, seq_id_dev, cut_rows_dev, phrase_group_dev, seq_group_dev,
                           cuts, p.s0, p.i0);
    } else {
        static PerDeviceOnce once;
        if (once.need()) HIP_TRY(hipFuncSetAttribute((const void*)dtwpq_scan_kernel<FMT_BF16>, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
        hipLaunchKernelGGL(dtwpq_scan_kernel<FMT_BF16>, grid, dim3(256), lds, s, q16, qn, row_meta_dev, slot_phrase_dev, block_rows_dev, n_phrases,
                           block_phrases, codes_dev, bad_dev, cb16, N, D, M, cn, m, seq_id_dev, cut_rows_dev, phrase_group_dev, seq_group_dev,
                           cuts, p.s0, p.i0);
    }
    HIP_TRY(hipGetLastError());
    if (kn_merge_lists(p, n_phrases, cuts, m, s)) return 1;
    const int64_t tot = (int64_t)n_phrases * m;
    hipLaunchKernelGGL(dtwpq_cand_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, p.s0, p.i0, tot, cand_dev, coarse_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

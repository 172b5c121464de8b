// Two-stage syllable search (sylber_amd/search.py: SyllableIndex.search_refined): a cheap 16-bit MFMA scan picks m = k * refine
// candidates per query, the exact fp32 score of sylber_knn_search re-ranks only those.
//   * knn16_pack_kernel: fp32 rows -> fp16 / bf16 rows, round to nearest even; fp16 saturates at +-65504 and counts the finite values
//     it had to saturate.
//   * knn16_scan_kernel: knn_search_kernel's tiling (128 queries x 128 database rows, 2 x 2 waves of 2 x 2 fragments of 32 x 32, grid
//     (query blocks) x S splits) on v_mfma_f32_32x32x16_{f16,bf16}: the C layout is that of the f32 MFMA, so the epilogue is the same
//     strip / kn_insert machinery over an m-entry list.  Coarse score t = fmaf(-2, dot16, c_j).  An output element is one MFMA chain
//     over K in ascending 16-wide steps whatever tile, split or block row computes it, so t's bits are a function of (i, j) alone and
//     the candidate list -- the m best under the strict order (t, j) -- does not depend on splits, chunking or the workspace.
//   * knn_rerank_kernel: one wave per query; each lane walks one candidate's fp32 row with the ascending fmaf chain from 0 that
//     v_mfma_f32_32x32x2_f32 performs in knn_search_kernel (kmeans.hip, fp32_path.hip), so s = fmaf(-2, q . x, c) has
//     sylber_knn_search's bits; then the m scores are ranked by (s, id) and the best k reported with knn_finish_kernel's formulas.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "knn_tile.h"
#include "knn_lists.h"
#include "knn16_tile.h"

constexpr int K16_STRIP = 32, K16_SP = 132;               // epilogue strip: 32 query rows x 128 scores, row stride 132 floats

template <int FMT> __device__ __forceinline__ bf16_t k16_cvt(float f) { return f2bf_dev(f); }
// IEEE half, saturating: NaN stays NaN, everything else is clamped to +-65504 before the (round to nearest even) conversion.  Not
// H16<FMT_F16>::cvt: its v_med3_f32 clamp does not promise to keep a NaN, which the activations it serves never are and a row here can be.
template <> __device__ __forceinline__ bf16_t k16_cvt<FMT_F16>(float f) {
    const float c = f != f ? f : fminf(fmaxf(f, -65504.0f), 65504.0f);
    return __builtin_bit_cast(unsigned short, (_Float16)c);
}

// thread g converts elements [8 g, 8 g + 8); sat (fp16 only, may be null) += the number of finite values beyond +-65504
template <int FMT>
__global__ __launch_bounds__(256) void knn16_pack_kernel(const float* __restrict__ x, int64_t groups, bf16_t* __restrict__ out,
                                                         int32_t* __restrict__ sat) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int over = 0;
    if (g < groups) {
        const float4 a = ((const float4*)x)[2 * g], b = ((const float4*)x)[2 * g + 1];
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        u16x8_t o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            o[e] = k16_cvt<FMT>(v[e]);
            if (FMT == FMT_F16) over += (fabsf(v[e]) > 65504.0f && fabsf(v[e]) < INFINITY) ? 1 : 0;
        }
        *(u16x8_t*)(out + 8 * g) = o;
    }
    if (FMT == FMT_F16 && sat) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) over += __shfl_xor(over, o, 64);
        if ((threadIdx.x & 63) == 0 && over) atomicAdd(sat, over);
    }
}

static size_t k16_lds_bytes(int m) { return (size_t)(KN_STAGE + 3 * KN_BN + 4) * 4 + (size_t)KN_BM * m * 8; }

// grid (ceil(n / 128), S), split sp walks database tiles [sp * tiles / S, (sp + 1) * tiles / S) as knn_search_kernel does.  q / x: the
// 16-bit planes [n, D] / [N, D]; cn: the fp32 ||x_j||^2 (L2) or null (c_j = 0).  Writes the sorted best m of every valid query row
// over its tiles to ps / pi [n][S][m]; entries that did not fill stay (+inf, INT_MAX).  D % 16 == 0: a last K step of 16 is
// completed with zeros on both sides.
template <int FMT>
__global__ __launch_bounds__(256) void knn16_scan_kernel(const bf16_t* __restrict__ q, int n, const bf16_t* __restrict__ x, int N, int D,
                                                         const float* __restrict__ cn, int m, const int32_t* __restrict__ qgrp,
                                                         const int32_t* __restrict__ xgrp, int S, float* __restrict__ ps,
                                                         int32_t* __restrict__ pi) {
    extern __shared__ __attribute__((aligned(16))) float kn_smem[];
    bf16_t* xs = (bf16_t*)kn_smem;                         // query rows [128][K16_LD]
    bf16_t* cs = xs + KN_BM * K16_LD;                      // database rows [128][K16_LD]
    float* strip = kn_smem;                                // epilogue strip, aliasing the staging
    float* cns = kn_smem + KN_STAGE;
    int* cgs = (int*)(cns + KN_BN);
    int* qgs = cgs + KN_BN;                                // the block's query groups
    int* flags = qgs + KN_BM;                              // [4]: strip s may hold a candidate that passes its row's threshold
    float* ls = (float*)(flags + 4);                       // [128][m] sorted coarse scores
    int* li = (int*)(ls + KN_BM * m);                      // [128][m] their database indices
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * KN_BM, sp = blockIdx.y;
    const int tiles = (N + KN_BN - 1) / KN_BN;
    const int tlo = (int)((int64_t)sp * tiles / S), thi = (int)((int64_t)(sp + 1) * tiles / S);
    for (int e = tid; e < KN_BM * m; e += 256) { ls[e] = INFINITY; li[e] = INT_MAX; }
    if (tid < KN_BM) { const int r = m0 + tid; qgs[tid] = qgrp ? qgrp[r < n ? r : n - 1] : 0; }
    // staging: thread -> operand row tid >> 1, halves [16 (tid & 1), 16 (tid & 1) + 16) of the K step
    const int sr = tid >> 1, sh = (tid & 1) * 16;
    int xm = m0 + sr; xm = xm < n ? xm : n - 1;
    const bf16_t* qrow = q + (size_t)xm * D + sh;
    bf16_t* xdst = xs + sr * K16_LD + sh;
    bf16_t* cdst = cs + sr * K16_LD + sh;
    const int frow = lane & 31, fh = lane >> 5;
    const int ksteps = (D + K16_BK - 1) / K16_BK, T = ksteps * (thi - tlo);

    f32x16_t acc[2][2];
    uint4 xa, xb, ca, cb;
    auto fetch = [&](int t) {
        const int tile = tlo + t / ksteps, k0 = (t % ksteps) * K16_BK;
        int cr = tile * KN_BN + sr; cr = cr < N ? cr : N - 1;
        if (k0 + sh < D) {
            const bf16_t* crow = x + (size_t)cr * D + sh + k0;
            xa = *(const uint4*)(qrow + k0); xb = *(const uint4*)(qrow + k0 + 8);
            ca = *(const uint4*)crow; cb = *(const uint4*)(crow + 8);
        } else {
            xa = xb = ca = cb = make_uint4(0, 0, 0, 0);
        }
    };
    if (T > 0) fetch(0);
    for (int t = 0; t < T; ++t) {
        const int tile = tlo + t / ksteps, ks = t % ksteps, n0 = tile * KN_BN;
        if (ks == 0) kn_zero(acc);
        __syncthreads();                                   // previous fragments, strip, cns / cgs and flags are all read
        *(uint4*)xdst = xa; *(uint4*)(xdst + 8) = xb;
        *(uint4*)cdst = ca; *(uint4*)(cdst + 8) = cb;
        if (ks == 0 && tid < KN_BN) {
            const int j = n0 + tid;
            cns[tid] = (cn && j < N) ? cn[j] : 0.f;
            cgs[tid] = (xgrp && j < N) ? xgrp[j] : 0;
            if (tid < 4) flags[tid] = 0;
        }
        __syncthreads();
        if (t + 1 < T) fetch(t + 1);
        // lane (frow, fh) holds k = 8 fh + 0..7 of its row for each MFMA: database rows are A, query rows B, as in kn_mma
#pragma unroll
        for (int kk = 0; kk < K16_BK / 16; ++kk) {
            bf16x8_t xf[2], cf[2];
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                xf[f] = *(const bf16x8_t*)(xs + (wm * 64 + f * 32 + frow) * K16_LD + kk * 16 + fh * 8);
                cf[f] = *(const bf16x8_t*)(cs + (wn * 64 + f * 32 + frow) * K16_LD + kk * 16 + fh * 8);
            }
#pragma unroll
            for (int fm = 0; fm < 2; ++fm)
#pragma unroll
                for (int fn = 0; fn < 2; ++fn) acc[fm][fn] = H16<FMT>::mfma(cf[fn], xf[fm], acc[fm][fn]);
        }
        if (ks != ksteps - 1) continue;
        // epilogue: lane holds query row wm*64 + fm*32 + frow against database rows n0 + wn*64 + fn*32 + 8g + 4fh + e.  Every lane
        // tests its 64 coarse scores against its rows' current m-th score with one compare each (t <= threshold: a superset of the
        // exact (t, j) test, NaN never passes; rows past n and columns past N never flag); the group test and the exact order are
        // applied to the survivors' strips only.
        bool pass[2] = {false, false};
        const bool partial = n0 + KN_BN > N;               // block-uniform: only the database's last tile has columns past N
#pragma unroll
        for (int fm = 0; fm < 2; ++fm) {
            const int rl = wm * 64 + fm * 32 + frow;
            const float tv = ls[rl * m + m - 1];
#pragma unroll
            for (int fn = 0; fn < 2; ++fn)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int cl = wn * 64 + fn * 32 + 8 * g + 4 * fh;
                    const float4 c4 = *(const float4*)(cns + cl);
                    const float cv[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float s = fmaf(-2.0f, acc[fm][fn][4 * g + e], cv[e]);
                        acc[fm][fn][4 * g + e] = s;
                        pass[fm] = pass[fm] || (s <= tv && !(partial && n0 + cl + e >= N));
                    }
                }
            pass[fm] = pass[fm] && m0 + rl < n;            // rows past n keep a +inf threshold: they must not flag their strip
        }
        if (pass[0]) flags[wm * 2 + 0] = 1;
        if (pass[1]) flags[wm * 2 + 1] = 1;
        __syncthreads();                                   // flags complete; every wave is past its fragment reads (strip may alias)
        const int fl = flags[0] | (flags[1] << 1) | (flags[2] << 2) | (flags[3] << 3);
        for (int st = 0; st < 4; ++st) {
            if (!((fl >> st) & 1)) continue;               // block-uniform
            if (wm == (st >> 1)) {
                const int fm = st & 1;
#pragma unroll
                for (int fn = 0; fn < 2; ++fn)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        *(float4*)(strip + frow * K16_SP + wn * 64 + fn * 32 + 8 * g + 4 * fh) =
                            make_float4(acc[fm][fn][4 * g], acc[fm][fn][4 * g + 1], acc[fm][fn][4 * g + 2], acc[fm][fn][4 * g + 3]);
            }
            __syncthreads();
            // each wave takes rows wave, wave + 4, ... of the strip: the admissible survivors of a row go into its list one at a time
            for (int rr = wave; rr < K16_STRIP; rr += 4) {
                const int rl = st * K16_STRIP + rr;
                if (m0 + rl >= n) break;
                float* lsr = ls + rl * m;
                int* lir = li + rl * m;
                const float tv = lsr[m - 1];
                const int ti = lir[m - 1];
                const int qg = qgs[rl];
                const float v0 = strip[rr * K16_SP + lane], v1 = strip[rr * K16_SP + 64 + lane];
                const bool ok0 = n0 + lane < N && !(xgrp && cgs[lane] == qg);
                const bool ok1 = n0 + 64 + lane < N && !(xgrp && cgs[64 + lane] == qg);
                uint64_t b0 = __ballot(ok0 && kn_better(v0, n0 + lane, tv, ti));
                uint64_t b1 = __ballot(ok1 && kn_better(v1, n0 + 64 + lane, tv, ti));
                while (b0) {
                    const int c = __ffsll((unsigned long long)b0) - 1;
                    b0 &= b0 - 1;
                    kn_insert(lsr, lir, m, lane, strip[rr * K16_SP + c], n0 + c);
                }
                while (b1) {
                    const int c = __ffsll((unsigned long long)b1) - 1;
                    b1 &= b1 - 1;
                    kn_insert(lsr, lir, m, lane, strip[rr * K16_SP + 64 + c], n0 + 64 + c);
                }
            }
            __syncthreads();                               // the strip is read before the next strip (or the staging) overwrites it
        }
    }
    __syncthreads();
    for (int rl = wave; rl < KN_BM; rl += 4) {
        if (m0 + rl >= n) break;
        const size_t o = ((size_t)(m0 + rl) * S + sp) * m;
        for (int e = lane; e < m; e += 64) { ps[o + e] = ls[rl * m + e]; pi[o + e] = li[rl * m + e]; }
    }
}

// the merged lists' ids as candidates: the (+inf, INT_MAX) fillers become -1
__global__ __launch_bounds__(256) void knn16_cand_kernel(const int32_t* __restrict__ li, int64_t tot, int32_t* __restrict__ cand) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tot) return;
    const int j = li[e];
    cand[e] = j == INT_MAX ? -1 : j;
}

// One wave per query i (4 per workgroup).  Lane p (and p + 64) owns candidate cand[i][p]: dot = the fmaf chain over ascending k from
// 0 -- explicit __builtin_fmaf calls: there is no separate multiply and add for the compiler to contract or reassociate --,
// s = fmaf(-2, dot, c_j).  A candidate that is -1, out of range or has a NaN s becomes a (+inf, INT_MAX) filler.  Rank = entries
// strictly before it under (s, id, position) (ids are distinct; the position only orders the fillers); ranks < k are reported:
// L2 max(0, ||q||^2 + s) with ||q||^2 the chain of km_sqnorm_kernel, inner product 0 - s / 2, fillers (+inf, -1).
__global__ __launch_bounds__(256) void knn_rerank_kernel(const float* __restrict__ q, int n, const float* __restrict__ x, int N, int D,
                                                         const float* __restrict__ cn, const int32_t* __restrict__ cand, int m, int k,
                                                         float* __restrict__ score, int64_t* __restrict__ idx) {
    __shared__ float ss[4][KN_KMAX];
    __shared__ int si[4][KN_KMAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int i = blockIdx.x * 4 + wave;
    const bool live = i < n;
    i = live ? i : n - 1;
    const float* qr = q + (size_t)i * D;
    float qsq = 0.f;
    if (cn) {
        for (int c = lane; c < D; c += 64) { const float v = qr[c]; qsq = __builtin_fmaf(v, v, qsq); }
        qsq = wave_sum(qsq);
    }
    float sv[KN_KMAX / 64];
    int sj[KN_KMAX / 64];
#pragma unroll
    for (int h = 0; h < KN_KMAX / 64; ++h) {
        const int p = lane + 64 * h;
        sv[h] = INFINITY; sj[h] = INT_MAX;
        if (p < m) {
            const int j = cand[(size_t)i * m + p];
            if (j >= 0 && j < N) {
                const float* xr = x + (size_t)j * D;
                float dot = 0.f;
                for (int c = 0; c < D; c += 4) {
                    const float4 a = *(const float4*)(xr + c), b = *(const float4*)(qr + c);
                    dot = __builtin_fmaf(a.x, b.x, dot);
                    dot = __builtin_fmaf(a.y, b.y, dot);
                    dot = __builtin_fmaf(a.z, b.z, dot);
                    dot = __builtin_fmaf(a.w, b.w, dot);
                }
                const float s = __builtin_fmaf(-2.0f, dot, cn ? cn[j] : 0.f);
                if (s == s) { sv[h] = s; sj[h] = j; }
            }
            ss[wave][p] = sv[h]; si[wave][p] = sj[h];
        }
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int h = 0; h < KN_KMAX / 64; ++h) {
        const int p = lane + 64 * h;
        if (p >= m) continue;
        int rank = 0;
        for (int e = 0; e < m; ++e) {
            const float ev = ss[wave][e];
            const int ej = si[wave][e];
            rank += (kn_better(ev, ej, sv[h], sj[h]) || (ev == sv[h] && ej == sj[h] && e < p)) ? 1 : 0;
        }
        if (rank < k) {
            const size_t o = (size_t)i * k + rank;
            if (sj[h] == INT_MAX) { score[o] = INFINITY; idx[o] = -1; }
            else { score[o] = cn ? fmaxf(0.f, qsq + sv[h]) : 0.f - 0.5f * sv[h]; idx[o] = sj[h]; }
        }
    }
}

extern "C" int sylber_knn16_pack(const float* x_dev, int32_t n, int32_t D, int32_t storage, void* out16_dev, int32_t* sat_count_dev,
                                 void* stream) {
    static const char* what = "sylber_knn16_pack";
    if (!x_dev || !out16_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1 || D < 16 || D % 16) { syl_set_error(what, "need n >= 1 and D a multiple of 16"); return 1; }
    if (storage != SYLBER_KNN16_FP16 && storage != SYLBER_KNN16_BF16) { syl_set_error(what, "unknown storage"); return 1; }
    const int64_t groups = (int64_t)n * D / 8, blocks = (groups + 255) / 256;
    if (blocks > INT32_MAX) { syl_set_error(what, "n x D is too large: pack in pieces"); return 1; }
    if (storage == SYLBER_KNN16_FP16)
        hipLaunchKernelGGL(knn16_pack_kernel<FMT_F16>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x_dev, groups,
                           (bf16_t*)out16_dev, sat_count_dev);
    else
        hipLaunchKernelGGL(knn16_pack_kernel<FMT_BF16>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x_dev, groups,
                           (bf16_t*)out16_dev, sat_count_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int64_t sylber_knn16_workspace_bytes(int32_t n, int32_t N, int32_t D, int32_t m, int32_t splits) {
    if (n < 1 || N < 1 || D < 1 || m < 1 || m > KN_KMAX) return -1;
    return kn_partials_bytes(n, sylber_knn_splits(n, N, splits), m);      // the S partial lists of coarse scores (KnPartials)
}

extern "C" int sylber_knn16_scan(const void* q16_dev, int32_t n, const void* db16_dev, int32_t N, int32_t D, const float* db_norm_dev,
                                 int32_t storage, int32_t m, const int32_t* q_group_dev, const int32_t* db_group_dev, int32_t splits,
                                 int32_t* cand_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_knn16_scan";
    hipStream_t s = (hipStream_t)stream;
    if (!q16_dev || !db16_dev || !cand_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1 || N < 1 || D < 16 || D % 16) { syl_set_error(what, "need n, N >= 1 and D a multiple of 16"); return 1; }
    if (m < 1 || m > KN_KMAX) { syl_set_error(what, "need 1 <= m <= 128"); return 1; }
    if (storage != SYLBER_KNN16_FP16 && storage != SYLBER_KNN16_BF16) { syl_set_error(what, "unknown storage"); return 1; }
    if (!q_group_dev != !db_group_dev) { syl_set_error(what, "q_group_dev and db_group_dev go together"); return 1; }
    const int S = sylber_knn_splits(n, N, splits);
    char* w = (char*)workspace_dev;
    KnPartials p = kn_partials_carve(w, n, S, m);
    const size_t lds = k16_lds_bytes(m);
    const unsigned nb = (unsigned)((n + KN_BM - 1) / KN_BM);
    const bf16_t* q16 = (const bf16_t*)q16_dev;
    const bf16_t* x16 = (const bf16_t*)db16_dev;
    if (storage == SYLBER_KNN16_FP16) {
        static PerDeviceOnce once;
        if (once.need()) HIP_TRY(hipFuncSetAttribute((const void*)knn16_scan_kernel<FMT_F16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k16_lds_bytes(KN_KMAX)));
        hipLaunchKernelGGL(knn16_scan_kernel<FMT_F16>, dim3(nb, (unsigned)S), dim3(256), lds, s, q16, n, x16, N, D, db_norm_dev, m, q_group_dev,
                           db_group_dev, S, p.s0, p.i0);
    } else {
        static PerDeviceOnce once;
        if (once.need()) HIP_TRY(hipFuncSetAttribute((const void*)knn16_scan_kernel<FMT_BF16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k16_lds_bytes(KN_KMAX)));
        hipLaunchKernelGGL(knn16_scan_kernel<FMT_BF16>, dim3(nb, (unsigned)S), dim3(256), lds, s, q16, n, x16, N, D, db_norm_dev, m, q_group_dev,
                           db_group_dev, S, p.s0, p.i0);
    }
    HIP_TRY(hipGetLastError());
    if (kn_merge_lists(p, n, S, m, s)) return 1;
    const int64_t tot = (int64_t)n * m;
    hipLaunchKernelGGL(knn16_cand_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, p.i0, tot, cand_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_knn_rerank(const float* q_dev, int32_t n, const float* db_dev, int32_t N, int32_t D, const float* db_norm_dev,
                                 int32_t metric, const int32_t* cand_dev, int32_t m, int32_t k, float* score_dev, int64_t* idx_dev,
                                 void* stream) {
    static const char* what = "sylber_knn_rerank";
    if (!q_dev || !db_dev || !cand_dev || !score_dev || !idx_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1 || N < 1 || D < 16 || D % 16) { syl_set_error(what, "need n, N >= 1 and D a multiple of 16"); return 1; }
    if (m < 1 || m > KN_KMAX || k < 1 || k > m) { syl_set_error(what, "need 1 <= k <= m <= 128"); return 1; }
    if (metric != SYLBER_KNN_L2 && metric != SYLBER_KNN_IP) { syl_set_error(what, "unknown metric"); return 1; }
    if (metric == SYLBER_KNN_L2 && !db_norm_dev) { syl_set_error(what, "the L2 metric needs db_norm_dev"); return 1; }
    hipLaunchKernelGGL(knn_rerank_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, q_dev, n, db_dev, N, D,
                       metric == SYLBER_KNN_L2 ? db_norm_dev : nullptr, cand_dev, m, k, score_dev, idx_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Exact k-nearest-neighbour search over a database of syllable embeddings (sylber_amd/search.py: SyllableIndex).
//   * knn_search_kernel: the exact-fp32 MFMA contraction of km_fused_assign_kernel (kmeans.hip) -- same operand roles, same k-pair
//     order, so a score's bits do not depend on where it is computed -- with a running per-row top-k in the epilogue instead of the
//     arg-min.  The grid is (query blocks) x S database splits; each split writes a sorted partial list per query row.
//   * ivf_scan_kernel (IVFSyllableIndex): the same contraction over the ragged lists of an inverted file, for gathered query rows.
//   * knn_merge_kernel: pairwise merges of the S partial lists, ceil(log2 S) rounds;  knn_finish_kernel: reported values and -1 / +inf
//     padding.
// Every list is ordered by (s, j), smaller score first, then smaller index.  That order is strict and total over the admissible
// candidates, so the top-k set and its order are unique: the result does not depend on the order in which candidates are inserted,
// hence not on the split count, the launch geometry or the query chunking.  A NaN score never passes km_better and never enters.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "knn_tile.h"
#include "knn_lists.h"

// contraction geometry, kn_better, kn_stage / kn_mma (one K step) and kn_insert: knn_tile.h, shared with dtw.hip
constexpr int KN_STRIP = 32, KN_SP = 132;                 // epilogue strip: 32 query rows x 128 scores, row stride 132 floats; aliases the staging
constexpr int KN_TARGET_BLOCKS = 512;                     // automatic splits: (query blocks) x S >= 2 workgroups per CU
constexpr int KN_MIN_TILES = 4;                           // ... but no split shorter than 4 database tiles

static size_t kn_lds_bytes(int k) { return (size_t)(KN_STAGE + 2 * KN_BN + 4) * 4 + (size_t)KN_BM * k * 8; }

// grid (ceil(n / 128), S).  Split sp walks database tiles [sp * tiles / S, (sp + 1) * tiles / S).  cn: ||x_j||^2 (L2) or null (inner
// product: c_j = 0).  Writes the sorted top-k of each valid query row over its tiles to ps / pi [n][S][k]; entries that did not fill
// stay (+inf, INT_MAX).
__global__ __launch_bounds__(256) void knn_search_kernel(const float* __restrict__ q, int n, const float* __restrict__ x, int N, int D,
                                                         const float* __restrict__ cn, int k, const int32_t* __restrict__ qgrp,
                                                         const int32_t* __restrict__ xgrp, int S, float* __restrict__ ps,
                                                         int32_t* __restrict__ pi) {
    extern __shared__ __attribute__((aligned(16))) float kn_smem[];
    float* xs = kn_smem;                                   // staging of the query rows (the "x" of km_fused_assign)
    float* cs = kn_smem + KN_BM * KN_LD;                   // staging of the database rows (its "c")
    float* strip = kn_smem;                                // epilogue strip, aliasing the staging
    float* cns = kn_smem + KN_STAGE;
    int* cgs = (int*)(cns + KN_BN);
    int* flags = cgs + KN_BN;                              // [4]: strip s holds a candidate that passes its row's threshold
    float* ls = (float*)(flags + 4);                       // [128][k] sorted scores
    int* li = (int*)(ls + KN_BM * k);                      // [128][k] their database indices
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * KN_BM, sp = blockIdx.y;
    const int tiles = (N + KN_BN - 1) / KN_BN;
    const int tlo = (int)((int64_t)sp * tiles / S), thi = (int)((int64_t)(sp + 1) * tiles / S);
    for (int e = tid; e < KN_BM * k; e += 256) { ls[e] = INFINITY; li[e] = INT_MAX; }
    const int sr = tid >> 1, sh = (tid & 1) * 8;
    int xm = m0 + sr; xm = xm < n ? xm : n - 1;
    const float* qrow = q + (size_t)xm * D + sh;
    float* xdst = xs + sr * KN_LD + (sh >> 1);
    float* cdst = cs + sr * KN_LD + (sh >> 1);
    const int frow = lane & 31, fh = lane >> 5;
    const int ksteps = D / KN_BK, T = ksteps * (thi - tlo);
    int qg[2] = {0, 0};
    if (qgrp) {
#pragma unroll
        for (int fm = 0; fm < 2; ++fm) { const int r = m0 + wm * 64 + fm * 32 + frow; qg[fm] = qgrp[r < n ? r : n - 1]; }
    }

    f32x16_t acc[2][2];
    float4 xa, xb, ca, cb;
    auto fetch = [&](int t) {
        const int tile = tlo + t / ksteps, k0 = (t % ksteps) * KN_BK;
        int cr = tile * KN_BN + sr; cr = cr < N ? cr : N - 1;
        const float* crow = x + (size_t)cr * D + sh + k0;
        xa = *(const float4*)(qrow + k0); xb = *(const float4*)(qrow + k0 + 4);
        ca = *(const float4*)crow; cb = *(const float4*)(crow + 4);
    };
    if (T > 0) fetch(0);
    for (int t = 0; t < T; ++t) {
        const int tile = tlo + t / ksteps, ks = t % ksteps, n0 = tile * KN_BN;
        if (ks == 0) kn_zero(acc);
        __syncthreads();                                   // previous fragments, strip, cns / cgs and flags are all read
        kn_stage(xdst, cdst, xa, xb, ca, cb);
        if (ks == 0 && tid < KN_BN) {
            const int j = n0 + tid;
            cns[tid] = (cn && j < N) ? cn[j] : 0.f;
            cgs[tid] = (xgrp && j < N) ? xgrp[j] : 0;
            if (tid < 4) flags[tid] = 0;
        }
        __syncthreads();
        if (t + 1 < T) fetch(t + 1);
        kn_mma(xs, cs, wm, wn, frow, fh, acc, true, true);
        if (ks != ksteps - 1) continue;
        // epilogue: lane holds query row wm*64 + fm*32 + frow against database rows n0 + wn*64 + fn*32 + 8g + 4fh + e.  Scores become
        // s = fmaf(-2, dot, c_j); inadmissible ones (past N, same group, past n) become NaN.  Test against the row's k-th entry.
        bool pass[2] = {false, false};
#pragma unroll
        for (int fm = 0; fm < 2; ++fm) {
            const int rl = wm * 64 + fm * 32 + frow;
            const float tv = ls[rl * k + k - 1];
            const int ti = li[rl * k + k - 1];
            const bool rowok = m0 + rl < n;
#pragma unroll
            for (int fn = 0; fn < 2; ++fn)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int cl = wn * 64 + fn * 32 + 8 * g + 4 * fh + e;
                        float s = fmaf(-2.0f, acc[fm][fn][4 * g + e], cns[cl]);
                        if (!rowok || n0 + cl >= N || (xgrp && cgs[cl] == qg[fm])) s = __builtin_nanf("");
                        acc[fm][fn][4 * g + e] = s;
                        pass[fm] = pass[fm] || kn_better(s, n0 + cl, tv, ti);
                    }
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
                        *(float4*)(strip + frow * KN_SP + wn * 64 + fn * 32 + 8 * g + 4 * fh) =
                            make_float4(acc[fm][fn][4 * g], acc[fm][fn][4 * g + 1], acc[fm][fn][4 * g + 2], acc[fm][fn][4 * g + 3]);
            }
            __syncthreads();
            // each wave takes rows wave, wave + 4, ... of the strip: the survivors of a row go into its list one at a time
            for (int rr = wave; rr < KN_STRIP; rr += 4) {
                const int rl = st * KN_STRIP + rr;
                if (m0 + rl >= n) break;
                float* lsr = ls + rl * k;
                int* lir = li + rl * k;
                const float tv = lsr[k - 1];
                const int ti = lir[k - 1];
                const float v0 = strip[rr * KN_SP + lane], v1 = strip[rr * KN_SP + 64 + lane];
                uint64_t b0 = __ballot(kn_better(v0, n0 + lane, tv, ti));
                uint64_t b1 = __ballot(kn_better(v1, n0 + 64 + lane, tv, ti));
                while (b0) {
                    const int c = __ffsll((unsigned long long)b0) - 1;
                    b0 &= b0 - 1;
                    kn_insert(lsr, lir, k, lane, strip[rr * KN_SP + c], n0 + c);
                }
                while (b1) {
                    const int c = __ffsll((unsigned long long)b1) - 1;
                    b1 &= b1 - 1;
                    kn_insert(lsr, lir, k, lane, strip[rr * KN_SP + 64 + c], n0 + 64 + c);
                }
            }
            __syncthreads();                               // the strip is read before the next strip (or the staging) overwrites it
        }
    }
    __syncthreads();
    for (int rl = wave; rl < KN_BM; rl += 4) {
        if (m0 + rl >= n) break;
        const size_t o = ((size_t)(m0 + rl) * S + sp) * k;
        for (int e = lane; e < k; e += 64) { ps[o + e] = ls[rl * k + e]; pi[o + e] = li[rl * k + e]; }
    }
}

// knn_merge_kernel and knn_finish_kernel: knn_lists.h, shared with knn16.hip

// y[r] = x[r] / sqrt(sum x[r]^2) (the sum an fmaf chain per lane in ascending column steps of 64, then the wave butterfly), 0 rows stay 0
__global__ __launch_bounds__(256) void knn_unit_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int D) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= n) return;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) { const float v = x[(size_t)r * D + c]; s = fmaf(v, v, s); }
    s = wave_sum(s);
    const float nrm = sqrtf(s);
    for (int c = lane; c < D; c += 64) y[(size_t)r * D + c] = s > 0.f ? x[(size_t)r * D + c] / nrm : 0.f;
}

// ---- inverted-file scan (sylber_amd/search.py: IVFSyllableIndex) ---------------------------------------------------------------------
// The database rows lie list by list (rows [row_lo, row_hi) of a work item belong to ONE list); rid maps a position to the row's
// original id, which is the id that orders, is reported and breaks ties.  A work item is 8 int32:
//   {list, pair_begin, pair_count <= 128, row_lo, row_hi, cut, last, tile_begin}
// It gathers the queries pair[pair_begin + r] / nprobe of its up to 128 (query, probe slot) pairs into the operand tile, walks the
// 128-row tiles of [row_lo, row_hi) with knn_search_kernel's contraction (same operand roles and k-pair order: same score bits) and
// writes each pair's sorted top-k to partial list (pair * C + cut) of ps / pi [n * nprobe][C][k].  The item with last != 0 also
// writes the fillers of the lists cut + 1 .. C - 1 of its pairs, so every partial list is written by exactly one item whatever the
// workspace held.  Positions >= row_hi (the next list, or the end of the database) are never read and never become candidates.
constexpr int IV_ITEM = 8;
constexpr int IV_ITEM_TILES = 16;                         // automatic: at most 16 tiles (2 048 rows) of a list per work item ...
constexpr int IV_TARGET_ITEMS = 512;                      // ... fewer while the launch has fewer than two work items per CU ...
constexpr int IV_MIN_TILES = 2;                           // ... but not below 2 tiles
constexpr int IV_MAX_CUTS = 16;                           // and never more than 16 cuts of one list (bounds the partial lists)

__global__ __launch_bounds__(256) void ivf_scan_kernel(const float* __restrict__ q, const int32_t* __restrict__ items,
                                                       const int32_t* __restrict__ pair, int nprobe, const float* __restrict__ x, int D,
                                                       const int32_t* __restrict__ rid, const float* __restrict__ cn, int k,
                                                       const int32_t* __restrict__ qgrp, const int32_t* __restrict__ xgrp, int C,
                                                       float* __restrict__ ps, int32_t* __restrict__ pi) {
    extern __shared__ __attribute__((aligned(16))) float kn_smem[];
    float* xs = kn_smem;
    float* cs = kn_smem + KN_BM * KN_LD;
    float* strip = kn_smem;
    float* cns = kn_smem + KN_STAGE;
    int* cgs = (int*)(cns + KN_BN);
    int* cids = cgs + KN_BN;                               // original ids of the tile's rows (INT_MAX behind the end)
    int* prs = cids + KN_BN;                               // the item's pairs
    int* flags = prs + KN_BM;
    float* ls = (float*)(flags + 4);
    int* li = (int*)(ls + KN_BM * k);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int32_t* it = items + (size_t)blockIdx.x * IV_ITEM;
    const int pbeg = it[1], cnt = it[2], rlo = it[3], rhi = it[4], cut = it[5], last = it[6];
    const int tiles = (rhi - rlo + KN_BN - 1) / KN_BN;
    for (int e = tid; e < KN_BM * k; e += 256) { ls[e] = INFINITY; li[e] = INT_MAX; }
    if (tid < KN_BM) prs[tid] = pair[pbeg + (tid < cnt ? tid : cnt - 1)];
    const int sr = tid >> 1, sh = (tid & 1) * 8;
    const int xm = pair[pbeg + (sr < cnt ? sr : cnt - 1)] / nprobe;
    const float* qrow = q + (size_t)xm * D + sh;
    float* xdst = xs + sr * KN_LD + (sh >> 1);
    float* cdst = cs + sr * KN_LD + (sh >> 1);
    const int frow = lane & 31, fh = lane >> 5;
    const int ksteps = D / KN_BK, T = ksteps * tiles;
    int qg[2] = {0, 0};
    bool live[2];                                          // wave-uniform: this wave's 32-row half holds a pair of the item
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
        live[fm] = wm * 64 + fm * 32 < cnt;
        if (qgrp) { const int r = wm * 64 + fm * 32 + frow; qg[fm] = qgrp[pair[pbeg + (r < cnt ? r : cnt - 1)] / nprobe]; }
    }

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
        __syncthreads();
        kn_stage(xdst, cdst, xa, xb, ca, cb);
        if (ks == 0 && tid < KN_BN) {
            const int j = n0 + tid;
            cns[tid] = (cn && j < rhi) ? cn[j] : 0.f;
            cgs[tid] = (xgrp && j < rhi) ? xgrp[j] : 0;
            cids[tid] = j < rhi ? rid[j] : INT_MAX;
            if (tid < 4) flags[tid] = 0;
        }
        __syncthreads();
        if (t + 1 < T) fetch(t + 1);
        // a half without pairs skips its MFMAs: its scores are masked below whatever they are
        kn_mma(xs, cs, wm, wn, frow, fh, acc, live[0], live[1]);
        if (ks != ksteps - 1) continue;
        bool pass[2] = {false, false};
#pragma unroll
        for (int fm = 0; fm < 2; ++fm) {
            const int rl = wm * 64 + fm * 32 + frow;
            const float tv = ls[rl * k + k - 1];
            const int ti = li[rl * k + k - 1];
            const bool rowok = rl < cnt;
#pragma unroll
            for (int fn = 0; fn < 2; ++fn)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int cl = wn * 64 + fn * 32 + 8 * g + 4 * fh + e;
                        float s = fmaf(-2.0f, acc[fm][fn][4 * g + e], cns[cl]);
                        if (!rowok || n0 + cl >= rhi || (xgrp && cgs[cl] == qg[fm])) s = __builtin_nanf("");
                        acc[fm][fn][4 * g + e] = s;
                        pass[fm] = pass[fm] || kn_better(s, cids[cl], tv, ti);
                    }
        }
        if (pass[0]) flags[wm * 2 + 0] = 1;
        if (pass[1]) flags[wm * 2 + 1] = 1;
        __syncthreads();
        const int fl = flags[0] | (flags[1] << 1) | (flags[2] << 2) | (flags[3] << 3);
        for (int st = 0; st < 4; ++st) {
            if (!((fl >> st) & 1)) continue;               // block-uniform
            if (wm == (st >> 1)) {
                const int fm = st & 1;
#pragma unroll
                for (int fn = 0; fn < 2; ++fn)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        *(float4*)(strip + frow * KN_SP + wn * 64 + fn * 32 + 8 * g + 4 * fh) =
                            make_float4(acc[fm][fn][4 * g], acc[fm][fn][4 * g + 1], acc[fm][fn][4 * g + 2], acc[fm][fn][4 * g + 3]);
            }
            __syncthreads();
            for (int rr = wave; rr < KN_STRIP; rr += 4) {
                const int rl = st * KN_STRIP + rr;
                if (rl >= cnt) break;
                float* lsr = ls + rl * k;
                int* lir = li + rl * k;
                const float tv = lsr[k - 1];
                const int ti = lir[k - 1];
                const float v0 = strip[rr * KN_SP + lane], v1 = strip[rr * KN_SP + 64 + lane];
                uint64_t b0 = __ballot(kn_better(v0, cids[lane], tv, ti));
                uint64_t b1 = __ballot(kn_better(v1, cids[64 + lane], tv, ti));
                while (b0) {
                    const int c = __ffsll((unsigned long long)b0) - 1;
                    b0 &= b0 - 1;
                    kn_insert(lsr, lir, k, lane, strip[rr * KN_SP + c], cids[c]);
                }
                while (b1) {
                    const int c = __ffsll((unsigned long long)b1) - 1;
                    b1 &= b1 - 1;
                    kn_insert(lsr, lir, k, lane, strip[rr * KN_SP + 64 + c], cids[64 + c]);
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int rl = wave; rl < cnt; rl += 4) {
        const size_t o = ((size_t)prs[rl] * C + cut) * k;
        for (int e = lane; e < k; e += 64) { ps[o + e] = ls[rl * k + e]; pi[o + e] = li[rl * k + e]; }
        if (last)
            for (int e = lane; e < (C - 1 - cut) * k; e += 64) { ps[o + k + e] = INFINITY; pi[o + k + e] = INT_MAX; }
    }
}

static size_t iv_lds_bytes(int k) { return (size_t)(KN_STAGE + 4 * KN_BN + 4) * 4 + (size_t)KN_BM * k * 8; }

static int kn_splits(int32_t n, int32_t N, int32_t splits) {
    const int64_t nb = ((int64_t)n + KN_BM - 1) / KN_BM, tiles = ((int64_t)N + KN_BN - 1) / KN_BN;
    int64_t S = splits;
    if (S <= 0) {
        S = (KN_TARGET_BLOCKS + nb - 1) / nb;
        const int64_t cap = tiles / KN_MIN_TILES;
        S = S < cap ? S : cap;
    }
    S = S < tiles ? S : tiles;
    S = S < 65535 ? S : 65535;
    return (int)(S < 1 ? 1 : S);
}

extern "C" int32_t sylber_knn_splits(int32_t n, int32_t N, int32_t splits) {
    if (n < 1 || N < 1) return -1;
    return kn_splits(n, N, splits);
}

extern "C" int64_t sylber_knn_workspace_bytes(int32_t n, int32_t N, int32_t D, int32_t k, int32_t splits) {
    if (n < 1 || N < 1 || D < 1 || k < 1 || k > KN_KMAX) return -1;
    return kn_al((int64_t)n * 4) + kn_partials_bytes(n, kn_splits(n, N, splits), k);      // ||q||^2 [n] | the S partial lists (KnPartials)
}

extern "C" int sylber_knn_row_norms(const float* x_dev, int32_t n, int32_t D, float* out_dev, void* stream) {
    if (!x_dev || !out_dev || n < 1 || D < 1) { syl_set_error("sylber_knn_row_norms", "bad argument"); return 1; }
    return launch_km_sqnorm(x_dev, out_dev, n, D, (hipStream_t)stream);
}

extern "C" int sylber_knn_unit_rows(const float* x_dev, int32_t n, int32_t D, float* y_dev, void* stream) {
    if (!x_dev || !y_dev || n < 1 || D < 1) { syl_set_error("sylber_knn_unit_rows", "bad argument"); return 1; }
    hipLaunchKernelGGL(knn_unit_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, x_dev, y_dev, n, D);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_knn_search(const float* q_dev, int32_t n, const float* db_dev, int32_t N, int32_t D, const float* db_norm_dev,
                                 int32_t metric, int32_t k, const int32_t* q_group_dev, const int32_t* db_group_dev, int32_t splits,
                                 float* score_dev, int64_t* idx_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_knn_search";
    hipStream_t s = (hipStream_t)stream;
    if (!q_dev || !db_dev || !score_dev || !idx_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1 || N < 1 || D < 16 || D % 16) { syl_set_error(what, "need n, N >= 1 and D a multiple of 16"); return 1; }
    if (k < 1 || k > KN_KMAX) { syl_set_error(what, "need 1 <= k <= 128"); return 1; }
    if (metric != SYLBER_KNN_L2 && metric != SYLBER_KNN_IP) { syl_set_error(what, "unknown metric"); return 1; }
    if (metric == SYLBER_KNN_L2 && !db_norm_dev) { syl_set_error(what, "the L2 metric needs db_norm_dev"); return 1; }
    if (!q_group_dev != !db_group_dev) { syl_set_error(what, "q_group_dev and db_group_dev go together"); return 1; }
    const int S = kn_splits(n, N, splits);
    char* w = (char*)workspace_dev;
    float* qsq = (float*)w;
    w += kn_al((int64_t)n * 4);
    KnPartials p = kn_partials_carve(w, n, S, k);
    if (metric == SYLBER_KNN_L2 && launch_km_sqnorm(q_dev, qsq, n, D, s)) return 1;
    const size_t lds = kn_lds_bytes(k);
    static PerDeviceOnce once;
    if (once.need()) HIP_TRY(hipFuncSetAttribute((const void*)knn_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kn_lds_bytes(KN_KMAX)));
    const unsigned nb = (unsigned)((n + KN_BM - 1) / KN_BM);
    hipLaunchKernelGGL(knn_search_kernel, dim3(nb, (unsigned)S), dim3(256), lds, s, q_dev, n, db_dev, N, D,
                       metric == SYLBER_KNN_L2 ? db_norm_dev : nullptr, k, q_group_dev, db_group_dev, S, p.s0, p.i0);
    HIP_TRY(hipGetLastError());
    if (kn_merge_lists(p, n, S, k, s)) return 1;
    const int64_t tot = (int64_t)n * k;
    hipLaunchKernelGGL(knn_finish_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, p.s0, p.i0, n, k,
                       metric == SYLBER_KNN_L2 ? qsq : nullptr, score_dev, idx_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Host only.  One work item per (probed list, block of up to 128 of its pairs, cut of its tiles); see ivf_scan_kernel.
extern "C" int32_t sylber_ivf_work_items(const int32_t* pair_counts_host, const int32_t* list_offsets_host, int32_t nlist, int32_t item_tiles,
                                         int32_t* items_host, int32_t capacity, int32_t* cuts_out) {
    if (!pair_counts_host || !list_offsets_host || nlist < 1 || item_tiles < 0) return -1;
    int64_t W0 = 0, TT = 0, maxt = 0;
    for (int l = 0; l < nlist; ++l) {
        const int64_t pc = pair_counts_host[l], sz = (int64_t)list_offsets_host[l + 1] - list_offsets_host[l];
        if (pc < 0 || sz < 0) return -1;
        if (!pc) continue;
        const int64_t tiles = (sz + KN_BN - 1) / KN_BN, qb = (pc + KN_BM - 1) / KN_BM;
        W0 += qb; TT += qb * (tiles > 1 ? tiles : 1);
        maxt = tiles > maxt ? tiles : maxt;
    }
    int64_t T = item_tiles;
    if (T <= 0) {
        T = IV_ITEM_TILES;
        if (W0 < IV_TARGET_ITEMS) {
            const int64_t t = (TT + IV_TARGET_ITEMS - 1) / IV_TARGET_ITEMS;
            T = t < IV_MIN_TILES ? IV_MIN_TILES : (t < IV_ITEM_TILES ? t : IV_ITEM_TILES);
        }
    }
    const int64_t floorT = (maxt + IV_MAX_CUTS - 1) / IV_MAX_CUTS;
    T = T < floorT ? floorT : T;
    int64_t W = 0, C = 1, pb = 0;
    for (int l = 0; l < nlist; ++l) {
        const int64_t pc = pair_counts_host[l];
        if (!pc) continue;
        const int64_t lo = list_offsets_host[l], hi = list_offsets_host[l + 1];
        const int64_t tiles = (hi - lo + KN_BN - 1) / KN_BN, cuts = tiles > T ? (tiles + T - 1) / T : 1;
        C = cuts > C ? cuts : C;
        for (int64_t b = 0; b < pc; b += KN_BM)
            for (int64_t c = 0; c < cuts; ++c, ++W) {
                if (!items_host) continue;
                if (W >= capacity) return -1;
                const int64_t t0 = c * T, t1 = (c + 1) * T < tiles ? (c + 1) * T : tiles;
                const int64_t r0 = lo + t0 * KN_BN, r1 = lo + t1 * KN_BN < hi ? lo + t1 * KN_BN : hi;
                int32_t* it = items_host + W * IV_ITEM;
                it[0] = l; it[1] = (int32_t)(pb + b); it[2] = (int32_t)(pc - b < KN_BM ? pc - b : KN_BM);
                it[3] = (int32_t)r0; it[4] = (int32_t)(r1 > r0 ? r1 : r0); it[5] = (int32_t)c; it[6] = c == cuts - 1; it[7] = (int32_t)t0;
            }
        pb += pc;
    }
    if (W > INT32_MAX) return -1;
    if (cuts_out) *cuts_out = (int32_t)C;
    return (int32_t)W;
}

extern "C" int64_t sylber_ivf_workspace_bytes(int32_t n, int32_t nprobe, int32_t k, int32_t cuts) {
    if (n < 1 || nprobe < 1 || nprobe > KN_KMAX || k < 1 || k > KN_KMAX || cuts < 1) return -1;
    return kn_al((int64_t)n * 4) + kn_partials_bytes(n, (int64_t)nprobe * cuts, k);      // ||q||^2 [n] | the nprobe x cuts partial lists (KnPartials)
}

extern "C" int sylber_ivf_search(const float* q_dev, int32_t n, int32_t D, int32_t nprobe, const int32_t* pair_dev,
                                 const int32_t* items_dev, int32_t n_items, int32_t cuts, const float* rows_dev,
                                 const int32_t* row_id_dev, const float* row_norm_dev, int32_t metric, int32_t k,
                                 const int32_t* q_group_dev, const int32_t* row_group_dev, float* score_dev, int64_t* idx_dev,
                                 void* workspace_dev, void* stream) {
    static const char* what = "sylber_ivf_search";
    hipStream_t s = (hipStream_t)stream;
    if (!q_dev || !pair_dev || !items_dev || !rows_dev || !row_id_dev || !score_dev || !idx_dev || !workspace_dev) {
        syl_set_error(what, "null argument"); return 1;
    }
    if (n < 1 || n_items < 1 || D < 16 || D % 16) { syl_set_error(what, "need n, n_items >= 1 and D a multiple of 16"); return 1; }
    if (nprobe < 1 || nprobe > KN_KMAX || cuts < 1 || cuts > IV_MAX_CUTS) { syl_set_error(what, "need 1 <= nprobe <= 128 and 1 <= cuts <= 16"); return 1; }
    if ((int64_t)n * nprobe * cuts > INT32_MAX / 2) { syl_set_error(what, "n x nprobe x cuts is too large: use smaller query chunks"); return 1; }
    if (k < 1 || k > KN_KMAX) { syl_set_error(what, "need 1 <= k <= 128"); return 1; }
    if (metric != SYLBER_KNN_L2 && metric != SYLBER_KNN_IP) { syl_set_error(what, "unknown metric"); return 1; }
    if (metric == SYLBER_KNN_L2 && !row_norm_dev) { syl_set_error(what, "the L2 metric needs row_norm_dev"); return 1; }
    if (!q_group_dev != !row_group_dev) { syl_set_error(what, "q_group_dev and row_group_dev go together"); return 1; }
    const int M = nprobe * cuts;
    char* w = (char*)workspace_dev;
    float* qsq = (float*)w;
    w += kn_al((int64_t)n * 4);
    KnPartials p = kn_partials_carve(w, n, M, k);
    if (metric == SYLBER_KNN_L2 && launch_km_sqnorm(q_dev, qsq, n, D, s)) return 1;
    static PerDeviceOnce once;
    if (once.need()) HIP_TRY(hipFuncSetAttribute((const void*)ivf_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)iv_lds_bytes(KN_KMAX)));
    hipLaunchKernelGGL(ivf_scan_kernel, dim3((unsigned)n_items), dim3(256), iv_lds_bytes(k), s, q_dev, items_dev, pair_dev, nprobe, rows_dev, D,
                       row_id_dev, metric == SYLBER_KNN_L2 ? row_norm_dev : nullptr, k, q_group_dev, row_group_dev, cuts, p.s0, p.i0);
    HIP_TRY(hipGetLastError());
    if (kn_merge_lists(p, n, M, k, s)) return 1;
    const int64_t tot = (int64_t)n * k;
    hipLaunchKernelGGL(knn_finish_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, p.s0, p.i0, n, k,
                       metric == SYLBER_KNN_L2 ? qsq : nullptr, score_dev, idx_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The pieces that knn.hip (knn_search_kernel, ivf_scan_kernel) and dtw.hip (dtw_search_kernel; the list insertion also through
// dtw_tile.h's wavefront, which dtwpq_scan_kernel runs too) share: the geometry and the K step of
// the exact-fp32 contraction of km_fused_assign_kernel (kmeans.hip), the (score, index) order, and the insertion into a sorted
// top-k list held in LDS.  One definition of the operand roles and the k-pair order is what keeps a score's bits the same wherever
// it is computed.
#pragma once
#include "kernels.h"
#include <climits>

// contraction geometry of km_fused_assign_kernel: 128 query rows x 128 database rows per tile, K step 16, LDS rows [0 2 .. 14 | 1 3 .. 15]
constexpr int KN_BM = 128, KN_BN = 128, KN_BK = 16, KN_LD = 20;
constexpr int KN_STAGE = 2 * KN_BM * KN_LD;               // floats of the operand staging
constexpr int KN_KMAX = 128;

static inline int64_t kn_al(int64_t bytes) { return (bytes + 255) / 256 * 256; }      // every piece of a search workspace starts at a multiple of 256

__device__ __forceinline__ bool kn_better(float v, int i, float bv, int bi) { return v < bv || (v == bv && i < bi); }   // km_better

__device__ __forceinline__ void kn_zero(f32x16_t (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// thread tid stages 8 floats of query row tid / 2 and of database row tid / 2 (columns k0 + (tid & 1) * 8 ..), even columns first
__device__ __forceinline__ void kn_stage(float* xdst, float* cdst, const float4& xa, const float4& xb, const float4& ca, const float4& cb) {
    *(float4*)xdst = make_float4(xa.x, xa.z, xb.x, xb.z);
    *(float4*)(xdst + 8) = make_float4(xa.y, xa.w, xb.y, xb.w);
    *(float4*)cdst = make_float4(ca.x, ca.z, cb.x, cb.z);
    *(float4*)(cdst + 8) = make_float4(ca.y, ca.w, cb.y, cb.w);
}

// one K step of 16: wave (wm, wn) accumulates its 64 x 64 quadrant; a 32-row half fm with live[fm] == false (wave-uniform) skips its
// MFMAs.  Every accumulator sees its k pairs in ascending order whatever the order of the halves.
__device__ __forceinline__ void kn_mma(const float* xs, const float* cs, int wm, int wn, int frow, int fh, f32x16_t (&acc)[2][2],
                                       bool live0, bool live1) {
    f32x4_t xf[2][2], cf[2][2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const float* xp = xs + (wm * 64 + f * 32 + frow) * KN_LD + fh * 8;
        const float* cp = cs + (wn * 64 + f * 32 + frow) * KN_LD + fh * 8;
        xf[f][0] = *(const f32x4_t*)xp; xf[f][1] = *(const f32x4_t*)(xp + 4);
        cf[f][0] = *(const f32x4_t*)cp; cf[f][1] = *(const f32x4_t*)(cp + 4);
    }
    if (live0 && live1) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int fm = 0; fm < 2; ++fm)
#pragma unroll
                for (int fn = 0; fn < 2; ++fn)
                    acc[fm][fn] = __builtin_amdgcn_mfma_f32_32x32x2f32(cf[fn][i >> 2][i & 3], xf[fm][i >> 2][i & 3], acc[fm][fn], 0, 0, 0);
        return;
    }
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
        if (!(fm ? live1 : live0)) continue;
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int fn = 0; fn < 2; ++fn)
                acc[fm][fn] = __builtin_amdgcn_mfma_f32_32x32x2f32(cf[fn][i >> 2][i & 3], xf[fm][i >> 2][i & 3], acc[fm][fn], 0, 0, 0);
    }
}

// one wave inserts candidate (v, j) [with payload pv] into the sorted list (ls, li [, lp])[0..k) if it is better than the k-th entry
template <bool PAYLOAD>
__device__ __forceinline__ void kn_insert_t(float* ls, int* li, int2* lp, int k, int lane, float v, int j, int2 pv) {
    if (!kn_better(v, j, ls[k - 1], li[k - 1])) return;
    // position = entries better than (v, j)
    int p = 0;
#pragma unroll
    for (int h = 0; h < KN_KMAX / 64; ++h) {
        const int q = lane + 64 * h;
        const bool b = q < k && kn_better(ls[q], li[q], v, j);
        p += __popcll(__ballot(b));
    }
    // shift [p, k - 1) up by one: all reads, then all writes (a wave's LDS operations complete in order)
    float sv[KN_KMAX / 64];
    int si[KN_KMAX / 64];
    int2 sp[KN_KMAX / 64];
#pragma unroll
    for (int h = 0; h < KN_KMAX / 64; ++h) {
        const int q = lane + 64 * h;
        if (q >= p && q < k - 1) { sv[h] = ls[q]; si[h] = li[q]; if (PAYLOAD) sp[h] = lp[q]; }
    }
#pragma unroll
    for (int h = 0; h < KN_KMAX / 64; ++h) {
        const int q = lane + 64 * h;
        if (q >= p && q < k - 1) { ls[q + 1] = sv[h]; li[q + 1] = si[h]; if (PAYLOAD) lp[q + 1] = sp[h]; }
    }
    if (lane == 0) { ls[p] = v; li[p] = j; if (PAYLOAD) lp[p] = pv; }
}

__device__ __forceinline__ void kn_insert(float* ls, int* li, int k, int lane, float v, int j) {
    kn_insert_t<false>(ls, li, nullptr, k, lane, v, j, make_int2(0, 0));
}

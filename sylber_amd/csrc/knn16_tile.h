// The 16-bit contraction that knn16.hip (knn16_scan_kernel), dtw16.hip (dtw16_scan_kernel) and dtwpq.hip (dtwpq_scan_kernel)
// share: knn_tile.h's tile (128 query rows x 128 database rows, 2 x 2 waves of 2 x 2 fragments of
// 32 x 32) on v_mfma_f32_32x32x16_{f16,bf16}, whose C layout is the fp32 MFMA's.  One definition of the operand roles and of the
// K order keeps a coarse score's bits the same wherever it is computed: an output element is one MFMA chain over K in ascending
// 16-wide steps.
#pragma once
#include "knn_tile.h"

constexpr int K16_BK = 32;                                // halves per K step through LDS: two MFMAs of K = 16 per fragment pair
constexpr int K16_LD = 40;                                // LDS row stride in halves (80 B: 16-byte aligned, staggered banks)
static_assert(2 * KN_BM * K16_LD * 2 == KN_STAGE * 4, "the 16-bit staging fills the fp32 kernel's staging exactly (what aliases one aliases the other)");

// one K step of 32 from the staging xs (query rows [128][K16_LD]) / cs (database rows): wave (wm, wn) accumulates its 64 x 64
// quadrant.  Lane (frow, fh) holds k = 8 fh + 0..7 of its row for each MFMA: database rows are A, query rows B, as in kn_mma.  A
// 32-row half fm of the queries with live[fm] == false (wave-uniform) skips its MFMAs.  knn16_scan_kernel keeps this loop written out
// in its body: called from here its instruction schedule came out different, and that kernel's stream is pinned.
template <int FMT>
__device__ __forceinline__ void k16_mma(const bf16_t* xs, const bf16_t* cs, int wm, int wn, int frow, int fh, f32x16_t (&acc)[2][2],
                                        bool live0, bool live1) {
#pragma unroll
    for (int kk = 0; kk < K16_BK / 16; ++kk) {
        bf16x8_t xf[2], cf[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            xf[f] = *(const bf16x8_t*)(xs + (wm * 64 + f * 32 + frow) * K16_LD + kk * 16 + fh * 8);
            cf[f] = *(const bf16x8_t*)(cs + (wn * 64 + f * 32 + frow) * K16_LD + kk * 16 + fh * 8);
        }
#pragma unroll
        for (int fm = 0; fm < 2; ++fm) {
            if (!(fm ? live1 : live0)) continue;
#pragma unroll
            for (int fn = 0; fn < 2; ++fn) acc[fm][fn] = H16<FMT>::mfma(cf[fn], xf[fm], acc[fm][fn]);
        }
    }
}

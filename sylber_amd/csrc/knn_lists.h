// The list kernels that knn.hip (sylber_knn_search, sylber_ivf_search) and knn16.hip (sylber_knn16_scan) share: the pairwise merge of
// sorted partial lists and the reported values.  They are static: each translation unit that launches them carries its own copy.
#pragma once
#include "knn_tile.h"

// one wave per (row, pair): lists 2p and 2p + 1 of row r (m lists of k per row in src) -> list p of row r (ceil(m / 2) per row in
// dst).  An element's rank in the merged list is its position plus the number of entries of the other list before it (A's elements go
// before B's equal ones: only the (+inf, INT_MAX) fillers can be equal), so every output slot < k is written exactly once.
static __global__ __launch_bounds__(64) void knn_merge_kernel(const float* __restrict__ ss, const int32_t* __restrict__ si, int m, int k,
                                                       float* __restrict__ ds, int32_t* __restrict__ di) {
    const int r = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    const int mo = (m + 1) / 2;
    const float* as = ss + ((size_t)r * m + 2 * p) * k;
    const int32_t* ai = si + ((size_t)r * m + 2 * p) * k;
    float* os = ds + ((size_t)r * mo + p) * k;
    int32_t* oi = di + ((size_t)r * mo + p) * k;
    if (2 * p + 1 >= m) {
        for (int e = lane; e < k; e += 64) { os[e] = as[e]; oi[e] = ai[e]; }
        return;
    }
    const float* bs = as + k;
    const int32_t* bi = ai + k;
    for (int e = lane; e < k; e += 64) {
        {   // A[e]: + #{B strictly better}
            const float v = as[e]; const int j = ai[e];
            int lo = 0, hi = k;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (kn_better(bs[mid], bi[mid], v, j)) lo = mid + 1; else hi = mid; }
            if (e + lo < k) { os[e + lo] = v; oi[e + lo] = j; }
        }
        {   // B[e]: + #{A not worse}
            const float v = bs[e]; const int j = bi[e];
            int lo = 0, hi = k;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (!kn_better(v, j, as[mid], ai[mid])) lo = mid + 1; else hi = mid; }
            if (e + lo < k) { os[e + lo] = v; oi[e + lo] = j; }
        }
    }
}

// reported values: L2 max(0, ||q||^2 + s), inner product -s / 2 (as 0 - s / 2, so that s = 0 reports +0); fillers -> (+inf, -1)
static __global__ __launch_bounds__(256) void knn_finish_kernel(const float* __restrict__ ls, const int32_t* __restrict__ li, int n, int k,
                                                         const float* __restrict__ qsq, float* __restrict__ score, int64_t* __restrict__ idx) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n * k) return;
    const int j = li[e];
    const float s = ls[e];
    if (j == INT_MAX) { score[e] = INFINITY; idx[e] = -1; return; }
    score[e] = qsq ? fmaxf(0.f, qsq[e / k] + s) : 0.f - 0.5f * s;
    idx[e] = j;
}

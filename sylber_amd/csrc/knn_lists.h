// The list kernels that knn.hip (sylber_knn_search, sylber_ivf_search), knn16.hip (sylber_knn16_scan), pq.hip (sylber_pq_scan,
// sylber_ivfpq_scan), dtw16_scan.h (sylber_dtw16_scan, sylber_dtwpq_scan) and dtw.hip (sylber_dtw_search) share: the pairwise merge
// of sorted partial lists and the reported values.  They are static: each translation unit that launches them carries its own
// copy.  Below knn_merge_kernel is the host side of the merge, written once for the entry points whose lists are (score, id): where
// the partial lists lie in a workspace (KnPartials, kn_partials_bytes, kn_partials_carve) and the merge rounds (kn_merge_lists).
// dtw.hip's lists carry a span: it launches knn_merge_kernel<true> from its own rounds and reports with its own dtw_finish_kernel.
#pragma once
#include "knn_tile.h"

// one wave per (row, pair): lists 2p and 2p + 1 of row r (m lists of k per row in src) -> list p of row r (ceil(m / 2) per row in
// dst).  An element's rank in the merged list is its position plus the number of entries of the other list before it (A's elements go
// before B's equal ones: only the (+inf, INT_MAX) fillers can be equal), so every output slot < k is written exactly once.  With
// PAYLOAD every entry carries an int2 (sp -> dp: dtw.hip's spans), as kn_insert_t's lists do; without, sp and dp are null.
template <bool PAYLOAD>
static __global__ __launch_bounds__(64) void knn_merge_kernel(const float* __restrict__ ss, const int32_t* __restrict__ si,
                                                              const int2* __restrict__ sp, int m, int k, float* __restrict__ ds,
                                                              int32_t* __restrict__ di, int2* __restrict__ dp) {
    const int r = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    const int mo = (m + 1) / 2;
    const size_t ao = ((size_t)r * m + 2 * p) * k, oo = ((size_t)r * mo + p) * k;
    const float* as = ss + ao; const int32_t* ai = si + ao; const int2* ap = PAYLOAD ? sp + ao : nullptr;
    float* os = ds + oo; int32_t* oi = di + oo; int2* op = PAYLOAD ? dp + oo : nullptr;
    if (2 * p + 1 >= m) {
        for (int e = lane; e < k; e += 64) { os[e] = as[e]; oi[e] = ai[e]; if (PAYLOAD) op[e] = ap[e]; }
        return;
    }
    const float* bs = as + k; const int32_t* bi = ai + k; const int2* bp = PAYLOAD ? ap + k : nullptr;
    for (int e = lane; e < k; e += 64) {
        {   // A[e]: + #{B strictly better}
            const float v = as[e]; const int j = ai[e];
            int lo = 0, hi = k;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (kn_better(bs[mid], bi[mid], v, j)) lo = mid + 1; else hi = mid; }
            if (e + lo < k) { os[e + lo] = v; oi[e + lo] = j; if (PAYLOAD) op[e + lo] = ap[e]; }
        }
        {   // B[e]: + #{A not worse}
            const float v = bs[e]; const int j = bi[e];
            int lo = 0, hi = k;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (!kn_better(v, j, as[mid], ai[mid])) lo = mid + 1; else hi = mid; }
            if (e + lo < k) { os[e + lo] = v; oi[e + lo] = j; if (PAYLOAD) op[e + lo] = bp[e]; }
        }
    }
}

// The partial lists of a search in its workspace: L sorted lists of k per row from the scan, and room for the ceil(L / 2) of the
// first merge round; the rounds ping-pong between the two.
//     scores [n][L][k] | ids [n][L][k] | scores [n][ceil(L/2)][k] | ids [n][ceil(L/2)][k]
struct KnPartials { float* s0; int32_t* i0; float* s1; int32_t* i1; };

static inline int64_t kn_partials_bytes(int64_t n, int64_t L, int64_t k) {
    return 2 * kn_al(n * L * k * 4) + 2 * kn_al(n * ((L + 1) / 2) * k * 4);
}

static inline KnPartials kn_partials_carve(char*& w, int64_t n, int64_t L, int64_t k) {
    KnPartials p;
    p.s0 = (float*)w; w += kn_al(n * L * k * 4);
    p.i0 = (int32_t*)w; w += kn_al(n * L * k * 4);
    p.s1 = (float*)w; w += kn_al(n * ((L + 1) / 2) * k * 4);
    p.i1 = (int32_t*)w; w += kn_al(n * ((L + 1) / 2) * k * 4);
    return p;
}

// the ceil(log2 L) merge rounds of the L lists per row in (p.s0, p.i0); on return (p.s0, p.i0) is the one merged list per row [n][k]
static inline int kn_merge_lists(KnPartials& p, int n, int L, int k, hipStream_t s) {
    for (int m = L; m > 1; m = (m + 1) / 2) {
        hipLaunchKernelGGL(knn_merge_kernel<false>, dim3((unsigned)n, (unsigned)((m + 1) / 2)), dim3(64), 0, s, p.s0, p.i0, (const int2*)nullptr, m, k,
                           p.s1, p.i1, (int2*)nullptr);
        HIP_TRY(hipGetLastError());
        float* ts = p.s0; p.s0 = p.s1; p.s1 = ts;
        int32_t* ti = p.i0; p.i0 = p.i1; p.i1 = ti;
    }
    return 0;
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

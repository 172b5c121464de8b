// The host side that the two occurrence entries share (dtw.hip: sylber_dtw_occurrences, dtw16.hip: sylber_dtw_rerank_occurrences):
// where the partial lists of (cost, start row, (start row, end row)) lie in a workspace, their merge rounds with
// knn_merge_kernel<true> (knn_lists.h) and the kernel that reports.  The device pieces of the scan itself are dtw_tile.h's
// (DtOcc, dt_occ_cell, dt_occ_wavefront).  Static, as knn_lists.h's kernels are: each of the two translation units carries a copy.
#pragma once
#include "dtw_tile.h"
#include "knn_lists.h"
#include <climits>

// L sorted lists of k per phrase and room for the ceil(L / 2) of the first merge round; the rounds ping-pong between the two:
//     costs, start rows, spans [n][L][k] | the same [n][ceil(L / 2)][k]
// (the layout of sylber_dtw_search's lists behind its ||q||^2, so that sylber_dtw_workspace_bytes sizes sylber_dtw_occurrences)
struct DtOccLists { float* s0; int32_t* i0; int2* p0; float* s1; int32_t* i1; int2* p1; };

static inline int64_t dt_occ_lists_bytes(int64_t n, int64_t L, int64_t k) {
    const int64_t a = n * L * k, b = n * ((L + 1) / 2) * k;
    return 2 * kn_al(a * 4) + kn_al(a * 8) + 2 * kn_al(b * 4) + kn_al(b * 8);
}

static inline DtOccLists dt_occ_lists_carve(char* w, int64_t n, int64_t L, int64_t k) {
    const int64_t a = n * L * k, b = n * ((L + 1) / 2) * k;
    DtOccLists p;
    p.s0 = (float*)w; w += kn_al(a * 4);
    p.i0 = (int32_t*)w; w += kn_al(a * 4);
    p.p0 = (int2*)w; w += kn_al(a * 8);
    p.s1 = (float*)w; w += kn_al(b * 4);
    p.i1 = (int32_t*)w; w += kn_al(b * 4);
    p.p1 = (int2*)w;
    return p;
}

// An entry's sequence is that of its start row: seqid[row] where the caller has the table (the scan), else the last s with
// soff[s] <= row (the re-rank, which has the offsets).  Fillers -> (+inf, -1, (-1, -1)); spans as (first row, one past the last).
static __global__ __launch_bounds__(256) void dtw_occ_finish_kernel(const float* __restrict__ ls, const int32_t* __restrict__ li,
                                                                    const int2* __restrict__ lp, int64_t tot, const int32_t* __restrict__ seqid,
                                                                    const int32_t* __restrict__ soff, int S, float* __restrict__ cost,
                                                                    int64_t* __restrict__ seq, int64_t* __restrict__ span) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tot) return;
    const int j = li[e];
    if (j == INT_MAX) { cost[e] = INFINITY; seq[e] = -1; span[2 * e] = -1; span[2 * e + 1] = -1; return; }
    int s;
    if (seqid) s = seqid[j];
    else {
        int lo = 0, hi = S;                                // soff[0] = 0 <= j < soff[S]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (soff[mid] <= j) lo = mid; else hi = mid; }
        s = lo;
    }
    const int2 p = lp[e];
    cost[e] = ls[e]; seq[e] = s; span[2 * e] = p.x; span[2 * e + 1] = (int64_t)p.y + 1;
}

// the ceil(log2 L) merge rounds of the L lists per phrase in (p.s0, p.i0, p.p0); on return those three are the one merged list
// per phrase [n][k] (unit_search.hip reports it itself: its costs are int32)
static inline int dt_occ_merge(DtOccLists& p, int n, int L, int k, hipStream_t s) {
    for (int m = L; m > 1; m = (m + 1) / 2) {
        hipLaunchKernelGGL(knn_merge_kernel<true>, dim3((unsigned)n, (unsigned)((m + 1) / 2)), dim3(64), 0, s, p.s0, p.i0, (const int2*)p.p0, m, k,
                           p.s1, p.i1, p.p1);
        HIP_TRY(hipGetLastError());
        float* ts = p.s0; p.s0 = p.s1; p.s1 = ts;
        int32_t* ti = p.i0; p.i0 = p.i1; p.i1 = ti;
        int2* tp = p.p0; p.p0 = p.p1; p.p1 = tp;
    }
    return 0;
}

// the merge rounds, then the report of the one list left
static inline int dt_occ_merge_finish(DtOccLists p, int n, int L, int k, const int32_t* seqid, const int32_t* soff, int S, float* cost_dev,
                                      int64_t* seq_dev, int64_t* span_dev, hipStream_t s) {
    if (dt_occ_merge(p, n, L, k, s)) return 1;
    const int64_t tot = (int64_t)n * k;
    hipLaunchKernelGGL(dtw_occ_finish_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, p.s0, p.i0, p.p0, tot, seqid, soff, S, cost_dev,
                       seq_dev, span_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

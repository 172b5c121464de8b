// Phrase search through the inverted file, stage 1b (sylber_amd/search.py: SyllableIndex.search_phrases_seeded; contract in
// include/sylber_hip.h, restated in tests/phrase_vote_ref.py): the per-row neighbours ("seeds") of a phrase's rows vote for candidate
// sequences.  bound(p, s) adds, over the phrase's rows in ascending order, the smallest local cost of a seed of that row in sequence
// s, or the row's floor (its largest valid seed cost) when it has none there: a lower bound of the subsequence-DTW cost whenever
// the seeds are each row's true nearest rows.  The m smallest admissible seen sequences under (bound, sequence) are the candidates.
//   * one workgroup per phrase; all of it lives in LDS.  A seed is slot = row * seeds + e; key[slot] = (sequence << 32 | row << 16 |
//     slot), d[slot] its local cost; an ignored seed and the padding up to the next power of two get the key ~0.  Keys are distinct,
//     so the bitonic sort has one result whatever the schedule.
//   * segment minima: the thread at the head of a (sequence, row) run (at most `seeds` long) scans it, leaves the minimum in the
//     head's d and the run's length in len[]: nobody else reads the d of that run.
//   * one lane per distinct sequence: from the head of the sequence's run it hops from (sequence, row) head to head (at most 64 of
//     them), adding floors for the rows between, one fp32 addition per row in ascending row order.
//   * selection: the keys are replaced by (ordered bits of the bound << 32 | sequence) at the sequence heads and ~0 elsewhere, and
//     sorted again; the first m are the output.  Every value is an fp32 min, max or add in a fixed order: no atomics on floats
//     (the floors use an integer max on order-preserving bits, which is exact), no global atomics, no [P, S] table.
// LDS: cap = the power of two >= 64 x seeds (<= 8 192): 8 cap (keys) + 4 cap (d) + 2 cap (run lengths) + 256 (floors) = at most
// 114 944 B, dynamic.  seeds <= 32 (cap <= 2 048) runs 256 threads, else 1 024: eight slots per thread either way.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "knn_tile.h"

constexpr int PV_MAX_ROWS = 64;                           // DT_MAX_M: rows of a phrase
constexpr int PV_MAX_SEEDS = 128;
constexpr int PV_PER = 8;                                 // slots per thread
constexpr unsigned long long PV_NONE = ~0ull;

static size_t pv_lds_bytes(int cap) { return (size_t)cap * 14 + PV_MAX_ROWS * 4; }

// order-preserving bits of a non-NaN float: a < b  <=>  pv_ord(a) < pv_ord(b) (and -0 < +0); never 0 and never ~0u
__device__ __forceinline__ uint32_t pv_ord(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float pv_unord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// ascending bitonic sort of key[0 .. n), n a power of two; every thread of the workgroup calls it
template <int NT>
__device__ __forceinline__ void pv_sort(unsigned long long* key, int n, int tid) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n >> 1); t += NT) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long a = key[lo], b = key[hi];
                if ((a > b) == ((lo & k) == 0)) { key[lo] = b; key[hi] = a; }
            }
            __syncthreads();
        }
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void phrase_vote_kernel(const float* __restrict__ score, const int64_t* __restrict__ ids, int seeds,
                                                         const int32_t* __restrict__ prow, const int32_t* __restrict__ plen,
                                                         const int32_t* __restrict__ soff, int S, int ip,
                                                         const int32_t* __restrict__ pgrp, const int32_t* __restrict__ sgrp, int m,
                                                         int cap, int32_t* __restrict__ cand, float* __restrict__ bound) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pv_smem[];
    unsigned long long* key = (unsigned long long*)pv_smem;              // [cap]
    float* d = (float*)(pv_smem + (size_t)cap * 8);                       // [cap]
    uint32_t* flo = (uint32_t*)(pv_smem + (size_t)cap * 12);              // [64] ordered bits of each row's floor, 0 = no valid seed
    uint16_t* len = (uint16_t*)(pv_smem + (size_t)cap * 12 + PV_MAX_ROWS * 4);   // [cap]
    const int tid = threadIdx.x, p = blockIdx.x;
    int mp = plen[p];
    mp = mp < 1 ? 1 : (mp > PV_MAX_ROWS ? PV_MAX_ROWS : mp);
    const int total = mp * seeds;                         // <= cap
    int n = 2;
    while (n < total) n <<= 1;                            // the sorted length, <= cap
    const int64_t N = soff[S];
    const size_t base = (size_t)prow[p] * seeds;
    if (tid < PV_MAX_ROWS) flo[tid] = 0u;
    __syncthreads();
    // the seeds: local cost, sequence by binary search, key
    for (int t = tid; t < n; t += NT) {
        unsigned long long kk = PV_NONE;
        if (t < total) {
            const int64_t id = ids[base + t];
            const float sc = score[base + t];
            const float dd = ip ? fmaxf(0.f, 1.f - sc) : sc;
            if (id >= 0 && id < N && sc == sc && dd != INFINITY) {
                int lo = 0, hi = S;                       // the s with soff[s] <= id < soff[s + 1]
                while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((int64_t)soff[mid] <= id) lo = mid; else hi = mid; }
                const int row = t / seeds;
                kk = ((unsigned long long)(uint32_t)lo << 32) | ((unsigned long long)row << 16) | (unsigned long long)t;
                d[t] = dd;
                atomicMax(&flo[row], pv_ord(dd));         // an integer max in LDS: exact, whatever the order
            }
        }
        key[t] = kk;
    }
    __syncthreads();
    pv_sort<NT>(key, n, tid);
    // segment minima: the head of each (sequence, row) run scans it
    for (int t = tid; t < n; t += NT) {
        const unsigned long long kk = key[t];
        if (kk == PV_NONE) continue;
        if (t > 0 && (key[t - 1] >> 16) == (kk >> 16)) continue;
        float mn = d[(int)(kk & 0xffffu)];
        int u = t + 1;
        for (; u < n; ++u) {
            const unsigned long long ku = key[u];
            if ((ku >> 16) != (kk >> 16)) break;
            mn = fminf(mn, d[(int)(ku & 0xffffu)]);
        }
        d[(int)(kk & 0xffffu)] = mn;
        len[t] = (uint16_t)(u - t);
    }
    __syncthreads();
    // one lane per distinct sequence: its bound, then (bound, sequence) as the key of the selection
    unsigned long long out[PV_PER];
#pragma unroll
    for (int c = 0; c < PV_PER; ++c) {
        const int t = tid + c * NT;
        out[c] = PV_NONE;
        if (t >= n) continue;
        const unsigned long long kk = key[t];
        if (kk == PV_NONE) continue;
        const uint32_t s = (uint32_t)(kk >> 32);
        if (t > 0 && (uint32_t)(key[t - 1] >> 32) == s) continue;
        if (pgrp && sgrp[s] == pgrp[p]) continue;         // seen, not admissible
        float acc = 0.f;
        int i = 0, u = t;
        while (u < n) {
            const unsigned long long ku = key[u];
            if ((uint32_t)(ku >> 32) != s) break;         // ~0 keys end the run too: a sequence number is below 2^31
            const int row = (int)((ku >> 16) & 0xffffu);
            for (; i < row; ++i) acc = acc + (flo[i] ? pv_unord(flo[i]) : 0.f);
            acc = acc + d[(int)(ku & 0xffffu)];
            i = row + 1;
            u += len[u];
        }
        for (; i < mp; ++i) acc = acc + (flo[i] ? pv_unord(flo[i]) : 0.f);
        if (acc < INFINITY) out[c] = ((unsigned long long)pv_ord(acc) << 32) | s;
    }
    __syncthreads();                                      // every lane is past its reads of the keys
#pragma unroll
    for (int c = 0; c < PV_PER; ++c) {
        const int t = tid + c * NT;
        if (t < n) key[t] = out[c];
    }
    __syncthreads();
    pv_sort<NT>(key, n, tid);
    for (int e = tid; e < m; e += NT) {
        const unsigned long long kk = e < n ? key[e] : PV_NONE;
        const size_t o = (size_t)p * m + e;
        if (kk == PV_NONE) { cand[o] = -1; bound[o] = INFINITY; }
        else { cand[o] = (int32_t)(kk & 0xffffffffu); bound[o] = pv_unord((uint32_t)(kk >> 32)); }
    }
}

extern "C" int sylber_phrase_vote(const float* seed_score_dev, const int64_t* seed_id_dev, int32_t seeds, const int32_t* phrase_row_dev,
                                  const int32_t* phrase_len_dev, int32_t n_phrases, const int32_t* seq_offsets_dev, int32_t n_seq,
                                  int32_t metric, const int32_t* phrase_group_dev, const int32_t* seq_group_dev, int32_t m,
                                  int32_t* cand_dev, float* bound_dev, void* stream) {
    static const char* what = "sylber_phrase_vote";
    hipStream_t s = (hipStream_t)stream;
    if (!seed_score_dev || !seed_id_dev || !phrase_row_dev || !phrase_len_dev || !seq_offsets_dev || !cand_dev || !bound_dev) {
        syl_set_error(what, "null argument"); return 1;
    }
    if (seeds < 1 || seeds > PV_MAX_SEEDS) { syl_set_error(what, "need 1 <= seeds <= 128"); return 1; }
    if (n_phrases < 1 || n_seq < 1) { syl_set_error(what, "need n_phrases, n_seq >= 1"); return 1; }
    if (m < 1 || m > KN_KMAX) { syl_set_error(what, "need 1 <= m <= 128"); return 1; }
    if (metric != SYLBER_KNN_L2 && metric != SYLBER_KNN_IP) { syl_set_error(what, "unknown metric"); return 1; }
    if (!phrase_group_dev != !seq_group_dev) { syl_set_error(what, "phrase_group_dev and seq_group_dev go together"); return 1; }
    if ((int64_t)n_phrases * m > INT32_MAX) { syl_set_error(what, "n_phrases x m is too large: use smaller phrase chunks"); return 1; }
    int cap = 2;
    while (cap < PV_MAX_ROWS * seeds) cap <<= 1;
    const size_t lds = pv_lds_bytes(cap);
    const int max_lds = (int)pv_lds_bytes(PV_MAX_ROWS * PV_MAX_SEEDS);
    const int ip = metric == SYLBER_KNN_IP;
    if (cap <= 256 * PV_PER) {
        static PerDeviceOnce once;
        if (once.need()) HIP_TRY(hipFuncSetAttribute((const void*)phrase_vote_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
        hipLaunchKernelGGL(phrase_vote_kernel<256>, dim3((unsigned)n_phrases), dim3(256), lds, s, seed_score_dev, seed_id_dev, seeds,
                           phrase_row_dev, phrase_len_dev, seq_offsets_dev, n_seq, ip, phrase_group_dev, seq_group_dev, m, cap, cand_dev,
                           bound_dev);
    } else {
        static PerDeviceOnce once;
        if (once.need()) HIP_TRY(hipFuncSetAttribute((const void*)phrase_vote_kernel<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
        hipLaunchKernelGGL(phrase_vote_kernel<1024>, dim3((unsigned)n_phrases), dim3(1024), lds, s, seed_score_dev, seed_id_dev, seeds,
                           phrase_row_dev, phrase_len_dev, seq_offsets_dev, n_seq, ip, phrase_group_dev, seq_group_dev, m, cap, cand_dev,
                           bound_dev);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

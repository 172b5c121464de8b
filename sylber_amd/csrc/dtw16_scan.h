// The host path that dtw16.hip (sylber_dtw16_scan: the database is a 16-bit plane of the rows) and dtwpq.hip (sylber_dtwpq_scan: the
// database is product-quantization codes, decoded into the MFMA) share: the argument checks, the partial lists, the launch, their
// merge and the candidates.  The two scan kernels themselves are built from dtw_tile.h's pieces in their own files:
// dtwpq_scan_kernel from all of them, dtw16_scan_kernel from the column data alone (see dtw16.hip for why).
#pragma once
#include <type_traits>
#include "../../include/sylber_hip.h"
#include "dtw_tile.h"
#include "knn16_tile.h"
#include "knn_lists.h"

static size_t d16_lds_bytes(int ph, int m) { return (size_t)DT_FIXED * 4 + (size_t)ph * m * 8; }

// the merged lists as candidates: the (+inf, INT_MAX) fillers become (+inf, -1)
static __global__ __launch_bounds__(256) void dtw16_cand_kernel(const float* __restrict__ ls, const int32_t* __restrict__ li, int64_t tot,
                                                                int32_t* __restrict__ cand, float* __restrict__ coarse) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tot) return;
    const int j = li[e];
    cand[e] = j == INT_MAX ? -1 : j;
    coarse[e] = j == INT_MAX ? INFINITY : ls[e];
}

// The host side of sylber_dtw16_scan and sylber_dtwpq_scan behind an entry's own null check: the checks that the two share in the
// order they had (db_error: the entry's verdict on its database arguments, or null), the partial lists, the launch, their merge and
// the candidates.  launch(std::integral_constant<int, FMT>, grid, lds bytes, the largest lds bytes, qn, cn, ps, pi) sets the dynamic-LDS limit of the
// entry's kernel once per device and launches it; a static of a generic lambda is one per FMT.
template <class Launch>
static int dt16_scan_host(const char* what, const char* db_error, const char* l2_error, int32_t n_blocks, int32_t n_phrases,
                          int32_t block_phrases, int32_t N, int32_t D, const float* db_norm_dev, const float* q_norm_dev, int32_t metric,
                          int32_t storage, int32_t m, int32_t cuts, const int32_t* phrase_group_dev, const int32_t* seq_group_dev,
                          int32_t* cand_dev, float* coarse_dev, void* workspace_dev, hipStream_t s, Launch launch) {
    if (n_blocks < 1 || n_phrases < 1 || N < 1 || D < 16 || D % 16) { syl_set_error(what, "need n_blocks, n_phrases, N >= 1 and D a multiple of 16"); return 1; }
    if (db_error) { syl_set_error(what, db_error); return 1; }
    if (m < 1 || m > KN_KMAX) { syl_set_error(what, "need 1 <= m <= 128"); return 1; }
    if (block_phrases < 1 || block_phrases > dt_block_phrases(m, 0)) { syl_set_error(what, "block_phrases exceeds what sylber_dtw_plan allows for this m"); return 1; }
    if (cuts < 1 || cuts > 65535) { syl_set_error(what, "need 1 <= cuts <= 65535"); return 1; }
    if (metric != SYLBER_KNN_L2 && metric != SYLBER_KNN_IP) { syl_set_error(what, "unknown metric"); return 1; }
    if (storage != SYLBER_KNN16_FP16 && storage != SYLBER_KNN16_BF16) { syl_set_error(what, "unknown storage"); return 1; }
    if (metric == SYLBER_KNN_L2 && (!db_norm_dev || !q_norm_dev)) { syl_set_error(what, l2_error); return 1; }
    if (!phrase_group_dev != !seq_group_dev) { syl_set_error(what, "phrase_group_dev and seq_group_dev go together"); return 1; }
    if ((int64_t)n_phrases * cuts * m > INT32_MAX / 2) { syl_set_error(what, "n_phrases x cuts x m is too large: use smaller phrase chunks"); return 1; }
    char* w = (char*)workspace_dev;
    KnPartials p = kn_partials_carve(w, n_phrases, cuts, m);
    const size_t lds = d16_lds_bytes(block_phrases, m);
    const int max_lds = (int)((size_t)DT_FIXED * 4 + DT_LIST_BYTES / 2);
    const float* qn = metric == SYLBER_KNN_L2 ? q_norm_dev : nullptr;
    const float* cn = metric == SYLBER_KNN_L2 ? db_norm_dev : nullptr;
    const dim3 grid((unsigned)n_blocks, (unsigned)cuts);
    if (storage == SYLBER_KNN16_FP16 ? launch(std::integral_constant<int, FMT_F16>(), grid, lds, max_lds, qn, cn, p.s0, p.i0)
                                     : launch(std::integral_constant<int, FMT_BF16>(), grid, lds, max_lds, qn, cn, p.s0, p.i0)) return 1;
    HIP_TRY(hipGetLastError());
    if (kn_merge_lists(p, n_phrases, cuts, m, s)) return 1;
    const int64_t tot = (int64_t)n_phrases * m;
    hipLaunchKernelGGL(dtw16_cand_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, p.s0, p.i0, tot, cand_dev, coarse_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The geometry that dtw.hip (dtw_search_kernel) and dtw16.hip (dtw16_scan_kernel, dtw_rerank_kernel) share: the cost tile that the
// dynamic programme reads, the limits of a phrase and of a sequence, and how many phrases sylber_dtw_plan packs into a query block.
#pragma once
#include "knn_tile.h"

constexpr int DT_LD = 132;                                // row stride of the cost tile: lane i reads d[i][t - i], bank (3 i + t) % 32
constexpr int DT_MAX_M = 64;                              // rows of a phrase: one wave
constexpr int DT_MAX_SEQ = 65536;                         // rows of a sequence (the DP along a sequence is serial)
constexpr int DT_FIXED = KN_BM * DT_LD + KN_BN + 132 + KN_BN;   // floats: cost tile (aliases the staging) | c_j | sequence ids | groups
constexpr int DT_LIST_BYTES = 65536;                      // LDS of a workgroup's lists, 16 B per entry: 32 phrases at k = 128

static_assert(DT_FIXED * 4 % 16 == 0, "the lists start 16-byte aligned");
static inline int dt_block_phrases(int k, int block_phrases) {
    int ph = DT_LIST_BYTES / (16 * k);
    ph = ph < KN_BM ? ph : KN_BM;
    return block_phrases > 0 && block_phrases < ph ? block_phrases : ph;
}

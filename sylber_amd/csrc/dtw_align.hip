// Warping paths (sylber_amd/search.py: SyllableIndex.align_phrases; contract in include/sylber_hip.h, restated in
// tests/align_ref.py): for a (phrase, window of rows) pair, which stored rows each phrase row was warped onto.
//   * dtw_align_kernel: dtw_rerank_kernel's sibling -- one wave per pair, lane l owns phrase row l, the window walked in chunks.
//     The lane's set-up, a chunk's local costs (the explicit ascending __builtin_fmaf chain) and the wavefront over a chunk are
//     dtw_pair.h's, the cell is dtw_tile.h's dt_cell, so every A[i][j] has the bits dtw_search_kernel gives it on that window
//     taken as one sequence.  Beside the cell each lane takes
//     down a 2-bit code of the predecessor the cell took (DA_NONE for row 0, DA_DIAG, DA_UP, DA_LEFT), from the comparisons
//     dt_cell makes, in dt_cell's order.  A lane's 32 codes of a chunk are one 64-bit word; the wave stores the chunk's words as
//     one coalesced row of 64 x 8 B, so the pair's slice of the workspace is [chunks][64] words = 16 B per column: cell (i, j) is
//     bits 2 ((j - a) % 32) .. + 1 of word [(j - a) / 32][i].  (A word per lane and chunk instead of two ballots per anti-diagonal:
//     the wavefront drains at every chunk edge, so an anti-diagonal is worked on in up to three chunks and its ballots would have
//     to be merged by read-modify-write; a lane's word is complete when the chunk is.)  Plain vector stores only.
//     After the walk, a fence and a barrier, lane 0 follows the codes from (m-1, b-1) back to row 0 -- at most W + m - 1 cells --
//     and writes the run of columns of every phrase row into LDS; the wave writes rows, steps and cost.  The walk keeps
//     dtw_rerank_kernel's start tracking (dt_cell<true>) and hands the tracked start of (m-1, b-1) out where the caller asks for
//     it: tests hold it against the backtracked one, i.e. the codes against the cell that formed them.
//     The kernel's body is dtw_align.h's da_align_pair, which dtw_codes.hip runs on a coded database.
// LDS: 9 216 B of costs (64 rows x 36 floats) + 512 B of runs, 64 threads: wave slots and registers bound the occupancy.
#include "kernels.h"
#include "dtw_align.h"

// dtw_align.h's da_align_pair on the fp32 rows x [N, D]
__global__ __launch_bounds__(64) void dtw_align_kernel(const float* __restrict__ q, const float* __restrict__ qsq, int qrows,
                                                       const int32_t* __restrict__ prow, const int32_t* __restrict__ plen, int P,
                                                       const float* __restrict__ x, int N, int D, const float* __restrict__ cn,
                                                       const int32_t* __restrict__ pp, const int2* __restrict__ win, int max_cols, int Mx,
                                                       int2* __restrict__ rows, int32_t* __restrict__ steps, float* __restrict__ cost,
                                                       int32_t* __restrict__ tstart, uint64_t* ws) {
    __shared__ float dsm[DT_MAX_M * DP_LD];
    __shared__ DaLds lds;
    da_align_pair(dsm, lds, DpRowsSrc{x, D}, q, qsq, qrows, prow, plen, P, N, D, cn, pp, win, max_cols, Mx, rows, steps, cost, tstart, ws);
}

extern "C" int64_t sylber_dtw_align_workspace_bytes(int32_t n_pairs, int32_t max_cols) {
    if (n_pairs < 1 || max_cols < 1 || max_cols > DA_MAX_COLS) return -1;
    return (int64_t)n_pairs * 16 * ((int64_t)max_cols + 63);
}

extern "C" int sylber_dtw_align(const float* q_dev, int32_t n_blocks, const float* q_norm_dev, const int32_t* phrase_row_dev,
                                const int32_t* phrase_len_dev, int32_t n_phrases, const float* db_dev, int32_t N, int32_t D,
                                const float* db_norm_dev, int32_t metric, const int32_t* pair_phrase_dev, const int32_t* pair_window_dev,
                                int32_t n_pairs, int32_t max_cols, int32_t max_rows, int32_t* rows_dev, int32_t* steps_dev, float* cost_dev,
                                int32_t* start_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_dtw_align";
    hipStream_t s = (hipStream_t)stream;
    if (!q_dev || !phrase_row_dev || !phrase_len_dev || !db_dev || !pair_phrase_dev || !pair_window_dev || !rows_dev || !steps_dev ||
        !cost_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    const float *qn, *cn;
    if (dt_pair_check(what, "need n_blocks, n_phrases, n_pairs, N >= 1 and D a multiple of 16",
                      max_cols < 1 || max_cols > DA_MAX_COLS ? "need 1 <= max_cols <= 65536: a window has at most 65536 rows"
                      : max_rows < 1 || max_rows > DT_MAX_M  ? "need 1 <= max_rows <= 64" : nullptr,
                      "too many phrase blocks: use smaller phrase chunks", n_blocks, n_phrases, n_pairs, N, D, q_norm_dev, db_norm_dev, metric, false,
                      qn, cn)) return 1;
    hipLaunchKernelGGL(dtw_align_kernel, dim3((unsigned)n_pairs), dim3(64), 0, s, q_dev, qn, n_blocks * KN_BM, phrase_row_dev, phrase_len_dev,
                       n_phrases, db_dev, N, D, cn, pair_phrase_dev, (const int2*)pair_window_dev, max_cols, max_rows, (int2*)rows_dev,
                       steps_dev, cost_dev, start_dev, (uint64_t*)workspace_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

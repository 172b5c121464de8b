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
// LDS: 9 216 B of costs (64 rows x 36 floats) + 512 B of runs, 64 threads: wave slots and registers bound the occupancy.
#include "kernels.h"
#include "dtw_pair.h"

constexpr int DA_MAX_COLS = 65536;                        // rows of a window: the DP along it is serial, as along a sequence
constexpr unsigned DA_NONE = 0, DA_DIAG = 1, DA_UP = 2, DA_LEFT = 3;

static_assert(DA_MAX_COLS == DT_MAX_SEQ, "a returned span lies inside one sequence");
static_assert(2 * DP_CH == 64, "the 2-bit codes of a lane's chunk fill one 64-bit word");

// the predecessor dt_cell takes for this cell: its comparisons on its operands, in its order -- (i-1, j-1), then (i-1, j), then
// (i, j-1), the first smallest.  Called before dt_cell moves the lane's state on.
__device__ __forceinline__ unsigned da_code(const DtLane& s, const DtUp& u, bool first, bool isstart) {
    if (first) return DA_NONE;
    float best = isstart ? INFINITY : u.a_prev;
    unsigned code = DA_DIAG;
    if (u.a_cur < best) { best = u.a_cur; code = DA_UP; }
    const float left = isstart ? INFINITY : s.a_cur;
    if (left < best) code = DA_LEFT;
    return code;
}

// every lane: the pair is padding on output
__device__ __forceinline__ void da_padding(int lane, size_t pair, int Mx, int2* __restrict__ rows, int32_t* __restrict__ steps,
                                           float* __restrict__ cost, int32_t* __restrict__ tstart) {
    for (int i = lane; i < Mx; i += 64) rows[pair * Mx + i] = make_int2(-1, -1);
    if (lane == 0) { steps[pair] = 0; cost[pair] = INFINITY; if (tstart) tstart[pair] = -1; }
}

// Workgroup (one wave) `pair`: phrase pp[pair] (rows prow[p] .. + plen[p] of the packed fp32 blocks q, qsq their ||q_i||^2 (L2) or
// null) against the window win[pair] = [a, b) of x.  ws: [pairs][chunks of max_cols][64] words.  Writes rows [pairs][Mx] (first row,
// one past the last row) per phrase row, steps, cost and, where tstart is not null, the start row the walk tracked; a window of
// (-1, -1), one outside [0, N] or longer than max_cols and a pair whose A[m-1][b-1] is not below +inf come back as padding:
// ((-1, -1) .., 0, +inf, -1).
__global__ __launch_bounds__(64) void dtw_align_kernel(const float* __restrict__ q, const float* __restrict__ qsq, int qrows,
                                                       const int32_t* __restrict__ prow, const int32_t* __restrict__ plen, int P,
                                                       const float* __restrict__ x, int N, int D, const float* __restrict__ cn,
                                                       const int32_t* __restrict__ pp, const int2* __restrict__ win, int max_cols, int Mx,
                                                       int2* __restrict__ rows, int32_t* __restrict__ steps, float* __restrict__ cost,
                                                       int32_t* __restrict__ tstart, uint64_t* ws) {
    __shared__ float dsm[DT_MAX_M * DP_LD];
    __shared__ int rlo[DT_MAX_M], rhi[DT_MAX_M];
    __shared__ int nstep;
    const int lane = threadIdx.x;
    const size_t pair = blockIdx.x;
    const int p = pp[pair];
    const int2 w = win[pair];
    const int j0 = w.x, j1 = w.y;
    if (p < 0 || p >= P || j0 < 0 || j1 > N || j1 <= j0 || j1 - j0 > max_cols) {      // workgroup-uniform
        da_padding(lane, pair, Mx, rows, steps, cost, tstart);
        return;
    }
    const DpLane L(q, qsq, qrows, prow, plen, p, D, lane, Mx);
    const int mp = L.mp;
    const int W = j1 - j0;
    uint64_t* wp = ws + pair * ((size_t)((max_cols + DP_CH - 1) / DP_CH) * 64);
    DtLane st;
    float* dr = dsm + lane * DP_LD;
    for (int n0 = j0; n0 < j1; n0 += DP_CH) {
        const int ncol = j1 - n0 < DP_CH ? j1 - n0 : DP_CH;
        dp_chunk_costs(dr, L, x, D, cn, qsq != nullptr, n0, ncol, j1);
        uint64_t codes = 0;
        dp_walk(st, L, lane, n0, ncol, j0, [&](int j, int col, bool isstart, const DtUp& u) {
            codes |= (uint64_t)da_code(st, u, lane == 0, isstart) << (2 * j);
            dt_cell<true>(st, u, lane == 0, false, isstart, dr[j], col);
        });
        wp[(size_t)((n0 - j0) / DP_CH) * 64 + lane] = codes;
    }
    const float A = __shfl(st.a_cur, mp - 1);              // A[m-1][b-1]: the last cell of the last row
    const int ts = __shfl(st.s_cur, mp - 1);               // and the start its path was tracked to
    if (!(A < INFINITY)) {                                 // wave-uniform
        da_padding(lane, pair, Mx, rows, steps, cost, tstart);
        return;
    }
    __threadfence_block();
    __syncthreads();                                       // every lane's words are written and visible to lane 0
    if (lane == 0) {
        int i = mp - 1, j = W - 1, n = 1;
        rhi[i] = j;
        // a finite cell's predecessor is finite and inside the window (what lies outside is +inf), so the chain reaches row 0 in
        // at most W + m - 1 cells; the bound and the j >= 0 test only keep a corrupted workspace from leading anywhere else
        for (int guard = W + mp; i > 0 && guard > 0; --guard) {
            const unsigned code = (unsigned)(wp[(size_t)(j / DP_CH) * 64 + i] >> (2 * (j % DP_CH))) & 3u;
            if (code != DA_LEFT) { rlo[i] = j; --i; }
            if (code != DA_UP) --j;
            if (j < 0) break;
            if (code != DA_LEFT) rhi[i] = j;
            ++n;
        }
        if (i == 0 && j >= 0) rlo[0] = j;
        nstep = i == 0 && j >= 0 ? n : 0;
    }
    __syncthreads();
    if (nstep == 0) {                                      // unreachable with the workspace this kernel wrote
        da_padding(lane, pair, Mx, rows, steps, cost, tstart);
        return;
    }
    for (int i = lane; i < Mx; i += 64) rows[pair * Mx + i] = i < mp ? make_int2(j0 + rlo[i], j0 + rhi[i] + 1) : make_int2(-1, -1);
    if (lane == 0) { steps[pair] = nstep; cost[pair] = A; if (tstart) tstart[pair] = ts; }
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

// The body of the warping-path kernels: dtw_align.hip's dtw_align_kernel on fp32 rows and dtw_codes.hip's dtw_align_codes_kernel on
// a coded database.  dtw_align.hip's header describes the walk, the 2-bit codes and the walk back; the rows come from a source of
// dtw_pair.h's kind.
#pragma once
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

// LDS of a pair beside the chunk's costs: the run of columns of every phrase row, and the steps of the path
struct DaLds { int rlo[DT_MAX_M], rhi[DT_MAX_M], nstep; };

// Workgroup (one wave) `pair`: phrase pp[pair] (rows prow[p] .. + plen[p] of the packed fp32 blocks q, qsq their ||q_i||^2 (L2) or
// null) against the window win[pair] = [a, b) of the N rows that src hands out.  dsm: DT_MAX_M * DP_LD floats of LDS, lds: the
// runs.  ws: [pairs][chunks of max_cols][64] words.  Writes rows [pairs][Mx] (first row, one past the last row) per phrase row,
// steps, cost and, where tstart is not null, the start row the walk tracked; a window of (-1, -1), one outside [0, N] or longer
// than max_cols and a pair whose A[m-1][b-1] is not below +inf come back as padding: ((-1, -1) .., 0, +inf, -1).
template <class Src>
__device__ __forceinline__ void da_align_pair(float* dsm, DaLds& lds, const Src& src, const float* __restrict__ q, const float* __restrict__ qsq,
                                              int qrows, const int32_t* __restrict__ prow, const int32_t* __restrict__ plen, int P, int N, int D,
                                              const float* __restrict__ cn, const int32_t* __restrict__ pp, const int2* __restrict__ win,
                                              int max_cols, int Mx, int2* __restrict__ rows, int32_t* __restrict__ steps,
                                              float* __restrict__ cost, int32_t* __restrict__ tstart, uint64_t* ws) {
    int (&rlo)[DT_MAX_M] = lds.rlo, (&rhi)[DT_MAX_M] = lds.rhi;
    int& nstep = lds.nstep;
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
        dp_chunk_costs(dr, L, src.chunk(lane, n0, ncol, j1), D, cn, qsq != nullptr, n0, ncol, j1);
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

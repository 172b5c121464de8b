// Edit scripts (sylber_amd/units.py: UnitIndex.align_phrases; contract in include/sylber_hip.h "Edit scripts", restated in
// tests/unit_align_ref.py): for a (phrase of unit ids, window of rows) pair, which stored row each phrase unit is paired with, what
// that pairing costs, and how many units are equal, substituted, deleted and inserted.  unit_search.hip's sibling as dtw_align.hip
// is the DTW scans': the scans keep a start row and no path, and the window DP on a returned span takes the scan's own path.
//   * unit_align_kernel<WP>: one wave per pair.  Lane i holds phrase unit i (its W ids padded to WP = 1, 2, 4 or 8 words with
//     zeros, as the scan pads them) and walks the window on unit_scan_body's anti-diagonal wavefront: at step st it works on column
//     st - i, so the wave is through after L + m - 1 steps and nothing drains in between.  A cell is (cost, start column) in two
//     int32 -- a window has up to 65 536 columns and, in global mode, costs up to (L + m) W, so the scan's packed word does not
//     hold it; the lane above's cell is fetched every step, and what the lane fetched at its previous column is its next diagonal.
//     The three predecessors are compared as the contract writes them: diagonal, then (i-1, j), then (i, j-1), strictly less to
//     replace.  The window's columns come through a ring of 128 columns in LDS, 32 new ones every 32 steps (a step reads columns
//     st - 63 .. st), loaded a chunk ahead.
//     Each lane takes down the predecessor it took as a 2-bit code (UA_DIAG, UA_UP, UA_LEFT); the codes of a chunk of
//     UA_CH = 32 STEPS are one 64-bit word and the wave stores a chunk's words as one coalesced row of 64 x 8 B.  So the pair's slice
//     of the workspace is [chunks of L + m - 1 steps][64] words -- 16 B per column, rounded up to chunks, plus the skew of up to 63
//     steps -- and cell (i, j) is bits 2 ((i + j) % 32) .. + 1 of word [(i + j) / 32][i].  Plain vector stores only.
//     After a fence and a barrier lane 0 follows the codes from (m-1, L-1) back to row -1 or column -1 -- at most L + m cells, the
//     word it reads kept while row and chunk stay -- and puts the pairing into LDS; the wave writes it out.  The walk forward keeps
//     the scan's start tracking and hands the tracked start of (m-1, L-1) out where the caller asks for it: tests hold it against
//     the first row of the backtracked path, i.e. the codes against the cells that formed them.
// LDS: 4 KiB of ring at WP = 8 and 0.5 KiB of pairing, 64 threads: wave slots bound the occupancy.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "unit_strip.h"                                   // the ring and the mismatch count
#include <climits>

constexpr int UA_CH = 32;                                 // steps of a chunk: their 2-bit codes fill one 64-bit word (units.py: ALIGN_CHUNK_COLS)
constexpr int UA_MAX_COLS = 65536, UA_MAX_M = 64, UA_MAX_W = 8;
constexpr unsigned UA_DIAG = 0, UA_UP = 1, UA_LEFT = 2;

static_assert(2 * UA_CH == 64, "the 2-bit codes of a lane's chunk fill one 64-bit word");
static_assert(UST_RING >= UA_MAX_M - 1 + 2 * UA_CH, "the ring holds a chunk's columns, the 63 behind them and the next chunk");

// the chunks of a window of `cols` columns against a phrase of up to 64 units: L + m - 1 <= cols + 63 steps
__host__ __device__ static inline int64_t ua_chunks(int64_t cols) { return (cols + UA_MAX_M - 1 + UA_CH - 1) / UA_CH; }

// every lane: the pair is padding on output
__device__ __forceinline__ void ua_padding(int lane, size_t pair, int Mx, int32_t* __restrict__ cols, int32_t* __restrict__ subs,
                                           int32_t* __restrict__ ops, int32_t* __restrict__ cost, int32_t* __restrict__ tstart) {
    for (int i = lane; i < Mx; i += 64) { cols[pair * Mx + i] = -1; subs[pair * Mx + i] = -1; }
    if (lane < 4) ops[pair * 4 + lane] = 0;
    if (lane == 0) { cost[pair] = INT_MAX; if (tstart) tstart[pair] = -1; }
}

// Workgroup (one wave) `pair`: phrase pp[pair] (rows prow[p] .. + plen[p] of q [R, W]) against the window win[pair] = [a, b) of
// x [N, W].  ws: [pairs][chunks of max_cols + 63 steps][64] words.  Writes cols, subs [pairs][Mx], ops [pairs][4], cost and, where
// tstart is not null, the first row the walk tracked; a bad pair (see the header) comes back as padding, having read its phrase
// number, its window and its phrase's row and length at most.
template <int WP>
__global__ __launch_bounds__(64) void unit_align_kernel(const int32_t* __restrict__ q, int R, int W, const int32_t* __restrict__ prow,
                                                        const int32_t* __restrict__ plen, int P, const int32_t* __restrict__ x, int N,
                                                        const int32_t* __restrict__ pp, const int2* __restrict__ win, int max_cols, int Mx,
                                                        int free_start, int32_t* __restrict__ cols, int32_t* __restrict__ subs,
                                                        int32_t* __restrict__ ops, int32_t* __restrict__ cost, int32_t* __restrict__ tstart,
                                                        uint64_t* ws) {
    __shared__ __attribute__((aligned(16))) int ring[UST_RING * WP];      // [column % 128][WP] ids of the window's columns
    __shared__ int ocol[UA_MAX_M], osub[UA_MAX_M], oops[4];
    const int lane = threadIdx.x;
    const size_t pair = blockIdx.x;
    const int p = pp[pair];
    const int2 w = win[pair];
    const int a = w.x, b = w.y;
    bool bad = p < 0 || p >= P || a < 0 || b > N || b <= a || b - a > max_cols;      // workgroup-uniform, as all that follows
    int m = 0, r0 = 0;
    if (!bad) {
        m = plen[p]; r0 = prow[p];
        bad = m < 1 || m > UA_MAX_M || m > Mx || r0 < 0 || (int64_t)r0 + m > R;
    }
    if (bad) { ua_padding(lane, pair, Mx, cols, subs, ops, cost, tstart); return; }
    const int L = b - a, nsteps = L + m - 1, nchunks = (nsteps + UA_CH - 1) / UA_CH;
    uint64_t* wp = ws + pair * ((size_t)ua_chunks(max_cols) * 64);
    const bool valid = lane < m, first = lane == 0, fs = free_start != 0;

    int pu[WP];
#pragma unroll
    for (int c = 0; c < WP; ++c) pu[c] = (valid && c < W) ? q[(size_t)(r0 + lane) * W + c] : 0;

    int xr[WP];
    auto fetch = [&](int chunk) {                          // lanes 0 .. 31: column chunk * 32 + lane of the window
        const int j = chunk * UA_CH + lane;
#pragma unroll
        for (int c = 0; c < WP; ++c) xr[c] = (lane < UA_CH && j < L && c < W) ? x[(size_t)(a + j) * W + c] : 0;
    };

    // the DP's state: (se, ss) = the cell [i][last column done], at first column -1: (i + 1) W with start 0; (de, ds) = the cell
    // [i-1][that column], the next diagonal: i W with start 0 (row 0: the corner of row -1, 0 in both modes)
    int se = (lane + 1) * W, ss = 0, de = lane * W, ds = 0;
    fetch(0);
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        if (lane < UA_CH) ust_ring_store<WP>(ring, chunk * UA_CH + lane, xr);
        __syncthreads();                                   // one wave: its LDS accesses stay in order, the barrier makes the writes visible
        fetch(chunk + 1);
        uint64_t codes = 0;
        const int st0 = chunk * UA_CH, ns = nsteps - st0 < UA_CH ? nsteps - st0 : UA_CH;
        for (int s = 0; s < ns; ++s) {
            int ue = __shfl_up(se, 1), us = __shfl_up(ss, 1);      // the cell [i-1][j] where this lane works on column j
            const int j = st0 + s - lane;
            if (valid && (unsigned)j < (unsigned)L) {
                int t[WP];
                ust_ring_load<WP>(ring, j, t);
                const int sub = ust_mismatches<WP>(pu, t);
                if (first) { ue = fs ? 0 : (j + 1) * W; us = fs ? j + 1 : 0; }      // row -1
                int best = de + sub, bs = ds;
                unsigned code = UA_DIAG;
                if (ue + W < best) { best = ue + W; bs = us; code = UA_UP; }
                if (se + W < best) { best = se + W; bs = ss; code = UA_LEFT; }
                de = ue; ds = us; se = best; ss = bs;
                codes |= (uint64_t)code << (2 * s);
            }
        }
        wp[(size_t)chunk * 64 + lane] = codes;
    }
    const int E = __shfl(se, m - 1);                       // E[m-1][L-1]
    const int ts = __shfl(ss, m - 1);                      // and the start column its path was tracked to
    __threadfence_block();
    __syncthreads();                                       // every lane's words are written and visible to lane 0
    if (lane == 0) {
        int i = m - 1, j = L - 1, eq = 0, sb = 0, del = 0, ins = 0;
        int hc = -1, hi = -1;                              // the chunk and the row of the word held
        uint64_t word = 0;
        // every step takes i or j down and the walk ends at row -1 or column -1, so it sees at most L + m - 1 cells whatever the
        // codes are; the bound only says so again
        for (int guard = L + m; i >= 0 && j >= 0 && guard > 0; --guard) {
            const int st = i + j, ch = st / UA_CH;
            if (ch != hc || i != hi) { word = wp[(size_t)ch * 64 + i]; hc = ch; hi = i; }
            const unsigned code = (unsigned)(word >> (2 * (st % UA_CH))) & 3u;
            if (code == UA_LEFT) { ++ins; --j; }
            else if (code == UA_UP) { ocol[i] = -1; osub[i] = W; ++del; --i; }
            else {
                int sub = 0;
                for (int c = 0; c < W; ++c) sub += q[(size_t)(r0 + i) * W + c] != x[(size_t)(a + j) * W + c] ? 1 : 0;
                ocol[i] = a + j; osub[i] = sub;
                if (sub) ++sb; else ++eq;
                --i; --j;
            }
        }
        for (; i >= 0; --i) { ocol[i] = -1; osub[i] = W; ++del; }      // column -1: units 0 .. i are deletions
        if (!fs && j >= 0) ins += j + 1;                   // global: along row -1 to the corner, leading insertions
        oops[0] = eq; oops[1] = sb; oops[2] = del; oops[3] = ins;
    }
    __syncthreads();
    for (int i = lane; i < Mx; i += 64) {
        cols[pair * Mx + i] = i < m ? ocol[i] : -1;
        subs[pair * Mx + i] = i < m ? osub[i] : -1;
    }
    if (lane < 4) ops[pair * 4 + lane] = oops[lane];
    if (lane == 0) { cost[pair] = E; if (tstart) tstart[pair] = fs ? a + ts : a; }
}

extern "C" int64_t sylber_unit_align_workspace_bytes(int32_t n_pairs, int32_t max_cols) {
    if (n_pairs < 1 || max_cols < 1 || max_cols > UA_MAX_COLS) return -1;
    return (int64_t)n_pairs * ua_chunks(max_cols) * 64 * 8;
}

extern "C" int sylber_unit_align(const int32_t* phrase_units_dev, int32_t R, int32_t W, const int32_t* phrase_row_dev,
                                 const int32_t* phrase_len_dev, int32_t n_phrases, const int32_t* units_dev, int32_t N,
                                 const int32_t* pair_phrase_dev, const int32_t* pair_window_dev, int32_t n_pairs, int32_t max_cols,
                                 int32_t max_rows, int32_t free_start, int32_t* cols_dev, int32_t* subs_dev, int32_t* ops_dev,
                                 int32_t* cost_dev, int32_t* start_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_unit_align";
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first device call
    if (!phrase_units_dev || !phrase_row_dev || !phrase_len_dev || !units_dev || !pair_phrase_dev || !pair_window_dev || !cols_dev ||
        !subs_dev || !ops_dev || !cost_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (W < 1 || W > UA_MAX_W) { syl_set_error(what, "need 1 <= W <= 8"); return 1; }
    if (R < 1 || N < 1 || n_phrases < 1 || n_pairs < 1) { syl_set_error(what, "need R, N, n_phrases, n_pairs >= 1"); return 1; }
    if (max_cols < 1 || max_cols > UA_MAX_COLS) { syl_set_error(what, "need 1 <= max_cols <= 65536: a window has at most 65536 rows"); return 1; }
    if (max_rows < 1 || max_rows > UA_MAX_M) { syl_set_error(what, "need 1 <= max_rows <= 64"); return 1; }
    if (free_start != 0 && free_start != 1) { syl_set_error(what, "free_start is 0 or 1"); return 1; }
    const int wp = W == 1 ? 1 : W == 2 ? 2 : W <= 4 ? 4 : 8;
#define UA_LAUNCH(WPV)                                                                                                                        \
    hipLaunchKernelGGL(unit_align_kernel<WPV>, dim3((unsigned)n_pairs), dim3(64), 0, s, phrase_units_dev, R, W, phrase_row_dev, phrase_len_dev, \
                       n_phrases, units_dev, N, pair_phrase_dev, (const int2*)pair_window_dev, max_cols, max_rows, free_start, cols_dev,        \
                       subs_dev, ops_dev, cost_dev, start_dev, (uint64_t*)workspace_dev)
    switch (wp) {
    case 1: UA_LAUNCH(1); break;
    case 2: UA_LAUNCH(2); break;
    case 4: UA_LAUNCH(4); break;
    default: UA_LAUNCH(8); break;
    }
#undef UA_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
}

// Embedding strings, one pair split across the chip (sylber_amd/search.py: align_sequences(split=...); contract in
// include/sylber_hip.h "Embedding strings", sylber_dtw_strings_align_split; the blocked recurrence restated in
// tests/dtw_strings_split_ref.py).  dtw_strings.hip runs one pair in one workgroup, which leaves 255 CUs idle when a call brings
// one long pair.  Here the matrix of a pair is cut into blocks of BR rows of x by BC columns of y, both multiples of 128, and the
// blocks of one anti-diagonal run side by side, one workgroup each:
//   * dtw_strings_split_kernel<PATH>, launch d: grid (pairs, the longest diagonal of the call); workgroup (pair, k) takes block
//     (b, c) = (max(0, d - nbc + 1) + k, d - b) of its pair and returns at once when its pair has no such block.  Inside the block
//     it is dtw_strings_kernel's loop, the same code (dtw_strings_walk.h: ds_walk_range): the 128 x 128 contraction with kn_stage /
//     kn_mma in the same k-pair order, dt_cost_tile, the two-wave wavefront with the same compare order, on the pair's global
//     128 / 64 grid of tiles and strips.  A cell makes the operations it makes there in the same order, so every d, every (A, n)
//     and every code word has the bits it has there.
//     Ordering between blocks comes from stream order between launches ONLY: block (b, c) reads what blocks (b-1, c) and (b, c-1)
//     wrote in launch d - 1, and the host enqueues the launches d = 0 .. nbr + nbc - 2 on one stream.  No flag, no atomic, no
//     wait on another workgroup: every loop is bounded by lengths that the host wrote down and every barrier is reached by all 256
//     threads with workgroup-uniform trip counts, so nothing waits and nothing can spin.
//   * Hand-over state, in the pair's slice of the workspace (ds_split_layout below), cells of (A, n), 8 B each:
//     - boundary rows, 2 x L: band b (the blocks (b, *)) writes its last row to row b & 1, columns of its own chunk, when x goes
//       on below; block (b+1, c) reads it in launch d + 1, and the next writer of that parity and chunk, (b+2, c), runs in d + 2.
//     - inner rows, 2 x L, when BR > 128: the rows between a block's own super-strips, alternating by the super-strip's parity as
//       in the one-workgroup kernel.  A block touches only the columns of its chunk c, and the blocks of one launch have
//       different c (b + c = d), so no other block of the launch touches them; behind the same fence and barrier as there.
//     - boundary columns, 2 x (m + nbr): chunk c writes each row's last cell to column c & 1 when y goes on to the right; band b's
//       cells lie at [b (BR + 1) + 1 ..], one per row.  Block (b, c+1) reads them in launch d + 1, the next writer of that parity
//       and band, (b, c+2), runs in d + 2.  A lane takes its cell as its last cell (a_cur / n_cur) at the block's first tile;
//       lane 0 of a strip takes the cell of the row above as (pa, pn).
//     - THE CORNER A[i0-1][c0-1] of block (b, c) is the last cell of boundary row b - 1 in chunk c - 1, written in launch d - 2.
//       It cannot be read from there: block (b+1, c-1) rewrites that parity and chunk in launch d, the launch that would read it.
//       So the corner travels with the column: the block to the left, (b, c-1), has read A[i0-1][c0-1] itself -- it is the last
//       cell of ITS upper row, lane 0's (pa, pn) after its last tile -- and stores it as the one extra leading cell of its column,
//       [b (BR + 1)].  That cell is written in launch d - 1 by the only block of that launch in band b, read in launch d by
//       block (b, c), and next written in launch d + 1 by (b, c+1): stream order separates all three.  In band 0 it is the +inf
//       cell above the matrix, written like any other.
//     - the last cell (A, n) of the pair, 8 B, from the block that holds (m-1, L-1) to the finishing launch.
//     Only cells that an earlier launch (or, for the inner rows, the same workgroup) wrote are read: nothing depends on what the
//     workspace held.
//   * PATH: the 2-bit codes go where dtw_strings_kernel puts them, [strip][tile][4][64] words by global index.
//   * dtw_strings_finish_kernel<PATH>: one workgroup per pair after the last diagonal, dtw_strings_kernel's end (ds_padding /
//     ds_finish): padding for an empty side or a cost not below +inf, else cost, steps and thread 0's walk back over the codes.
//   Plain vector loads and stores only.
// LDS: dtw_strings_kernel's 70 160 B.
#include "dtw_strings_walk.h"
#include <vector>

constexpr int DSS_BLOCK_ROWS = 128, DSS_BLOCK_COLS = 128;      // the library's choice: profiles/dtw_strings_split_bench.md

// Where a pair's hand-over state lies, as byte offsets from the start of its slice; every piece starts at a multiple of 256
struct DsSplitLayout { int64_t fin, brow, inner, bcol, total; int nbr, nbc; };
__host__ __device__ static inline int64_t dss_al(int64_t bytes) { return (bytes + 255) / 256 * 256; }
__host__ __device__ static inline DsSplitLayout ds_split_layout(int64_t m, int64_t L, int64_t BR, int64_t BC) {
    DsSplitLayout o = {0, 0, 0, 0, 0, 0, 0};
    if (m <= 0 || L <= 0) return o;                        // an empty side has no state
    o.nbr = (int)((m + BR - 1) / BR); o.nbc = (int)((L + BC - 1) / BC);
    int64_t at = 256;                                      // fin
    o.brow = at; at += o.nbr > 1 ? dss_al(2 * 8 * L) : 0;
    o.inner = at; at += BR > KN_BM && m > KN_BM ? dss_al(2 * 8 * L) : 0;
    o.bcol = at; at += o.nbc > 1 ? dss_al(2 * 8 * (m + o.nbr)) : 0;
    o.total = at;
    return o;
}

// Launch d, workgroup (pair, k); tab, ws as dtw_strings_kernel takes them, tab[4]: the pair's hand-over state
template <bool PATH>
__global__ __launch_bounds__(256) void dtw_strings_split_kernel(const float* __restrict__ x, int x_rows, const float* __restrict__ xn,
                                                                const float* __restrict__ y, int y_rows, const float* __restrict__ cn, int D,
                                                                const int64_t* __restrict__ tab, char* ws, int d, int BR, int BC) {
    extern __shared__ __attribute__((aligned(16))) float ds_smem[];
    const DsLds S(ds_smem);
    const size_t pair = blockIdx.x;
    const int64_t* t_ = tab + pair * DS_TAB;               // workgroup-uniform, as all that follows from it
    const DsPair P(t_, x_rows, y_rows);
    if (P.m == 0 || P.L == 0) return;                      // the finishing launch writes its padding
    const DsSplitLayout lay = ds_split_layout(P.m, P.L, BR, BC);
    const int b = (d - (lay.nbc - 1) > 0 ? d - (lay.nbc - 1) : 0) + (int)blockIdx.y, c = d - b;
    if (b >= lay.nbr || c < 0) return;                     // the pair has no such block on this diagonal
    char* st = ws + t_[4];
    int2* brow = (int2*)(st + lay.brow);
    int2* bcol = (int2*)(st + lay.bcol);
    const int RS = BR / KN_BM, CT = BC / KN_BN;            // super-strips and tiles of a block
    const int SS = (P.m + KN_BM - 1) / KN_BM, tiles = (P.L + KN_BN - 1) / KN_BN;
    const size_t colrow = (size_t)P.m + lay.nbr, band = (size_t)b * (BR + 1);
    DsEdges e;
    e.ss_lo = b * RS; e.ss_hi = (b + 1) * RS < SS ? (b + 1) * RS : SS;
    e.tile_lo = c * CT; e.tile_hi = (c + 1) * CT < tiles ? (c + 1) * CT : tiles;
    e.inner = (int2*)(st + lay.inner);                     // used only between the super-strips of a block: RS > 1
    e.top = b > 0 ? brow + (size_t)((b + 1) & 1) * P.L : nullptr;
    e.bottom = b + 1 < lay.nbr ? brow + (size_t)(b & 1) * P.L : nullptr;
    e.left = c > 0 ? bcol + (size_t)((c + 1) & 1) * colrow + band : nullptr;
    e.right = c + 1 < lay.nbc ? bcol + (size_t)(c & 1) * colrow + band : nullptr;
    ds_walk_range<PATH, true>(S, x, xn, y, cn, D, P, e, (uint64_t*)(ws + t_[5]));
    if (b + 1 == lay.nbr && c + 1 == lay.nbc && threadIdx.x == 0) *(int2*)st = make_int2(S.fin[0], S.fin[1]);
}

// After the last diagonal, workgroup `pair`: the outputs
template <bool PATH>
__global__ __launch_bounds__(256) void dtw_strings_finish_kernel(int x_rows, int y_rows, const int64_t* __restrict__ tab, int2* __restrict__ rows,
                                                                 int32_t* __restrict__ steps, float* __restrict__ cost,
                                                                 int32_t* __restrict__ steps_walk, const char* ws) {
    const size_t pair = blockIdx.x;
    const int64_t* t_ = tab + pair * DS_TAB;
    const DsPair P(t_, x_rows, y_rows);
    if (P.m == 0 || P.L == 0) { ds_padding<PATH>(P, pair, rows, steps, cost, steps_walk); return; }
    const int2 fin = *(const int2*)(ws + t_[4]);
    ds_finish<PATH>(P, pair, __int_as_float(fin.x), fin.y, (const uint64_t*)(ws + t_[5]), rows, steps, cost, steps_walk);
}

// block sizes as the caller gave them -> the sizes used, or false
static bool dss_blocks(int32_t block_rows, int32_t block_cols, int& BR, int& BC) {
    if (block_rows < 0 || block_cols < 0 || block_rows % KN_BM || block_cols % KN_BN || block_rows > DS_MAX_LEN || block_cols > DS_MAX_LEN) return false;
    BR = block_rows ? block_rows : DSS_BLOCK_ROWS; BC = block_cols ? block_cols : DSS_BLOCK_COLS;
    return true;
}

extern "C" int64_t sylber_dtw_strings_split_workspace_bytes(const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs, int32_t path,
                                                            int32_t block_rows, int32_t block_cols) {
    int BR, BC;
    if (ds_check(x_win_host, y_win_host, n_pairs, path) || !dss_blocks(block_rows, block_cols, BR, BC)) return -1;
    int64_t bytes = ds_table_bytes(n_pairs);               // the pairs' table | per pair: its hand-over state, its codes
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t m = x_win_host[2 * p + 1], L = y_win_host[2 * p + 1];
        bytes += ds_split_layout(m, L, BR, BC).total + (path ? ds_codes_bytes(m, L) : 0);
    }
    return bytes;
}

static int dss_run(const float* x_dev, int32_t x_rows, const float* x_norm_dev, const float* y_dev, int32_t y_rows, const float* y_norm_dev,
                   int32_t D, int32_t metric, const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs, int32_t path,
                   const int64_t* rows_offset_host, int32_t* rows_dev, int32_t* steps_dev, float* cost_dev, int32_t* steps_walk_dev,
                   int32_t block_rows, int32_t block_cols, void* workspace_dev, void* stream) {
    static const char* what = "sylber_dtw_strings_align_split";
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first device call
    if (const char* bad = ds_check_call(x_dev, x_rows, x_norm_dev, y_dev, y_rows, y_norm_dev, D, metric, x_win_host, y_win_host, n_pairs, path,
                                        rows_offset_host, rows_dev, steps_dev, cost_dev, workspace_dev)) { syl_set_error(what, bad); return 1; }
    int BR, BC;
    if (!dss_blocks(block_rows, block_cols, BR, BC)) { syl_set_error(what, "block_rows and block_cols are multiples of 128, at most 65536, or 0"); return 1; }
    // where each pair's slice lies and how many diagonals and blocks per diagonal the call has: host arithmetic on the lengths
    std::vector<int64_t> tab((size_t)n_pairs * DS_TAB);
    int64_t at = ds_table_bytes(n_pairs);
    int diagonals = 0, widest = 1;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t m = x_win_host[2 * p + 1], L = y_win_host[2 * p + 1];
        const DsSplitLayout lay = ds_split_layout(m, L, BR, BC);
        int64_t* e = tab.data() + (size_t)p * DS_TAB;
        e[0] = x_win_host[2 * p]; e[1] = m; e[2] = y_win_host[2 * p]; e[3] = L;
        e[4] = at; at += lay.total;
        e[5] = at; at += path ? ds_codes_bytes(m, L) : 0;
        e[6] = path ? rows_offset_host[p] : 0; e[7] = 0;
        if (lay.nbr > 0) {
            diagonals = lay.nbr + lay.nbc - 1 > diagonals ? lay.nbr + lay.nbc - 1 : diagonals;
            const int w = lay.nbr < lay.nbc ? lay.nbr : lay.nbc;
            widest = w > widest ? w : widest;
        }
    }
    // the table is pageable host memory: the copy is staged before the call returns, in stream order on the device
    HIP_TRY(hipMemcpyAsync(workspace_dev, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
    const bool l2 = metric == SYLBER_KNN_L2;
    static PerDeviceOnce once[2];
    if (once[path].need())
        HIP_TRY(hipFuncSetAttribute(path ? (const void*)dtw_strings_split_kernel<true> : (const void*)dtw_strings_split_kernel<false>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)DS_LDS_BYTES));
    // one launch per anti-diagonal of blocks, all pairs of the call in each; stream order is the only order between blocks
    for (int d = 0; d < diagonals; ++d) {
        // the blocks of diagonal d of any pair: at most min(d + 1, widest, diagonals - d)
        int k = d + 1 < widest ? d + 1 : widest;
        k = diagonals - d < k ? diagonals - d : k;
        const dim3 grid((unsigned)n_pairs, (unsigned)k);
#define DSS_LAUNCH(PV)                                                                                                                      \
    hipLaunchKernelGGL((dtw_strings_split_kernel<PV>), grid, dim3(256), DS_LDS_BYTES, s, x_dev, x_rows, l2 ? x_norm_dev : nullptr, y_dev, y_rows, \
                       l2 ? y_norm_dev : nullptr, D, (const int64_t*)workspace_dev, (char*)workspace_dev, d, BR, BC)
        if (path) DSS_LAUNCH(true);
        else DSS_LAUNCH(false);
#undef DSS_LAUNCH
    }
    if (path)
        hipLaunchKernelGGL((dtw_strings_finish_kernel<true>), dim3((unsigned)n_pairs), dim3(256), 0, s, x_rows, y_rows, (const int64_t*)workspace_dev,
                           (int2*)rows_dev, steps_dev, cost_dev, steps_walk_dev, (const char*)workspace_dev);
    else
        hipLaunchKernelGGL((dtw_strings_finish_kernel<false>), dim3((unsigned)n_pairs), dim3(256), 0, s, x_rows, y_rows, (const int64_t*)workspace_dev,
                           (int2*)rows_dev, steps_dev, cost_dev, steps_walk_dev, (const char*)workspace_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_dtw_strings_align_split(const float* x_dev, int32_t x_rows, const float* x_norm_dev, const float* y_dev, int32_t y_rows,
                                              const float* y_norm_dev, int32_t D, int32_t metric, const int32_t* x_win_host,
                                              const int32_t* y_win_host, int32_t n_pairs, int32_t path, const int64_t* rows_offset_host,
                                              int32_t* rows_dev, int32_t* steps_dev, float* cost_dev, int32_t* steps_walk_dev,
                                              int32_t block_rows, int32_t block_cols, void* workspace_dev, void* stream) {
    try {
        return dss_run(x_dev, x_rows, x_norm_dev, y_dev, y_rows, y_norm_dev, D, metric, x_win_host, y_win_host, n_pairs, path, rows_offset_host,
                       rows_dev, steps_dev, cost_dev, steps_walk_dev, block_rows, block_cols, workspace_dev, stream);
    } catch (...) { syl_set_error("sylber_dtw_strings_align_split", "out of host memory"); return 1; }
}

// Embedding strings (sylber_amd/search.py: align_sequences / SyllableIndex.align_sequences; contract in include/sylber_hip.h
// "Embedding strings", restated in tests/dtw_strings_ref.py): the GLOBAL DTW of two WHOLE embedding sequences of up to 65 536 rows
// on each side, many pairs per call -- cost, the cells on the path and optionally the run of y rows that every x row is warped
// onto.  unit_strings.hip's sibling on embeddings, and dtw.hip's without the 64-row limit of a phrase: there one wave holds a whole
// phrase, here x is cut into strips of 64 rows that waves 0 and 1 take in turn.
// The walk described here lives in dtw_strings_walk.h (ds_walk_range), shared with dtw_strings_split.hip, which cuts ONE pair into
// blocks for many workgroups; this file runs it over the whole pair.
//   * dtw_strings_kernel<PATH>: one workgroup of 256 threads per pair; nothing is handed between workgroups, every loop is bounded
//     by lengths that the host wrote down and every barrier is reached by all 256 threads with workgroup-uniform trip counts, so
//     nothing waits and nothing can spin.  x is taken in super-strips of 128 rows (KN_BM), y in tiles of 128 columns (KN_BN).
//     The contraction: all four waves contract one 128 x 128 tile over D with dtw_scan_body's staging and K loop (kn_stage / kn_mma
//     of knn_tile.h: x in the role of the phrase, y in the role of the database, the same k-pair order), so every local cost has
//     the bits of sylber_dtw_search's, i.e. of the ascending fmaf chain (dtw_pair.h states that equivalence).  A 32-row half
//     without a live x row skips its MFMAs: a pair with m <= 64 does half the matrix work.  dt_cost_tile turns the accumulators
//     into d in the LDS cost tile, which aliases the staging behind a barrier.
//     The DP: wave 0 owns rows 0 .. 63 of the super-strip and wave 1 rows 64 .. 127; both run dtw_tile.h's anti-diagonal wavefront
//     (lane l works on column t - l at step t, the lane above arrives through DPP wave_shr:1) on cells of (A, n), n = the cells on
//     the path so far, which is why the counts need no path.  A lane keeps its last two cells for the next tile, so the wavefront
//     drains at every tile edge.  Lane 0 of a strip takes its upper row from LDS: wave 0's is the +inf row above the matrix or the
//     row that the super-strip before left in the workspace, copied in a tile at a time; wave 1's is what wave 0's lane 63 left
//     there, 128 x 8 B per tile, and wave 1 walks a tile's lower strip after wave 0 has finished the upper one, a barrier
//     between.  (Running wave 1 one tile behind wave 0 needs a second half cost tile; profiles/dtw_strings_bench.md has what
//     the DP phase costs.)
//     Between super-strips: lane 63 of wave 1 writes its (A, n) row, 8 B per column, to one of TWO rows of the pair's slice of the
//     workspace, super-strips alternating, and the next super-strip reads the other.  A fence and a barrier stand between
//     super-strips; a pair stays inside one workgroup, whose waves share one vector L1, so workgroup scope is enough
//     (unit_strings.hip's header has the argument).  Only columns below L are read, and the super-strip before wrote every one of
//     them: nothing depends on what the workspace held.
//     PATH: each lane also packs the 2-bit predecessor code of its cells, taken from the comparisons the cell makes in the cell's
//     order; a lane's 128 cells of one tile are four 64-bit words and the wave stores them as four coalesced rows:
//     [strip of 64 rows][tile][4][64] words; cell (i, j) is bits 2 (j % 32) .. + 1 of word [i / 64][j / 128][(j / 32) % 4][i % 64].
//     After the last super-strip, a fence and a barrier, thread 0 follows the codes from (m-1, L-1) to (0, 0) -- at most m + L - 1
//     cells -- and writes the runs; it counts its own cells and hands the count out where the caller asks for it: tests hold it
//     against the carried n, i.e. the codes against the cells that formed them.
//     Plain vector loads and stores only.
// LDS: 67 584 B of cost tile (aliasing 20 480 B of staging) + 512 B of c_j + 2 x 1 024 B of upper rows + 16 B = 70 160 B, which is
// DT_FIXED's order: two workgroups fit a CU, one contracts while the other walks.
#include "dtw_strings_walk.h"
#include <vector>

static inline int64_t ds_rows_bytes(int64_t m, int64_t L) { return m > KN_BM && L > 0 ? kn_al(2 * 8 * L) : 0; }

// Workgroup `pair`: rows tab[0] .. + tab[1] of x [*, D] against rows tab[2] .. + tab[3] of y [*, D]; xn / cn: their ||row||^2 (L2)
// or null; tab[4], tab[5]: where in ws its two rows and its codes lie; tab[6]: x's flat row in rows.  Writes cost, steps [pairs] and,
// PATH, rows [*, 2] and steps_walk where it is not null.  The walk itself is dtw_strings_walk.h's, over the whole pair.
template <bool PATH>
__global__ __launch_bounds__(256) void dtw_strings_kernel(const float* __restrict__ x, int x_rows, const float* __restrict__ xn,
                                                          const float* __restrict__ y, int y_rows, const float* __restrict__ cn, int D,
                                                          const int64_t* __restrict__ tab,
                                                          int2* __restrict__ rows, int32_t* __restrict__ steps, float* __restrict__ cost,
                                                          int32_t* __restrict__ steps_walk, char* ws) {
    extern __shared__ __attribute__((aligned(16))) float ds_smem[];
    const DsLds S(ds_smem);
    const size_t pair = blockIdx.x;
    const int64_t* t_ = tab + pair * DS_TAB;               // workgroup-uniform, as all that follows from it
    const DsPair P(t_, x_rows, y_rows);
    if (P.m == 0 || P.L == 0) { ds_padding<PATH>(P, pair, rows, steps, cost, steps_walk); return; }
    uint64_t* codes = (uint64_t*)(ws + t_[5]);
    const DsEdges e = {0, (P.m + KN_BM - 1) / KN_BM, 0, (P.L + KN_BN - 1) / KN_BN, (int2*)(ws + t_[4]), nullptr, nullptr, nullptr, nullptr};
    ds_walk_range<PATH, false>(S, x, xn, y, cn, D, P, e, codes);
    ds_finish<PATH>(P, pair, __int_as_float(S.fin[0]), S.fin[1], codes, rows, steps, cost, steps_walk);
}

extern "C" int64_t sylber_dtw_strings_workspace_bytes(const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs, int32_t path) {
    if (ds_check(x_win_host, y_win_host, n_pairs, path)) return -1;
    int64_t bytes = ds_table_bytes(n_pairs);               // the pairs' table | per pair: its two rows, its codes
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t m = x_win_host[2 * p + 1], L = y_win_host[2 * p + 1];
        bytes += ds_rows_bytes(m, L) + (path ? ds_codes_bytes(m, L) : 0);
    }
    return bytes;
}

static int ds_run(const float* x_dev, int32_t x_rows, const float* x_norm_dev, const float* y_dev, int32_t y_rows, const float* y_norm_dev,
                  int32_t D, int32_t metric, const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs, int32_t path,
                  const int64_t* rows_offset_host, int32_t* rows_dev, int32_t* steps_dev, float* cost_dev, int32_t* steps_walk_dev,
                  void* workspace_dev, void* stream) {
    static const char* what = "sylber_dtw_strings_align";
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first device call
    if (const char* bad = ds_check_call(x_dev, x_rows, x_norm_dev, y_dev, y_rows, y_norm_dev, D, metric, x_win_host, y_win_host, n_pairs, path,
                                        rows_offset_host, rows_dev, steps_dev, cost_dev, workspace_dev)) { syl_set_error(what, bad); return 1; }
    // where each pair's slice lies: host arithmetic on the lengths
    std::vector<int64_t> tab((size_t)n_pairs * DS_TAB);
    int64_t at = ds_table_bytes(n_pairs);
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t m = x_win_host[2 * p + 1], L = y_win_host[2 * p + 1];
        int64_t* e = tab.data() + (size_t)p * DS_TAB;
        e[0] = x_win_host[2 * p]; e[1] = m; e[2] = y_win_host[2 * p]; e[3] = L;
        e[4] = at; at += ds_rows_bytes(m, L);
        e[5] = at; at += path ? ds_codes_bytes(m, L) : 0;
        e[6] = path ? rows_offset_host[p] : 0; e[7] = 0;
    }
    // the table is pageable host memory: the copy is staged before the call returns, in stream order on the device
    HIP_TRY(hipMemcpyAsync(workspace_dev, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
    const bool l2 = metric == SYLBER_KNN_L2;
    static PerDeviceOnce once[2];
    if (once[path].need())
        HIP_TRY(hipFuncSetAttribute(path ? (const void*)dtw_strings_kernel<true> : (const void*)dtw_strings_kernel<false>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)DS_LDS_BYTES));
#define DS_LAUNCH(PV)                                                                                                                       \
    hipLaunchKernelGGL((dtw_strings_kernel<PV>), dim3((unsigned)n_pairs), dim3(256), DS_LDS_BYTES, s, x_dev, x_rows, l2 ? x_norm_dev : nullptr, y_dev, \
                       y_rows, l2 ? y_norm_dev : nullptr, D, (const int64_t*)workspace_dev, (int2*)rows_dev, steps_dev, cost_dev, steps_walk_dev,   \
                       (char*)workspace_dev)
    if (path) DS_LAUNCH(true);
    else DS_LAUNCH(false);
#undef DS_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_dtw_strings_align(const float* x_dev, int32_t x_rows, const float* x_norm_dev, const float* y_dev, int32_t y_rows,
                                        const float* y_norm_dev, int32_t D, int32_t metric, const int32_t* x_win_host,
                                        const int32_t* y_win_host, int32_t n_pairs, int32_t path, const int64_t* rows_offset_host,
                                        int32_t* rows_dev, int32_t* steps_dev, float* cost_dev, int32_t* steps_walk_dev, void* workspace_dev,
                                        void* stream) {
    try {
        return ds_run(x_dev, x_rows, x_norm_dev, y_dev, y_rows, y_norm_dev, D, metric, x_win_host, y_win_host, n_pairs, path, rows_offset_host,
                      rows_dev, steps_dev, cost_dev, steps_walk_dev, workspace_dev, stream);
    } catch (...) { syl_set_error("sylber_dtw_strings_align", "out of host memory"); return 1; }
}

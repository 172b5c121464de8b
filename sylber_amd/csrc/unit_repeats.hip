// Unit repeats (sylber_amd/units.py: local_align_unit_strings / UnitIndex.find_repeats; contract in include/sylber_hip.h "Unit
// repeats", restated in tests/unit_repeats_ref.py): the LOCAL alignment (Smith-Waterman) of two unit strings of any length up to
// 65 536 units on each side, many pairs per call -- the best-scoring pair of sub-spans, i.e. what is said in both recordings, found
// without a query.  unit_strings.hip's sibling on the same strips (unit_strip.h), with a floor at 0 in the recurrence, a cell that
// carries where its path began instead of its counts, and a running best in every lane instead of the last cell (ul_cell there).
//   * unit_local_kernel<WP>: one wave per pair walks the strips, every lane keeping the best cell it has seen; after the last
//     strip a butterfly over the 64 lanes under (H descending, i ascending) picks the pair's cell.
//     No predecessor codes, no traceback.  Plain vector loads and stores only.
// LDS: 4 KiB of ring at WP = 8, 64 threads: wave slots bound the occupancy.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "unit_strip.h"

// Workgroup (one wave) `pair`: rows tab[0] .. + tab[1] of x [*, W] against rows tab[2] .. + tab[3] of y [*, W]; tab[4]: where in ws
// its two rows lie.  sw = match * W, pen = match + mismatch, gw = gap * W: s(i, j) = sw - pen * sub(i, j).  Writes score [pairs] and
// span [pairs][4] = (a0, a1, b0, b1).
template <int WP>
__global__ __launch_bounds__(64) void unit_local_kernel(const int32_t* __restrict__ x, const int32_t* __restrict__ y, int W,
                                                        const int64_t* __restrict__ tab, int sw, int pen, int gw,
                                                        int32_t* __restrict__ score, int32_t* __restrict__ span, char* ws) {
    __shared__ __attribute__((aligned(16))) int ring[UST_RING * WP];      // [column % 128][WP] ids of y's columns
    const int lane = threadIdx.x;
    const size_t pair = blockIdx.x;
    const int64_t* t = tab + pair * UST_TAB;              // workgroup-uniform, as all that follows from it
    const int64_t xo = t[0], yo = t[2];
    const int m = (int)t[1], L = (int)t[3];
    if (m == 0 || L == 0) {                                // no DP step: what the contract says of an empty side
        if (lane == 0) score[pair] = 0;
        if (lane < 4) span[pair * 4 + lane] = -1;
        return;
    }
    int32_t* rows = (int32_t*)(ws + t[4]);
    const int S = (m + UST_ROWS - 1) / UST_ROWS;

    ul_best b;                                             // this lane's best cell
    ul_cell<false> cell{b, sw, pen, gw};
    for (int s = 0; s < S; ++s) ust_strip<WP>(cell, ring, x, y, W, xo, yo, m, L, rows, s, S);
    b.butterfly();                                         // the pair's cell
    if (lane == 0) {
        score[pair] = b.h;
        int32_t* sp = span + pair * 4;
        if (b.h > 0) { sp[0] = b.si; sp[1] = b.i + 1; sp[2] = b.sj; sp[3] = b.j + 1; }
        else { sp[0] = -1; sp[1] = -1; sp[2] = -1; sp[3] = -1; }
    }
}

extern "C" int64_t sylber_unit_local_workspace_bytes(const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs) {
    if (ust_check_lengths(x_win_host, y_win_host, n_pairs)) return -1;
    int64_t bytes = ust_table_bytes(n_pairs, UST_TAB);    // the pairs' table | per pair: its two rows
    for (int32_t p = 0; p < n_pairs; ++p) bytes += ust_rows_bytes(x_win_host[2 * (size_t)p + 1], y_win_host[2 * (size_t)p + 1]);
    return bytes;
}

extern "C" int sylber_unit_local_align(const int32_t* x_units_dev, int32_t x_rows, const int32_t* y_units_dev, int32_t y_rows, int32_t W,
                                       const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs, int32_t match,
                                       int32_t mismatch, int32_t gap, int32_t* score_dev, int32_t* span_dev, void* workspace_dev,
                                       void* stream) {
    static const char* what = "sylber_unit_local_align";
    return ust_entry(what, [&]() -> int {
        hipStream_t s = (hipStream_t)stream;
        // every check comes before the first device call
        if (!x_units_dev || !y_units_dev || !score_dev || !span_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
        if (W < 1 || W > UST_MAX_W) { syl_set_error(what, "need 1 <= W <= 8"); return 1; }
        if (const char* bad = ust_check_lengths(x_win_host, y_win_host, n_pairs)) { syl_set_error(what, bad); return 1; }
        if (const char* bad = ust_check_scoring(match, mismatch, gap)) { syl_set_error(what, bad); return 1; }
        if (const char* bad = ust_check_windows(x_win_host, x_rows, y_win_host, y_rows, nullptr, n_pairs)) { syl_set_error(what, bad); return 1; }
        ust_table tab(n_pairs, UST_TAB);
        for (int32_t p = 0; p < n_pairs; ++p)
            tab.add(p, x_win_host[2 * (size_t)p], x_win_host[2 * (size_t)p + 1], y_win_host[2 * (size_t)p], y_win_host[2 * (size_t)p + 1]);
        // the table is pageable host memory: the copy is staged before the call returns, in stream order on the device
        HIP_TRY(hipMemcpyAsync(workspace_dev, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
        UST_WITH_WP(W, hipLaunchKernelGGL((unit_local_kernel<WPV>), dim3((unsigned)n_pairs), dim3(64), 0, s, x_units_dev, y_units_dev, W,
                                         (const int64_t*)workspace_dev, match * W, match + mismatch, gap * W, score_dev, span_dev,
                                         (char*)workspace_dev));
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

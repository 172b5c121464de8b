// Unit repeats, every one (sylber_amd/units.py: local_align_unit_strings_all / UnitIndex.find_repeats with per_pair or within;
// contract in include/sylber_hip.h "Unit repeats, every one", restated in tests/unit_repeats_all_ref.py): up to n_best repeats of
// a pair of unit strings, and with a band below the diagonal the repeats inside ONE string.  unit_repeats.hip's sibling: the same
// strips and the same cell (unit_strip.h), run n_best times over the pair with the cells of the earlier rounds' rectangles, and
// of the band, held at H = 0.
//   * unit_local_all_kernel<WP>: one 64-thread workgroup (one wave) per pair runs ALL the rounds of its pair; nothing goes through
//     the host between rounds, nothing is read back from the outputs, nothing is handed between workgroups, and every loop is
//     bounded by lengths the host wrote down and by n_best.  After a round's butterfly every lane holds the round's cell; lane 0
//     writes its rectangle (a0, a1, b0, b1) to rect[round] in LDS, 32 x 4 ints, and the next rounds read it from there.
//     Blocked cells.  Round 0 of a pair with sep = 0 has nothing to block, and that is wave-uniform: one branch per round picks
//     the strip body without any blocking in it, which is unit_local_kernel's (a uniform test inside the cell loop cost a long
//     pair 12 to 21 %, profiles/unit_repeats_all_bench.md).  Otherwise a lane derives, once per strip, a 32-bit mask of the
//     rectangles whose rows contain its row i; a cell tests column ranges only when that mask is non-zero, one rectangle per set
//     bit, and the band is one compare, j - i < sep.  A blocked cell gets H = 0: it never beats a lane's best (replaced on a
//     strictly larger H only), its start is a don't-care as for every H = 0, and in the strip's last row it still writes H = 0
//     to the carried row, so the next strip reads this round's row, never an earlier round's or stale workspace.
//     A round whose score is below min_score ends the pair: it and the later rounds get score 0 and spans -1.
//     No predecessor codes, no traceback.  Plain vector loads and stores only.
// LDS: 4 KiB of ring at WP = 8 and 512 B of rectangles, 64 threads: wave slots bound the occupancy.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "unit_strip.h"

constexpr int ULA_TAB = UST_TAB + 1;                      // int64 per pair: UST_TAB, sep
constexpr int ULA_MAX_BEST = 32;                          // rounds of a pair: one bit each in a lane's mask

// Workgroup (one wave) `pair`: rows tab[0] .. + tab[1] of x [*, W] against rows tab[2] .. + tab[3] of y [*, W]; tab[4]: where in ws
// its two rows lie; tab[5]: its sep.  sw = match * W, pen = match + mismatch, gw = gap * W: s(i, j) = sw - pen * sub(i, j).  Writes
// score [pairs][R] and span [pairs][R][4] = (a0, a1, b0, b1).
template <int WP>
__global__ __launch_bounds__(64) void unit_local_all_kernel(const int32_t* __restrict__ x, const int32_t* __restrict__ y, int W,
                                                            const int64_t* __restrict__ tab, int sw, int pen, int gw, int R, int floor,
                                                            int32_t* __restrict__ score, int32_t* __restrict__ span, char* ws) {
    __shared__ __attribute__((aligned(16))) int ring[UST_RING * WP];      // [column % 128][WP] ids of y's columns
    __shared__ __attribute__((aligned(16))) int rect[ULA_MAX_BEST * 4];  // [round] (a0, a1, b0, b1) of the rounds done
    const int lane = threadIdx.x;
    const size_t pair = blockIdx.x;
    const int64_t* t = tab + pair * ULA_TAB;               // workgroup-uniform, as all that follows from it
    const int64_t xo = t[0], yo = t[2];
    const int m = (int)t[1], L = (int)t[3], sep = (int)t[5];
    int32_t* rows = (int32_t*)(ws + t[4]);
    int32_t* sc = score + pair * R;
    int32_t* sp = span + pair * R * 4;
    const int S = (m + UST_ROWS - 1) / UST_ROWS;

    int r = 0;
    for (; r < R && m > 0 && L > 0; ++r) {                 // an empty side: no DP step, every round is padding
        ul_best b;                                         // this lane's best cell of the round
        if (r > 0 || sep > 0) {                            // wave-uniform: round 0 without a band has no blocked cell
            ul_cell<true> cell{b, sw, pen, gw, sep, rect, r};
            for (int s = 0; s < S; ++s) { cell.strip(s); ust_strip<WP>(cell, ring, x, y, W, xo, yo, m, L, rows, s, S); }
        } else {
            ul_cell<false> cell{b, sw, pen, gw};
            for (int s = 0; s < S; ++s) ust_strip<WP>(cell, ring, x, y, W, xo, yo, m, L, rows, s, S);
        }
        b.butterfly();                                     // the round's cell, in every lane
        if (b.h < floor) break;                            // uniform: this round and the later ones are padding
        if (lane == 0) {
            sc[r] = b.h;
            sp[4 * r] = b.si; sp[4 * r + 1] = b.i + 1; sp[4 * r + 2] = b.sj; sp[4 * r + 3] = b.j + 1;
            rect[4 * r] = b.si; rect[4 * r + 1] = b.i + 1; rect[4 * r + 2] = b.sj; rect[4 * r + 3] = b.j + 1;
        }
        __syncthreads();                                   // the rectangle is visible to the wave before the next round reads it
    }
    for (int q = r * 5 + lane; q < R * 5; q += UST_ROWS) {  // the rounds not run: score 0, spans -1
        const int e = q / 5, c = q - e * 5;
        if (c == 0) sc[e] = 0;
        else sp[4 * e + c - 1] = -1;
    }
}

extern "C" int64_t sylber_unit_local_all_workspace_bytes(const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs) {
    if (ust_check_lengths(x_win_host, y_win_host, n_pairs)) return -1;
    int64_t bytes = ust_table_bytes(n_pairs, ULA_TAB);    // the pairs' table | per pair: its two rows
    for (int32_t p = 0; p < n_pairs; ++p) bytes += ust_rows_bytes(x_win_host[2 * (size_t)p + 1], y_win_host[2 * (size_t)p + 1]);
    return bytes;
}

extern "C" int sylber_unit_local_align_all(const int32_t* x_units_dev, int32_t x_rows, const int32_t* y_units_dev, int32_t y_rows,
                                           int32_t W, const int32_t* x_win_host, const int32_t* y_win_host, const int32_t* sep_host,
                                           int32_t n_pairs, int32_t match, int32_t mismatch, int32_t gap, int32_t n_best,
                                           int32_t min_score, int32_t* score_dev, int32_t* span_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_unit_local_align_all";
    return ust_entry(what, [&]() -> int {
        hipStream_t s = (hipStream_t)stream;
        // every check comes before the first device call
        if (!x_units_dev || !y_units_dev || !score_dev || !span_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
        if (W < 1 || W > UST_MAX_W) { syl_set_error(what, "need 1 <= W <= 8"); return 1; }
        if (const char* bad = ust_check_lengths(x_win_host, y_win_host, n_pairs)) { syl_set_error(what, bad); return 1; }
        if (const char* bad = ust_check_scoring(match, mismatch, gap)) { syl_set_error(what, bad); return 1; }
        if (n_best < 1 || n_best > ULA_MAX_BEST) { syl_set_error(what, "need 1 <= n_best <= 32"); return 1; }
        if (min_score < 1) { syl_set_error(what, "need min_score >= 1"); return 1; }
        if (const char* bad = ust_check_windows(x_win_host, x_rows, y_win_host, y_rows, sep_host, n_pairs)) { syl_set_error(what, bad); return 1; }
        ust_table tab(n_pairs, ULA_TAB);
        for (int32_t p = 0; p < n_pairs; ++p)
            tab.add(p, x_win_host[2 * (size_t)p], x_win_host[2 * (size_t)p + 1], y_win_host[2 * (size_t)p], y_win_host[2 * (size_t)p + 1])[5] =
                sep_host ? sep_host[p] : 0;
        // the table is pageable host memory: the copy is staged before the call returns, in stream order on the device
        HIP_TRY(hipMemcpyAsync(workspace_dev, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
        UST_WITH_WP(W, hipLaunchKernelGGL((unit_local_all_kernel<WPV>), dim3((unsigned)n_pairs), dim3(64), 0, s, x_units_dev, y_units_dev, W,
                                         (const int64_t*)workspace_dev, match * W, match + mismatch, gap * W, n_best, min_score, score_dev,
                                         span_dev, (char*)workspace_dev));
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

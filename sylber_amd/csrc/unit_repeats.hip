// Unit repeats (sylber_amd/units.py: local_align_unit_strings / UnitIndex.find_repeats; contract in include/sylber_hip.h "Unit
// repeats", restated in tests/unit_repeats_ref.py): the LOCAL alignment (Smith-Waterman) of two unit strings of any length up to
// 65 536 units on each side, many pairs per call -- the best-scoring pair of sub-spans, i.e. what is said in both recordings, found
// without a query.  unit_strings.hip's sibling: the same strips of 64 rows and the same anti-diagonal wavefront, with a floor at 0
// in the recurrence, a cell that carries where its path began instead of its counts, and a running best in every lane instead of
// the last cell.
//   * unit_local_kernel<WP>: one 64-thread workgroup (one wave) per pair; nothing is handed between workgroups and every loop is
//     bounded by lengths that the host wrote down, so nothing waits and nothing can spin.  Inside strip s lane i holds unit
//     64 s + i of x (its W ids padded to WP = 1, 2, 4 or 8 words with zeros) and walks y on the anti-diagonal wavefront: column
//     st - i at step st, the columns through a ring of 128 columns in LDS, 32 new ones every 32 steps, loaded a chunk ahead.
//     A cell is (H, si, sj): (si, sj) = the first cell of the path that the chosen candidate tracked, a don't-care where H = 0 --
//     nothing reads it there: a diagonal step from a cell with H = 0 starts anew at its own (i, j), and an up or left candidate
//     from such a cell is negative and loses to the floor.  Row -1 and column -1 are H = 0.
//     Between strips: lane 63 of every strip but the last writes its row, 12 B per column, to one of TWO rows of the pair's slice
//     of the workspace, strips alternating, and lane 0 of the next strip takes it as its upper row: lanes 0 .. 31 load a chunk of
//     it ahead, beside the ring's columns, and at step k of the chunk lane 0 works on the very column that lane k loaded, so a
//     v_readlane hands it over.  The lane above's cell comes through DPP (wave_shr:1).  A strip reads one row and writes the
//     other, and a fence and a barrier stand between strips (workgroup scope: a pair stays inside one workgroup).  Only columns
//     below L are read, and the strip before wrote every one of them: nothing depends on what the workspace held.
//     The best cell: every lane keeps (H, i, j, si, sj) of the best cell it has seen, replaced on a strictly larger H only.  A
//     lane meets its cells by ascending row (strip after strip) and inside a row by ascending column, so it keeps the smallest i
//     and then the smallest j of its largest H.  After the last strip a butterfly over the 64 lanes under (H descending, i
//     ascending) picks the pair's cell; two lanes never hold the same row, so j needs no comparison.
//     No predecessor codes, no traceback.  Plain vector loads and stores only.
// LDS: 4 KiB of ring at WP = 8, 64 threads: wave slots bound the occupancy.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "unit_local.h"                                   // the strip's shape, the limits, the DPP exchange, the host's length checks
#include <vector>

constexpr int UL_TAB = 5;                                 // int64 per pair: x row, m, y row, L, byte offset of the two rows

// Workgroup (one wave) `pair`: rows tab[0] .. + tab[1] of x [*, W] against rows tab[2] .. + tab[3] of y [*, W]; tab[4]: where in ws
// its two rows lie.  sw = match * W, pen = match + mismatch, gw = gap * W: s(i, j) = sw - pen * sub(i, j).  Writes score [pairs] and
// span [pairs][4] = (a0, a1, b0, b1).
template <int WP>
__global__ __launch_bounds__(64) void unit_local_kernel(const int32_t* __restrict__ x, const int32_t* __restrict__ y, int W,
                                                        const int64_t* __restrict__ tab, int sw, int pen, int gw,
                                                        int32_t* __restrict__ score, int32_t* __restrict__ span, char* ws) {
    __shared__ __attribute__((aligned(16))) int ring[UL_RING * WP];      // [column % 128][WP] ids of y's columns
    const int lane = threadIdx.x;
    const size_t pair = blockIdx.x;
    const int64_t* t = tab + pair * UL_TAB;                // workgroup-uniform, as all that follows from it
    const int64_t xo = t[0], yo = t[2];
    const int m = (int)t[1], L = (int)t[3];
    if (m == 0 || L == 0) {                                // no DP step: what the contract says of an empty side
        if (lane == 0) score[pair] = 0;
        if (lane < 4) span[pair * 4 + lane] = -1;
        return;
    }
    int32_t* rows = (int32_t*)(ws + t[4]);
    const int S = (m + UL_ROWS - 1) / UL_ROWS;
    const bool first = lane == 0;

    int bh = 0, bi = -1, bj = -1, bsi = -1, bsj = -1;      // this lane's best cell
    for (int s = 0; s < S; ++s) {
        const int i = s * UL_ROWS + lane, ms = m - s * UL_ROWS < UL_ROWS ? m - s * UL_ROWS : UL_ROWS;
        const bool valid = lane < ms, top = s == 0, carry = s + 1 < S;
        const size_t up = (size_t)((s + 1) & 1) * 3 * L, down = (size_t)(s & 1) * 3 * L;     // the row strip s - 1 wrote, the row this one writes

        int pu[WP];
#pragma unroll
        for (int c = 0; c < WP; ++c) pu[c] = (valid && c < W) ? x[(size_t)(xo + i) * W + c] : 0;

        int xr[WP], ar[3] = {0, 0, 0};
        auto fetch = [&](int chunk) {                      // lanes 0 .. 31: column chunk * 32 + lane of y and of the row above
            const int j = chunk * UL_CH + lane;
            const bool in = lane < UL_CH && j < L;
#pragma unroll
            for (int c = 0; c < WP; ++c) xr[c] = (in && c < W) ? y[(size_t)(yo + j) * W + c] : 0;
            if (!top) {
#pragma unroll
                for (int c = 0; c < 3; ++c) ar[c] = in ? rows[up + (size_t)j * 3 + c] : 0;
            }
        };

        // (sh, ssi, ssj) = the cell [i][last column done], column -1 at first; (dh, dsi, dsj) = the cell [i-1][that column], the
        // next diagonal
        int sh = 0, ssi = 0, ssj = 0, dh = 0, dsi = 0, dsj = 0;
        const int nsteps = L + ms - 1, nchunks = (nsteps + UL_CH - 1) / UL_CH;
        fetch(0);
        for (int chunk = 0; chunk < nchunks; ++chunk) {
            if (lane < UL_CH) {
                const int slot = (chunk * UL_CH + lane) & (UL_RING - 1);
                int* dst = ring + slot * WP;
                if constexpr (WP == 1) dst[0] = xr[0];
                else if constexpr (WP == 2) *(int2*)dst = make_int2(xr[0], xr[1]);
                else {
#pragma unroll
                    for (int c = 0; c < WP; c += 4) *(int4*)(dst + c) = make_int4(xr[c], xr[c + 1], xr[c + 2], xr[c + 3]);
                }
            }
            __syncthreads();                               // one wave: its LDS accesses stay in order, the barrier makes the writes visible
            const int a0 = ar[0], a1 = ar[1], a2 = ar[2];  // lane k: (H, si, sj) of column chunk * 32 + k of the row above the strip
            fetch(chunk + 1);
            const int st0 = chunk * UL_CH, ns = nsteps - st0 < UL_CH ? nsteps - st0 : UL_CH;
            for (int k = 0; k < ns; ++k) {
                int uh = ul_lane_above(sh), usi = ul_lane_above(ssi), usj = ul_lane_above(ssj);      // the cell [i-1][j] where this lane works on column j
                const int j = st0 + k - lane;
                if (top) {                                 // lane 0, column st0 + k: row -1, or the last row of the strip before
                    if (first) { uh = 0; usi = 0; usj = 0; }
                } else {
                    const int b0 = __builtin_amdgcn_readlane(a0, k), b1 = __builtin_amdgcn_readlane(a1, k), b2 = __builtin_amdgcn_readlane(a2, k);
                    if (first) { uh = b0; usi = b1; usj = b2; }
                }
                if (valid && (unsigned)j < (unsigned)L) {
                    const int* src = ring + (j & (UL_RING - 1)) * WP;
                    int v[WP];
                    if constexpr (WP == 1) v[0] = src[0];
                    else if constexpr (WP == 2) { const int2 q = *(const int2*)src; v[0] = q.x; v[1] = q.y; }
                    else {
#pragma unroll
                        for (int c = 0; c < WP; c += 4) {
                            const int4 q = *(const int4*)(src + c);
                            v[c] = q.x; v[c + 1] = q.y; v[c + 2] = q.z; v[c + 3] = q.w;
                        }
                    }
                    int sub = 0;
#pragma unroll
                    for (int c = 0; c < WP; ++c) sub += pu[c] != v[c] ? 1 : 0;
                    int best = dh + sw - pen * sub, ci = dh > 0 ? dsi : i, cj = dh > 0 ? dsj : j;
                    if (uh - gw > best) { best = uh - gw; ci = usi; cj = usj; }
                    if (sh - gw > best) { best = sh - gw; ci = ssi; cj = ssj; }
                    if (best < 0) best = 0;
                    dh = uh; dsi = usi; dsj = usj; sh = best; ssi = ci; ssj = cj;
                    if (best > bh) { bh = best; bi = i; bj = j; bsi = ci; bsj = cj; }
                    if (carry && lane == UL_ROWS - 1) {
                        int32_t* dst = rows + down + (size_t)j * 3;
                        dst[0] = best; dst[1] = ci; dst[2] = cj;
                    }
                }
            }
        }
        __threadfence_block();
        __syncthreads();                                   // the strip's row is written and visible to the wave
    }
    // the pair's cell: the largest H, then the smallest i; lanes that never saw a positive cell hold H = 0 and lose or tie at 0
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int oh = __shfl_xor(bh, o), oi = __shfl_xor(bi, o), oj = __shfl_xor(bj, o), osi = __shfl_xor(bsi, o), osj = __shfl_xor(bsj, o);
        if (oh > bh || (oh == bh && oh > 0 && oi < bi)) { bh = oh; bi = oi; bj = oj; bsi = osi; bsj = osj; }
    }
    if (lane == 0) {
        score[pair] = bh;
        int32_t* sp = span + pair * 4;
        if (bh > 0) { sp[0] = bsi; sp[1] = bi + 1; sp[2] = bsj; sp[3] = bj + 1; }
        else { sp[0] = -1; sp[1] = -1; sp[2] = -1; sp[3] = -1; }
    }
}

static inline int64_t ul_table_bytes(int32_t n_pairs) { return ul_al((int64_t)n_pairs * UL_TAB * 8); }

extern "C" int64_t sylber_unit_local_workspace_bytes(const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs) {
    if (ul_check(x_win_host, y_win_host, n_pairs)) return -1;
    int64_t bytes = ul_table_bytes(n_pairs);               // the pairs' table | per pair: its two rows
    for (int32_t p = 0; p < n_pairs; ++p) bytes += ul_rows_bytes(x_win_host[2 * (size_t)p + 1], y_win_host[2 * (size_t)p + 1]);
    return bytes;
}

static int ul_run(const int32_t* x_units_dev, int32_t x_rows, const int32_t* y_units_dev, int32_t y_rows, int32_t W,
                  const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs, int32_t match, int32_t mismatch, int32_t gap,
                  int32_t* score_dev, int32_t* span_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_unit_local_align";
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first device call
    if (!x_units_dev || !y_units_dev || !score_dev || !span_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (W < 1 || W > UL_MAX_W) { syl_set_error(what, "need 1 <= W <= 8"); return 1; }
    if (const char* bad = ul_check(x_win_host, y_win_host, n_pairs)) { syl_set_error(what, bad); return 1; }
    if (match < 1 || match > UL_MAX_PARAM) { syl_set_error(what, "need 1 <= match <= 64"); return 1; }
    if (mismatch < 0 || mismatch > UL_MAX_PARAM) { syl_set_error(what, "need 0 <= mismatch <= 64"); return 1; }
    if (gap < 1 || gap > UL_MAX_PARAM) { syl_set_error(what, "need 1 <= gap <= 64"); return 1; }
    if (x_rows < 0 || y_rows < 0) { syl_set_error(what, "need x_rows, y_rows >= 0"); return 1; }
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int64_t xa = x_win_host[2 * (size_t)p], m = x_win_host[2 * (size_t)p + 1], ya = y_win_host[2 * (size_t)p], L = y_win_host[2 * (size_t)p + 1];
        if (xa < 0 || xa + m > x_rows || ya < 0 || ya + L > y_rows) { syl_set_error(what, "a window lies outside its buffer"); return 1; }
    }
    // where each pair's slice lies: host arithmetic on the lengths
    std::vector<int64_t> tab((size_t)n_pairs * UL_TAB);
    int64_t at = ul_table_bytes(n_pairs);
    for (int32_t p = 0; p < n_pairs; ++p) {
        int64_t* e = tab.data() + (size_t)p * UL_TAB;
        e[0] = x_win_host[2 * (size_t)p]; e[1] = x_win_host[2 * (size_t)p + 1];
        e[2] = y_win_host[2 * (size_t)p]; e[3] = y_win_host[2 * (size_t)p + 1];
        e[4] = at; at += ul_rows_bytes(e[1], e[3]);
    }
    // the table is pageable host memory: the copy is staged before the call returns, in stream order on the device
    HIP_TRY(hipMemcpyAsync(workspace_dev, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
    const int wp = W == 1 ? 1 : W == 2 ? 2 : W <= 4 ? 4 : 8;
#define UL_LAUNCH(WPV)                                                                                                                      \
    hipLaunchKernelGGL((unit_local_kernel<WPV>), dim3((unsigned)n_pairs), dim3(64), 0, s, x_units_dev, y_units_dev, W,                      \
                       (const int64_t*)workspace_dev, match * W, match + mismatch, gap * W, score_dev, span_dev, (char*)workspace_dev)
    switch (wp) {
    case 1: UL_LAUNCH(1); break;
    case 2: UL_LAUNCH(2); break;
    case 4: UL_LAUNCH(4); break;
    default: UL_LAUNCH(8); break;
    }
#undef UL_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_unit_local_align(const int32_t* x_units_dev, int32_t x_rows, const int32_t* y_units_dev, int32_t y_rows, int32_t W,
                                       const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs, int32_t match,
                                       int32_t mismatch, int32_t gap, int32_t* score_dev, int32_t* span_dev, void* workspace_dev,
                                       void* stream) {
    try {
        return ul_run(x_units_dev, x_rows, y_units_dev, y_rows, W, x_win_host, y_win_host, n_pairs, match, mismatch, gap, score_dev,
                      span_dev, workspace_dev, stream);
    } catch (...) { syl_set_error("sylber_unit_local_align", "out of host memory"); return 1; }
}

// Unit repeats, every one (sylber_amd/units.py: local_align_unit_strings_all / UnitIndex.find_repeats with per_pair or within;
// contract in include/sylber_hip.h "Unit repeats, every one", restated in tests/unit_repeats_all_ref.py): up to n_best repeats of
// a pair of unit strings, and with a band below the diagonal the repeats inside ONE string.  unit_repeats.hip's sibling: the same
// strips of 64 rows, ring of 128 columns, DPP exchange and two carried rows (unit_local.h), run n_best times over the pair with
// the cells of the earlier rounds' rectangles, and of the band, held at H = 0.
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
#include "unit_local.h"
#include <vector>

constexpr int ULA_TAB = 6;                                // int64 per pair: x row, m, y row, L, byte offset of the two rows, sep
constexpr int ULA_MAX_BEST = 32;                          // rounds of a pair: one bit each in a lane's mask

// Strip s of round r of a pair, for the wave: rows 64 s .. of x against all of y.  BLOCK: the round has blocked cells -- the band
// (sep > 0) or the rectangles rect[0 .. r) of the rounds done; without it the body is unit_local_kernel's strip, instruction for
// instruction.  (bh, bi, bj, bsi, bsj): this lane's best cell of the round.
template <int WP, bool BLOCK>
__device__ __forceinline__ void ula_strip(int* ring, const int* rect, const int32_t* __restrict__ x, const int32_t* __restrict__ y, int W,
                                          int64_t xo, int64_t yo, int m, int L, int sep, int32_t* rows, int s, int S, int r, int sw,
                                          int pen, int gw, int& bh, int& bi, int& bj, int& bsi, int& bsj) {
    const int lane = threadIdx.x;
    const bool first = lane == 0;
    const int i = s * UL_ROWS + lane, ms = m - s * UL_ROWS < UL_ROWS ? m - s * UL_ROWS : UL_ROWS;
    const bool valid = lane < ms, top = s == 0, carry = s + 1 < S;
    const size_t up = (size_t)((s + 1) & 1) * 3 * L, down = (size_t)(s & 1) * 3 * L;     // the row strip s - 1 wrote, the row this one writes

    unsigned mask = 0;                                     // bit q: row i lies in the rows of round q's rectangle
    if constexpr (BLOCK) {
        for (int q = 0; q < r; ++q) mask |= (i >= rect[4 * q] && i < rect[4 * q + 1]) ? 1u << q : 0u;
    }

    int pu[WP];
#pragma unroll
    for (int c = 0; c < WP; ++c) pu[c] = (valid && c < W) ? x[(size_t)(xo + i) * W + c] : 0;

    int xr[WP], ar[3] = {0, 0, 0};
    auto fetch = [&](int chunk) {                          // lanes 0 .. 31: column chunk * 32 + lane of y and of the row above
        const int j = chunk * UL_CH + lane;
        const bool in = lane < UL_CH && j < L;
#pragma unroll
        for (int c = 0; c < WP; ++c) xr[c] = (in && c < W) ? y[(size_t)(yo + j) * W + c] : 0;
        if (!top) {
#pragma unroll
            for (int c = 0; c < 3; ++c) ar[c] = in ? rows[up + (size_t)j * 3 + c] : 0;
        }
    };

    // (sh, ssi, ssj) = the cell [i][last column done], column -1 at first; (dh, dsi, dsj) = the cell [i-1][that column], the next
    // diagonal
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
        __syncthreads();                                   // one wave: its LDS accesses stay in order, the barrier makes the writes visible
        const int a0 = ar[0], a1 = ar[1], a2 = ar[2];      // lane k: (H, si, sj) of column chunk * 32 + k of the row above the strip
        fetch(chunk + 1);
        const int st0 = chunk * UL_CH, ns = nsteps - st0 < UL_CH ? nsteps - st0 : UL_CH;
        for (int k = 0; k < ns; ++k) {
            int uh = ul_lane_above(sh), usi = ul_lane_above(ssi), usj = ul_lane_above(ssj);  // the cell [i-1][j] where this lane works on column j
            const int j = st0 + k - lane;
            if (top) {                                     // lane 0, column st0 + k: row -1, or the last row of the strip before
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
                if constexpr (BLOCK) {                     // the band, then the columns of the rectangles that hold row i
                    bool blocked = sep > 0 && j - i < sep;
                    for (unsigned rest = mask; rest && !blocked; rest &= rest - 1) {
                        const int q = __builtin_ctz(rest);
                        blocked = j >= rect[4 * q + 2] && j < rect[4 * q + 3];
                    }
                    if (blocked) best = 0;
                }
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
    __syncthreads();                                       // the strip's row is written and visible to the wave
}

// Workgroup (one wave) `pair`: rows tab[0] .. + tab[1] of x [*, W] against rows tab[2] .. + tab[3] of y [*, W]; tab[4]: where in ws
// its two rows lie; tab[5]: its sep.  sw = match * W, pen = match + mismatch, gw = gap * W: s(i, j) = sw - pen * sub(i, j).  Writes
// score [pairs][R] and span [pairs][R][4] = (a0, a1, b0, b1).
template <int WP>
__global__ __launch_bounds__(64) void unit_local_all_kernel(const int32_t* __restrict__ x, const int32_t* __restrict__ y, int W,
                                                            const int64_t* __restrict__ tab, int sw, int pen, int gw, int R, int floor,
                                                            int32_t* __restrict__ score, int32_t* __restrict__ span, char* ws) {
    __shared__ __attribute__((aligned(16))) int ring[UL_RING * WP];      // [column % 128][WP] ids of y's columns
    __shared__ __attribute__((aligned(16))) int rect[ULA_MAX_BEST * 4];  // [round] (a0, a1, b0, b1) of the rounds done
    const int lane = threadIdx.x;
    const size_t pair = blockIdx.x;
    const int64_t* t = tab + pair * ULA_TAB;               // workgroup-uniform, as all that follows from it
    const int64_t xo = t[0], yo = t[2];
    const int m = (int)t[1], L = (int)t[3], sep = (int)t[5];
    int32_t* rows = (int32_t*)(ws + t[4]);
    int32_t* sc = score + pair * R;
    int32_t* sp = span + pair * R * 4;
    const int S = (m + UL_ROWS - 1) / UL_ROWS;

    int r = 0;
    for (; r < R && m > 0 && L > 0; ++r) {                 // an empty side: no DP step, every round is padding
        int bh = 0, bi = -1, bj = -1, bsi = -1, bsj = -1;  // this lane's best cell of the round
        if (r > 0 || sep > 0) {                            // wave-uniform: round 0 without a band has no blocked cell
            for (int s = 0; s < S; ++s) ula_strip<WP, true>(ring, rect, x, y, W, xo, yo, m, L, sep, rows, s, S, r, sw, pen, gw, bh, bi, bj, bsi, bsj);
        } else {
            for (int s = 0; s < S; ++s) ula_strip<WP, false>(ring, rect, x, y, W, xo, yo, m, L, sep, rows, s, S, r, sw, pen, gw, bh, bi, bj, bsi, bsj);
        }
        // the round's cell: the largest H, then the smallest i; lanes that never saw a positive cell hold H = 0 and lose or tie at
        // 0.  The butterfly leaves it in every lane.
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int oh = __shfl_xor(bh, o), oi = __shfl_xor(bi, o), oj = __shfl_xor(bj, o), osi = __shfl_xor(bsi, o), osj = __shfl_xor(bsj, o);
            if (oh > bh || (oh == bh && oh > 0 && oi < bi)) { bh = oh; bi = oi; bj = oj; bsi = osi; bsj = osj; }
        }
        if (bh < floor) break;                             // uniform: this round and the later ones are padding
        if (lane == 0) {
            sc[r] = bh;
            sp[4 * r] = bsi; sp[4 * r + 1] = bi + 1; sp[4 * r + 2] = bsj; sp[4 * r + 3] = bj + 1;
            rect[4 * r] = bsi; rect[4 * r + 1] = bi + 1; rect[4 * r + 2] = bsj; rect[4 * r + 3] = bj + 1;
        }
        __syncthreads();                                   // the rectangle is visible to the wave before the next round reads it
    }
    for (int q = r * 5 + lane; q < R * 5; q += UL_ROWS) {  // the rounds not run: score 0, spans -1
        const int e = q / 5, c = q - e * 5;
        if (c == 0) sc[e] = 0;
        else sp[4 * e + c - 1] = -1;
    }
}

static inline int64_t ula_table_bytes(int32_t n_pairs) { return ul_al((int64_t)n_pairs * ULA_TAB * 8); }

extern "C" int64_t sylber_unit_local_all_workspace_bytes(const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs) {
    if (ul_check(x_win_host, y_win_host, n_pairs)) return -1;
    int64_t bytes = ula_table_bytes(n_pairs);              // the pairs' table | per pair: its two rows
    for (int32_t p = 0; p < n_pairs; ++p) bytes += ul_rows_bytes(x_win_host[2 * (size_t)p + 1], y_win_host[2 * (size_t)p + 1]);
    return bytes;
}

static int ula_run(const int32_t* x_units_dev, int32_t x_rows, const int32_t* y_units_dev, int32_t y_rows, int32_t W,
                   const int32_t* x_win_host, const int32_t* y_win_host, const int32_t* sep_host, int32_t n_pairs, int32_t match,
                   int32_t mismatch, int32_t gap, int32_t n_best, int32_t min_score, int32_t* score_dev, int32_t* span_dev,
                   void* workspace_dev, void* stream) {
    static const char* what = "sylber_unit_local_align_all";
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first device call
    if (!x_units_dev || !y_units_dev || !score_dev || !span_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (W < 1 || W > UL_MAX_W) { syl_set_error(what, "need 1 <= W <= 8"); return 1; }
    if (const char* bad = ul_check(x_win_host, y_win_host, n_pairs)) { syl_set_error(what, bad); return 1; }
    if (match < 1 || match > UL_MAX_PARAM) { syl_set_error(what, "need 1 <= match <= 64"); return 1; }
    if (mismatch < 0 || mismatch > UL_MAX_PARAM) { syl_set_error(what, "need 0 <= mismatch <= 64"); return 1; }
    if (gap < 1 || gap > UL_MAX_PARAM) { syl_set_error(what, "need 1 <= gap <= 64"); return 1; }
    if (n_best < 1 || n_best > ULA_MAX_BEST) { syl_set_error(what, "need 1 <= n_best <= 32"); return 1; }
    if (min_score < 1) { syl_set_error(what, "need min_score >= 1"); return 1; }
    if (x_rows < 0 || y_rows < 0) { syl_set_error(what, "need x_rows, y_rows >= 0"); return 1; }
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int64_t xa = x_win_host[2 * (size_t)p], m = x_win_host[2 * (size_t)p + 1], ya = y_win_host[2 * (size_t)p], L = y_win_host[2 * (size_t)p + 1];
        if (xa < 0 || xa + m > x_rows || ya < 0 || ya + L > y_rows) { syl_set_error(what, "a window lies outside its buffer"); return 1; }
        if (sep_host && sep_host[p] < 0) { syl_set_error(what, "need sep >= 0"); return 1; }
    }
    // where each pair's slice lies: host arithmetic on the lengths
    std::vector<int64_t> tab((size_t)n_pairs * ULA_TAB);
    int64_t at = ula_table_bytes(n_pairs);
    for (int32_t p = 0; p < n_pairs; ++p) {
        int64_t* e = tab.data() + (size_t)p * ULA_TAB;
        e[0] = x_win_host[2 * (size_t)p]; e[1] = x_win_host[2 * (size_t)p + 1];
        e[2] = y_win_host[2 * (size_t)p]; e[3] = y_win_host[2 * (size_t)p + 1];
        e[4] = at; at += ul_rows_bytes(e[1], e[3]);
        e[5] = sep_host ? sep_host[p] : 0;
    }
    // the table is pageable host memory: the copy is staged before the call returns, in stream order on the device
    HIP_TRY(hipMemcpyAsync(workspace_dev, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
    const int wp = W == 1 ? 1 : W == 2 ? 2 : W <= 4 ? 4 : 8;
#define ULA_LAUNCH(WPV)                                                                                                                     \
    hipLaunchKernelGGL((unit_local_all_kernel<WPV>), dim3((unsigned)n_pairs), dim3(64), 0, s, x_units_dev, y_units_dev, W,                  \
                       (const int64_t*)workspace_dev, match * W, match + mismatch, gap * W, n_best, min_score, score_dev, span_dev,         \
                       (char*)workspace_dev)
    switch (wp) {
    case 1: ULA_LAUNCH(1); break;
    case 2: ULA_LAUNCH(2); break;
    case 4: ULA_LAUNCH(4); break;
    default: ULA_LAUNCH(8); break;
    }
#undef ULA_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_unit_local_align_all(const int32_t* x_units_dev, int32_t x_rows, const int32_t* y_units_dev, int32_t y_rows,
                                           int32_t W, const int32_t* x_win_host, const int32_t* y_win_host, const int32_t* sep_host,
                                           int32_t n_pairs, int32_t match, int32_t mismatch, int32_t gap, int32_t n_best,
                                           int32_t min_score, int32_t* score_dev, int32_t* span_dev, void* workspace_dev, void* stream) {
    try {
        return ula_run(x_units_dev, x_rows, y_units_dev, y_rows, W, x_win_host, y_win_host, sep_host, n_pairs, match, mismatch, gap,
                       n_best, min_score, score_dev, span_dev, workspace_dev, stream);
    } catch (...) { syl_set_error("sylber_unit_local_align_all", "out of host memory"); return 1; }
}

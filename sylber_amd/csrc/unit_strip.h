// The anti-diagonal strip behind the three alignments of whole unit strings (unit_strings.hip: global alignment; unit_repeats.hip:
// one repeat per pair; unit_repeats_all.hip: every repeat, round by round), the ring of columns that unit_align.hip walks too, and
// the host's arithmetic and checks on the pairs.  A kernel brings a cell policy and what it does around the strips.
//   * One 64-thread workgroup (one wave) per pair; nothing is handed between workgroups and every loop is bounded by lengths that
//     the host wrote down, so nothing waits and nothing can spin.  x is cut into strips of 64 rows that the wave takes one after
//     another.  Inside strip s lane i holds unit 64 s + i of x (its W ids padded to WP = 1, 2, 4 or 8 words with zeros) and walks y
//     on the anti-diagonal wavefront: column st - i at step st, the columns through a ring of 128 columns in LDS, 32 new ones every
//     32 steps, loaded a chunk ahead.  A cell is three ints, and what they mean is the policy's.
//   * Between strips: lane 63 of every strip but the last writes its row, 12 B per column, to one of TWO rows of the pair's slice
//     of the workspace, strips alternating, and lane 0 of the next strip takes it as its upper row: lanes 0 .. 31 load a chunk of
//     it ahead, beside the ring's columns, and at step k of the chunk lane 0 works on the very column that lane k loaded, so a
//     v_readlane hands it over; strip 0's upper row is the policy's row -1.  The lane above's cell comes through DPP (wave_shr:1,
//     VALU) and not through ds_bpermute (an LDS round trip).  A strip reads one row and writes the other, and a fence and a barrier
//     stand between strips (a workgroup's waves share one vector L1, so workgroup scope is enough; it would not be between
//     workgroups, which is why a pair stays inside one).  Only columns below L are read, and the strip before wrote every one of
//     them: nothing depends on what the workspace held.
//   * One wave takes about 400 cycles per anti-diagonal step (profiles/unit_strings_bench.md: 0.37 Gcells/s on a single long pair),
//     bound by the instructions of a step and not by the exchange; several rows per lane is the known next step, to be taken here.
//   * A policy is a plain struct, held by reference and inlined: what a kernel does not need is not in its loop (a wave-uniform
//     flag inside the cell loop cost a long pair 12 to 21 %, profiles/unit_repeats_all_bench.md).
#pragma once
#include "common.h"
#include <vector>

constexpr int UST_CH = 32;                                // steps of a chunk: lanes 0 .. 31 stage its columns
constexpr int UST_RING = 128;                             // columns of the ring: a step reads back 63 columns, a chunk is staged 32 ahead
constexpr int UST_ROWS = 64;                              // rows of x in a strip: one per lane
constexpr int UST_MAX_LEN = 65536, UST_MAX_W = 8, UST_MAX_PARAM = 64;
constexpr int UST_TAB = 5;                                // int64 every table has per pair: x row, m, y row, L, byte offset of the two rows

static_assert(UST_RING >= UST_ROWS - 1 + 2 * UST_CH && (UST_RING & (UST_RING - 1)) == 0, "the ring holds a chunk's columns, the 63 behind them and the next chunk");

// lane l: v of lane l - 1 (lane 0: its own), DPP wave_shr:1
__device__ __forceinline__ int ust_lane_above(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

// ---- the ring: [column % 128][WP] ids ----
template <int WP>
__device__ __forceinline__ void ust_ring_store(int* ring, int col, const int (&v)[WP]) {
    int* dst = ring + (col & (UST_RING - 1)) * WP;
    if constexpr (WP == 1) dst[0] = v[0];
    else if constexpr (WP == 2) *(int2*)dst = make_int2(v[0], v[1]);
    else {
#pragma unroll
        for (int c = 0; c < WP; c += 4) *(int4*)(dst + c) = make_int4(v[c], v[c + 1], v[c + 2], v[c + 3]);
    }
}

template <int WP>
__device__ __forceinline__ void ust_ring_load(const int* ring, int col, int (&v)[WP]) {
    const int* src = ring + (col & (UST_RING - 1)) * WP;
    if constexpr (WP == 1) v[0] = src[0];
    else if constexpr (WP == 2) { const int2 q = *(const int2*)src; v[0] = q.x; v[1] = q.y; }
    else {
#pragma unroll
        for (int c = 0; c < WP; c += 4) {
            const int4 q = *(const int4*)(src + c);
            v[c] = q.x; v[c + 1] = q.y; v[c + 2] = q.z; v[c + 3] = q.w;
        }
    }
}

// in how many of their words two units differ
template <int WP>
__device__ __forceinline__ int ust_mismatches(const int (&a)[WP], const int (&b)[WP]) {
    int sub = 0;
#pragma unroll
    for (int c = 0; c < WP; ++c) sub += a[c] != b[c] ? 1 : 0;
    return sub;
}

// ---- the strip ----
struct ust_cell { int a, b, c; };

// Strip s of S of a pair, for the wave: rows xo + 64 s .. of x [*, W] (m in all) against rows yo .. + L of y [*, W]; rows: the
// pair's two carried rows.  -> the lane's cell at the last column it did.  The policy:
//   ust_cell left(i), diag(i)              the cells [i][-1] and [i-1][-1]: the lane's state at column -1
//   ust_cell top(j)                        the cell [-1][j]: lane 0's upper row in strip 0
//   ust_cell step(d, u, l, sub, i, j, k)   the cell [i][j], done at step k of its chunk, from [i-1][j-1], [i-1][j], [i][j-1] and
//                                          the mismatches of the two units; whatever else the kernel keeps of a cell it keeps in here
//   void chunk_end(chunk)                  after the 32 steps of a chunk
template <int WP, class Policy>
__device__ __forceinline__ ust_cell ust_strip(Policy& pol, int* ring, const int32_t* __restrict__ x, const int32_t* __restrict__ y, int W,
                                              int64_t xo, int64_t yo, int m, int L, int32_t* rows, int s, int S) {
    const int lane = threadIdx.x;
    const bool first = lane == 0;
    const int i = s * UST_ROWS + lane, ms = m - s * UST_ROWS < UST_ROWS ? m - s * UST_ROWS : UST_ROWS;
    const bool valid = lane < ms, top = s == 0, carry = s + 1 < S;
    const size_t up = (size_t)((s + 1) & 1) * 3 * L, down = (size_t)(s & 1) * 3 * L;     // the row strip s - 1 wrote, the row this one writes

    int pu[WP];
#pragma unroll
    for (int c = 0; c < WP; ++c) pu[c] = (valid && c < W) ? x[(size_t)(xo + i) * W + c] : 0;

    int xr[WP], ar[3] = {0, 0, 0};
    auto fetch = [&](int chunk) {                          // lanes 0 .. 31: column chunk * 32 + lane of y and of the row above
        const int j = chunk * UST_CH + lane;
        const bool in = lane < UST_CH && j < L;
#pragma unroll
        for (int c = 0; c < WP; ++c) xr[c] = (in && c < W) ? y[(size_t)(yo + j) * W + c] : 0;
        if (!top) {
#pragma unroll
            for (int c = 0; c < 3; ++c) ar[c] = in ? rows[up + (size_t)j * 3 + c] : 0;
        }
    };

    ust_cell lf = pol.left(i), dg = pol.diag(i);          // the cell [i][last column done], and [i-1][that column]: the next diagonal
    const int nsteps = L + ms - 1, nchunks = (nsteps + UST_CH - 1) / UST_CH;
    fetch(0);
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        if (lane < UST_CH) ust_ring_store<WP>(ring, chunk * UST_CH + lane, xr);
        __syncthreads();                                   // one wave: its LDS accesses stay in order, the barrier makes the writes visible
        const int a0 = ar[0], a1 = ar[1], a2 = ar[2];      // lane k: the cell of column chunk * 32 + k of the row above the strip
        fetch(chunk + 1);
        const int st0 = chunk * UST_CH, ns = nsteps - st0 < UST_CH ? nsteps - st0 : UST_CH;
        for (int k = 0; k < ns; ++k) {
            // the cell [i-1][j] where this lane works on column j; three ints and not a ust_cell: lane 0's hand-over then compiles
            // to selects, as a struct to a branch, which cost a long pair 5 to 7 %
            int ua = ust_lane_above(lf.a), ub = ust_lane_above(lf.b), uc = ust_lane_above(lf.c);
            const int j = st0 + k - lane;
            if (top) {                                     // lane 0, column st0 + k: row -1, or the last row of the strip before
                const ust_cell t = pol.top(j);
                if (first) { ua = t.a; ub = t.b; uc = t.c; }
            } else {
                const int b0 = __builtin_amdgcn_readlane(a0, k), b1 = __builtin_amdgcn_readlane(a1, k), b2 = __builtin_amdgcn_readlane(a2, k);
                if (first) { ua = b0; ub = b1; uc = b2; }
            }
            if (valid && (unsigned)j < (unsigned)L) {
                int v[WP];
                ust_ring_load<WP>(ring, j, v);
                const ust_cell u = {ua, ub, uc}, n = pol.step(dg, u, lf, ust_mismatches<WP>(pu, v), i, j, k);
                dg = u; lf = n;
                if (carry && lane == UST_ROWS - 1) {
                    int32_t* dst = rows + down + (size_t)j * 3;
                    dst[0] = n.a; dst[1] = n.b; dst[2] = n.c;
                }
            }
        }
        pol.chunk_end(chunk);
    }
    __threadfence_block();
    __syncthreads();                                       // what the strip wrote is visible to the wave
    return lf;
}

// ---- local alignment: the cell of unit_repeats.hip and unit_repeats_all.hip ----
// A cell is (H, si, sj): (si, sj) = the first cell of the path that the chosen candidate tracked, a don't-care where H = 0 --
// nothing reads it there: a diagonal step from a cell with H = 0 starts anew at its own (i, j), and an up or left candidate from
// such a cell is negative and loses to the floor.  Row -1 and column -1 are H = 0.  No predecessor codes, no traceback.

// The best cell a lane has seen, replaced on a strictly larger H only.  A lane meets its cells by ascending row (strip after
// strip) and inside a row by ascending column, so it keeps the smallest i and then the smallest j of its largest H.
struct ul_best {
    int h = 0, i = -1, j = -1, si = -1, sj = -1;
    // the wave's cell into every lane: the largest H, then the smallest i; lanes that never saw a positive cell hold H = 0 and lose
    // or tie at 0.  Two lanes never hold the same row, so j needs no comparison.
    __device__ __forceinline__ void butterfly() {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int oh = __shfl_xor(h, o), oi = __shfl_xor(i, o), oj = __shfl_xor(j, o), osi = __shfl_xor(si, o), osj = __shfl_xor(sj, o);
            if (oh > h || (oh == h && oh > 0 && oi < i)) { h = oh; i = oi; j = oj; si = osi; sj = osj; }
        }
    }
};

// sw = match * W, pen = match + mismatch, gw = gap * W: s(i, j) = sw - pen * sub(i, j).  BLOCK (unit_repeats_all.hip): cells below
// the band (j - i < sep, where sep > 0) and inside the rectangles rect[0 .. r) = (a0, a1, b0, b1) are held at H = 0; mask, bit q:
// the strip's row i lies in the rows of rectangle q, so a cell tests column ranges only where that is non-zero, one per set bit.
template <bool BLOCK>
struct ul_cell {
    ul_best& best;
    int sw, pen, gw, sep = 0;
    const int* rect = nullptr;
    int r = 0;
    unsigned mask = 0;
    __device__ __forceinline__ void strip(int s) {         // BLOCK: before every strip
        const int i = s * UST_ROWS + threadIdx.x;
        mask = 0;
        for (int q = 0; q < r; ++q) mask |= (i >= rect[4 * q] && i < rect[4 * q + 1]) ? 1u << q : 0u;
    }
    __device__ __forceinline__ ust_cell left(int) const { return {0, 0, 0}; }
    __device__ __forceinline__ ust_cell diag(int) const { return {0, 0, 0}; }
    __device__ __forceinline__ ust_cell top(int) const { return {0, 0, 0}; }
    __device__ __forceinline__ ust_cell step(const ust_cell& d, const ust_cell& u, const ust_cell& l, int sub, int i, int j, int) {
        int h = d.a + sw - pen * sub, ci = d.a > 0 ? d.b : i, cj = d.a > 0 ? d.c : j;
        if (u.a - gw > h) { h = u.a - gw; ci = u.b; cj = u.c; }
        if (l.a - gw > h) { h = l.a - gw; ci = l.b; cj = l.c; }
        if (h < 0) h = 0;
        if constexpr (BLOCK) {                             // the band, then the columns of the rectangles that hold row i
            bool blocked = sep > 0 && j - i < sep;
            for (unsigned rest = mask; rest && !blocked; rest &= rest - 1) {
                const int q = __builtin_ctz(rest);
                blocked = j >= rect[4 * q + 2] && j < rect[4 * q + 3];
            }
            if (blocked) h = 0;
        }
        if (h > best.h) { best.h = h; best.i = i; best.j = j; best.si = ci; best.sj = cj; }
        return {h, ci, cj};
    }
    __device__ __forceinline__ void chunk_end(int) {}
};

// ---- the host ----
static inline int64_t ust_al(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
// the two rows between strips: a cell per column, only where there is a second strip
static inline int64_t ust_rows_bytes(int64_t m, int64_t L) { return m > UST_ROWS && L > 0 ? ust_al(2 * 12 * L) : 0; }
static inline int64_t ust_table_bytes(int32_t n_pairs, int cols) { return ust_al((int64_t)n_pairs * cols * 8); }

// The pairs' table, int64 [n_pairs][cols], first in the workspace: where each pair's slice lies is host arithmetic on the lengths.
struct ust_table {
    int cols;
    int64_t at;                                            // the first byte of the workspace not given away
    std::vector<int64_t> tab;
    ust_table(int32_t n_pairs, int cols) : cols(cols), at(ust_table_bytes(n_pairs, cols)), tab((size_t)n_pairs * cols) {}
    // pair p: its UST_TAB columns, its two rows after what is given away -> its entry, for the columns past UST_TAB
    int64_t* add(int32_t p, int64_t xo, int64_t m, int64_t yo, int64_t L) {
        int64_t* e = tab.data() + (size_t)p * cols;
        e[0] = xo; e[1] = m; e[2] = yo; e[3] = L;
        e[4] = at; at += ust_rows_bytes(m, L);
        return e;
    }
    const int64_t* data() const { return tab.data(); }
    size_t size() const { return tab.size(); }
};

// STMT with WPV = the words a unit of W ids is padded to
#define UST_WITH_WP(W, STMT)                                                                                                                 \
    switch ((W) == 1 ? 1 : (W) == 2 ? 2 : (W) <= 4 ? 4 : 8) {                                                                               \
    case 1: { constexpr int WPV = 1; STMT; } break;                                                                                         \
    case 2: { constexpr int WPV = 2; STMT; } break;                                                                                         \
    case 4: { constexpr int WPV = 4; STMT; } break;                                                                                         \
    default: { constexpr int WPV = 8; STMT; } break;                                                                                        \
    }

// a C entry's body under the catch that its host vectors need
template <class F>
static inline int ust_entry(const char* what, F body) {
    try { return body(); } catch (...) { syl_set_error(what, "out of host memory"); return 1; }
}

// the host's checks -> nullptr or what is wrong
// windows (row, rows) [n_pairs][2]: their lengths
static inline const char* ust_check_lengths(const int32_t* x_win, const int32_t* y_win, int32_t n_pairs) {
    if (!x_win || !y_win) return "null argument";
    if (n_pairs < 1) return "need n_pairs >= 1";
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int64_t m = x_win[2 * (size_t)p + 1], L = y_win[2 * (size_t)p + 1];
        if (m < 0 || L < 0) return "a window has a negative number of rows";
        if (m > UST_MAX_LEN || L > UST_MAX_LEN) return "a string has at most 65536 units";
    }
    return nullptr;
}

static inline const char* ust_check_scoring(int32_t match, int32_t mismatch, int32_t gap) {
    if (match < 1 || match > UST_MAX_PARAM) return "need 1 <= match <= 64";
    if (mismatch < 0 || mismatch > UST_MAX_PARAM) return "need 0 <= mismatch <= 64";
    if (gap < 1 || gap > UST_MAX_PARAM) return "need 1 <= gap <= 64";
    return nullptr;
}

// the windows against their buffers and, where sep is not null, each pair's sep
static inline const char* ust_check_windows(const int32_t* x_win, int32_t x_rows, const int32_t* y_win, int32_t y_rows, const int32_t* sep,
                                           int32_t n_pairs) {
    if (x_rows < 0 || y_rows < 0) return "need x_rows, y_rows >= 0";
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int64_t xa = x_win[2 * (size_t)p], m = x_win[2 * (size_t)p + 1], ya = y_win[2 * (size_t)p], L = y_win[2 * (size_t)p + 1];
        if (xa < 0 || xa + m > x_rows || ya < 0 || ya + L > y_rows) return "a window lies outside its buffer";
        if (sep && sep[p] < 0) return "need sep >= 0";
    }
    return nullptr;
}

// Embedding strings, local (sylber_amd/search.py: local_align_sequences / SyllableIndex.local_align_sequences; contract in
// include/sylber_hip.h "Embedding strings, local", restated in tests/dtw_strings_local_ref.py): the LOCAL alignment of two WHOLE
// embedding sequences of up to 65 536 rows on each side, up to 32 repeats per pair, and with a band below the diagonal the repeats
// inside ONE sequence.  dtw_strings.hip's walk, dtw_local.hip's recurrence, unit_repeats_all.hip's rounds, rectangles and band.
//   * dtw_strings_local_kernel: one workgroup of 256 threads per pair runs ALL the rounds of its pair; nothing is handed between
//     workgroups, every loop is bounded by lengths that the host wrote down and by n_best, every barrier is reached by all 256
//     threads with workgroup-uniform trip counts, so nothing waits and nothing can spin.  The contraction is
//     dtw_strings_kernel<false>'s: super-strips of 128 rows of x (KN_BM) against tiles of 128 columns of y (KN_BN), kn_stage /
//     kn_mma / dt_cost_tile in the same k-pair order, so every local cost has the bits of sylber_dtw_search's.  Every round repeats
//     it: m L costs are up to 16 GiB per pair and are not kept.
//     The DP: wave 0 walks rows 0 .. 63 of a super-strip and, behind a barrier, wave 1 rows 64 .. 127, on the anti-diagonal
//     wavefront with the DPP wave_shr:1 hand-down.  A cell is 8 bytes, (H bits, si << 16 | sj): the size of the global kernel's
//     (A, n), so the upper rows in LDS and the two alternating carried rows in the workspace keep their sizes.  The row above
//     the matrix and column -1 are H = 0.
//     Blocked cells.  Round 0 of a pair with sep = 0 has nothing to block: one workgroup-uniform branch per tile picks the walk
//     without any test in it.  Otherwise a lane derives, once per super-strip, a 32-bit mask of the rectangles whose rows contain
//     its row; a cell tests column ranges only where that mask is non-zero, and the band is one compare, j - i < sep.  A blocked
//     cell gets H = 0: it never beats a lane's best (strict >), its start is never read, and in a strip's last row it still
//     writes H = 0 to up1 and to the carried row, so nothing reads an earlier round's row or stale workspace.
//     Skipped tiles.  The tiles of a super-strip that lie wholly in the band, n0 + 127 - i0 < sep, are a prefix of its tiles:
//     they skip their K loop and their walk, the carried row gets zeros in their columns, and the walk starts behind them from
//     zero cells.  A sequence against itself does about half the work.
//     Best cell.  Every lane of waves 0 and 1 keeps its best (H, i, j, start) under a strict >, across tiles and super-strips:
//     its rows ascend and its columns ascend inside a row, so it holds the first of its largest cells.  After the last
//     super-strip the 128 bests go through LDS and wave 0 reduces them under (H descending, i ascending) -- two lanes never hold
//     the same row.  Lane 0 writes the round's outputs, its rectangle to rect[round] in LDS and whether the pair goes on; all 256
//     threads read that behind a barrier.
//     Plain vector loads and stores only.
// LDS: dtw_strings_kernel's 70 144 B + 512 B of rectangles + 2 048 B of bests + 16 B = 72 720 B: two workgroups fit a CU.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "dtw_tile.h"
#include <cmath>
#include <vector>

constexpr int DSL_MAX_LEN = 65536;
constexpr int DSL_TAB = 8;                                // int64 per pair: x row, m, y row, L, byte offset of the two rows, sep, 0, 0
constexpr int DSL_STRIP = 64;                             // x rows of a strip: one per lane
constexpr int DSL_MAX_BEST = 32;                          // rounds of a pair: one bit each in a lane's mask
constexpr int DSL_LDS_FLOATS = KN_BM * DT_LD + KN_BN + 2 * 2 * KN_BN + DSL_MAX_BEST * 4 + 2 * DSL_STRIP * 4 + 4;
constexpr size_t DSL_LDS_BYTES = (size_t)DSL_LDS_FLOATS * 4;      // cost tile | c_j | upper rows of waves 0 and 1 | rectangles | bests | goes on

static_assert(KN_BM == 2 * DSL_STRIP && KN_BN == 128, "a super-strip is two strips");
static_assert(KN_STAGE <= KN_BM * DT_LD, "the cost tile covers the staging it aliases");
static_assert((KN_BM * DT_LD + KN_BN) * 4 % 16 == 0, "the upper rows are 8-byte cells, the bests 16-byte entries");
static_assert(2 * DSL_LDS_BYTES <= 160 * 1024, "two workgroups fit a CU");

// lane l: v of lane l - 1 (lane 0: its own), DPP wave_shr:1
__device__ __forceinline__ int dsl_above(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ float dsl_above(float v) { return __int_as_float(dsl_above(__float_as_int(v))); }

static inline int64_t dsl_rows_bytes(int64_t m, int64_t L) { return m > KN_BM && L > 0 ? kn_al(2 * 8 * L) : 0; }
static inline int64_t dsl_table_bytes(int32_t n_pairs) { return kn_al((int64_t)n_pairs * DSL_TAB * 8); }

// One lane of waves 0 and 1 = one row of the super-strip
struct DslLane {
    float h_cur = 0.f, h_prev = 0.f;                       // H of the lane's last two cells; column -1 is 0
    int t_cur = 0, t_prev = 0;                             // their starts, si << 16 | sj (read only where H > 0)
    float pa = 0.f;                                        // lane 0: the previous cell of the row above
    int pt = 0;
    float bh = 0.f;                                        // the lane's best cell of the round; 0: none
    int bi = 0x7fffffff, bj = 0, bt = 0;
};

// The walk of one strip over one tile: dr = the lane's row of the cost tile, upr = the row above the strip in this tile's columns.
// hands: the lane writes its cells to up1 (the row above wave 1's strip); keeps: to the carried row below the super-strip.
// BLOCK: cells of the band (sep > 0 and j - i < sep) and of the rectangles rect[q] = (a0, a1, b0, b1), q a set bit of mask, get H = 0.
template <bool BLOCK>
__device__ __forceinline__ void dsl_walk(DslLane& s, const float* dr, const int2* upr, int2* up1, int2* below, bool hands, bool keeps, int lane,
                                         int rw, int ncol, int i, int n0, float radius, float gap, int sep, unsigned mask, const int* rect) {
    for (int st = 0; st < ncol + rw - 1; ++st) {
        float uh = dsl_above(s.h_cur), uhp = dsl_above(s.h_prev);      // H[i-1][j], H[i-1][j-1] where this lane works on column j
        int ut = dsl_above(s.t_cur), utp = dsl_above(s.t_prev);
        const int j = st - lane;
        if (lane < rw && j >= 0 && j < ncol) {
            if (lane == 0) {
                const int2 u = upr[j];
                uh = __int_as_float(u.x); ut = u.y; uhp = s.pa; utp = s.pt;
                s.pa = uh; s.pt = ut;
            }
            const int gj = n0 + j;
            const float sc = radius - dr[j], sg = sc - gap;            // d = +inf: both -inf, every candidate -inf, H = 0
            float v = uhp + sc;                            // c_diag, then c_up, then c_left: the first largest
            int t = uhp > 0.f ? utp : (int)((unsigned)i << 16 | (unsigned)gj);
            const float cu = uh + sg;
            if (cu > v) { v = cu; t = ut; }
            const float cl = s.h_cur + sg;
            if (cl > v) { v = cl; t = s.t_cur; }
            float H = v > 0.f ? v : 0.f;
            if constexpr (BLOCK) {                         // the band, then the columns of the rectangles that hold row i
                bool blocked = sep > 0 && gj - i < sep;
                for (unsigned rest = mask; rest && !blocked; rest &= rest - 1) {
                    const int q = __builtin_ctz(rest);
                    blocked = gj >= rect[4 * q + 2] && gj < rect[4 * q + 3];
                }
                if (blocked) H = 0.f;
            }
            s.h_prev = s.h_cur; s.t_prev = s.t_cur; s.h_cur = H; s.t_cur = t;
            if (H > s.bh) { s.bh = H; s.bi = i; s.bj = gj; s.bt = t; }
            if (hands) up1[j] = make_int2(__float_as_int(H), t);
            if (keeps) below[gj] = make_int2(__float_as_int(H), t);
        }
    }
}

// (H, i) of a against b: the larger H, then the smaller row
__device__ __forceinline__ bool dsl_better(float ha, int ia, float hb, int ib) { return ha > hb || (ha == hb && ia < ib); }

// Workgroup `pair`: rows tab[0] .. + tab[1] of x [*, D] against rows tab[2] .. + tab[3] of y [*, D]; xn / cn: their ||row||^2 (L2)
// or null; tab[4]: where in ws its two rows lie; tab[5]: its sep.  Writes score [pairs][R] and span [pairs][R][4] = (a0, a1, b0, b1).
__global__ __launch_bounds__(256) void dtw_strings_local_kernel(const float* __restrict__ x, int x_rows, const float* __restrict__ xn,
                                                                const float* __restrict__ y, int y_rows, const float* __restrict__ cn, int D,
                                                                const int64_t* __restrict__ tab, float radius, float gap, float min_score, int R,
                                                                float* __restrict__ score, int32_t* __restrict__ span, char* ws) {
    extern __shared__ __attribute__((aligned(16))) float dsl_smem[];
    float* xs = dsl_smem;                                  // staging of the x rows
    float* cs = dsl_smem + KN_BM * KN_LD;                  // staging of the y rows
    float* dm = dsl_smem;                                  // [128][DT_LD] local costs of the tile, aliasing the staging
    float* cns = dsl_smem + KN_BM * DT_LD;                 // [128] c_j of the tile's columns
    int2* up0 = (int2*)(cns + KN_BN);                      // [128] (H, start) of the row above wave 0's strip, this tile's columns
    int2* up1 = up0 + KN_BN;                               // [128] the same above wave 1's strip: wave 0's last row
    int* rect = (int*)(up1 + KN_BN);                       // [32][4] (a0, a1, b0, b1) of the rounds done
    int4* bst = (int4*)(rect + DSL_MAX_BEST * 4);          // [128] (H, i, j, start): the bests of the lanes of waves 0 and 1
    int* ctl = (int*)(bst + 2 * DSL_STRIP);                // [0]: the pair goes on to the next round
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const size_t pair = blockIdx.x;
    const int64_t* t_ = tab + pair * DSL_TAB;              // workgroup-uniform, as all that follows from it
    float* sco = score + pair * R;
    int32_t* spo = span + pair * R * 4;
    // the table is what the host checked and wrote; the windows are clamped into their buffers all the same
    const int64_t xo = t_[0] < 0 ? 0 : (t_[0] < x_rows ? t_[0] : x_rows), yo = t_[2] < 0 ? 0 : (t_[2] < y_rows ? t_[2] : y_rows);
    const int64_t mw = x_rows - xo < DSL_MAX_LEN ? x_rows - xo : DSL_MAX_LEN, Lw = y_rows - yo < DSL_MAX_LEN ? y_rows - yo : DSL_MAX_LEN;
    const int m = (int)(t_[1] < 0 ? 0 : (t_[1] < mw ? t_[1] : mw)), L = (int)(t_[3] < 0 ? 0 : (t_[3] < Lw ? t_[3] : Lw));
    const int sep = (int)(t_[5] < 0 ? 0 : (t_[5] < 2 * DSL_MAX_LEN ? t_[5] : 2 * DSL_MAX_LEN));     // beyond m + L it blocks every cell anyway
    int2* carried = (int2*)(ws + t_[4]);
    const bool l2 = xn != nullptr;
    const int SS = (m + KN_BM - 1) / KN_BM, tiles = (L + KN_BN - 1) / KN_BN;
    const int sr = tid >> 1, sh = (tid & 1) * 8;
    float* xdst = xs + sr * KN_LD + (sh >> 1);
    float* cdst = cs + sr * KN_LD + (sh >> 1);
    const int frow = lane & 31, fh = lane >> 5;
    const int ksteps = D / KN_BK, T = ksteps * tiles;

    int r = 0;
    for (; r < R && m > 0 && L > 0; ++r) {                 // an empty side: no DP step, every round is padding
        const bool block = r > 0 || sep > 0;               // round 0 without a band has no blocked cell
        DslLane s;
        for (int ss = 0; ss < SS; ++ss) {
            const int i0 = ss * KN_BM, ms = m - i0 < KN_BM ? m - i0 : KN_BM;   // the super-strip's rows
            const bool carry = ss + 1 < SS;                // then ms = 128 and wave 1's lane 63 holds its last row
            const int2* above = carried + (size_t)((ss + 1) & 1) * L;         // the row super-strip ss - 1 wrote
            int2* below = carried + (size_t)(ss & 1) * L;                     // the row this one writes
            const int rw = wave < 2 ? (ms - wave * DSL_STRIP < 0 ? 0 : (ms - wave * DSL_STRIP < DSL_STRIP ? ms - wave * DSL_STRIP : DSL_STRIP)) : 0;
            const int i = i0 + wave * DSL_STRIP + lane;    // the lane's row (waves 0 and 1)
            // the tiles wholly inside the band, n0 + 127 - i0 < sep: the first ft of them
            const int band = sep + i0 - (KN_BN - 1);
            const int ft = sep > 0 && band > 0 ? ((band + KN_BN - 1) / KN_BN < tiles ? (band + KN_BN - 1) / KN_BN : tiles) : 0;
            if (carry) {
                const int zc = ft * KN_BN < L ? ft * KN_BN : L;
                for (int c = tid; c < zc; c += 256) below[c] = make_int2(0, 0);
            }
            // the lane's last two cells are those of column -1 or of a skipped tile: H = 0.  Lane 0 of wave 0 reads its upper row
            // one column back, and that row is not in the band
            s.h_cur = 0.f; s.h_prev = 0.f; s.t_cur = 0; s.t_prev = 0; s.pa = 0.f; s.pt = 0;
            if (ft > 0 && ft < tiles && ss > 0 && tid == 0) {
                const int2 u = above[ft * KN_BN - 1];
                s.pa = __int_as_float(u.x); s.pt = u.y;
            }
            unsigned mask = 0;
            if (wave < 2)
                for (int q = 0; q < r; ++q) mask |= (i >= rect[4 * q] && i < rect[4 * q + 1]) ? 1u << q : 0u;
            int xr = i0 + sr; xr = xr < m ? xr : m - 1;
            const float* xrow = x + (size_t)(xo + xr) * D + sh;
            bool live[2];                                  // wave-uniform: this wave's 32-row half holds x rows
            float qn[2] = {0.f, 0.f};
#pragma unroll
            for (int fm = 0; fm < 2; ++fm) {
                live[fm] = wm * 64 + fm * 32 < ms;
                int rr = i0 + wm * 64 + fm * 32 + frow; rr = rr < m ? rr : m - 1;
                if (l2) qn[fm] = xn[xo + rr];
            }

            f32x16_t acc[2][2];
            float4 xa, xb, ca, cb;
            auto fetch = [&](int t) {
                const int tile = t / ksteps, k0 = (t % ksteps) * KN_BK;
                int cr = tile * KN_BN + sr; cr = cr < L ? cr : L - 1;
                const float* crow = y + (size_t)(yo + cr) * D + sh + k0;
                xa = *(const float4*)(xrow + k0); xb = *(const float4*)(xrow + k0 + 4);
                ca = *(const float4*)crow; cb = *(const float4*)(crow + 4);
            };
            const int t0 = ft * ksteps;
            if (t0 < T) fetch(t0);
            for (int t = t0; t < T; ++t) {
                const int tile = t / ksteps, ks = t % ksteps, n0 = tile * KN_BN;
                if (ks == 0) kn_zero(acc);
                __syncthreads();                           // previous fragments, the cost tile, cns and the upper rows are all read
                kn_stage(xdst, cdst, xa, xb, ca, cb);
                if (ks == 0 && tid < KN_BN) {
                    const int j = n0 + tid;
                    cns[tid] = (cn && j < L) ? cn[yo + j] : 0.f;
                    up0[tid] = (ss > 0 && j < L) ? above[j] : make_int2(0, 0);
                }
                __syncthreads();
                if (t + 1 < T) fetch(t + 1);
                kn_mma(xs, cs, wm, wn, frow, fh, acc, live[0], live[1]);
                if (ks != ksteps - 1) continue;
                __syncthreads();                           // every wave is past its fragment reads: the cost tile aliases the staging
                dt_cost_tile(dm, cns, acc, l2, qn, live, wm, wn, frow, fh);
                const int ncol = L - n0 < KN_BN ? L - n0 : KN_BN;
                // wave 0 walks the upper strip, then, behind a barrier, wave 1 the lower one: wave 0's lane 63 has left its row in up1
#pragma unroll 1
                for (int w = 0; w < 2; ++w) {
                    __syncthreads();
                    if (wave != w || rw == 0) continue;    // wave-uniform
                    const float* dr = dm + (w * DSL_STRIP + lane) * DT_LD;
                    const int2* upr = w ? up1 : up0;
                    const bool hands = w == 0 && ms > DSL_STRIP && lane == DSL_STRIP - 1;     // the row above wave 1's strip
                    const bool keeps = carry && w == 1 && lane == DSL_STRIP - 1;             // the row above the next super-strip
                    if (block) dsl_walk<true>(s, dr, upr, up1, below, hands, keeps, lane, rw, ncol, i, n0, radius, gap, sep, mask, rect);
                    else dsl_walk<false>(s, dr, upr, up1, below, hands, keeps, lane, rw, ncol, i, n0, radius, gap, 0, 0u, rect);
                }
            }
            __threadfence_block();
            __syncthreads();                               // the super-strip's row is written and visible to the workgroup
        }
        // the round's cell: the 128 bests through LDS, wave 0 reduces them
        if (wave < 2) bst[tid] = make_int4(__float_as_int(s.bh), s.bi, s.bj, s.bt);
        __syncthreads();
        if (wave == 0) {
            const int4 a = bst[lane], b = bst[lane + DSL_STRIP];
            const bool ab = dsl_better(__int_as_float(b.x), b.y, __int_as_float(a.x), a.y);
            float h = __int_as_float(ab ? b.x : a.x);
            int bi = ab ? b.y : a.y, bj = ab ? b.z : a.z, bt = ab ? b.w : a.w;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float oh = __shfl_xor(h, o);
                const int oi = __shfl_xor(bi, o), oj = __shfl_xor(bj, o), ot = __shfl_xor(bt, o);
                if (dsl_better(oh, oi, h, bi)) { h = oh; bi = oi; bj = oj; bt = ot; }
            }
            if (lane == 0) {
                const bool found = h > 0.f && h >= min_score;
                ctl[0] = found ? 1 : 0;
                if (found) {
                    const int si = (int)((unsigned)bt >> 16), sj = bt & 0xffff;
                    sco[r] = h;
                    spo[4 * r] = si; spo[4 * r + 1] = bi + 1; spo[4 * r + 2] = sj; spo[4 * r + 3] = bj + 1;
                    rect[4 * r] = si; rect[4 * r + 1] = bi + 1; rect[4 * r + 2] = sj; rect[4 * r + 3] = bj + 1;
                }
            }
        }
        __syncthreads();                                   // the decision and the rectangle are visible to all 256 threads
        if (!ctl[0]) break;                                // uniform: this round and the later ones are padding
    }
    for (int q = r * 5 + tid; q < R * 5; q += 256) {       // the rounds not run: score 0, spans -1
        const int e = q / 5, c = q - e * 5;
        if (c == 0) sco[e] = 0.f;
        else spo[4 * e + c - 1] = -1;
    }
}

// the host's checks of the windows -> nullptr or what is wrong
static const char* dsl_check(const int32_t* x_win, const int32_t* y_win, int32_t n_pairs) {
    if (!x_win || !y_win) return "null argument";
    if (n_pairs < 1) return "need n_pairs >= 1";
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t m = x_win[2 * p + 1], L = y_win[2 * p + 1];
        if (m < 0 || L < 0) return "a window has a negative length";
        if (m > DSL_MAX_LEN || L > DSL_MAX_LEN) return "a window has at most 65536 rows";
    }
    return nullptr;
}

extern "C" int64_t sylber_dtw_strings_local_workspace_bytes(const int32_t* x_win_host, const int32_t* y_win_host, int32_t n_pairs) {
    if (dsl_check(x_win_host, y_win_host, n_pairs)) return -1;
    int64_t bytes = dsl_table_bytes(n_pairs);              // the pairs' table | per pair: its two rows; every round uses them again
    for (int64_t p = 0; p < n_pairs; ++p) bytes += dsl_rows_bytes(x_win_host[2 * p + 1], y_win_host[2 * p + 1]);
    return bytes;
}

static int dsl_run(const float* x_dev, int32_t x_rows, const float* x_norm_dev, const float* y_dev, int32_t y_rows, const float* y_norm_dev,
                   int32_t D, int32_t metric, const int32_t* x_win_host, const int32_t* y_win_host, const int32_t* sep_host, int32_t n_pairs,
                   float radius, float gap, float min_score, int32_t n_best, float* scores_dev, int32_t* spans_dev, void* workspace_dev,
                   void* stream) {
    static const char* what = "sylber_dtw_strings_local";
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first device call
    if (!x_dev || !y_dev || !scores_dev || !spans_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (D < 16 || D % 16) { syl_set_error(what, "need D a multiple of 16"); return 1; }
    if (metric != SYLBER_KNN_L2 && metric != SYLBER_KNN_IP) { syl_set_error(what, "unknown metric"); return 1; }
    if (metric == SYLBER_KNN_L2 && (!x_norm_dev || !y_norm_dev)) { syl_set_error(what, "the L2 metric needs x_norm_dev and y_norm_dev"); return 1; }
    if (const char* bad = dsl_check(x_win_host, y_win_host, n_pairs)) { syl_set_error(what, bad); return 1; }
    if (!std::isfinite(radius) || !(radius > 0.f)) { syl_set_error(what, "need a finite radius > 0"); return 1; }
    if (!std::isfinite(gap) || !(gap >= 0.f)) { syl_set_error(what, "need a finite gap >= 0"); return 1; }
    if (!std::isfinite(min_score) || !(min_score > 0.f)) { syl_set_error(what, "need a finite min_score > 0"); return 1; }
    if (n_best < 1 || n_best > DSL_MAX_BEST) { syl_set_error(what, "need 1 <= n_best <= 32"); return 1; }
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t xa = x_win_host[2 * p], ya = y_win_host[2 * p];
        if (xa < 0 || ya < 0 || xa + x_win_host[2 * p + 1] > x_rows || ya + y_win_host[2 * p + 1] > y_rows) {
            syl_set_error(what, "a window lies outside its buffer"); return 1;
        }
        if (sep_host && sep_host[p] < 0) { syl_set_error(what, "sep must not be negative"); return 1; }
    }
    // where each pair's slice lies: host arithmetic on the lengths
    std::vector<int64_t> tab((size_t)n_pairs * DSL_TAB);
    int64_t at = dsl_table_bytes(n_pairs);
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t m = x_win_host[2 * p + 1], L = y_win_host[2 * p + 1];
        int64_t* e = tab.data() + (size_t)p * DSL_TAB;
        e[0] = x_win_host[2 * p]; e[1] = m; e[2] = y_win_host[2 * p]; e[3] = L;
        e[4] = at; at += dsl_rows_bytes(m, L);
        e[5] = sep_host ? sep_host[p] : 0; e[6] = 0; e[7] = 0;
    }
    // the table is pageable host memory: the copy is staged before the call returns, in stream order on the device
    HIP_TRY(hipMemcpyAsync(workspace_dev, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
    const bool l2 = metric == SYLBER_KNN_L2;
    static PerDeviceOnce once;
    if (once.need())
        HIP_TRY(hipFuncSetAttribute((const void*)dtw_strings_local_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DSL_LDS_BYTES));
    hipLaunchKernelGGL(dtw_strings_local_kernel, dim3((unsigned)n_pairs), dim3(256), DSL_LDS_BYTES, s, x_dev, x_rows, l2 ? x_norm_dev : nullptr,
                       y_dev, y_rows, l2 ? y_norm_dev : nullptr, D, (const int64_t*)workspace_dev, radius, gap, min_score, n_best, scores_dev,
                       spans_dev, (char*)workspace_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_dtw_strings_local(const float* x_dev, int32_t x_rows, const float* x_norm_dev, const float* y_dev, int32_t y_rows,
                                        const float* y_norm_dev, int32_t D, int32_t metric, const int32_t* x_win_host,
                                        const int32_t* y_win_host, const int32_t* sep_host, int32_t n_pairs, float radius, float gap,
                                        float min_score, int32_t n_best, float* scores_dev, int32_t* spans_dev, void* workspace_dev,
                                        void* stream) {
    try {
        return dsl_run(x_dev, x_rows, x_norm_dev, y_dev, y_rows, y_norm_dev, D, metric, x_win_host, y_win_host, sep_host, n_pairs, radius, gap,
                       min_score, n_best, scores_dev, spans_dev, workspace_dev, stream);
    } catch (...) { syl_set_error("sylber_dtw_strings_local", "out of host memory"); return 1; }
}

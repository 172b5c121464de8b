// What the two global embedding-string kernels share (dtw_strings.hip: one workgroup per pair; dtw_strings_split.hip: one pair cut
// into blocks that run on many workgroups): the geometry, the LDS carve, the walk of a RANGE of super-strips and tiles -- the
// 128 x 128 contraction over D, dt_cost_tile, the two-wave anti-diagonal wavefront on cells of (A, n) with the 2-bit predecessor
// codes -- the padding, the walk back over the codes, and the host's checks.  One cell body and one contraction: a cell makes the
// same operations in the same order whoever calls the range, which is why the split form returns the one-workgroup kernel's bits.
// dtw_strings.hip's header describes the walk; what a range adds is where its four edges come from (DsEdges below).
// Plain vector loads and stores only.
#pragma once
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "dtw_tile.h"

constexpr int DS_MAX_LEN = 65536;
constexpr int DS_TAB = 8;                                 // int64 per pair: x row, m, y row, L, byte offsets of its hand-over state and of the codes, x's flat row in rows_dev, 0
constexpr int DS_STRIP = 64;                              // x rows of a strip: one per lane
constexpr unsigned DS_DIAG = 0, DS_UP = 1, DS_LEFT = 2;
constexpr int DS_LDS_FLOATS = KN_BM * DT_LD + KN_BN + 2 * 2 * KN_BN + 4;     // cost tile | c_j | upper rows of waves 0 and 1 | the last cell
constexpr size_t DS_LDS_BYTES = (size_t)DS_LDS_FLOATS * 4;

static_assert(KN_BM == 2 * DS_STRIP && KN_BN == 128, "a super-strip is two strips, a lane's codes of a tile are four 64-bit words");
static_assert(KN_STAGE <= KN_BM * DT_LD, "the cost tile covers the staging it aliases");
static_assert((KN_BM * DT_LD + KN_BN) * 4 % 8 == 0, "the upper rows are 8-byte cells");

// lane l: v of lane l - 1 (lane 0: its own), DPP wave_shr:1
__device__ __forceinline__ int ds_above(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ float ds_above(float v) { return __int_as_float(ds_above(__float_as_int(v))); }

static inline int64_t ds_codes_bytes(int64_t m, int64_t L) {
    return m > 0 && L > 0 ? (m + DS_STRIP - 1) / DS_STRIP * ((L + KN_BN - 1) / KN_BN) * 2048 : 0;
}
static inline int64_t ds_table_bytes(int32_t n_pairs) { return kn_al((int64_t)n_pairs * DS_TAB * 8); }

// A workgroup's dynamic LDS, DS_LDS_BYTES
struct DsLds {
    float* xs;                                             // staging of the x rows
    float* cs;                                             // staging of the y rows
    float* dm;                                             // [128][DT_LD] local costs of the tile, aliasing the staging
    float* cns;                                            // [128] c_j of the tile's columns
    int2* up0;                                             // [128] (A, n) of the row above wave 0's strip, this tile's columns
    int2* up1;                                             // [128] the same above wave 1's strip: wave 0's last row
    int* fin;                                              // (A, n) of the cell (m-1, L-1)
    __device__ __forceinline__ DsLds(float* smem) {
        xs = smem; cs = smem + KN_BM * KN_LD; dm = smem;
        cns = smem + KN_BM * DT_LD;
        up0 = (int2*)(cns + KN_BN); up1 = up0 + KN_BN;
        fin = (int*)(up1 + KN_BN);
    }
};

// A pair's windows as the kernels take them from its table entry: what the host checked and wrote, clamped into the buffers all the same
struct DsPair {
    int64_t xo, yo, ro;
    int m, L;
    __device__ __forceinline__ DsPair(const int64_t* t_, int x_rows, int y_rows) {
        xo = t_[0] < 0 ? 0 : (t_[0] < x_rows ? t_[0] : x_rows); yo = t_[2] < 0 ? 0 : (t_[2] < y_rows ? t_[2] : y_rows); ro = t_[6];
        const int64_t mw = x_rows - xo < DS_MAX_LEN ? x_rows - xo : DS_MAX_LEN, Lw = y_rows - yo < DS_MAX_LEN ? y_rows - yo : DS_MAX_LEN;
        m = (int)(t_[1] < 0 ? 0 : (t_[1] < mw ? t_[1] : mw)); L = (int)(t_[3] < 0 ? 0 : (t_[3] < Lw ? t_[3] : Lw));
    }
};

// The range of a walk, super-strips [ss_lo, ss_hi) by tiles [tile_lo, tile_hi) on the pair's global 128 / 128 grid, and its edges;
// all of it workgroup-uniform.  The one-workgroup kernel walks the whole pair: every edge is the edge of the matrix.
//   inner:  two alternating rows of L cells, by the parity of the super-strip, between the super-strips of the range
//   top:    the row above super-strip ss_lo by global column, null: the +inf row above the matrix      (SPLIT)
//   bottom: where super-strip ss_hi - 1 leaves its last row when x goes on below it                   (SPLIT)
//   left:   the column left of tile_lo as [1 + rows of the range] cells, null: column -1, +inf.  left[0] is the corner, the cell
//           above its first row; left[1 + r] belongs to row ss_lo * 128 + r                           (SPLIT)
//   right:  where the range leaves its last column in that form, null: nobody reads it               (SPLIT)
// A lane takes A[i][left column] as its last cell; lane 0 of a strip takes the cell above that as the previous cell of the row
// above: left[0] for the range's first strip, the left column's own cell for every other.  The cell before the lane's last one
// (a_prev) is never read: the lane above has always finished a cell of the tile before the lane below reads its a_prev.
struct DsEdges {
    int ss_lo, ss_hi, tile_lo, tile_hi;
    int2* inner;
    const int2* top;
    int2* bottom;
    const int2* left;
    int2* right;
};

// All 256 threads: the cells of the range, every local cost and every cell with the operations of dtw_strings.hip's header.  Writes
// the edges, PATH: the code words by global (strip, tile), and S.fin when the range holds the cell (m-1, L-1); ends behind a fence
// and a barrier.
template <bool PATH, bool SPLIT>
__device__ __forceinline__ void ds_walk_range(const DsLds& S, const float* __restrict__ x, const float* __restrict__ xn, const float* __restrict__ y,
                                              const float* __restrict__ cn, int D, const DsPair& P, const DsEdges& e, uint64_t* codes) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int m = P.m, L = P.L;
    const int64_t xo = P.xo, yo = P.yo;
    const bool l2 = xn != nullptr;
    const int SS = (m + KN_BM - 1) / KN_BM, tiles = (L + KN_BN - 1) / KN_BN;
    const int sr = tid >> 1, sh = (tid & 1) * 8;
    float* xdst = S.xs + sr * KN_LD + (sh >> 1);
    float* cdst = S.cs + sr * KN_LD + (sh >> 1);
    float* const dm = S.dm;
    float* const cns = S.cns;
    int2* const up0 = S.up0;
    int2* const up1 = S.up1;
    const int frow = lane & 31, fh = lane >> 5;
    // the one-workgroup kernel's range is the whole pair: said here, so that nothing of the range is left to fold
    const int ss_lo = SPLIT ? e.ss_lo : 0, ss_hi = SPLIT ? e.ss_hi : SS, tile_lo = SPLIT ? e.tile_lo : 0, tile_hi = SPLIT ? e.tile_hi : tiles;
    const int ksteps = D / KN_BK, T = ksteps * (tile_hi - tile_lo);

    for (int ss = ss_lo; ss < ss_hi; ++ss) {
        const int i0 = ss * KN_BM, ms = m - i0 < KN_BM ? m - i0 : KN_BM;       // the super-strip's rows
        const bool carry = ss + 1 < SS;                    // then ms = 128 and wave 1's lane 63 holds its last row
        const bool first = SPLIT && ss == ss_lo, last = SPLIT && ss + 1 == ss_hi;
        const int2* above = first ? e.top : e.inner + (size_t)((ss + 1) & 1) * L;         // the row super-strip ss - 1 wrote
        int2* below = last ? e.bottom : e.inner + (size_t)(ss & 1) * L;                   // the row this one writes
        const bool has_above = first ? e.top != nullptr : ss > 0;
        const int rw = wave < 2 ? (ms - wave * DS_STRIP < 0 ? 0 : (ms - wave * DS_STRIP < DS_STRIP ? ms - wave * DS_STRIP : DS_STRIP)) : 0;
        const int i = i0 + wave * DS_STRIP + lane;         // the lane's row (waves 0 and 1)
        int xr = i0 + sr; xr = xr < m ? xr : m - 1;
        const float* xrow = x + (size_t)(xo + xr) * D + sh;
        bool live[2];                                      // wave-uniform: this wave's 32-row half holds x rows
        float qn[2] = {0.f, 0.f};
#pragma unroll
        for (int fm = 0; fm < 2; ++fm) {
            live[fm] = wm * 64 + fm * 32 < ms;
            int r = i0 + wm * 64 + fm * 32 + frow; r = r < m ? r : m - 1;
            if (l2) qn[fm] = xn[xo + r];
        }
        // the lane's last two cells, and lane 0's previous cell of the row above: column -1 is +inf
        float a_cur = INFINITY, a_prev = INFINITY, pa = INFINITY;
        int n_cur = 0, n_prev = 0, pn = 0;
        if constexpr (SPLIT) {
            if (e.left && lane < rw) {                     // rw > 0: waves 0 and 1
                const int2* lc = e.left + 1 + (i - ss_lo * KN_BM);
                const int2 c = lc[0];
                a_cur = __int_as_float(c.x); n_cur = c.y;
                if (lane == 0) { const int2 p = lc[-1]; pa = __int_as_float(p.x); pn = p.y; }
            }
        }

        f32x16_t acc[2][2];
        float4 xa, xb, ca, cb;
        auto fetch = [&](int t) {
            const int tile = tile_lo + t / ksteps, k0 = (t % ksteps) * KN_BK;
            int cr = tile * KN_BN + sr; cr = cr < L ? cr : L - 1;
            const float* crow = y + (size_t)(yo + cr) * D + sh + k0;
            xa = *(const float4*)(xrow + k0); xb = *(const float4*)(xrow + k0 + 4);
            ca = *(const float4*)crow; cb = *(const float4*)(crow + 4);
        };
        fetch(0);
        for (int t = 0; t < T; ++t) {
            const int tile = tile_lo + t / ksteps, ks = t % ksteps, n0 = tile * KN_BN;
            if (ks == 0) kn_zero(acc);
            __syncthreads();                               // previous fragments, the cost tile, cns and the upper rows are all read
            kn_stage(xdst, cdst, xa, xb, ca, cb);
            if (ks == 0 && tid < KN_BN) {
                const int j = n0 + tid;
                cns[tid] = (cn && j < L) ? cn[yo + j] : 0.f;
                up0[tid] = (has_above && j < L) ? above[j] : make_int2(__float_as_int(INFINITY), 0);
            }
            __syncthreads();
            if (t + 1 < T) fetch(t + 1);
            kn_mma(S.xs, S.cs, wm, wn, frow, fh, acc, live[0], live[1]);
            if (ks != ksteps - 1) continue;
            __syncthreads();                               // every wave is past its fragment reads: the cost tile aliases the staging
            dt_cost_tile(dm, cns, acc, l2, qn, live, wm, wn, frow, fh);
            const int ncol = L - n0 < KN_BN ? L - n0 : KN_BN;
            // wave 0 walks the upper strip, then, behind a barrier, wave 1 the lower one: wave 0's lane 63 has left its row in up1
#pragma unroll 1
            for (int w = 0; w < 2; ++w) {
                __syncthreads();
                if (wave != w || rw == 0) continue;        // wave-uniform
                const float* dr = dm + (w * DS_STRIP + lane) * DT_LD;
                const int2* upr = w ? up1 : up0;
                const bool hands = w == 0 && ms > DS_STRIP && lane == DS_STRIP - 1;       // the row above wave 1's strip
                const bool keeps = carry && w == 1 && lane == DS_STRIP - 1;               // the row above the next super-strip
                uint64_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
                for (int st = 0; st < ncol + rw - 1; ++st) {
                    float ua = ds_above(a_cur), uap = ds_above(a_prev);     // A[i-1][j], A[i-1][j-1] where this lane works on column j
                    int un = ds_above(n_cur), unp = ds_above(n_prev);
                    const int j = st - lane;
                    if (lane < rw && j >= 0 && j < ncol) {
                        if (lane == 0) {
                            const int2 u = upr[j];
                            ua = __int_as_float(u.x); un = u.y; uap = pa; unp = pn;
                            pa = ua; pn = un;
                        }
                        float best = uap;                  // (i-1, j-1), then (i-1, j), then (i, j-1): the first smallest
                        int nb = unp;
                        unsigned code = DS_DIAG;
                        if (ua < best) { best = ua; nb = un; code = DS_UP; }
                        if (a_cur < best) { best = a_cur; nb = n_cur; code = DS_LEFT; }
                        const bool origin = i == 0 && n0 + j == 0;
                        const float A = origin ? dr[j] : dr[j] + best;
                        const int n = origin ? 1 : nb + 1;
                        a_prev = a_cur; n_prev = n_cur; a_cur = A; n_cur = n;
                        if (hands) up1[j] = make_int2(__float_as_int(A), n);
                        if (keeps) below[n0 + j] = make_int2(__float_as_int(A), n);
                        if constexpr (PATH) {
                            const uint64_t bits = (uint64_t)code << (2 * (j & 31));
                            const int q = j >> 5;
                            w0 |= q == 0 ? bits : 0; w1 |= q == 1 ? bits : 0; w2 |= q == 2 ? bits : 0; w3 |= q == 3 ? bits : 0;
                        }
                    }
                }
                if constexpr (PATH) {
                    uint64_t* wp = codes + ((size_t)(ss * 2 + w) * tiles + tile) * 256 + lane;
                    wp[0] = w0; wp[64] = w1; wp[128] = w2; wp[192] = w3;
                }
                if constexpr (SPLIT) {
                    if (e.right && tile + 1 == tile_hi) {                // the range's last column: every lane's last cell
                        int2* rc = e.right + 1 + (i - ss_lo * KN_BM);
                        if (lane < rw) rc[0] = make_int2(__float_as_int(a_cur), n_cur);
                        if (first && w == 0 && lane == 0) rc[-1] = make_int2(__float_as_int(pa), pn);     // the corner of the range to the right
                    }
                }
            }
        }
        if (ss + 1 == SS && (!SPLIT || tile_hi == tiles) && wave == (((m - 1) >> 6) & 1) && lane == ((m - 1) & 63)) {
            S.fin[0] = __float_as_int(a_cur); S.fin[1] = n_cur;
        }
        __threadfence_block();
        __syncthreads();                                   // the super-strip's row and words are written and visible to the workgroup
    }
}

// all 256 threads of a padding pair's workgroup: what the contract says of an empty side and of a cost not below +inf
template <bool PATH>
__device__ __forceinline__ void ds_padding(const DsPair& P, size_t pair, int2* __restrict__ rows, int32_t* __restrict__ steps,
                                           float* __restrict__ cost, int32_t* __restrict__ steps_walk) {
    const int tid = threadIdx.x;
    if constexpr (PATH)
        for (int i = tid; i < P.m; i += 256) rows[P.ro + i] = make_int2(-1, -1);
    if (tid == 0) {
        cost[pair] = INFINITY; steps[pair] = 0;
        if (PATH && steps_walk) steps_walk[pair] = 0;
    }
}

// all 256 threads, behind whatever makes the pair's code words visible to them: the outputs of a pair whose last cell is (A, n).
// Thread 0 follows the codes from (m-1, L-1) to (0, 0) -- at most m + L - 1 cells -- and writes the runs.
template <bool PATH>
__device__ __forceinline__ void ds_finish(const DsPair& P, size_t pair, float A, int n, const uint64_t* codes, int2* __restrict__ rows,
                                          int32_t* __restrict__ steps, float* __restrict__ cost, int32_t* __restrict__ steps_walk) {
    if (!(A < INFINITY)) { ds_padding<PATH>(P, pair, rows, steps, cost, steps_walk); return; }    // a path through a +inf cell is no path
    if (threadIdx.x != 0) return;
    cost[pair] = A; steps[pair] = n;
    if constexpr (PATH) {
        const int m = P.m, L = P.L, tiles = (L + KN_BN - 1) / KN_BN;
        const int64_t ro = P.ro;
        int i = m - 1, j = L - 1, hi = L, cells = 1;
        int hq = -1, hrow = -1;                            // the quarter-tile and the row of the word held
        uint64_t word = 0;
        // every step takes i or j down and a step out of the matrix is bent along its edge, so the walk ends in (0, 0) after at
        // most m + L - 2 steps whatever the codes are; the bound only says so again
        for (int guard = m + L; (i > 0 || j > 0) && guard > 0; --guard) {
            if ((j >> 5) != hq || i != hrow) {
                word = codes[((size_t)(i >> 6) * tiles + (j >> 7)) * 256 + ((j >> 5) & 3) * 64 + (i & 63)];
                hq = j >> 5; hrow = i;
            }
            unsigned code = (unsigned)(word >> (2 * (j & 31))) & 3u;
            if (i == 0) code = DS_LEFT;
            else if (j == 0) code = DS_UP;
            if (code == DS_LEFT) --j;
            else {
                rows[ro + i] = make_int2(j, hi);
                --i;
                if (code != DS_UP) --j;
                hi = j + 1;
            }
            ++cells;
        }
        rows[ro] = make_int2(0, hi);
        if (steps_walk) steps_walk[pair] = cells;
    }
}

// ---- the host's checks, shared by the two entries ---------------------------------------------------------------------------------
// the windows -> nullptr or what is wrong
static inline const char* ds_check(const int32_t* x_win, const int32_t* y_win, int32_t n_pairs, int32_t path) {
    if (!x_win || !y_win) return "null argument";
    if (n_pairs < 1) return "need n_pairs >= 1";
    if (path != 0 && path != 1) return "path is 0 or 1";
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t m = x_win[2 * p + 1], L = y_win[2 * p + 1];
        if (m < 0 || L < 0) return "a window has a negative length";
        if (m > DS_MAX_LEN || L > DS_MAX_LEN) return "a window has at most 65536 rows";
    }
    return nullptr;
}

// every argument of an entry -> nullptr or what is wrong; no device call
static inline const char* ds_check_call(const float* x_dev, int32_t x_rows, const float* x_norm_dev, const float* y_dev, int32_t y_rows,
                                        const float* y_norm_dev, int32_t D, int32_t metric, const int32_t* x_win_host, const int32_t* y_win_host,
                                        int32_t n_pairs, int32_t path, const int64_t* rows_offset_host, const int32_t* rows_dev,
                                        const int32_t* steps_dev, const float* cost_dev, const void* workspace_dev) {
    if (!x_dev || !y_dev || !steps_dev || !cost_dev || !workspace_dev) return "null argument";
    if (D < 16 || D % 16) return "need D a multiple of 16";
    if (metric != SYLBER_KNN_L2 && metric != SYLBER_KNN_IP) return "unknown metric";
    if (metric == SYLBER_KNN_L2 && (!x_norm_dev || !y_norm_dev)) return "the L2 metric needs x_norm_dev and y_norm_dev";
    if (const char* bad = ds_check(x_win_host, y_win_host, n_pairs, path)) return bad;
    if (path && (!rows_offset_host || !rows_dev)) return "path needs rows_offset_host and rows_dev";
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t xa = x_win_host[2 * p], ya = y_win_host[2 * p];
        if (xa < 0 || ya < 0 || xa + x_win_host[2 * p + 1] > x_rows || ya + y_win_host[2 * p + 1] > y_rows) return "a window lies outside its buffer";
        if (path && rows_offset_host[p] < 0) return "rows_offset_host must not be negative";
    }
    return nullptr;
}

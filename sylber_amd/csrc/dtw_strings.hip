// Embedding strings (sylber_amd/search.py: align_sequences / SyllableIndex.align_sequences; contract in include/sylber_hip.h
// "Embedding strings", restated in tests/dtw_strings_ref.py): the GLOBAL DTW of two WHOLE embedding sequences of up to 65 536 rows
// on each side, many pairs per call -- cost, the cells on the path and optionally the run of y rows that every x row is warped
// onto.  unit_strings.hip's sibling on embeddings, and dtw.hip's without the 64-row limit of a phrase: there one wave holds a whole
// phrase, here x is cut into strips of 64 rows that waves 0 and 1 take in turn.
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
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "dtw_tile.h"
#include <vector>

constexpr int DS_MAX_LEN = 65536;
constexpr int DS_TAB = 8;                                 // int64 per pair: x row, m, y row, L, byte offsets of the two rows and of the codes, x's flat row in rows_dev, 0
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

static inline int64_t ds_rows_bytes(int64_t m, int64_t L) { return m > KN_BM && L > 0 ? kn_al(2 * 8 * L) : 0; }
static inline int64_t ds_codes_bytes(int64_t m, int64_t L) {
    return m > 0 && L > 0 ? (m + DS_STRIP - 1) / DS_STRIP * ((L + KN_BN - 1) / KN_BN) * 2048 : 0;
}
static inline int64_t ds_table_bytes(int32_t n_pairs) { return kn_al((int64_t)n_pairs * DS_TAB * 8); }

// Workgroup `pair`: rows tab[0] .. + tab[1] of x [*, D] against rows tab[2] .. + tab[3] of y [*, D]; xn / cn: their ||row||^2 (L2)
// or null; tab[4], tab[5]: where in ws its two rows and its codes lie; tab[6]: x's flat row in rows.  Writes cost, steps [pairs] and,
// PATH, rows [*, 2] and steps_walk where it is not null.
template <bool PATH>
__global__ __launch_bounds__(256) void dtw_strings_kernel(const float* __restrict__ x, int x_rows, const float* __restrict__ xn,
                                                          const float* __restrict__ y, int y_rows, const float* __restrict__ cn, int D,
                                                          const int64_t* __restrict__ tab,
                                                          int2* __restrict__ rows, int32_t* __restrict__ steps, float* __restrict__ cost,
                                                          int32_t* __restrict__ steps_walk, char* ws) {
    extern __shared__ __attribute__((aligned(16))) float ds_smem[];
    float* xs = ds_smem;                                   // staging of the x rows
    float* cs = ds_smem + KN_BM * KN_LD;                   // staging of the y rows
    float* dm = ds_smem;                                   // [128][DT_LD] local costs of the tile, aliasing the staging
    float* cns = ds_smem + KN_BM * DT_LD;                  // [128] c_j of the tile's columns
    int2* up0 = (int2*)(cns + KN_BN);                      // [128] (A, n) of the row above wave 0's strip, this tile's columns
    int2* up1 = up0 + KN_BN;                               // [128] the same above wave 1's strip: wave 0's last row
    int* fin = (int*)(up1 + KN_BN);                        // (A, n) of the cell (m-1, L-1)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const size_t pair = blockIdx.x;
    const int64_t* t_ = tab + pair * DS_TAB;               // workgroup-uniform, as all that follows from it
    // the table is what the host checked and wrote; the windows are clamped into their buffers all the same
    const int64_t xo = t_[0] < 0 ? 0 : (t_[0] < x_rows ? t_[0] : x_rows), yo = t_[2] < 0 ? 0 : (t_[2] < y_rows ? t_[2] : y_rows), ro = t_[6];
    const int64_t mw = x_rows - xo < DS_MAX_LEN ? x_rows - xo : DS_MAX_LEN, Lw = y_rows - yo < DS_MAX_LEN ? y_rows - yo : DS_MAX_LEN;
    const int m = (int)(t_[1] < 0 ? 0 : (t_[1] < mw ? t_[1] : mw)), L = (int)(t_[3] < 0 ? 0 : (t_[3] < Lw ? t_[3] : Lw));
    if (m == 0 || L == 0) {                                // padding: what the contract says of an empty side
        if constexpr (PATH)
            for (int i = tid; i < m; i += 256) rows[ro + i] = make_int2(-1, -1);
        if (tid == 0) {
            cost[pair] = INFINITY; steps[pair] = 0;
            if (PATH && steps_walk) steps_walk[pair] = 0;
        }
        return;
    }
    int2* carried = (int2*)(ws + t_[4]);
    uint64_t* codes = (uint64_t*)(ws + t_[5]);
    const bool l2 = xn != nullptr;
    const int SS = (m + KN_BM - 1) / KN_BM, tiles = (L + KN_BN - 1) / KN_BN;
    const int sr = tid >> 1, sh = (tid & 1) * 8;
    float* xdst = xs + sr * KN_LD + (sh >> 1);
    float* cdst = cs + sr * KN_LD + (sh >> 1);
    const int frow = lane & 31, fh = lane >> 5;
    const int ksteps = D / KN_BK, T = ksteps * tiles;

    for (int ss = 0; ss < SS; ++ss) {
        const int i0 = ss * KN_BM, ms = m - i0 < KN_BM ? m - i0 : KN_BM;       // the super-strip's rows
        const bool carry = ss + 1 < SS;                    // then ms = 128 and wave 1's lane 63 holds its last row
        const int2* above = carried + (size_t)((ss + 1) & 1) * L;             // the row super-strip ss - 1 wrote
        int2* below = carried + (size_t)(ss & 1) * L;                         // the row this one writes
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

        f32x16_t acc[2][2];
        float4 xa, xb, ca, cb;
        auto fetch = [&](int t) {
            const int tile = t / ksteps, k0 = (t % ksteps) * KN_BK;
            int cr = tile * KN_BN + sr; cr = cr < L ? cr : L - 1;
            const float* crow = y + (size_t)(yo + cr) * D + sh + k0;
            xa = *(const float4*)(xrow + k0); xb = *(const float4*)(xrow + k0 + 4);
            ca = *(const float4*)crow; cb = *(const float4*)(crow + 4);
        };
        fetch(0);
        for (int t = 0; t < T; ++t) {
            const int tile = t / ksteps, ks = t % ksteps, n0 = tile * KN_BN;
            if (ks == 0) kn_zero(acc);
            __syncthreads();                               // previous fragments, the cost tile, cns and the upper rows are all read
            kn_stage(xdst, cdst, xa, xb, ca, cb);
            if (ks == 0 && tid < KN_BN) {
                const int j = n0 + tid;
                cns[tid] = (cn && j < L) ? cn[yo + j] : 0.f;
                up0[tid] = (ss > 0 && j < L) ? above[j] : make_int2(__float_as_int(INFINITY), 0);
            }
            __syncthreads();
            if (t + 1 < T) fetch(t + 1);
            kn_mma(xs, cs, wm, wn, frow, fh, acc, live[0], live[1]);
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
            }
        }
        if (ss + 1 == SS && wave == (((m - 1) >> 6) & 1) && lane == ((m - 1) & 63)) { fin[0] = __float_as_int(a_cur); fin[1] = n_cur; }
        __threadfence_block();
        __syncthreads();                                   // the super-strip's row and words are written and visible to the workgroup
    }

    const float A = __int_as_float(fin[0]);
    const int n = fin[1];
    if (!(A < INFINITY)) {                                 // padding: a path through a +inf cell is no path
        if constexpr (PATH)
            for (int i = tid; i < m; i += 256) rows[ro + i] = make_int2(-1, -1);
        if (tid == 0) {
            cost[pair] = INFINITY; steps[pair] = 0;
            if (PATH && steps_walk) steps_walk[pair] = 0;
        }
        return;
    }
    if (tid != 0) return;
    cost[pair] = A; steps[pair] = n;
    if constexpr (PATH) {
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

// the host's checks of the windows -> nullptr or what is wrong
static const char* ds_check(const int32_t* x_win, const int32_t* y_win, int32_t n_pairs, int32_t path) {
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
    if (!x_dev || !y_dev || !steps_dev || !cost_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (D < 16 || D % 16) { syl_set_error(what, "need D a multiple of 16"); return 1; }
    if (metric != SYLBER_KNN_L2 && metric != SYLBER_KNN_IP) { syl_set_error(what, "unknown metric"); return 1; }
    if (metric == SYLBER_KNN_L2 && (!x_norm_dev || !y_norm_dev)) { syl_set_error(what, "the L2 metric needs x_norm_dev and y_norm_dev"); return 1; }
    if (const char* bad = ds_check(x_win_host, y_win_host, n_pairs, path)) { syl_set_error(what, bad); return 1; }
    if (path && (!rows_offset_host || !rows_dev)) { syl_set_error(what, "path needs rows_offset_host and rows_dev"); return 1; }
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t xa = x_win_host[2 * p], ya = y_win_host[2 * p];
        if (xa < 0 || ya < 0 || xa + x_win_host[2 * p + 1] > x_rows || ya + y_win_host[2 * p + 1] > y_rows) {
            syl_set_error(what, "a window lies outside its buffer"); return 1;
        }
        if (path && rows_offset_host[p] < 0) { syl_set_error(what, "rows_offset_host must not be negative"); return 1; }
    }
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

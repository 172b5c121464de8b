// Unit strings (sylber_amd/units.py: align_unit_strings / unit_error_rate; contract in include/sylber_hip.h "Unit strings", restated
// in tests/unit_strings_ref.py): the global alignment of WHOLE unit strings of any length up to 65 536 units on each side, many
// pairs per call -- the operation counts, optionally the pairing of every reference unit, and from them the unit error rate of two
// tokenisations.  unit_align.hip's sibling without its 64-unit limit: there one lane holds one phrase unit of one wave, here the
// reference is cut into strips of 64 rows that the same wave takes one after another (unit_strip.h).
//   * unit_strings_kernel<WP, PAIRING>: one wave per pair walks the strips.
//     A cell is (cost, d, sb): d = the diagonal steps on the path that the chosen predecessor tracked, sb = those of them with
//     sub > 0; both are 0 on row -1 and on column -1.  So equal = d - sb, substituted = sb, deleted = m - d, inserted = L - d fall
//     out of the last cell and the counts need no path: the counts-only kernel writes no predecessor codes.
//     PAIRING: each lane also packs the 2-bit predecessor codes of a chunk of 32 STEPS into one 64-bit word and the wave stores a
//     chunk's words as one coalesced row: [strip][chunks of L + 63 steps][64] words, about m L / 4 bytes; cell (i, j) is bits
//     2 ((i % 64 + j) % 32) .. + 1 of word [i / 64][(i % 64 + j) / 32][i % 64].  After the last strip, whose fence and barrier make
//     the words visible, lane 0 follows the codes from (m-1, L-1) back across the strips -- at most m + L cells -- and writes
//     cols / subs straight to their flat outputs; it counts its own (equal, substituted, deleted, inserted) and hands them out
//     where the caller asks for them: tests hold them against the carried counters, i.e. the codes against the cells that formed
//     them.
//     Plain vector loads and stores only.
// LDS: 4 KiB of ring at WP = 8, 64 threads: wave slots bound the occupancy.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "unit_strip.h"

constexpr int UT_TAB = UST_TAB + 1;                       // int64 per pair: UST_TAB, byte offset of the codes
constexpr unsigned UT_DIAG = 0, UT_UP = 1, UT_LEFT = 2;

static_assert(2 * UST_CH == 64, "the 2-bit codes of a lane's chunk fill one 64-bit word");

// the chunks of a strip against L columns: at most L + 63 steps
__host__ __device__ static inline int64_t ut_chunks(int64_t L) { return (L + UST_ROWS - 1 + UST_CH - 1) / UST_CH; }
static inline int64_t ut_codes_bytes(int64_t m, int64_t L) { return m > 0 && L > 0 ? (m + UST_ROWS - 1) / UST_ROWS * ut_chunks(L) * 64 * 8 : 0; }

// The cell of the global alignment; PAIRING: word = the codes of the lane's chunk so far, wp = the words of the strip.
template <bool PAIRING>
struct ut_cell {
    int W;
    uint64_t* wp = nullptr;
    uint64_t word = 0;
    // column -1: (i + 1) W without a diagonal step; the first diagonal: i W (row 0: the corner, 0); row -1: (j + 1) W
    __device__ __forceinline__ ust_cell left(int i) const { return {(i + 1) * W, 0, 0}; }
    __device__ __forceinline__ ust_cell diag(int i) const { return {i * W, 0, 0}; }
    __device__ __forceinline__ ust_cell top(int j) const { return {(j + 1) * W, 0, 0}; }
    __device__ __forceinline__ ust_cell step(const ust_cell& d, const ust_cell& u, const ust_cell& l, int sub, int, int, int k) {
        int best = d.a + sub, bd = d.b + 1, bsb = d.c + (sub ? 1 : 0);
        unsigned code = UT_DIAG;
        if (u.a + W < best) { best = u.a + W; bd = u.b; bsb = u.c; code = UT_UP; }
        if (l.a + W < best) { best = l.a + W; bd = l.b; bsb = l.c; code = UT_LEFT; }
        if constexpr (PAIRING) word |= (uint64_t)code << (2 * k);
        return {best, bd, bsb};
    }
    __device__ __forceinline__ void chunk_end(int chunk) {
        if constexpr (PAIRING) { wp[(size_t)chunk * 64 + threadIdx.x] = word; word = 0; }
    }
};

// Workgroup (one wave) `pair`: reference rows tab[0] .. + tab[1] of r [*, W] against hypothesis rows tab[2] .. + tab[3] of h [*, W];
// tab[4], tab[5]: where in ws its two rows and its codes lie.  Writes ops [pairs][4], cost [pairs] and, PAIRING, cols / subs at the
// reference's flat rows and ops_walk where it is not null.
template <int WP, bool PAIRING>
__global__ __launch_bounds__(64) void unit_strings_kernel(const int32_t* __restrict__ r, const int32_t* __restrict__ h, int W,
                                                          const int64_t* __restrict__ tab, int32_t* __restrict__ cols,
                                                          int32_t* __restrict__ subs, int32_t* __restrict__ ops,
                                                          int32_t* __restrict__ cost, int32_t* __restrict__ ops_walk, char* ws) {
    __shared__ __attribute__((aligned(16))) int ring[UST_RING * WP];      // [column % 128][WP] ids of the hypothesis' columns
    const int lane = threadIdx.x;
    const size_t pair = blockIdx.x;
    const int64_t* t = tab + pair * UT_TAB;                // workgroup-uniform, as all that follows from it
    const int64_t ro = t[0], ho = t[2];
    const int m = (int)t[1], L = (int)t[3];
    if (m == 0 || L == 0) {                                // no DP step: what the contract says of an empty side
        if constexpr (PAIRING)
            for (int i = lane; i < m; i += 64) { cols[ro + i] = -1; subs[ro + i] = W; }
        if (lane < 4) {
            const int v = lane == 2 ? m : lane == 3 ? L : 0;
            ops[pair * 4 + lane] = v;
            if (PAIRING && ops_walk) ops_walk[pair * 4 + lane] = v;
        }
        if (lane == 0) cost[pair] = (m + L) * W;
        return;
    }
    int32_t* rows = (int32_t*)(ws + t[4]);
    uint64_t* codes = (uint64_t*)(ws + t[5]);
    const int S = (m + UST_ROWS - 1) / UST_ROWS, nch = (int)ut_chunks(L);

    ut_cell<PAIRING> cell{W};
    ust_cell e = {0, 0, 0};                               // the lane's cell at the last column
    for (int s = 0; s < S; ++s) {
        cell.wp = codes + (size_t)s * nch * 64;
        e = ust_strip<WP>(cell, ring, r, h, W, ro, ho, m, L, rows, s, S);
    }
    const int last = (m - 1) & (UST_ROWS - 1);
    const int E = __shfl(e.a, last), D = __shfl(e.b, last), SB = __shfl(e.c, last);      // the cell (m-1, L-1)
    if (lane == 0) {
        ops[pair * 4] = D - SB; ops[pair * 4 + 1] = SB; ops[pair * 4 + 2] = m - D; ops[pair * 4 + 3] = L - D;
        cost[pair] = E;
    }
    if constexpr (PAIRING) {
        if (lane == 0) {
            int i = m - 1, j = L - 1, eq = 0, sb = 0, del = 0, ins = 0;
            int hc = -1, hi = -1;                          // the chunk and the row of the word held
            uint64_t word = 0;
            // every step takes i or j down and the walk ends at row -1 or column -1, so it sees at most m + L - 1 cells whatever
            // the codes are; the bound only says so again
            for (int guard = m + L; i >= 0 && j >= 0 && guard > 0; --guard) {
                const int li = i & (UST_ROWS - 1), st = li + j, ch = st / UST_CH;
                if (ch != hc || i != hi) { word = codes[((size_t)(i / UST_ROWS) * nch + ch) * 64 + li]; hc = ch; hi = i; }
                const unsigned code = (unsigned)(word >> (2 * (st % UST_CH))) & 3u;
                if (code == UT_LEFT) { ++ins; --j; }
                else if (code == UT_UP) { cols[ro + i] = -1; subs[ro + i] = W; ++del; --i; }
                else {
                    int sub = 0;
                    for (int c = 0; c < W; ++c) sub += r[(size_t)(ro + i) * W + c] != h[(size_t)(ho + j) * W + c] ? 1 : 0;
                    cols[ro + i] = j; subs[ro + i] = sub;
                    if (sub) ++sb; else ++eq;
                    --i; --j;
                }
            }
            for (; i >= 0; --i) { cols[ro + i] = -1; subs[ro + i] = W; ++del; }      // column -1: units 0 .. i are deletions
            if (j >= 0) ins += j + 1;                      // along row -1 to the corner: leading insertions
            if (ops_walk) { ops_walk[pair * 4] = eq; ops_walk[pair * 4 + 1] = sb; ops_walk[pair * 4 + 2] = del; ops_walk[pair * 4 + 3] = ins; }
        }
    }
}

// the host's checks of the offsets -> nullptr or what is wrong
static const char* ut_check(const int32_t* ref_off, const int32_t* hyp_off, int32_t n_pairs, int32_t pairing) {
    if (!ref_off || !hyp_off) return "null argument";
    if (n_pairs < 1) return "need n_pairs >= 1";
    if (pairing != 0 && pairing != 1) return "pairing is 0 or 1";
    if (ref_off[0] != 0 || hyp_off[0] != 0) return "offsets start at 0";
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int64_t m = (int64_t)ref_off[p + 1] - ref_off[p], L = (int64_t)hyp_off[p + 1] - hyp_off[p];
        if (m < 0 || L < 0) return "offsets must not descend";
        if (m > UST_MAX_LEN || L > UST_MAX_LEN) return "a string has at most 65536 units";
    }
    return nullptr;
}

extern "C" int64_t sylber_unit_strings_workspace_bytes(const int32_t* ref_offsets_host, const int32_t* hyp_offsets_host, int32_t n_pairs,
                                                       int32_t pairing) {
    if (ut_check(ref_offsets_host, hyp_offsets_host, n_pairs, pairing)) return -1;
    int64_t bytes = ust_table_bytes(n_pairs, UT_TAB);     // the pairs' table | per pair: its two rows, its codes
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int64_t m = ref_offsets_host[p + 1] - ref_offsets_host[p], L = hyp_offsets_host[p + 1] - hyp_offsets_host[p];
        bytes += ust_rows_bytes(m, L) + (pairing ? ut_codes_bytes(m, L) : 0);
    }
    return bytes;
}

extern "C" int sylber_unit_strings_align(const int32_t* ref_units_dev, const int32_t* ref_offsets_host, const int32_t* hyp_units_dev,
                                         const int32_t* hyp_offsets_host, int32_t W, int32_t n_pairs, int32_t pairing, int32_t* cols_dev,
                                         int32_t* subs_dev, int32_t* ops_dev, int32_t* cost_dev, int32_t* ops_walk_dev, void* workspace_dev,
                                         void* stream) {
    static const char* what = "sylber_unit_strings_align";
    return ust_entry(what, [&]() -> int {
        hipStream_t s = (hipStream_t)stream;
        // every check comes before the first device call
        if (!ref_units_dev || !hyp_units_dev || !ops_dev || !cost_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
        if (W < 1 || W > UST_MAX_W) { syl_set_error(what, "need 1 <= W <= 8"); return 1; }
        if (const char* bad = ut_check(ref_offsets_host, hyp_offsets_host, n_pairs, pairing)) { syl_set_error(what, bad); return 1; }
        if (pairing && (!cols_dev || !subs_dev)) { syl_set_error(what, "pairing needs cols_dev and subs_dev"); return 1; }
        ust_table tab(n_pairs, UT_TAB);
        for (int32_t p = 0; p < n_pairs; ++p) {
            const int64_t m = ref_offsets_host[p + 1] - ref_offsets_host[p], L = hyp_offsets_host[p + 1] - hyp_offsets_host[p];
            int64_t* e = tab.add(p, ref_offsets_host[p], m, hyp_offsets_host[p], L);
            e[5] = tab.at; tab.at += pairing ? ut_codes_bytes(m, L) : 0;
        }
        // the table is pageable host memory: the copy is staged before the call returns, in stream order on the device
        HIP_TRY(hipMemcpyAsync(workspace_dev, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
#define UT_LAUNCH(PV)                                                                                                                       \
    UST_WITH_WP(W, hipLaunchKernelGGL((unit_strings_kernel<WPV, PV>), dim3((unsigned)n_pairs), dim3(64), 0, s, ref_units_dev, hyp_units_dev, \
                                     W, (const int64_t*)workspace_dev, cols_dev, subs_dev, ops_dev, cost_dev, ops_walk_dev,                 \
                                     (char*)workspace_dev))
        if (pairing) { UT_LAUNCH(true); } else { UT_LAUNCH(false); }
#undef UT_LAUNCH
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

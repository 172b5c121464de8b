// Unit strings (sylber_amd/units.py: align_unit_strings / unit_error_rate; contract in include/sylber_hip.h "Unit strings", restated
// in tests/unit_strings_ref.py): the global alignment of WHOLE unit strings of any length up to 65 536 units on each side, many
// pairs per call -- the operation counts, optionally the pairing of every reference unit, and from them the unit error rate of two
// tokenisations.  unit_align.hip's sibling without its 64-unit limit: there one lane holds one phrase unit of one wave, here the
// reference is cut into strips of 64 rows that the same wave takes one after another.
//   * unit_strings_kernel<WP, PAIRING>: one 64-thread workgroup (one wave) per pair; nothing is handed between workgroups and
//     every loop is bounded by lengths that the host wrote down, so nothing waits and nothing can spin.  Inside strip s lane i holds
//     reference unit 64 s + i (its W ids padded to WP = 1, 2, 4 or 8 words with zeros) and walks the hypothesis on
//     unit_align_kernel's anti-diagonal wavefront: column st - i at step st, the columns through a ring of 128 columns in LDS, 32
//     new ones every 32 steps, loaded a chunk ahead.
//     A cell is (cost, d, sb): d = the diagonal steps on the path that the chosen predecessor tracked, sb = those of them with
//     sub > 0; both are 0 on row -1 and on column -1.  So equal = d - sb, substituted = sb, deleted = m - d, inserted = L - d fall
//     out of the last cell and the counts need no path: the counts-only kernel writes no predecessor codes.
//     Between strips: lane 63 of every strip but the last writes its row, 12 B per column, to one of TWO rows of the pair's slice
//     of the workspace, strips alternating, and lane 0 of the next strip takes it as its upper row: lanes 0 .. 31 load a chunk of
//     it ahead, beside the ring's columns, and at step k of the chunk lane 0 works on the very column that lane k loaded, so a
//     v_readlane hands it over; strip 0's upper row is the contract's row -1.  The lane above's cell comes through DPP
//     (wave_shr:1, VALU) and not through ds_bpermute (an LDS round trip).  A strip reads one row and writes the other, and a
//     fence and a barrier stand between strips (a workgroup's waves share one vector L1, so workgroup scope is enough; it would
//     not be between workgroups, which is why a pair stays inside one).  Only columns below L are read, and the strip before
//     wrote every one of them: nothing depends on what the workspace held.
//     One wave takes about 400 cycles per anti-diagonal step (profiles/unit_strings_bench.md: 0.37 Gcells/s on a single long
//     pair), bound by the instructions of a step and not by the exchange; several reference rows per lane is the known next step.
//     PAIRING: each lane also packs the 2-bit predecessor codes of a chunk of 32 STEPS into one 64-bit word and the wave stores a
//     chunk's words as one coalesced row: [strip][chunks of L + 63 steps][64] words, about m L / 4 bytes; cell (i, j) is bits
//     2 ((i % 64 + j) % 32) .. + 1 of word [i / 64][(i % 64 + j) / 32][i % 64].  After the last strip, a fence and a barrier,
//     lane 0 follows the codes from (m-1, L-1) back across the strips -- at most m + L cells -- and writes cols / subs straight to
//     their flat outputs; it counts its own (equal, substituted, deleted, inserted) and hands them out where the caller asks for
//     them: tests hold them against the carried counters, i.e. the codes against the cells that formed them.
//     Plain vector loads and stores only.
// LDS: 4 KiB of ring at WP = 8, 64 threads: wave slots bound the occupancy.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include <vector>

constexpr int UT_CH = 32;                                 // steps of a chunk: their 2-bit codes fill one 64-bit word
constexpr int UT_RING = 128;                              // columns of the ring: a step reads back 63 columns, a chunk is staged 32 ahead
constexpr int UT_ROWS = 64;                               // reference rows of a strip: one per lane
constexpr int UT_MAX_LEN = 65536, UT_MAX_W = 8;
constexpr int UT_TAB = 6;                                 // int64 per pair: ref row, m, hyp row, L, byte offsets of the two rows and of the codes
constexpr unsigned UT_DIAG = 0, UT_UP = 1, UT_LEFT = 2;

static_assert(2 * UT_CH == 64, "the 2-bit codes of a lane's chunk fill one 64-bit word");
static_assert(UT_RING >= UT_ROWS - 1 + 2 * UT_CH && (UT_RING & (UT_RING - 1)) == 0, "the ring holds a chunk's columns, the 63 behind them and the next chunk");

// the chunks of a strip against L columns: at most L + 63 steps
__host__ __device__ static inline int64_t ut_chunks(int64_t L) { return (L + UT_ROWS - 1 + UT_CH - 1) / UT_CH; }
// lane l: v of lane l - 1 (lane 0: its own), DPP wave_shr:1
__device__ __forceinline__ int ut_lane_above(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
static inline int64_t ut_al(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
// the two rows between strips: (cost, d, sb) per column, only where there is a second strip
static inline int64_t ut_rows_bytes(int64_t m, int64_t L) { return m > UT_ROWS && L > 0 ? ut_al(2 * 12 * L) : 0; }
static inline int64_t ut_codes_bytes(int64_t m, int64_t L) { return m > 0 && L > 0 ? (m + UT_ROWS - 1) / UT_ROWS * ut_chunks(L) * 64 * 8 : 0; }

// Workgroup (one wave) `pair`: reference rows tab[0] .. + tab[1] of r [*, W] against hypothesis rows tab[2] .. + tab[3] of h [*, W];
// tab[4], tab[5]: where in ws its two rows and its codes lie.  Writes ops [pairs][4], cost [pairs] and, PAIRING, cols / subs at the
// reference's flat rows and ops_walk where it is not null.
template <int WP, bool PAIRING>
__global__ __launch_bounds__(64) void unit_strings_kernel(const int32_t* __restrict__ r, const int32_t* __restrict__ h, int W,
                                                          const int64_t* __restrict__ tab, int32_t* __restrict__ cols,
                                                          int32_t* __restrict__ subs, int32_t* __restrict__ ops,
                                                          int32_t* __restrict__ cost, int32_t* __restrict__ ops_walk, char* ws) {
    __shared__ __attribute__((aligned(16))) int ring[UT_RING * WP];      // [column % 128][WP] ids of the hypothesis' columns
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
    const int S = (m + UT_ROWS - 1) / UT_ROWS, nch = (int)ut_chunks(L);
    const bool first = lane == 0;

    int se = 0, sd = 0, ssb = 0;                           // the cell [i][last column done]
    for (int s = 0; s < S; ++s) {
        const int i = s * UT_ROWS + lane, ms = m - s * UT_ROWS < UT_ROWS ? m - s * UT_ROWS : UT_ROWS;
        const bool valid = lane < ms, top = s == 0, carry = s + 1 < S;
        const size_t up = (size_t)((s + 1) & 1) * 3 * L, down = (size_t)(s & 1) * 3 * L;     // the row strip s - 1 wrote, the row this one writes
        uint64_t* wp = codes + (size_t)s * nch * 64;

        int pu[WP];
#pragma unroll
        for (int c = 0; c < WP; ++c) pu[c] = (valid && c < W) ? r[(size_t)(ro + i) * W + c] : 0;

        int xr[WP], ar[3] = {0, 0, 0};
        auto fetch = [&](int chunk) {                      // lanes 0 .. 31: column chunk * 32 + lane of the hypothesis and of the row above
            const int j = chunk * UT_CH + lane;
            const bool in = lane < UT_CH && j < L;
#pragma unroll
            for (int c = 0; c < WP; ++c) xr[c] = (in && c < W) ? h[(size_t)(ho + j) * W + c] : 0;
            if (!top) {
#pragma unroll
                for (int c = 0; c < 3; ++c) ar[c] = in ? rows[up + (size_t)j * 3 + c] : 0;
            }
        };

        // (se, sd, ssb) at first column -1: (i + 1) W without a diagonal step; (de, dd, dsb) = the cell [i-1][that column], the next
        // diagonal: i W (row 0: the corner, 0)
        se = (i + 1) * W; sd = 0; ssb = 0;
        int de = i * W, dd = 0, dsb = 0;
        const int nsteps = L + ms - 1, nchunks = (nsteps + UT_CH - 1) / UT_CH;
        fetch(0);
        for (int chunk = 0; chunk < nchunks; ++chunk) {
            if (lane < UT_CH) {
                const int slot = (chunk * UT_CH + lane) & (UT_RING - 1);
                int* dst = ring + slot * WP;
                if constexpr (WP == 1) dst[0] = xr[0];
                else if constexpr (WP == 2) *(int2*)dst = make_int2(xr[0], xr[1]);
                else {
#pragma unroll
                    for (int c = 0; c < WP; c += 4) *(int4*)(dst + c) = make_int4(xr[c], xr[c + 1], xr[c + 2], xr[c + 3]);
                }
            }
            __syncthreads();                               // one wave: its LDS accesses stay in order, the barrier makes the writes visible
            const int a0 = ar[0], a1 = ar[1], a2 = ar[2];  // lane k: (cost, d, sb) of column chunk * 32 + k of the row above the strip
            fetch(chunk + 1);
            uint64_t word = 0;
            const int st0 = chunk * UT_CH, ns = nsteps - st0 < UT_CH ? nsteps - st0 : UT_CH;
            for (int k = 0; k < ns; ++k) {
                int ue = ut_lane_above(se), ud = ut_lane_above(sd), usb = ut_lane_above(ssb);      // the cell [i-1][j] where this lane works on column j
                const int j = st0 + k - lane;
                if (top) {                                 // lane 0, column st0 + k: row -1, or the last row of the strip before
                    if (first) { ue = (j + 1) * W; ud = 0; usb = 0; }
                } else {
                    const int b0 = __builtin_amdgcn_readlane(a0, k), b1 = __builtin_amdgcn_readlane(a1, k), b2 = __builtin_amdgcn_readlane(a2, k);
                    if (first) { ue = b0; ud = b1; usb = b2; }
                }
                if (valid && (unsigned)j < (unsigned)L) {
                    const int* src = ring + (j & (UT_RING - 1)) * WP;
                    int x[WP];
                    if constexpr (WP == 1) x[0] = src[0];
                    else if constexpr (WP == 2) { const int2 v = *(const int2*)src; x[0] = v.x; x[1] = v.y; }
                    else {
#pragma unroll
                        for (int c = 0; c < WP; c += 4) {
                            const int4 v = *(const int4*)(src + c);
                            x[c] = v.x; x[c + 1] = v.y; x[c + 2] = v.z; x[c + 3] = v.w;
                        }
                    }
                    int sub = 0;
#pragma unroll
                    for (int c = 0; c < WP; ++c) sub += pu[c] != x[c] ? 1 : 0;
                    int best = de + sub, bd = dd + 1, bsb = dsb + (sub ? 1 : 0);
                    unsigned code = UT_DIAG;
                    if (ue + W < best) { best = ue + W; bd = ud; bsb = usb; code = UT_UP; }
                    if (se + W < best) { best = se + W; bd = sd; bsb = ssb; code = UT_LEFT; }
                    de = ue; dd = ud; dsb = usb; se = best; sd = bd; ssb = bsb;
                    if (carry && lane == UT_ROWS - 1) {
                        int32_t* dst = rows + down + (size_t)j * 3;
                        dst[0] = best; dst[1] = bd; dst[2] = bsb;
                    }
                    if constexpr (PAIRING) word |= (uint64_t)code << (2 * k);
                }
            }
            if constexpr (PAIRING) wp[(size_t)chunk * 64 + lane] = word;
        }
        __threadfence_block();
        __syncthreads();                                   // the strip's row and words are written and visible to the wave
    }
    const int last = (m - 1) & (UT_ROWS - 1);
    const int E = __shfl(se, last), D = __shfl(sd, last), SB = __shfl(ssb, last);      // the cell (m-1, L-1)
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
                const int li = i & (UT_ROWS - 1), st = li + j, ch = st / UT_CH;
                if (ch != hc || i != hi) { word = codes[((size_t)(i / UT_ROWS) * nch + ch) * 64 + li]; hc = ch; hi = i; }
                const unsigned code = (unsigned)(word >> (2 * (st % UT_CH))) & 3u;
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
        if (m > UT_MAX_LEN || L > UT_MAX_LEN) return "a string has at most 65536 units";
    }
    return nullptr;
}

static inline int64_t ut_table_bytes(int32_t n_pairs) { return ut_al((int64_t)n_pairs * UT_TAB * 8); }

extern "C" int64_t sylber_unit_strings_workspace_bytes(const int32_t* ref_offsets_host, const int32_t* hyp_offsets_host, int32_t n_pairs,
                                                       int32_t pairing) {
    if (ut_check(ref_offsets_host, hyp_offsets_host, n_pairs, pairing)) return -1;
    int64_t bytes = ut_table_bytes(n_pairs);               // the pairs' table | per pair: its two rows, its codes
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int64_t m = ref_offsets_host[p + 1] - ref_offsets_host[p], L = hyp_offsets_host[p + 1] - hyp_offsets_host[p];
        bytes += ut_rows_bytes(m, L) + (pairing ? ut_codes_bytes(m, L) : 0);
    }
    return bytes;
}

static int ut_run(const int32_t* ref_units_dev, const int32_t* ref_offsets_host, const int32_t* hyp_units_dev,
                  const int32_t* hyp_offsets_host, int32_t W, int32_t n_pairs, int32_t pairing, int32_t* cols_dev, int32_t* subs_dev,
                  int32_t* ops_dev, int32_t* cost_dev, int32_t* ops_walk_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_unit_strings_align";
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first device call
    if (!ref_units_dev || !hyp_units_dev || !ops_dev || !cost_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (W < 1 || W > UT_MAX_W) { syl_set_error(what, "need 1 <= W <= 8"); return 1; }
    if (const char* bad = ut_check(ref_offsets_host, hyp_offsets_host, n_pairs, pairing)) { syl_set_error(what, bad); return 1; }
    if (pairing && (!cols_dev || !subs_dev)) { syl_set_error(what, "pairing needs cols_dev and subs_dev"); return 1; }
    // where each pair's slice lies: host arithmetic on the lengths
    std::vector<int64_t> tab((size_t)n_pairs * UT_TAB);
    int64_t at = ut_table_bytes(n_pairs);
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int64_t m = ref_offsets_host[p + 1] - ref_offsets_host[p], L = hyp_offsets_host[p + 1] - hyp_offsets_host[p];
        int64_t* e = tab.data() + (size_t)p * UT_TAB;
        e[0] = ref_offsets_host[p]; e[1] = m; e[2] = hyp_offsets_host[p]; e[3] = L;
        e[4] = at; at += ut_rows_bytes(m, L);
        e[5] = at; at += pairing ? ut_codes_bytes(m, L) : 0;
    }
    // the table is pageable host memory: the copy is staged before the call returns, in stream order on the device
    HIP_TRY(hipMemcpyAsync(workspace_dev, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
    const int wp = W == 1 ? 1 : W == 2 ? 2 : W <= 4 ? 4 : 8;
#define UT_LAUNCH(WPV, PV)                                                                                                                  \
    hipLaunchKernelGGL((unit_strings_kernel<WPV, PV>), dim3((unsigned)n_pairs), dim3(64), 0, s, ref_units_dev, hyp_units_dev, W,            \
                       (const int64_t*)workspace_dev, cols_dev, subs_dev, ops_dev, cost_dev, ops_walk_dev, (char*)workspace_dev)
    if (pairing) {
        switch (wp) {
        case 1: UT_LAUNCH(1, true); break;
        case 2: UT_LAUNCH(2, true); break;
        case 4: UT_LAUNCH(4, true); break;
        default: UT_LAUNCH(8, true); break;
        }
    } else {
        switch (wp) {
        case 1: UT_LAUNCH(1, false); break;
        case 2: UT_LAUNCH(2, false); break;
        case 4: UT_LAUNCH(4, false); break;
        default: UT_LAUNCH(8, false); break;
        }
    }
#undef UT_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_unit_strings_align(const int32_t* ref_units_dev, const int32_t* ref_offsets_host, const int32_t* hyp_units_dev,
                                         const int32_t* hyp_offsets_host, int32_t W, int32_t n_pairs, int32_t pairing, int32_t* cols_dev,
                                         int32_t* subs_dev, int32_t* ops_dev, int32_t* cost_dev, int32_t* ops_walk_dev, void* workspace_dev,
                                         void* stream) {
    try {
        return ut_run(ref_units_dev, ref_offsets_host, hyp_units_dev, hyp_offsets_host, W, n_pairs, pairing, cols_dev, subs_dev, ops_dev,
                      cost_dev, ops_walk_dev, workspace_dev, stream);
    } catch (...) { syl_set_error("sylber_unit_strings_align", "out of host memory"); return 1; }
}

// Unit search: phrases of syllable unit ids against every sequence of a UnitIndex by semi-global edit distance (Sellers'
// approximate string matching; sylber_amd/units.py: UnitIndex.search_phrases / search_occurrences; contract in
// include/sylber_hip.h, restated in tests/unit_search_ref.py).  A unit is a row of W int32 ids; a substitution costs the number of
// columns that differ, an insertion or a deletion W.  All arithmetic is int32, so every result is exact.
//   * unit_scan_kernel<WP, OCC>: grid (phrase blocks) x C database cuts.  A phrase block holds whole phrases in 256 packed rows,
//     four waves of 64; a phrase lies inside one wave.  A cut is a run of whole sequences.  The workgroup stages a tile of
//     US_TILE columns into LDS (the W ids padded to WP = 1, 2, 4 or 8 words with zeros on both sides, which differ nowhere; a
//     start / end flag; the sequence; its group) and ALL four waves walk it on dt_wavefront's anti-diagonal wavefront: lane l
//     holds one phrase row i with its ids in registers and works on column st - i at step st.  A cell is one word (cost and
//     start packed, see the body): [i-1][j] is the last result of lane l - 1, fetched every step; [i-1][j-1] is what the lane
//     fetched at its previous column, so one exchange of one word per step carries both.  A lane that is through the tile keeps
//     its state for the next one.  The three predecessors compete with their rank (0 diagonal, 1 upper, 2 left) under the cost
//     in one min3, which is the contract's order on ties.  A sequence start puts the column -1 boundary (i + 1) W in place of
//     the left and diagonal terms.  The local cost is WP compares, no contraction: no
//     wave waits for a matrix unit, unlike the DTW scans.
//     At a sequence end (OCC: whenever the pending occurrence is pushed out) the lane of a phrase's last row hands
//     (cost, sequence or start row, span) to the phrase's sorted top-k list in LDS through kn_insert_t; costs are at most 512, so
//     they are exact as the floats the list helpers carry.
//   * knn_merge_kernel<true> (knn_lists.h) through dt_occ_merge (dtw_occ.h) merges the C partial lists of a phrase;
//     unit_finish_kernel reports int32 costs, padding (INT_MAX, -1, (-1, -1)).
// The two entry points differ in the template argument alone: us_run<OCC> holds the checks, the plan and the launches.  A bit-parallel
// (Myers) pre-scan that skips sequences without an admissible column is the known next step and is not here.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "knn_lists.h"
#include "dtw_occ.h"
#include <climits>
#include <vector>

constexpr int US_TILE = 256;                              // columns of a tile: one per thread of the staging (units.py: TILE_COLS)
constexpr int US_ROWS = 256;                              // packed phrase rows of a workgroup: 4 waves x 64
constexpr int US_MAX_W = 8, US_MAX_M = 64, US_MAX_SEQ = 65536;
constexpr int US_LIST_BYTES = 65536;                      // LDS of a workgroup's lists, 16 B per entry: 32 phrases at k = 128
constexpr int US_TARGET_BLOCKS = 2048;                    // automatic cuts: (phrase blocks) x C >= 8 workgroups per CU (the DP is latency bound)
constexpr int US_MIN_TILES = 4;                           // ... of no less than 4 tiles on average

static inline int us_fixed_bytes(int wp) { return US_TILE * (wp + 3) * 4; }      // ids | flags | sequences | groups
static inline int us_block_phrases(int k) { const int ph = US_LIST_BYTES / (16 * k); return ph < US_ROWS ? ph : US_ROWS; }

// meta[r] of packed row r: -1 = padding, else (row of its phrase) | (is the phrase's last row) << 7 | (phrase slot in the block) << 8;
// rowsrc[r]: its row in q [R, W].  slot_phrase / slot_thr / slot_grp [b * 256 + slot]: the phrase of a slot (-1: none), its
// threshold and its group.
template <int WP, bool OCC>
__device__ __forceinline__ void unit_scan_body(const int32_t* __restrict__ q, int W, const int32_t* __restrict__ meta,
                                               const int32_t* __restrict__ rowsrc, const int32_t* __restrict__ slot_phrase,
                                               const int32_t* __restrict__ slot_thr, const int32_t* __restrict__ slot_grp, int P, int ph,
                                               const int32_t* __restrict__ x, int N, int k, const int32_t* __restrict__ seqid,
                                               const int32_t* __restrict__ cuts, const int32_t* __restrict__ sgrp, int C,
                                               float* __restrict__ ps, int32_t* __restrict__ pi, int2* __restrict__ pp) {
    extern __shared__ __attribute__((aligned(16))) int us_smem[];
    int* ids = us_smem;                                    // [US_TILE][WP] ids of the tile's columns
    int* flg = ids + US_TILE * WP;                         // [US_TILE] 1: the column begins a sequence, 2: it ends one
    int* sqs = flg + US_TILE;                              // [US_TILE] sequence of each column
    int* sgs = sqs + US_TILE;                              // [US_TILE] group of each column's sequence
    int2* lp = (int2*)(sgs + US_TILE);                     // [ph][k] (first row, last row) of each entry
    float* ls = (float*)(lp + ph * k);                     // [ph][k] sorted costs
    int* li = (int*)(ls + ph * k);                         // [ph][k] their sequences (OCC: start rows)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.x, cut = blockIdx.y;
    int rlo = cuts[cut], rhi = cuts[cut + 1];
    rlo = rlo < 0 ? 0 : rlo; rhi = rhi > N ? N : rhi;
    const int tiles = rhi > rlo ? (rhi - rlo + US_TILE - 1) / US_TILE : 0;
    for (int e = tid; e < ph * k; e += 256) { ls[e] = INFINITY; li[e] = INT_MAX; lp[e] = make_int2(-1, -1); }

    // the lane's phrase row
    const int mt = meta[(size_t)b * US_ROWS + tid];
    const int i = mt & 127, slot = (mt >> 8) & 255;
    const bool lastrow = (mt >> 7) & 1, valid = mt >= 0 && slot < ph, first = i == 0;
    int maxi = valid ? i : -1;                             // the wave's largest phrase row (-1: the wave holds none)
#pragma unroll
    for (int o = 32; o; o >>= 1) { const int v = __shfl_xor(maxi, o); maxi = v > maxi ? v : maxi; }
    int pu[WP];
#pragma unroll
    for (int c = 0; c < WP; ++c) pu[c] = (valid && c < W) ? q[(size_t)rowsrc[(size_t)b * US_ROWS + tid] * W + c] : 0;
    int thr = -1, pg = 0;
    if (valid && lastrow) { thr = slot_thr[(size_t)b * US_ROWS + slot]; pg = slot_grp[(size_t)b * US_ROWS + slot]; }
    const bool grouped = sgrp != nullptr;
    // A cell is one word: E << 10 | (start as B = column - start + 1).  E <= (i + 1) W <= 512 (the vertical path from row -1), and a
    // path to row i has at most i + 1 diagonal steps and no more left steps than that (each costs W, and E <= (i + 1) W), so
    // B <= 128 fits bits 0 .. 7.  Bits 8 .. 9 take the predecessor's rank (0 diagonal, 1 upper, 2 left) while the three compete:
    // one min3 picks the smallest E, the first in that order on ties, and B rides along.  Row -1 and column -1 have B = 0.
    const int US_E = 10, US_RANK = 8;
    const int c_up = (W << US_E) | (1 << US_RANK), c_left = (W << US_E) | (2 << US_RANK) | 1;
    const int g_start = first ? 0 : (i * W) << US_E;        // E[i-1][-1] = i W; row -1 is 0
    const int l_start = ((i + 1) * W) << US_E;              // E[i][-1]

    // the DP's state: sp = the cell [i][last column done]; dp = the cell [i-1][that column], the next diagonal (0 on a phrase's
    // first row: row -1); (oc, os, oe) of a phrase's last row: the best of the current sequence, OCC: the pending occurrence
    // (oc = INT_MAX: none)
    int sp = 0, dp = 0, oc = INT_MAX, os = 0, oe = 0;
    [[maybe_unused]] const int thr_cell = thr < 0 ? -1 : (thr << US_E) | ((1 << US_E) - 1);     // a cell is admissible at or below it

    int xr[WP], xseq = 0, xflag = 0, xgrp = 0;
    auto fetch = [&](int tile) {
        const int col = rlo + tile * US_TILE + tid;
        xflag = 0; xseq = 0; xgrp = 0;
#pragma unroll
        for (int c = 0; c < WP; ++c) xr[c] = 0;
        if (col < rhi) {
#pragma unroll
            for (int c = 0; c < WP; ++c) if (c < W) xr[c] = x[(size_t)col * W + c];
            xseq = seqid[col];
            const bool bs = col == rlo || seqid[col - 1] != xseq, es = col + 1 == rhi || seqid[col + 1] != xseq;
            xflag = (bs ? 1 : 0) | (es ? 2 : 0);
            xgrp = grouped ? sgrp[xseq] : 0;
        }
    };
    auto hand = [&](uint64_t fb, int v, int key, int s0, int s1) {       // one hand-off per set bit: lane c's entry into its phrase's list
        while (fb) {
            const int c = __ffsll((unsigned long long)fb) - 1;
            fb &= fb - 1;
            const int cv = __shfl(v, c), ck = __shfl(key, c), c0 = __shfl(s0, c), c1 = __shfl(s1, c), sl = __shfl(slot, c);
            kn_insert_t<true>(ls + sl * k, li + sl * k, lp + sl * k, k, lane, (float)cv, ck, make_int2(c0, c1));
        }
    };

    if (tiles > 0) fetch(0);
    for (int tile = 0; tile < tiles; ++tile) {
        const int n0 = rlo + tile * US_TILE;
        __syncthreads();                                   // every wave is through the previous tile (first tile: the lists are clear)
        if constexpr (WP == 1) ids[tid] = xr[0];
        else if constexpr (WP == 2) *(int2*)(ids + tid * 2) = make_int2(xr[0], xr[1]);
        else {
#pragma unroll
            for (int c = 0; c < WP; c += 4) *(int4*)(ids + tid * WP + c) = make_int4(xr[c], xr[c + 1], xr[c + 2], xr[c + 3]);
        }
        flg[tid] = xflag; sqs[tid] = xseq; sgs[tid] = xgrp;
        __syncthreads();
        if (tile + 1 < tiles) fetch(tile + 1);
        if (maxi < 0) continue;                            // wave-uniform
        const int ncol = rhi - n0 < US_TILE ? rhi - n0 : US_TILE;
        for (int st = 0; st < ncol + maxi; ++st) {
            const int up = __shfl_up(sp, 1);               // the cell [i-1][j] where this lane works on column j
            const int j = st - i;
            bool fin = false, fin2 = false;
            int ec = 0, es = 0, ee = 0;
            if (valid && (unsigned)j < (unsigned)ncol) {
                int t[WP];
                if constexpr (WP == 1) t[0] = ids[j];
                else if constexpr (WP == 2) { const int2 v = *(const int2*)(ids + j * 2); t[0] = v.x; t[1] = v.y; }
                else {
#pragma unroll
                    for (int c = 0; c < WP; c += 4) {
                        const int4 v = *(const int4*)(ids + j * WP + c);
                        t[c] = v.x; t[c + 1] = v.y; t[c + 2] = v.z; t[c + 3] = v.w;
                    }
                }
                int sub = 0;
#pragma unroll
                for (int c = 0; c < WP; ++c) sub += pu[c] != t[c] ? 1 : 0;
                const int f = flg[j], col = n0 + j;
                const bool isstart = f & 1, isend = f & 2;
                // a sequence start puts column -1 in place of the left and diagonal cells
                const int u = first ? 0 : up, g = isstart ? g_start : dp, l = isstart ? l_start : sp;
                const int cg = g + (sub << US_E) + 1, cu = u + c_up, cl = l + c_left;
                int best = cg < cu ? cg : cu;
                best = best < cl ? best : cl;                // diagonal, then (i-1, j), then (i, j-1): the first smallest
                best &= ~(3 << US_RANK);
                dp = u; sp = best;
                if (lastrow) {
                    if (isstart) oc = INT_MAX;               // a new sequence
                    const float* tv = ls + slot * k + k - 1;   // the list's tail, read only where an entry is ready
                    const int* ti = li + slot * k + k - 1;
                    if constexpr (OCC) {
                        const int A = best >> US_E, as = col + 1 - (best & 255);
                        const bool adm = !(grouped && sgs[j] == pg);
                        bool out = false;
                        if (A <= thr) {                      // an admissible column, offered by itself as (E[j], start[j], j)
                            if (oc != INT_MAX && as > oe) {  // disjoint from the pending one: that one is an occurrence
                                ec = oc; es = os; ee = oe;
                                oc = A; os = as; oe = col;
                                out = true;
                            } else if (A < oc) { oc = A; os = as; oe = col; }      // the cheaper stays, the pending one on ties
                        }
                        fin = out && adm && kn_better((float)ec, es, *tv, *ti);
                        fin2 = adm && isend && oc != INT_MAX && kn_better((float)oc, os, *tv, *ti);
                    } else {
                        // oc is the sequence's best CELL here, cost and start packed: strictly cheaper <=> below oc's cost bits, so
                        // ties keep the smallest end column; the entry is unpacked only at a sequence end that has one
                        if (best < (oc & ~((1 << US_E) - 1))) { oc = best; oe = col; }
                        if (isend && oc <= thr_cell && !(grouped && sgs[j] == pg)) {
                            ec = oc >> US_E; es = sqs[j]; os = oe + 1 - (oc & 255);
                            fin = kn_better((float)ec, es, *tv, *ti);
                        }
                    }
                }
            }
            if constexpr (OCC) {
                hand(__ballot(fin), ec, es, es, ee);
                hand(__ballot(fin2), oc, os, os, oe);      // kn_insert_t tests the tail again: the first hand-off may have moved it
            } else hand(__ballot(fin), ec, es, os, oe);
        }
    }
    __syncthreads();
    // the block's lists to ps / pi / pp [P][C][k]; entries that did not fill stay (+inf, INT_MAX, (-1, -1))
    for (int sl = wave; sl < ph; sl += 4) {
        const int pid = slot_phrase[(size_t)b * US_ROWS + sl];
        if (pid < 0 || pid >= P) break;
        const size_t o = ((size_t)pid * C + cut) * k;
        for (int e = lane; e < k; e += 64) { ps[o + e] = ls[sl * k + e]; pi[o + e] = li[sl * k + e]; pp[o + e] = lp[sl * k + e]; }
    }
}

template <int WP, bool OCC>
__global__ __launch_bounds__(256) void unit_scan_kernel(const int32_t* __restrict__ q, int W, const int32_t* __restrict__ meta,
                                                        const int32_t* __restrict__ rowsrc, const int32_t* __restrict__ slot_phrase,
                                                        const int32_t* __restrict__ slot_thr, const int32_t* __restrict__ slot_grp, int P,
                                                        int ph, const int32_t* __restrict__ x, int N, int k,
                                                        const int32_t* __restrict__ seqid, const int32_t* __restrict__ cuts,
                                                        const int32_t* __restrict__ sgrp, int C, float* __restrict__ ps,
                                                        int32_t* __restrict__ pi, int2* __restrict__ pp) {
    unit_scan_body<WP, OCC>(q, W, meta, rowsrc, slot_phrase, slot_thr, slot_grp, P, ph, x, N, k, seqid, cuts, sgrp, C, ps, pi, pp);
}

// An entry's key is its sequence (seqid null) or its start row, mapped to the sequence through seqid.  Costs are exact small
// integers carried as floats.  Fillers -> (INT_MAX, -1, (-1, -1)); spans as (first row, one past the last row).
__global__ __launch_bounds__(256) void unit_finish_kernel(const float* __restrict__ ls, const int32_t* __restrict__ li,
                                                          const int2* __restrict__ lp, int64_t tot, const int32_t* __restrict__ seqid,
                                                          int32_t* __restrict__ cost, int64_t* __restrict__ seq, int64_t* __restrict__ span) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tot) return;
    const int j = li[e];
    if (j == INT_MAX) { cost[e] = INT_MAX; seq[e] = -1; span[2 * e] = -1; span[2 * e + 1] = -1; return; }
    const int2 p = lp[e];
    cost[e] = (int32_t)ls[e]; seq[e] = seqid ? seqid[j] : j; span[2 * e] = p.x; span[2 * e + 1] = (int64_t)p.y + 1;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// How a call is laid out: the phrases, in order, packed into blocks of 256 rows (a phrase inside one 64-row wave, at most
// us_block_phrases(k) phrases per block) and the database cut at sequence starts.
struct UsPlan {
    int nb = 0, ph = 0, C = 0;                             // blocks, the most phrases in any block, cuts
    std::vector<int32_t> place, cut_rows;                  // first packed row of each phrase; [C + 1]
};

// the checks that need the host arrays, then the plan; returns what is wrong, or null
static const char* us_plan(const int32_t* len, int32_t P, const int32_t* off, int32_t S, int32_t k, int32_t splits, UsPlan& pl) {
    if (!len || !off) return "null argument";
    if (P < 1 || S < 1) return "need n_phrases, n_seq >= 1";
    if (k < 1 || k > KN_KMAX) return "need 1 <= k <= 128";
    if (splits < 0) return "need splits >= 0";
    if (off[0] != 0) return "seq_offsets_host must ascend from 0";
    for (int32_t s = 0; s < S; ++s) {
        const int64_t l = (int64_t)off[s + 1] - off[s];
        if (l < 1) return "seq_offsets_host must ascend without an empty sequence";
        if (l > US_MAX_SEQ) return "a sequence has more than 65536 rows";
    }
    const int cap = us_block_phrases(k);
    pl.place.resize(P);
    int64_t blk = 0;
    int r = 0, cnt = 0, ph = 0;
    for (int32_t p = 0; p < P; ++p) {
        const int m = len[p];
        if (m < 1 || m > US_MAX_M) return "a phrase has between 1 and 64 units";
        if ((r & 63) + m > 64) r = (r + 63) & ~63;         // a phrase lies inside one 64-row wave
        if (r + m > US_ROWS || cnt == cap) { ++blk; r = 0; cnt = 0; }
        pl.place[p] = (int32_t)(blk * US_ROWS + r);
        r += m; ++cnt;
        ph = cnt > ph ? cnt : ph;
        if ((blk + 1) * US_ROWS > INT32_MAX / 2) return "too many phrases: use smaller phrase chunks";
    }
    pl.nb = (int)(blk + 1); pl.ph = ph;
    const int64_t N = off[S], tiles = (N + US_TILE - 1) / US_TILE;
    int64_t Cw = splits;
    if (Cw <= 0) {
        Cw = (US_TARGET_BLOCKS + pl.nb - 1) / pl.nb;
        const int64_t most = tiles / US_MIN_TILES;
        Cw = Cw < most ? Cw : most;
    }
    Cw = Cw < 65535 ? Cw : 65535;
    Cw = Cw < 1 ? 1 : Cw;
    // cut c begins at the first sequence start at or after row c N / Cw; equal boundaries collapse
    pl.cut_rows.assign(1, 0);
    int64_t last = 0;
    int32_t s = 0;
    for (int64_t c = 1; c < Cw; ++c) {
        const int64_t target = c * N / Cw;
        while (s < S && off[s] < target) ++s;
        if (s >= S) break;
        if (off[s] <= last) continue;
        pl.cut_rows.push_back(off[s]);
        last = off[s];
    }
    pl.cut_rows.push_back((int32_t)N);
    pl.C = (int)pl.cut_rows.size() - 1;
    if ((int64_t)P * pl.C * k > INT32_MAX / 2) return "n_phrases x cuts x k is too large: use smaller phrase chunks";
    return nullptr;
}

static inline int64_t us_table_ints(const UsPlan& pl) { return 5 * (int64_t)pl.nb * US_ROWS + pl.C + 1; }

extern "C" int64_t sylber_unit_workspace_bytes(const int32_t* phrase_len_host, int32_t n_phrases, const int32_t* seq_offsets_host,
                                               int32_t n_seq, int32_t k, int32_t splits) {
    try {
        UsPlan pl;
        if (us_plan(phrase_len_host, n_phrases, seq_offsets_host, n_seq, k, splits, pl)) return -1;
        // the tables of the plan | costs, keys, spans [P][C][k] | the same [P][ceil(C / 2)][k]
        return kn_al(us_table_ints(pl) * 4) + dt_occ_lists_bytes(n_phrases, pl.C, k);
    } catch (...) { return -1; }
}

template <int WP, bool OCC>
static int us_launch(dim3 grid, size_t lds, hipStream_t s, const int32_t* q, int W, const int32_t* tab, int nb, int P, int ph, const int32_t* x,
                     int N, int k, const int32_t* seqid, const int32_t* sgrp, int C, const DtOccLists& l) {
    static PerDeviceOnce once;
    if (once.need())
        HIP_TRY(hipFuncSetAttribute((const void*)unit_scan_kernel<WP, OCC>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    us_fixed_bytes(WP) + US_LIST_BYTES));
    const size_t R = (size_t)nb * US_ROWS;
    hipLaunchKernelGGL((unit_scan_kernel<WP, OCC>), grid, dim3(256), lds, s, q, W, tab, tab + R, tab + 2 * R, tab + 3 * R, tab + 4 * R, P, ph, x,
                       N, k, seqid, tab + 5 * R, sgrp, C, l.s0, l.i0, l.p0);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <bool OCC>
static int us_run(const char* what, const int32_t* phrase_units_dev, int32_t R, int32_t W, const int32_t* phrase_row_host,
                  const int32_t* phrase_len_host, const int32_t* thr_host, int32_t n_phrases, const int32_t* units_dev, int32_t N,
                  const int32_t* seq_offsets_host, int32_t n_seq, const int32_t* seq_id_dev, const int32_t* phrase_group_host,
                  const int32_t* seq_group_dev, int32_t splits, int32_t k, int32_t* cost_dev, int64_t* seq_dev, int64_t* span_dev,
                  void* workspace_dev, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    // every check comes before the first device call
    if (!phrase_units_dev || !phrase_row_host || !phrase_len_host || !thr_host || !units_dev || !seq_offsets_host || !seq_id_dev || !cost_dev ||
        !seq_dev || !span_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (W < 1 || W > US_MAX_W) { syl_set_error(what, "need 1 <= W <= 8"); return 1; }
    if (R < 1 || N < 1) { syl_set_error(what, "need R, N >= 1"); return 1; }
    if (!phrase_group_host != !seq_group_dev) { syl_set_error(what, "phrase_group_host and seq_group_dev go together"); return 1; }
    UsPlan pl;
    if (const char* bad = us_plan(phrase_len_host, n_phrases, seq_offsets_host, n_seq, k, splits, pl)) { syl_set_error(what, bad); return 1; }
    if (seq_offsets_host[n_seq] != N) { syl_set_error(what, "seq_offsets_host must end at N"); return 1; }
    for (int32_t p = 0; p < n_phrases; ++p) {
        if (thr_host[p] < 0) { syl_set_error(what, "need thr >= 0"); return 1; }
        if (phrase_row_host[p] < 0 || (int64_t)phrase_row_host[p] + phrase_len_host[p] > R) { syl_set_error(what, "a phrase lies outside its R rows"); return 1; }
    }
    // the tables of the plan: row meta | row source | slot -> phrase | slot thr | slot group [nb * 256] each, then the cut rows
    const size_t B = (size_t)pl.nb * US_ROWS;
    std::vector<int32_t> tab((size_t)us_table_ints(pl), -1);
    {
        int64_t blk = -1;
        int slot = 0;
        for (int32_t p = 0; p < n_phrases; ++p) {
            const int32_t r0 = pl.place[p], m = phrase_len_host[p];
            if (r0 / US_ROWS != blk) { blk = r0 / US_ROWS; slot = 0; }
            for (int32_t i = 0; i < m; ++i) {
                tab[r0 + i] = i | ((i == m - 1) << 7) | (slot << 8);
                tab[B + r0 + i] = phrase_row_host[p] + i;
            }
            const size_t e = (size_t)blk * US_ROWS + slot;
            const int32_t cap = m * W - 1;                 // thr = min(max_cost, m W - 1): a match has a diagonal step
            tab[2 * B + e] = p;
            tab[3 * B + e] = thr_host[p] < cap ? thr_host[p] : cap;
            tab[4 * B + e] = phrase_group_host ? phrase_group_host[p] : 0;
            ++slot;
        }
        for (int c = 0; c <= pl.C; ++c) tab[5 * B + c] = pl.cut_rows[c];
    }
    char* w = (char*)workspace_dev;
    int32_t* tab_dev = (int32_t*)w; w += kn_al((int64_t)tab.size() * 4);
    const DtOccLists lists = dt_occ_lists_carve(w, n_phrases, pl.C, k);
    // the tables are pageable host memory: the copy is staged before the call returns, in stream order on the device
    HIP_TRY(hipMemcpyAsync(tab_dev, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
    const dim3 grid((unsigned)pl.nb, (unsigned)pl.C);
    const int wp = W == 1 ? 1 : W == 2 ? 2 : W <= 4 ? 4 : 8;
    const size_t lds = (size_t)us_fixed_bytes(wp) + (size_t)pl.ph * k * 16;
    int rc;
    switch (wp) {
    case 1: rc = us_launch<1, OCC>(grid, lds, s, phrase_units_dev, W, tab_dev, pl.nb, n_phrases, pl.ph, units_dev, N, k, seq_id_dev, seq_group_dev, pl.C, lists); break;
    case 2: rc = us_launch<2, OCC>(grid, lds, s, phrase_units_dev, W, tab_dev, pl.nb, n_phrases, pl.ph, units_dev, N, k, seq_id_dev, seq_group_dev, pl.C, lists); break;
    case 4: rc = us_launch<4, OCC>(grid, lds, s, phrase_units_dev, W, tab_dev, pl.nb, n_phrases, pl.ph, units_dev, N, k, seq_id_dev, seq_group_dev, pl.C, lists); break;
    default: rc = us_launch<8, OCC>(grid, lds, s, phrase_units_dev, W, tab_dev, pl.nb, n_phrases, pl.ph, units_dev, N, k, seq_id_dev, seq_group_dev, pl.C, lists); break;
    }
    if (rc) return 1;
    DtOccLists l = lists;
    if (dt_occ_merge(l, n_phrases, pl.C, k, s)) return 1;
    const int64_t tot = (int64_t)n_phrases * k;
    hipLaunchKernelGGL(unit_finish_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, l.s0, l.i0, l.p0, tot,
                       OCC ? seq_id_dev : (const int32_t*)nullptr, cost_dev, seq_dev, span_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_unit_search(const int32_t* phrase_units_dev, int32_t R, int32_t W, const int32_t* phrase_row_host,
                                  const int32_t* phrase_len_host, const int32_t* thr_host, int32_t n_phrases, const int32_t* units_dev,
                                  int32_t N, const int32_t* seq_offsets_host, int32_t n_seq, const int32_t* seq_id_dev,
                                  const int32_t* phrase_group_host, const int32_t* seq_group_dev, int32_t splits, int32_t k,
                                  int32_t* cost_dev, int64_t* seq_dev, int64_t* span_dev, void* workspace_dev, void* stream) {
    try {
        return us_run<false>("sylber_unit_search", phrase_units_dev, R, W, phrase_row_host, phrase_len_host, thr_host, n_phrases, units_dev, N,
                             seq_offsets_host, n_seq, seq_id_dev, phrase_group_host, seq_group_dev, splits, k, cost_dev, seq_dev, span_dev,
                             workspace_dev, stream);
    } catch (...) { syl_set_error("sylber_unit_search", "out of host memory"); return 1; }
}

extern "C" int sylber_unit_occurrences(const int32_t* phrase_units_dev, int32_t R, int32_t W, const int32_t* phrase_row_host,
                                       const int32_t* phrase_len_host, const int32_t* thr_host, int32_t n_phrases, const int32_t* units_dev,
                                       int32_t N, const int32_t* seq_offsets_host, int32_t n_seq, const int32_t* seq_id_dev,
                                       const int32_t* phrase_group_host, const int32_t* seq_group_dev, int32_t splits, int32_t k,
                                       int32_t* cost_dev, int64_t* seq_dev, int64_t* span_dev, void* workspace_dev, void* stream) {
    try {
        return us_run<true>("sylber_unit_occurrences", phrase_units_dev, R, W, phrase_row_host, phrase_len_host, thr_host, n_phrases, units_dev,
                            N, seq_offsets_host, n_seq, seq_id_dev, phrase_group_host, seq_group_dev, splits, k, cost_dev, seq_dev, span_dev,
                            workspace_dev, stream);
    } catch (...) { syl_set_error("sylber_unit_occurrences", "out of host memory"); return 1; }
}

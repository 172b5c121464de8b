// Compressed phrase search (sylber_amd/pq.py: PQSyllableIndex.search_phrases; contract in include/sylber_hip.h, restated in
// tests/dtwpq_ref.py): stage 1 of the two-stage phrase search of dtw16.hip, run on the M-byte product-quantization codes instead of
// a 16-bit plane of the rows.  Decode into the MFMA, not table look-ups: a 128-row query block's ADC tables would be 128 M KiB and
// cannot sit in LDS, while decoding a 128-column tile is 128 M gathers of dsub halves from the 16-bit codebooks (512 D bytes,
// L2-resident), amortised over all 128 phrase rows by v_mfma_f32_32x32x16_{f16,bf16}.
//   * dtwpq_scan_kernel<FMT> is dtw16_scan_kernel<FMT> with the database side of `fetch` replaced: thread (sr, sh) needs halves
//     [k0 + sh, k0 + sh + 16) of row cr; (D / M) % 16 == 0, so they lie in one sub-space mm = (k0 + sh) / dsub at offset
//     o = (k0 + sh) % dsub, and the thread loads 32 B from codebooks16 + ((mm * 256 + codes[cr * M + mm]) * dsub + o).  Rounding is
//     element-wise, so that gather IS round16(decode(code)) and the staged bits are those of the materialised plane
//     sylber_knn16_pack(sylber_pq_decode(codes)): with db_norm = recon_norm the candidates and coarse costs equal
//     sylber_dtw16_scan's on that plane bit for bit.  The LDS carve, the column data, the epilogue, the lane state, the wavefront with
//     the list insertion and the write-out are dtw_tile.h's pieces (SPAN = false), the host path dtw16_scan.h's; the query side, the
//     `in` test for D % 32 == 16, the row clamp and the K loop around k16_mma are dtw16_scan_kernel's, which keeps its own text.
//     What is particular to the codes (where 16 halves lie, the mask, the bytes staged per tile) is the struct Dt16Codes, which the
//     body takes as a parameter: written straight into the body the same statements made the compiler spill 36 B per lane.
//   * the mask: the epilogue reads cns[cl] in both metrics, so a masked row (bad[j] != 0) needs only cns = NaN where the tile's cns
//     is filled; its local cost is then +inf against every phrase row, as a NaN row's.
//   * the dependent load (code byte, then gather): the tile's 128 x M code bytes are copied to LDS at ks == 0 beside cns / sq / sgs
//     and the fetches of the tile's K steps 1 .. read their byte from there.  The one fetch issued for the NEXT tile's first K step,
//     before the current tile's epilogue and DP, reads its byte from global memory: its latency lies under the DP.
// LDS and occupancy (a CU has 160 KiB): no byte more than dtw16_scan_kernel.
//   dtwpq_scan_kernel   69 136 B fixed (cost tile 67 584 | c_j, sequence ids, groups) + 8 B x (phrases of the block) x m <= 32 KiB of
//                       lists = at most 101 904 B.  The code bytes ([128][M] <= 8 192 B) lie at byte 20 480 of the cost-tile region,
//                       behind the 20 480 B staging that the K loop uses: that part is dead from the end of one tile's DP (the
//                       barrier at the top of the next K step) to the next epilogue's first store (behind the barrier after the last
//                       k16_mma, by which every fetch of the tile has been issued and has returned its byte: the byte feeds an
//                       address).  Two workgroups per CU where dtw16_scan_kernel has two: lists <= 12 784 B.
#include "kernels.h"
#include "dtw16_scan.h"

constexpr int DPQ_MAX_M = 64;                             // PQ_MAX_M of pq.hip
constexpr int DPQ_KSUB = 256;                             // centroids per sub-space
constexpr int DPQ_CODE_OFF = KN_STAGE * 4;                // byte offset of the tile's code bytes in the cost-tile region
static_assert(DPQ_CODE_OFF + KN_BN * DPQ_MAX_M <= KN_BM * DT_LD * 4, "the code bytes fit in the cost tile behind the staging");

// codes [N][M] (bad [N] or null: 1 = masked row) and cb16 [M][256][dsub], the 16-bit codebooks; dsub % 16 == 0, so the 16 halves lie
// in one sub-space mm at offset o, and they are 32 B of codebook row code[cr][mm]: round16(decode(code)), rounding being
// element-wise.  The load depends on the code byte.  The tile's 128 x M code bytes are copied to LDS at ks == 0 and the fetches of
// the tile's K steps 1 .. read their byte from there; the one fetch issued for the NEXT tile's first K step, before the current
// tile's epilogue and DP, reads its byte from global memory: its latency lies under the DP.
struct Dt16Codes {
    const uint8_t* codes;
    const uint8_t* bad;
    const bf16_t* cb16;
    int M, dsub;
    __device__ __forceinline__ const bf16_t* halves(int cr, int kc, int ks, int sr, const uint8_t* cds) const {
        const int mm = kc / dsub, o = kc - mm * dsub;
        const int code = ks == 0 ? codes[(size_t)cr * M + mm] : cds[sr * M + mm];
        return cb16 + ((size_t)(mm * DPQ_KSUB + code) * dsub + o);
    }
    __device__ __forceinline__ bool masked(int j) const { return bad && bad[j]; }
    // the two threads of a staging row copy its bytes; a row past the cut repeats the cut's last row, as the fetch clamps it
    __device__ __forceinline__ void stage(uint8_t* cds, int n0, int rhi, int tid) const {
        const int sr = tid >> 1;
        int cr = n0 + sr; cr = cr < rhi ? cr : rhi - 1;
        for (int mm = tid & 1; mm < M; mm += 2) cds[sr * M + mm] = codes[(size_t)cr * M + mm];
    }
};

// dtw16_scan_kernel's arguments with the database rows given by db; built from dtw_tile.h's pieces.  256 threads.
template <int FMT, class Db>
__device__ __forceinline__ void dt16_scan_body(const bf16_t* __restrict__ q, const float* __restrict__ qsq, const int32_t* __restrict__ meta,
                                               const int32_t* __restrict__ slot_phrase, const int32_t* __restrict__ block_rows, int P, int ph,
                                               const Db db, int N, int D, const float* __restrict__ cn, int m,
                                               const int32_t* __restrict__ seqid, const int32_t* __restrict__ cuts,
                                               const int32_t* __restrict__ pgrp, const int32_t* __restrict__ sgrp, int C,
                                               float* __restrict__ ps, int32_t* __restrict__ pi) {
    extern __shared__ __attribute__((aligned(16))) float dt_smem[];
    bf16_t* xs = (bf16_t*)dt_smem;                         // staging of the query rows [128][K16_LD]
    bf16_t* cs = xs + KN_BM * K16_LD;                      // staging of the database rows
    uint8_t* cds = (uint8_t*)dt_smem + DPQ_CODE_OFF;       // what Db::stage keeps of the tile, in the cost tile behind the staging
    const DtLds<false> L(dt_smem, ph, m);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int b = blockIdx.x, cut = blockIdx.y;
    int rlo = cuts[cut], rhi = cuts[cut + 1];
    rlo = rlo < 0 ? 0 : rlo; rhi = rhi > N ? N : rhi;
    const int nrow = block_rows[b];
    const int tiles = rhi > rlo ? (rhi - rlo + KN_BN - 1) / KN_BN : 0;
    L.clear(tid, ph, m);
    // staging: thread -> operand row tid >> 1, halves [16 (tid & 1), 16 (tid & 1) + 16) of the K step, as knn16_scan_kernel
    const int sr = tid >> 1, sh = (tid & 1) * 16;
    const bf16_t* qrow = q + ((size_t)b * KN_BM + sr) * D;
    bf16_t* xdst = xs + sr * K16_LD + sh;
    bf16_t* cdst = cs + sr * K16_LD + sh;
    const int frow = lane & 31, fh = lane >> 5;
    const int ksteps = (D + K16_BK - 1) / K16_BK, T = ksteps * tiles;
    bool live[2];                                          // wave-uniform: this wave's 32-row half holds phrase rows
    float qn[2] = {0.f, 0.f};
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
        live[fm] = wm * 64 + fm * 32 < nrow;
        if (qsq) qn[fm] = qsq[(size_t)b * KN_BM + wm * 64 + fm * 32 + frow];
    }
    const DtRow row(meta, slot_phrase, pgrp, b, P, ph, wave, lane);
    DtLane st;

    f32x16_t acc[2][2];
    uint4 xa, xb, ca, cb;
    auto fetch = [&](int t) {
        const int tile = t / ksteps, ks = t % ksteps, k0 = ks * K16_BK;
        int cr = rlo + tile * KN_BN + sr; cr = cr < rhi ? cr : rhi - 1;
        const bool in = k0 + sh < D;                       // D % 16 == 0: a last K step of 16 is completed with zeros on both sides
        const int kc = in ? sh + k0 : 0;                   // the loads stay inside the rows (and the codebooks) either way
        const bf16_t* crow = db.halves(cr, kc, ks, sr, cds);
        const uint4 z = make_uint4(0, 0, 0, 0);
        xa = *(const uint4*)(qrow + kc); xb = *(const uint4*)(qrow + kc + 8);
        ca = *(const uint4*)crow; cb = *(const uint4*)(crow + 8);
        if (!in) { xa = z; xb = z; ca = z; cb = z; }
    };
    if (T > 0) fetch(0);
    for (int t = 0; t < T; ++t) {
        const int tile = t / ksteps, ks = t % ksteps, n0 = rlo + tile * KN_BN;
        if (ks == 0) kn_zero(acc);
        __syncthreads();                                   // previous fragments, the cost tile, cns / sq / sgs are all read
        *(uint4*)xdst = xa; *(uint4*)(xdst + 8) = xb;
        *(uint4*)cdst = ca; *(uint4*)(cdst + 8) = cb;
        if (ks == 0) {
            dt_tile_meta(L, tid, n0, rlo, rhi, cn, seqid, sgrp, [&](int j) { return db.masked(j); });
            if (ksteps > 1) db.stage(cds, n0, rhi, tid);
        }
        __syncthreads();
        if (t + 1 < T) fetch(t + 1);
        k16_mma<FMT>(xs, cs, wm, wn, frow, fh, acc, live[0], live[1]);
        if (ks != ksteps - 1) continue;
        __syncthreads();                                   // every wave is past its fragment reads: the cost tile aliases the staging
        dt_cost_tile(L.dm, L.cns, acc, qsq != nullptr, qn, live, wm, wn, frow, fh);
        __syncthreads();
        if (wave >= 2 || row.maxi < 0) continue;           // wave-uniform
        dt_wavefront(L, row, st, lane, n0, rhi - n0 < KN_BN ? rhi - n0 : KN_BN, sgrp != nullptr, m);
    }
    __syncthreads();
    dt_write_lists(L, slot_phrase, b, P, ph, C, cut, m, wave, lane, ps, pi, nullptr);
}

// As dtw16_scan_kernel, the database given as codes [N][M] (bad [N] or null: 1 = masked row) and cb16 [M][256][D / M], the 16-bit
// codebooks; cn: the fp32 ||decode(code_j)||^2 (L2) or null.
template <int FMT>
__global__ __launch_bounds__(256) void dtwpq_scan_kernel(const bf16_t* __restrict__ q, const float* __restrict__ qsq,
                                                         const int32_t* __restrict__ meta, const int32_t* __restrict__ slot_phrase,
                                                         const int32_t* __restrict__ block_rows, int P, int ph,
                                                         const uint8_t* __restrict__ codes, const uint8_t* __restrict__ bad,
                                                         const bf16_t* __restrict__ cb16, int N, int D, int M,
                                                         const float* __restrict__ cn, int m, const int32_t* __restrict__ seqid,
                                                         const int32_t* __restrict__ cuts, const int32_t* __restrict__ pgrp,
                                                         const int32_t* __restrict__ sgrp, int C, float* __restrict__ ps,
                                                         int32_t* __restrict__ pi) {
    dt16_scan_body<FMT>(q, qsq, meta, slot_phrase, block_rows, P, ph, Dt16Codes{codes, bad, cb16, M, D / M}, N, D, cn, m, seqid, cuts, pgrp,
                        sgrp, C, ps, pi);
}

extern "C" int sylber_dtwpq_scan(const void* q16_dev, int32_t n_blocks, const int32_t* row_meta_dev, const int32_t* slot_phrase_dev,
                                 const int32_t* block_rows_dev, int32_t n_phrases, int32_t block_phrases, const uint8_t* codes_dev,
                                 const uint8_t* bad_dev, const void* codebooks16_dev, int32_t N, int32_t D, int32_t M,
                                 const float* recon_norm_dev, const float* q_norm_dev, int32_t metric, int32_t storage, int32_t m,
                                 const int32_t* seq_id_dev, const int32_t* cut_rows_dev, int32_t cuts, const int32_t* phrase_group_dev,
                                 const int32_t* seq_group_dev, int32_t* cand_dev, float* coarse_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_dtwpq_scan";
    hipStream_t s = (hipStream_t)stream;
    if (!q16_dev || !row_meta_dev || !slot_phrase_dev || !block_rows_dev || !codes_dev || !codebooks16_dev || !seq_id_dev || !cut_rows_dev ||
        !cand_dev || !coarse_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    const char* db_error = (M < 1 || M > DPQ_MAX_M || D % M || (D / M) % 16) ? "need 1 <= M <= 64, D % M == 0 and D / M a multiple of 16" : nullptr;
    return dt16_scan_host(what, db_error, "the L2 metric needs recon_norm_dev and q_norm_dev", n_blocks, n_phrases, block_phrases, N, D,
                          recon_norm_dev, q_norm_dev, metric, storage, m, cuts, phrase_group_dev, seq_group_dev, cand_dev, coarse_dev,
                          workspace_dev, s,
                          [&](auto fmt, dim3 grid, size_t lds, int max_lds, const float* qn, const float* cn, float* ps, int32_t* pi) {
        constexpr int FMT = decltype(fmt)::value;
        static PerDeviceOnce once;
        if (once.need()) HIP_TRY(hipFuncSetAttribute((const void*)dtwpq_scan_kernel<FMT>, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
        hipLaunchKernelGGL(dtwpq_scan_kernel<FMT>, grid, dim3(256), lds, s, (const bf16_t*)q16_dev, qn, row_meta_dev, slot_phrase_dev,
                           block_rows_dev, n_phrases, block_phrases, codes_dev, bad_dev, (const bf16_t*)codebooks16_dev, N, D, M, cn, m,
                           seq_id_dev, cut_rows_dev, phrase_group_dev, seq_group_dev, cuts, ps, pi);
        return 0;
    });
}

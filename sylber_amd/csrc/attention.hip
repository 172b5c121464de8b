// Flash-style multi-head self-attention for gfx950 (12 heads x 64, bidirectional, key-padding mask).
//
// Reference semantics (transformers HubertAttention / sdpa, TP:234-344, reached from
// sylber/model/sylber.py:122): ctx = softmax(q k^T * 64^-0.5 + mask) v where the additive mask is
// -inf on PADDED KEYS only (padded queries are still computed), and absent when nothing is padded.
//
// Everything is kept "query = lane & 31":
//   S^T[key][q] = K . Q^T      A = K tile (LDS, rows = keys), B = Q (registers, loaded once)
//   O^T[d][q]   = V^T . P^T    A = V^T tile (LDS, rows = d),  B = P (registers, straight from S^T)
// With v_mfma_f32_32x32x16_bf16 the C layout of S^T gives lane (q, h = lane>>5) the keys
// 8g + 4h + e (g < 4, e < 4) of a 32-key tile; those 16 values, rounded to bf16, ARE the B operand of
// the two 16-key P.V MFMAs if V^T's key axis is stored with bits 2 and 3 swapped (done for free by the
// QKV GEMM epilogue, see gemm_bf16.hip).  So there is no P transpose, no cross-lane traffic for P, and
// the online-softmax running max / sum / rescale are lane-local (one shuffle with lane^32 per tile).
// K and V^T tiles (64 keys) are staged with global_load_lds_dwordx4 into a double buffer, XOR-swizzled
// through the source address so the ds_read_b128 fragment reads are bank-conflict free.
#include "kernels.h"
#include "lds_dma.h"
#include <type_traits>

#define AT_QBLK 128      // queries per workgroup (4 waves x 32)
#define AT_KV 64         // keys per tile
#define AT_TILE 8192     // bytes of one K or V^T tile
#define AT_LDS (4 * AT_TILE)

// 1/l and the store of one 32-query sub-tile: ctx[b*Tp + q][head*64 + d] (or its MXFP8 form)
template <bool F8, int FMT>
__device__ __forceinline__ void attn_finalize(const f32x16_t (&oacc)[2], float l_run, bf16_t* __restrict__ ctx, uint8_t* __restrict__ ctx_scale,
                                              long scale_rows, int b, int head, int q_first, int ql, int h, int T, int Tp, long lo_ctx = 0) {
        const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
        // an utterance without a single valid key (valid[b] == 0: sylber_forward rejects such lengths, the op-level entry point does not)
        // leaves l = 0 and O = 0: its context rows are written as zeros, not as 0 x inf = NaN (which would reach every later layer through V^T)
        const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
        const int q = q_first + ql;
        if constexpr (F8) {
            // SYLBER_FP8: the context leaves as MXFP8 for the out-projection GEMM.  A 32-wide d block of a head is one
            // scale block: 16 values in this lane, 16 in lane ^ 32; the halves swap two runs so that each lane stores
            // 16 contiguous bytes (a whole 32-byte sector per lane pair); the two scales of a (token, head) are the
            // adjacent pair of the K-pair-major layout
            // rows [T, Tp) of an utterance (padded queries) are written too, as zeros with scale 1: the context buffer aliases the FFN
            // intermediate, and a stale byte read as an E8M0 scale (up to 2^127) would overflow the out-projection row, whose V^T
            // column then turns the NEXT layer's P.V into NaN for every query (0 x inf) -- found with a batch-shape change on one handle
            const bool live = q < T, inrow = q < Tp;
            uint8_t* dst8 = (uint8_t*)ctx + ((size_t)b * Tp + (inrow ? q : 0)) * SYL_HIDDEN + head * 64;
#pragma unroll
            for (int ds = 0; ds < 2; ++ds) {
                float amax = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) amax = fmaxf(amax, live ? fabsf(oacc[ds][r] * inv) : 0.f);
                amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
                const unsigned e = mx_e8m0(amax);
                const float sc = live ? inv * mx_inv_scale(e) : 0.f;
                unsigned w[4];
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    w[g] = live ? pack_fp8x4(oacc[ds][4 * g + 0] * sc, oacc[ds][4 * g + 1] * sc, oacc[ds][4 * g + 2] * sc, oacc[ds][4 * g + 3] * sc) : 0u;
                const unsigned s0 = h ? w[0] : w[2], s1 = h ? w[1] : w[3];
                const unsigned g0 = (unsigned)__shfl_xor((int)s0, 32, 64), g1 = (unsigned)__shfl_xor((int)s1, 32, 64);
                const uint4 out = h ? make_uint4(g0, w[2], g1, w[3]) : make_uint4(w[0], g0, w[1], g1);
                if (inrow) {
                    *(uint4*)(dst8 + 32 * ds + 16 * h) = out;
                    if (h == 0) ctx_scale[mx_scale_index((long)b * Tp + q, 2 * head + ds, scale_rows)] = (uint8_t)e;
                }
            }
        } else {
            // the store tail is store-ISSUE bound (16 dwordx2 per lane): the lane halves swap one 4-feature run per pair
            // of runs, so that each lane stores 8 consecutive features = 8 dwordx4 per lane, whole 32-byte sectors per
            // lane pair (lane h = 0: d = 16p .. 16p+7, lane h = 1: d = 16p+8 .. 16p+15)
            // (rows [T, Tp) are written as zeros: the buffer aliases other activations, and a stale NaN pattern there would come back
            //  through the next layer's V^T as 0 x NaN for every query; tests/test_gpu_encoder.py poisons the workspace to check)
            const bool live = q < T, inrow = q < Tp;
            bf16_t* dst = ctx + ((size_t)b * Tp + (inrow ? q : 0)) * SYL_HIDDEN + head * 64;
#pragma unroll
            for (int ds = 0; ds < 2; ++ds)
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    uint2 ra, rb;
                    ra.x = H16<FMT>::pack2(oacc[ds][8 * pr + 0] * inv, oacc[ds][8 * pr + 1] * inv);
                    ra.y = H16<FMT>::pack2(oacc[ds][8 * pr + 2] * inv, oacc[ds][8 * pr + 3] * inv);
                    rb.x = H16<FMT>::pack2(oacc[ds][8 * pr + 4] * inv, oacc[ds][8 * pr + 5] * inv);
                    rb.y = H16<FMT>::pack2(oacc[ds][8 * pr + 6] * inv, oacc[ds][8 * pr + 7] * inv);
                    const uint2 keep = h ? rb : ra, send = h ? ra : rb;
                    uint2 got;
                    got.x = (unsigned)__shfl_xor((int)send.x, 32, 64); got.y = (unsigned)__shfl_xor((int)send.y, 32, 64);
                    const uint4 out = !live ? make_uint4(0u, 0u, 0u, 0u) : (h ? make_uint4(got.x, got.y, keep.x, keep.y) : make_uint4(keep.x, keep.y, got.x, got.y));
                    if (inrow) *(uint4*)(dst + 32 * ds + 16 * pr + 8 * h) = out;
                    if constexpr (FMT == FMT_SPLIT) {
                        // the lo halves of the same eight values, exchanged the same way
                        uint2 la, lb;
                        la.x = H16<FMT>::pack2_lo(oacc[ds][8 * pr + 0] * inv, oacc[ds][8 * pr + 1] * inv, ra.x);
                        la.y = H16<FMT>::pack2_lo(oacc[ds][8 * pr + 2] * inv, oacc[ds][8 * pr + 3] * inv, ra.y);
                        lb.x = H16<FMT>::pack2_lo(oacc[ds][8 * pr + 4] * inv, oacc[ds][8 * pr + 5] * inv, rb.x);
                        lb.y = H16<FMT>::pack2_lo(oacc[ds][8 * pr + 6] * inv, oacc[ds][8 * pr + 7] * inv, rb.y);
                        const uint2 keepl = h ? lb : la, sendl = h ? la : lb;
                        uint2 gl;
                        gl.x = (unsigned)__shfl_xor((int)sendl.x, 32, 64); gl.y = (unsigned)__shfl_xor((int)sendl.y, 32, 64);
                        const uint4 outl = !live ? make_uint4(0u, 0u, 0u, 0u) : (h ? make_uint4(gl.x, gl.y, keepl.x, keepl.y) : make_uint4(keepl.x, keepl.y, gl.x, gl.y));
                        if (inrow) *(uint4*)(dst + lo_ctx + 32 * ds + 16 * pr + 8 * h) = outl;
                    }
                }
        }
}

// QW = 32-query sub-tiles per wave.  QW = 2 halves the LDS fragment reads and the LDS-DMA instructions per
// MFMA (every K / V^T fragment feeds two MFMAs) but runs three waves per SIMD instead of four; the kernel is bound by
// the dependent chain S -> max -> exp -> P.V inside a wave (removing the exps, or either MFMA group, outright buys
// 10-15 %: tools/ubench/attn_ablate.sh), so the extra resident wave wins.
// FMT_SPLIT: q, k, V^T and the probabilities are hi / lo half pairs; S^T and O^T take three MFMA passes each
// (hi.hi + lo.hi + hi.lo); the K / V^T stage holds four tiles (two planes); lo planes lo_qk / lo_vt / lo_ctx elements on.
template <int QW, bool F8 = false, int FMT = FMT_BF16>
__global__ __launch_bounds__(256, FMT == FMT_SPLIT ? 2 : (QW == 2 ? 3 : 4)) void attention_bf16_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                const bf16_t* __restrict__ Vt, const int* __restrict__ valid,
                                                                bf16_t* __restrict__ ctx, int T, int Tp, int Tpv,
                                                                uint8_t* __restrict__ ctx_scale, long scale_rows,
                                                                long lo_qk, long lo_vt, long lo_ctx) {
    constexpr bool SP = FMT == FMT_SPLIT;
    constexpr int STG = (SP ? 4 : 2) * AT_TILE;      // bytes of one stage: K, V^T (and their lo planes)
    extern __shared__ __attribute__((aligned(256))) char smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // 1-D launch, XCD-aware: workgroup i runs on XCD i % 8; xcd_remap hands every XCD a contiguous run of
    // (utterance, head, query block) triples with the utterance slowest, i.e. the SAME utterances whose rows the
    // q/k/v GEMM tiles of that XCD just wrote and whose context rows its out-projection tiles will read (both GEMMs
    // split their row range into 8 contiguous chunks) -> producer and consumer share one 4 MB L2
    const int nqb = (T + 128 * QW - 1) / (128 * QW);
    const int vid = xcd_remap(blockIdx.x, gridDim.x);
    const int b = vid / (nqb * SYL_HEADS);
    const int head = (vid / nqb) % SYL_HEADS;
    const int q0 = (vid % nqb) * (128 * QW) + wave * (32 * QW);
    const int ql = lane & 31, h = lane >> 5;
    int nvalid = valid ? valid[b] : T;
    nvalid = nvalid < T ? nvalid : T;
    const size_t bh = (size_t)b * SYL_HEADS + head;
    const bf16_t* Qb = Q + bh * Tp * 64;
    const bf16_t* Kb = K + bh * Tp * 64;
    const bf16_t* Vb = Vt + bh * 64 * Tpv;

    // Q fragments (B operand): lane (q, h) holds d = 16 ks + 8 h .. +8
    bf16x8_t qf[QW][4], qfl[SP ? QW : 1][4];
#pragma unroll
    for (int qs = 0; qs < QW; ++qs) {
        int qr = q0 + 32 * qs + ql; qr = qr < Tp ? qr : Tp - 1;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qf[qs][ks] = *(const bf16x8_t*)(Qb + (size_t)qr * 64 + ks * 16 + h * 8);
            if constexpr (SP) qfl[qs][ks] = *(const bf16x8_t*)(Qb + lo_qk + (size_t)qr * 64 + ks * 16 + h * 8);
        }
    }
    // staging: wave w fills rows [16w, 16w+16) of the K tile and of the V^T tile, 8 rows per instruction
    const int srow = lane >> 3, spos = lane & 7;
    // K rows beyond Tp (a last tile of 64 keys when Tp % 64 == 32) are read from whatever follows -- the next head's rows or
    // the next workspace buffer, finite or not: their scores are REPLACED by -inf through the key mask (a select, no
    // arithmetic), and V^T's key tail is kept zero by its producer
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(Kb), rv = make_rsrc(Vb);
    const __amdgpu_buffer_rsrc_t rkl = make_rsrc(Kb + lo_qk), rvl = make_rsrc(Vb + lo_vt);
    int kvoff[2], vvoff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = wave * 16 + i * 8 + srow;
        const int c = spos ^ ((r >> 1) & 7);
        kvoff[i] = (r * 64 + c * 8) * 2;           // + key tile * 64 rows in the scalar offset
        vvoff[i] = (r * Tpv + c * 8) * 2;          // + first key of the tile
    }
    const int lds_piece = wave * 16 * 128;

    const int swz = (lane >> 1) & 7;
    const int frow = ql * 128;

    f32x16_t oacc[QW][2];
#pragma unroll
    for (int qs = 0; qs < QW; ++qs)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[qs][i][r] = 0.f;
    float m_run[QW], l_run[QW];
#pragma unroll
    for (int qs = 0; qs < QW; ++qs) { m_run[qs] = -INFINITY; l_run[qs] = 0.f; }
    // (q arrives pre-scaled by log2(e) / 8: the scores are in log2 units)

    const int nt = (nvalid + AT_KV - 1) / AT_KV;
    {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            glds16b(rk, kvoff[i], 0, smem + lds_piece + i * 1024);
            glds16b(rv, vvoff[i], 0, smem + AT_TILE + lds_piece + i * 1024);
            if constexpr (SP) {
                glds16b(rkl, kvoff[i], 0, smem + 2 * AT_TILE + lds_piece + i * 1024);
                glds16b(rvl, vvoff[i], 0, smem + 3 * AT_TILE + lds_piece + i * 1024);
            }
        }
    }
    // One 64-key tile, as two 32-key halves: S^T half -> softmax -> P.V half.  The softmax is the bottleneck of this
    // kernel, not the matrix pipe: per 64 keys a wave issues 32 MFMAs (1024 cycles) against ~64 v_exp_f32 (quarter
    // rate, 1024 cycles) plus the fma / add / max / convert of every score, so every VALU instruction per score counts:
    //   * the key-padding mask (compare + select per score) sits behind a real, wave-uniform branch: only the last
    //     tile of an utterance pays for it (left to itself the compiler if-converts it into selects on every tile);
    //   * the running maximum is LAZY: scores are exponentiated against a stale maximum as long as the new one exceeds
    //     it by less than 2^8 (p <= 256: exact in the fp32 sums, in range for bf16 and fp16 P); the rescale of the 32
    //     accumulator registers per query sub-tile (and the exp of alpha) then runs on the first half-tile and almost
    //     never again.  O and l carry the same factor, so O / l is unchanged up to rounding; the decision is per query
    //     (lanes that do not need it keep alpha = 1), so a query's result does not depend on its wave neighbours;
    //   * 32 keys at a time halves the live score registers (213 -> <= 168 VGPRs): three waves per SIMD, which is what
    //     makes 32 x 12 x 2 workgroups of the 10 s batch ONE round over the chip instead of one and a half.
    auto tile = [&](const char* kb, const char* vb, int kv0, const bool TAIL) {
#pragma unroll 1
        for (int s2 = 0; s2 < 2; ++s2) {                                 // NOT unrolled: the scheduler would interleave the halves
            if (TAIL && kv0 + 32 * s2 >= nvalid) break;                  // a half with no valid key (uniform)
            f32x16_t sacc[QW];
#pragma unroll
            for (int qs = 0; qs < QW; ++qs)
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[qs][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8_t kf = *(const bf16x8_t*)(kb + s2 * 32 * 128 + frow + (((2 * ks + h) ^ swz) << 4));
#pragma unroll
                for (int qs = 0; qs < QW; ++qs) sacc[qs] = H16<FMT>::mfma(kf, qf[qs][ks], sacc[qs]);
                if constexpr (SP) {
                    const bf16x8_t kfl = *(const bf16x8_t*)(kb + 2 * AT_TILE + s2 * 32 * 128 + frow + (((2 * ks + h) ^ swz) << 4));
#pragma unroll
                    for (int qs = 0; qs < QW; ++qs) {
                        sacc[qs] = H16<FMT>::mfma(kfl, qf[qs][ks], sacc[qs]);
                        sacc[qs] = H16<FMT>::mfma(kf, qfl[qs][ks], sacc[qs]);
                    }
                }
            }
            bf16x8_t pf[QW][2], pfl[SP ? QW : 1][2];
#pragma unroll
            for (int qs = 0; qs < QW; ++qs) {
                if (TAIL) {
                    asm volatile("; key-padding mask (last tile only)");     // keeps this a real branch: no if-conversion
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = kv0 + 32 * s2 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        if (key >= nvalid) sacc[qs][r] = -INFINITY;
                    }
                }
                float mx = -INFINITY;
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[qs][r]);
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                // first half-tile: m_run = -inf, mx finite (key 0 is always valid) -> need; a fully masked half has
                // mx = -inf -> no need, p = exp2(-inf) = 0
                const bool need = (mx - m_run[qs]) > 8.0f;
                if (__builtin_amdgcn_ballot_w64(need)) {
                    const float m_new = need ? mx : m_run[qs];
                    const float alpha = need ? __builtin_amdgcn_exp2f(m_run[qs] - m_new) : 1.0f;
                    m_run[qs] = m_new;
                    l_run[qs] *= alpha;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) oacc[qs][i][r] *= alpha;
                }
                const float mb = m_run[qs];
                float psum = 0.f;
                // P is converted in PAIRS (one v_cvt_pk per two scores) and, in the fp16 format, without the saturating
                // clamp every other conversion carries: 0 <= p <= 2^8 by construction of the lazy maximum
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    uint32_t pw[4], pwl[4];
#pragma unroll
                    for (int e = 0; e < 8; e += 2) {
                        const float p0 = __builtin_amdgcn_exp2f(sacc[qs][8 * j + e] - mb);
                        const float p1 = __builtin_amdgcn_exp2f(sacc[qs][8 * j + e + 1] - mb);
                        psum += p0;
                        psum += p1;
                        pw[e >> 1] = H16<FMT>::pack2_bounded(p0, p1);
                        if constexpr (SP) pwl[e >> 1] = H16<FMT_SPLIT>::pack2_lo(p0, p1, pw[e >> 1]);
                    }
                    typedef uint32_t u32x4v_t __attribute__((ext_vector_type(4)));
                    const u32x4v_t pv = {pw[0], pw[1], pw[2], pw[3]};
                    pf[qs][j] = __builtin_bit_cast(bf16x8_t, pv);
                    if constexpr (SP) {
                        const u32x4v_t pl = {pwl[0], pwl[1], pwl[2], pwl[3]};
                        pfl[qs][j] = __builtin_bit_cast(bf16x8_t, pl);
                    }
                }
                l_run[qs] += psum;
            }
            // O^T += V^T . P^T for these 32 keys (two 16-key groups x two 32-wide d blocks; a V^T fragment feeds QW MFMAs)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int ds = 0; ds < 2; ++ds) {
                    const bf16x8_t vf = *(const bf16x8_t*)(vb + ds * 32 * 128 + frow + (((2 * (2 * s2 + j) + h) ^ swz) << 4));
#pragma unroll
                    for (int qs = 0; qs < QW; ++qs) oacc[qs][ds] = H16<FMT>::mfma(vf, pf[qs][j], oacc[qs][ds]);
                    if constexpr (SP) {
                        const bf16x8_t vfl = *(const bf16x8_t*)(vb + 2 * AT_TILE + ds * 32 * 128 + frow + (((2 * (2 * s2 + j) + h) ^ swz) << 4));
#pragma unroll
                        for (int qs = 0; qs < QW; ++qs) {
                            oacc[qs][ds] = H16<FMT>::mfma(vfl, pf[qs][j], oacc[qs][ds]);
                            oacc[qs][ds] = H16<FMT>::mfma(vf, pfl[qs][j], oacc[qs][ds]);
                        }
                    }
                }
        }
    };
    for (int t = 0; t < nt; ++t) {
        // LDS-DMA completion is NOT covered by __syncthreads(): retire this wave's pieces of tile t explicitly,
        // then meet the other waves (their pieces are retired the same way) before any fragment read.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < nt) {
            char* nb = smem + ((t + 1) & 1) * STG;
            const int kv1 = (t + 1) * AT_KV;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                glds16b(rk, kvoff[i], kv1 * 128, nb + lds_piece + i * 1024);
                glds16b(rv, vvoff[i], kv1 * 2, nb + AT_TILE + lds_piece + i * 1024);
                if constexpr (SP) {
                    glds16b(rkl, kvoff[i], kv1 * 128, nb + 2 * AT_TILE + lds_piece + i * 1024);
                    glds16b(rvl, vvoff[i], kv1 * 2, nb + 3 * AT_TILE + lds_piece + i * 1024);
                }
            }
        }
        const char* kb = smem + (t & 1) * STG;
        const int kv0 = t * AT_KV;
        tile(kb, kb + AT_TILE, kv0, kv0 + AT_KV > nvalid);
    }
    // ---- finalize: 1/l, store ctx[b*Tp + q][head*64 + d]
#pragma unroll
    for (int qs = 0; qs < QW; ++qs) attn_finalize<F8, FMT>(oacc[qs], l_run[qs], ctx, ctx_scale, scale_rows, b, head, q0 + 32 * qs, ql, h, T, Tp, lo_ctx);
}

// ------------------------------------------------------------------------------------------------
// The same attention on MXFP8 operands (BASELINE configs[4] as worded: "fp8 MFMA for attention + FFN GEMMs").
//   q8, k8: [B,H,Tp,64] e4m3 bytes + E8M0 scales [B,H,Tp,2] (one per 32 features: the contraction of QK^T);
//   vt8:    [B,H,64,Tpv] e4m3 bytes in NATURAL key order + scales [B,H,64,Tpv/32] (one per 32 keys: the contraction of PV);
//   P is quantised in registers to e4m3 with a bias of 2^7 (see the loop): its normals cover 2^-13 <= p <= 2.
// v_mfma_scale_f32_32x32x64_f8f6f4 operand layout (gemm_mxfp8.hip, probed): lane (r, h) supplies row r, bytes
// k = 16 h .. 16 h + 15 (registers 0-3) and 32 + 16 h .. + 15 (registers 4-7) of the 64-wide contraction, and the scale of
// (row r, 32-block h).  A 64-key tile is two S^T MFMAs (keys [32 m, 32 m + 32), m = 0, 1; 64 features each) instead of eight,
// and two P.V MFMAs (32 features each, 64 keys) instead of eight.  MFMA row rho of S^T m is key
// 32 m + 16 ((rho >> 2) & 1) + 4 (rho >> 3) + (rho & 3): then lane (q, h) receives, in register order, the scores of keys
// 32 m + 16 h .. + 15 -- which are exactly the contraction slots 16 h .. (m = 0) and 32 + 16 h .. (m = 1) of its P operand,
// so P needs no cross-lane traffic and V^T no key permutation.
typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef int i32x4v_t __attribute__((ext_vector_type(4)));
#define AT8_TILE 4096    // bytes of one K or V^T tile (64 rows x 64 bytes)

template <bool F8OUT>
__global__ __launch_bounds__(256, 4) void attention_f8_kernel(const uint8_t* __restrict__ Q8, const uint8_t* __restrict__ Qs,
                                                              const uint8_t* __restrict__ K8, const uint8_t* __restrict__ Ks,
                                                              const uint8_t* __restrict__ V8, const uint8_t* __restrict__ Vs,
                                                              const int* __restrict__ valid, bf16_t* __restrict__ ctx, int T, int Tp, int Tpv,
                                                              uint8_t* __restrict__ ctx_scale, long scale_rows) {
    __shared__ __attribute__((aligned(256))) char smem[4 * AT8_TILE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nqb = (T + 127) / 128;
    const int vid = xcd_remap(blockIdx.x, gridDim.x);
    const int b = vid / (nqb * SYL_HEADS);
    const int head = (vid / nqb) % SYL_HEADS;
    const int q0 = (vid % nqb) * 128 + wave * 32;
    const int ql = lane & 31, h = lane >> 5;
    int nvalid = valid ? valid[b] : T;
    nvalid = nvalid < T ? nvalid : T;
    const size_t bh = (size_t)b * SYL_HEADS + head;
    const uint8_t* Qb = Q8 + bh * Tp * 64;
    const uint8_t* Kb = K8 + bh * Tp * 64;
    const uint8_t* Vb = V8 + bh * 64 * Tpv;
    const uint8_t* Ksb = Ks + bh * Tp * 2;
    const uint8_t* Vsb = Vs + bh * 64 * (Tpv / 32);

    // Q operand (B of S^T): lane (q, h): features 16 h .. and 32 + 16 h ..; its scale = block h of its row
    i32x8_t qf;
    int qsc;
    {
        int qr = q0 + ql; qr = qr < Tp ? qr : Tp - 1;
        const i32x4v_t lo = *(const i32x4v_t*)(Qb + (size_t)qr * 64 + 16 * h), hi = *(const i32x4v_t*)(Qb + (size_t)qr * 64 + 32 + 16 * h);
        qf = i32x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        qsc = Qs[(bh * Tp + qr) * 2 + h];
    }
    // staging: wave w fills rows [16 w, 16 w + 16) of the K tile and of the V^T tile, ONE 16-byte piece per lane and operand;
    // chunk c of row r lands at position c ^ ((r >> 1) & 3) (bank swizzle of the 64-byte rows)
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(Kb), rv = make_rsrc(Vb);
    int kvoff, vvoff;
    {
        const int r = wave * 16 + (lane >> 2);
        const int c = (lane & 3) ^ ((r >> 1) & 3);
        kvoff = r * 64 + c * 16;                     // + key tile * 64 rows in the scalar offset
        vvoff = r * Tpv + c * 16;                    // + first key of the tile
    }
    const int lds_piece = wave * 1024;
    // fragment rows: S^T m: key row of MFMA row ql; P.V ds: feature row 32 ds + ql.  Chunks h and 2 + h of the row.
    int kaddr[2][2], vaddr[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int kr = 32 * m + 16 * ((ql >> 2) & 1) + 4 * (ql >> 3) + (ql & 3);
        const int vr = 32 * m + ql;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            kaddr[m][j] = kr * 64 + (((2 * j + h) ^ ((kr >> 1) & 3)) << 4);
            vaddr[m][j] = vr * 64 + (((2 * j + h) ^ ((vr >> 1) & 3)) << 4);
        }
    }
    const int krow[2] = {16 * ((ql >> 2) & 1) + 4 * (ql >> 3) + (ql & 3), 32 + 16 * ((ql >> 2) & 1) + 4 * (ql >> 3) + (ql & 3)};

    f32x16_t oacc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const float LOG2E = 1.44269504088896341f;
    const int nt = (nvalid + AT_KV - 1) / AT_KV;
    const int vsp = Tpv / 32;

    int ksc[2], vsc[2];                               // scales of the tile about to be used (requested one tile ahead)
    auto request = [&](int t, char* stage) {
        const int kv = t * AT_KV;
        glds16b(rk, kvoff, kv * 64, stage + lds_piece);
        glds16b(rv, vvoff, kv, stage + AT8_TILE + lds_piece);
    };
    auto scales = [&](int t, int (&ks)[2], int (&vs)[2]) {
        const int kv = t * AT_KV;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            ks[m] = Ksb[(size_t)(kv + krow[m]) * 2 + h];
            vs[m] = Vsb[(size_t)(32 * m + ql) * vsp + (kv >> 5) + h];
        }
    };
    request(0, smem);
    scales(0, ksc, vsc);
    for (int t = 0; t < nt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int ksn[2] = {127, 127}, vsn[2] = {127, 127};
        if (t + 1 < nt) { request(t + 1, smem + ((t + 1) & 1) * 2 * AT8_TILE); scales(t + 1, ksn, vsn); }
        const char* kb = smem + (t & 1) * 2 * AT8_TILE;
        const char* vb = kb + AT8_TILE;
        const int kv0 = t * AT_KV;
        const bool TAIL = kv0 + AT_KV > nvalid;
        // ---- S^T: two MFMAs, keys [0, 32) and [32, 64) of the tile
        f32x16_t sacc[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[m][r] = 0.f;
            const i32x4v_t lo = *(const i32x4v_t*)(kb + kaddr[m][0]), hi = *(const i32x4v_t*)(kb + kaddr[m][1]);
            const i32x8_t kf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            sacc[m] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf, qf, sacc[m], 0, 0, 0, ksc[m], 0, qsc);
        }
        if (TAIL) {
            asm volatile("; key-padding mask (last tile only)");
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (kv0 + 32 * m + 16 * h + r >= nvalid) sacc[m][r] = -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[m][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        // lazy maximum as in the 16-bit kernel, but P is an e4m3 operand: its normal range starts at 2^-6, so the probabilities are
        // carried with a bias of 2^7 (l and O carry it too: O / l is unchanged) and the maximum may lag by at most 2^1:
        // 2^-13 <= p <= 2^1 maps to e4m3's normals 2^-6 .. 2^8 = 256 <= 448
        const bool need = (mx - m_run) * LOG2E > 1.0f;
        if (__builtin_amdgcn_ballot_w64(need)) {
            const float m_new = need ? mx : m_run;
            const float alpha = need ? __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E) : 1.0f;
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
        }
        const float mb = m_run * LOG2E - 7.0f;
        float psum = 0.f;
        int pw[8];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float p0 = __builtin_amdgcn_exp2f(fmaf(sacc[m][4 * g + 0], LOG2E, -mb));
                const float p1 = __builtin_amdgcn_exp2f(fmaf(sacc[m][4 * g + 1], LOG2E, -mb));
                const float p2 = __builtin_amdgcn_exp2f(fmaf(sacc[m][4 * g + 2], LOG2E, -mb));
                const float p3 = __builtin_amdgcn_exp2f(fmaf(sacc[m][4 * g + 3], LOG2E, -mb));
                psum += p0; psum += p1; psum += p2; psum += p3;
                pw[4 * m + g] = (int)pack_fp8x4(p0, p1, p2, p3);
            }
        l_run += psum;
        const i32x8_t pf = {pw[0], pw[1], pw[2], pw[3], pw[4], pw[5], pw[6], pw[7]};
        // ---- O^T += V^T . P^T: two MFMAs (features [0, 32) and [32, 64)), 64 keys each
#pragma unroll
        for (int ds = 0; ds < 2; ++ds) {
            const i32x4v_t lo = *(const i32x4v_t*)(vb + vaddr[ds][0]), hi = *(const i32x4v_t*)(vb + vaddr[ds][1]);
            const i32x8_t vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            oacc[ds] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf, pf, oacc[ds], 0, 0, 0, vsc[ds], 0, 127);
        }
        ksc[0] = ksn[0]; ksc[1] = ksn[1]; vsc[0] = vsn[0]; vsc[1] = vsn[1];
    }
    attn_finalize<F8OUT, FMT_BF16>(oacc, l_run, ctx, ctx_scale, scale_rows, b, head, q0, ql, h, T, Tp);
}

// ------------------------------------------------------------------------------------------------
// The same attention with a HAND-SCHEDULED key loop (round 5; tools/gen_attn_asm.py -> attn_asm_{bf16,f16}.inc): one inline-asm
// statement per wave, software-pipelined over 32-key half-tiles -- S^T of half-tile i + 1 and O^T += V^T P^T of half-tile i - 1 alternate
// on the matrix pipe while the softmax of half-tile i fills the gaps between them; fragments four MFMAs ahead through a register ring,
// K / V^T tiles through a three-slot LDS ring (one barrier per 64-key tile), lazy maximum without a cross-lane exchange on the fast
// path.  Geometry, operand layout and finalisation are attention_bf16_kernel<1>'s (32 queries per wave, "query = lane"), which stays
// as the compiler-scheduled reference (SYLBER_OPT_ATTN_QUERIES_PER_WAVE = 32 / 64).  156 fixed registers: three waves per SIMD.
// The schedule is executed on the CPU by tools/attn_asm_emu.py (tests/test_attn_asm_gen.py) and checked for the issue hazards the
// compiler cannot see inside an asm statement.
#define ATA_SLOT 16384
// PK (packed layout, launch_attention_packed): q / k [H][Tp][64] and V^T [H][64][Tpv] of ONE pseudo-utterance of Tp = Tpv frames that
// holds `nclip` utterances in slots; pk = [slot offsets (nclip + 1) | frames (nclip) | prefix of 128-query blocks (nclip + 1)].  Workgroup
// -> (utterance, head, query block) through the prefix table; Q, K and V^T are based at the utterance's slot, the key bound is its own
// frame count, and the context rows [frames, slot end) are written as zeros.  The generated key loop sees the same operands as for a
// lone utterance: its frames' keys in tiles of 64 from the slot start (slots are multiples of 64 frames), V^T's row pitch Tpv.
template <bool F8, int FMT, int VAR = 0, bool PK = false>
__global__ __launch_bounds__(256, 3) void attention_asm_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                               const bf16_t* __restrict__ Vt, const int* __restrict__ valid,
                                                               bf16_t* __restrict__ ctx, int T, int Tp, int Tpv,
                                                               uint8_t* __restrict__ ctx_scale, long scale_rows,
                                                               const int* __restrict__ pk, int nclip) {
    static_assert(FMT == FMT_BF16 || FMT == FMT_F16, "16-bit single-plane formats");
    __shared__ __attribute__((aligned(1024))) char smem[3 * ATA_SLOT];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int vid = xcd_remap(blockIdx.x, gridDim.x);
    int b, head, q0, nvalid;
    const bf16_t *Qb, *Kb, *Vb;
    if constexpr (PK) {
        const int* qbp = pk + 2 * nclip + 1;
        const int blk = vid / SYL_HEADS;               // (utterance b owns workgroups [12 qbp[b], 12 qbp[b + 1]))
        int lo = 0, hi = nclip - 1;                    // the last b with qbp[b] <= blk
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (qbp[mid] <= blk) lo = mid; else hi = mid - 1; }
        b = __builtin_amdgcn_readfirstlane(lo);
        const int nqb = qbp[b + 1] - qbp[b], local = vid - SYL_HEADS * qbp[b];
        head = local / nqb;
        q0 = (local % nqb) * 128 + wave * 32;
        const int s0 = pk[b];
        nvalid = __builtin_amdgcn_readfirstlane(pk[nclip + 1 + b]);
        T = nvalid;
        const size_t hb = (size_t)head * Tp + s0;      // this utterance's first row in head `head`
        Qb = Q + hb * 64;
        Kb = K + hb * 64;
        Vb = Vt + (size_t)head * 64 * Tpv + s0;
        ctx += (size_t)s0 * SYL_HIDDEN;
        Tp = pk[b + 1] - s0;                           // from here on: the slot's frames (query clamp, zeroed context rows)
        b = 0;
    } else {
        const int nqb = (T + 127) / 128;
        b = vid / (nqb * SYL_HEADS);
        head = (vid / nqb) % SYL_HEADS;
        q0 = (vid % nqb) * 128 + wave * 32;
        nvalid = valid ? valid[b] : T;
        nvalid = nvalid < T ? nvalid : T;
        nvalid = __builtin_amdgcn_readfirstlane(nvalid);
        const size_t bh = (size_t)b * SYL_HEADS + head;
        Qb = Q + bh * Tp * 64;
        Kb = K + bh * Tp * 64;
        Vb = Vt + bh * 64 * Tpv;
    }
    const int ql = lane & 31, h = lane >> 5;
    f32x16_t oacc[2];
    float lsum = 0.f;
    const int nt = __builtin_amdgcn_readfirstlane((nvalid + 63) / 64);
    if (nt > 0) {
        bf16x8_t qf[4];
        int qr = q0 + ql; qr = qr < Tp ? qr : Tp - 1;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const bf16x8_t*)(Qb + (size_t)qr * 64 + ks * 16 + h * 8);
        const int lds0 = (int)(unsigned)(unsigned long long)(lds_vptr)smem;
        const int swz = (lane >> 1) & 7;
        int off[4], kvoff[2], vvoff[2];
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) off[kx] = lds0 + ql * 128 + (((2 * kx + h) ^ swz) << 4);
        const int srow = lane >> 3, spos = lane & 7;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = wave * 16 + i * 8 + srow;
            const int c = spos ^ ((r >> 1) & 7);
            kvoff[i] = (r * 64 + c * 8) * 2;
            vvoff[i] = (r * Tpv + c * 8) * 2;
        }
        const i32x4_t rsk = rsrc_words(Kb), rsv = rsrc_words(Vb);
        const int ldsw = __builtin_amdgcn_readfirstlane(lds0 + wave * 2048);
        const int limbase = nvalid - 4 * h;
        const int kvl0 = __builtin_amdgcn_readfirstlane(64 * (nt - 1)), kvl1 = __builtin_amdgcn_readfirstlane(64 * (nt - 1) + 32);
        f32x16_t o0, o1;
        int koff, voff, resc, snext, dslot, tdma, tleft;
        if constexpr (FMT == FMT_F16) {
#define MF "v_mfma_f32_32x32x16_f16"
#include "attn_asm_f16.inc"
#undef MF
        } else {
#define MF "v_mfma_f32_32x32x16_bf16"
#ifdef SYLBER_GEMM_ASM_EXPERIMENTS
            if constexpr (VAR == 1) {
#include "attn_asm_bf16_v1.inc"
            } else if constexpr (VAR == 2) {
#include "attn_asm_bf16_v2.inc"
            } else if constexpr (VAR == 3) {
#include "attn_asm_bf16_v3.inc"
            } else if constexpr (VAR == 4) {
#include "attn_asm_bf16_v4.inc"
            } else if constexpr (VAR == 5) {
#include "attn_asm_bf16_v5.inc"
            } else if constexpr (VAR == 6) {
#include "attn_asm_bf16_v6.inc"
            } else if constexpr (VAR == 7) {
#include "attn_asm_bf16_v7.inc"
            } else if constexpr (VAR == 8) {
#include "attn_asm_bf16_v8.inc"
            } else if constexpr (VAR == 9) {
#include "attn_asm_bf16_v9.inc"
            } else
#endif
            {
#include "attn_asm_bf16.inc"
            }
#undef MF
        }
        (void)koff; (void)voff; (void)resc; (void)snext; (void)dslot; (void)tdma; (void)tleft;
        oacc[0] = o0; oacc[1] = o1;
    } else {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    }
    attn_finalize<F8, FMT>(oacc, lsum, ctx, ctx_scale, scale_rows, b, head, q0, ql, h, T, Tp);
}

int launch_attention_f8(const uint8_t* q8, const uint8_t* qs, const uint8_t* k8, const uint8_t* ks, const uint8_t* v8, const uint8_t* vs,
                        const int* valid, void* ctx, uint8_t* ctx_scale, long scale_rows, int B, int T, int Tp, int Tpv, hipStream_t s) {
    if (Tpv % 64 != 0 || Tpv < T || Tp % 32 != 0) { syl_set_error("launch_attention_f8", "Tp % 32 == 0, Tpv % 64 == 0, Tpv >= T"); return 1; }
    const dim3 grid(((T + 127) / 128) * SYL_HEADS * B);
    if (ctx_scale) hipLaunchKernelGGL((attention_f8_kernel<true>), grid, dim3(256), 0, s, q8, qs, k8, ks, v8, vs, valid, (bf16_t*)ctx, T, Tp, Tpv, ctx_scale, scale_rows);
    else hipLaunchKernelGGL((attention_f8_kernel<false>), grid, dim3(256), 0, s, q8, qs, k8, ks, v8, vs, valid, (bf16_t*)ctx, T, Tp, Tpv, nullptr, 0L);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int launch_attention_any(const bf16_t* q, const bf16_t* k, const bf16_t* vt, const int* valid, void* ctx, uint8_t* ctx_scale,
                                long scale_rows, int B, int T, int Tp, int Tpv, int force_qw, int fmt, hipStream_t s,
                                long lo_qk = 0, long lo_vt = 0, long lo_ctx = 0) {
    if (Tpv % 64 != 0 || Tpv < T) { syl_set_error("launch_attention", "Tpv must be a multiple of 64 and >= T"); return 1; }
    bf16_t* c = (bf16_t*)ctx;
    // 32 queries per wave (106 VGPRs, four waves per SIMD) is the faster shape inside the forward at every length
    // measured (10 s batch 0.409 vs 0.429 ms per forward, 8 x 60 s 2.71 vs 2.95); 64 per wave stays selectable
    int qw = 1;
    if (force_qw == 1 || force_qw == 2) qw = force_qw;
    if (fmt == FMT_SPLIT) qw = 1;
#ifdef SYLBER_GEMM_ASM_EXPERIMENTS
    if (force_qw >= 101 && force_qw <= 109) {       // knock-out variants of the key loop (timing only, results wrong): tools/attn_bench.py
        const dim3 grid_a(((T + 127) / 128) * SYL_HEADS * B);
#define ATA_VAR(N) case 100 + N: hipLaunchKernelGGL((attention_asm_kernel<false, FMT_BF16, N>), grid_a, dim3(256), 0, s, q, k, vt, valid, c, T, Tp, Tpv, nullptr, 0L, nullptr, 0); break;
        switch (force_qw) { ATA_VAR(1) ATA_VAR(2) ATA_VAR(3) ATA_VAR(4) ATA_VAR(5) ATA_VAR(6) ATA_VAR(7) ATA_VAR(8) ATA_VAR(9) }
#undef ATA_VAR
        HIP_TRY(hipGetLastError());
        return 0;
    }
#endif
    if (force_qw == 0 && fmt != FMT_SPLIT) {
        // default since round 5: the hand-scheduled key loop (attention_asm_kernel); 32 / 64 queries per wave select the
        // compiler-scheduled kernels, kept as its reference
        const dim3 grid_a(((T + 127) / 128) * SYL_HEADS * B);
        if (ctx_scale) hipLaunchKernelGGL((attention_asm_kernel<true, FMT_BF16>), grid_a, dim3(256), 0, s, q, k, vt, valid, c, T, Tp, Tpv, ctx_scale, scale_rows, nullptr, 0);
        else if (fmt == FMT_F16) hipLaunchKernelGGL((attention_asm_kernel<false, FMT_F16>), grid_a, dim3(256), 0, s, q, k, vt, valid, c, T, Tp, Tpv, nullptr, 0L, nullptr, 0);
        else hipLaunchKernelGGL((attention_asm_kernel<false, FMT_BF16>), grid_a, dim3(256), 0, s, q, k, vt, valid, c, T, Tp, Tpv, nullptr, 0L, nullptr, 0);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const dim3 grid((qw == 2 ? (T + 255) / 256 : (T + 127) / 128) * SYL_HEADS * B);
    if (fmt == FMT_SPLIT) {
        static PerDeviceOnce attr_once;
        auto kern = attention_bf16_kernel<1, false, FMT_SPLIT>;
        if (attr_once.need()) HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * AT_LDS));
        hipLaunchKernelGGL(kern, grid, dim3(256), 2 * AT_LDS, s, q, k, vt, valid, c, T, Tp, Tpv, nullptr, 0L, lo_qk, lo_vt, lo_ctx);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (ctx_scale) {
        if (qw == 2) hipLaunchKernelGGL((attention_bf16_kernel<2, true>), grid, dim3(256), AT_LDS, s, q, k, vt, valid, c, T, Tp, Tpv, ctx_scale, scale_rows, 0L, 0L, 0L);
        else hipLaunchKernelGGL((attention_bf16_kernel<1, true>), grid, dim3(256), AT_LDS, s, q, k, vt, valid, c, T, Tp, Tpv, ctx_scale, scale_rows, 0L, 0L, 0L);
    } else if (fmt == FMT_F16) {
        if (qw == 2) hipLaunchKernelGGL((attention_bf16_kernel<2, false, FMT_F16>), grid, dim3(256), AT_LDS, s, q, k, vt, valid, c, T, Tp, Tpv, nullptr, 0L, 0L, 0L, 0L);
        else hipLaunchKernelGGL((attention_bf16_kernel<1, false, FMT_F16>), grid, dim3(256), AT_LDS, s, q, k, vt, valid, c, T, Tp, Tpv, nullptr, 0L, 0L, 0L, 0L);
    } else {
        if (qw == 2) hipLaunchKernelGGL((attention_bf16_kernel<2, false>), grid, dim3(256), AT_LDS, s, q, k, vt, valid, c, T, Tp, Tpv, nullptr, 0L, 0L, 0L, 0L);
        else hipLaunchKernelGGL((attention_bf16_kernel<1, false>), grid, dim3(256), AT_LDS, s, q, k, vt, valid, c, T, Tp, Tpv, nullptr, 0L, 0L, 0L, 0L);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// packed layout (see attention_asm_kernel's PK): total_qb = the sum of every utterance's ceil(frames / 128); bf16 / fp16
int launch_attention_packed(const bf16_t* q, const bf16_t* k, const bf16_t* vt, const int* pk, int nclip, int total_qb, bf16_t* ctx,
                            int Ptot, hipStream_t s, int fmt) {
    if (Ptot % 64 != 0) { syl_set_error("launch_attention_packed", "slots must be whole 64-key tiles"); return 1; }
    const dim3 grid(total_qb * SYL_HEADS);
    if (fmt == FMT_F16) hipLaunchKernelGGL((attention_asm_kernel<false, FMT_F16, 0, true>), grid, dim3(256), 0, s, q, k, vt, nullptr, ctx, 0, Ptot, Ptot, nullptr, 0L, pk, nclip);
    else if (fmt == FMT_BF16) hipLaunchKernelGGL((attention_asm_kernel<false, FMT_BF16, 0, true>), grid, dim3(256), 0, s, q, k, vt, nullptr, ctx, 0, Ptot, Ptot, nullptr, 0L, pk, nclip);
    else { syl_set_error("launch_attention_packed", "bf16 / fp16 only"); return 1; }
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_attention(const bf16_t* q, const bf16_t* k, const bf16_t* vt, const int* valid, bf16_t* ctx, int B, int T, int Tp,
                     int Tpv, int qw, hipStream_t s, int fmt, long lo_qk, long lo_vt, long lo_ctx) {
    return launch_attention_any(q, k, vt, valid, ctx, nullptr, 0, B, T, Tp, Tpv, qw, fmt, s, lo_qk, lo_vt, lo_ctx);
}

// same attention, context written as MXFP8 ([B*Tp][768] e4m3 + K-pair-major E8M0 scales with row pitch scale_rows)
int launch_attention_f8out(const bf16_t* q, const bf16_t* k, const bf16_t* vt, const int* valid, uint8_t* ctx8, uint8_t* ctx_scale,
                           long scale_rows, int B, int T, int Tp, int Tpv, int qw, hipStream_t s) {
    return launch_attention_any(q, k, vt, valid, ctx8, ctx_scale, scale_rows, B, T, Tp, Tpv, qw, FMT_BF16, s);
}

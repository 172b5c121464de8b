// Op-level and debug entry points of libsylber_hip.so (include/sylber_hip_dev.h and the sylber_op_* part of sylber_hip.h): single launches on
// operands the caller supplies, and the GEMM / attention micro-benchmarks.  Only the tests and tools/ call them; the forward does not.
#include "ctx.h"

// ------------------------------------------------------------------------------------------------
// single-op entry points for unit parity tests
struct TmpBuf {
    void* p = nullptr;
    ~TmpBuf() { if (p) hipFree(p); }
    int alloc(size_t bytes) { return hipMalloc(&p, bytes) == hipSuccess ? 0 : 1; }
};

// `tile` argument of the op-level entry points: -1 = automatic, else tile id + 1000 x (workgroups per CU; 9 = one workgroup per tile)
// + 100000 x t (tail policy of the launch, GemmArgs::tune_tail: t = 1 never split by rows, t >= 2 force a split with tail tile id t - 2)
static void decode_tile(int tile, GemmArgs& g) {
    if (tile >= 1000000) { g.tune_mfma16 = -1; tile -= 1000000; if (tile == 999) tile = -1; }   // tile + 1000000: the 16-bit-output role on the 32x32x16 kernels (GemmArgs::tune_mfma16); 1000999 = that with the automatic tile
    const int t = tile >= 100000 ? tile / 100000 : 0;
    if (tile >= 100000) tile %= 100000;
    g.tune_tail = t == 0 ? 0 : (t == 1 ? -1 : t - 1);
    g.tune_cfg = tile < 0 ? 0 : tile % 1000 + 1;
    g.tune_persist = tile >= 9000 ? -1 : (tile >= 1000 ? tile / 1000 : 0);
}

extern "C" int sylber_op_linear(const float* a_dev, const float* w_dev, const float* bias_dev, float* c_dev, int32_t M,
                                int32_t N, int32_t K, int32_t act, int32_t precision, int32_t tile, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (precision == SYLBER_FP8) {
        // both operands quantised to MXFP8 on the device, contraction on the block-scaled fp8 MFMA
        if (K % 128 != 0) { syl_set_error("sylber_op_linear", "fp8 needs K % 128 == 0"); return 1; }
        TmpBuf a8, as, w8, wsc;
        const long Mp = ((long)M + 255) & ~255L, Np = ((long)N + 255) & ~255L;
        if (a8.alloc((size_t)M * K) || as.alloc((size_t)Mp * (K / 32)) || w8.alloc((size_t)N * K) || wsc.alloc((size_t)Np * (K / 32))) {
            syl_set_error("sylber_op_linear", "alloc"); return 1;
        }
        HIP_TRY(hipMemsetAsync(as.p, 127, (size_t)Mp * (K / 32), s)); HIP_TRY(hipMemsetAsync(wsc.p, 127, (size_t)Np * (K / 32), s));
        if (launch_mx_quant_rows(a_dev, K, (uint8_t*)a8.p, K, (uint8_t*)as.p, Mp, M, K, s)) return 1;
        if (launch_mx_quant_rows(w_dev, K, (uint8_t*)w8.p, K, (uint8_t*)wsc.p, Np, N, K, s)) return 1;
        GemmF8Args g = {};
        g.g.M = M; g.g.N = N; g.g.K = K; g.g.bias = bias_dev; g.g.act = act; g.g.out0 = c_dev; g.g.ld0 = N;
        g.g.tune_cfg = tile < 0 ? 0 : tile + 1;
        g.X8 = (uint8_t*)a8.p; g.ldx8 = K; g.XS = (uint8_t*)as.p; g.xs_rows = Mp; g.W8 = (uint8_t*)w8.p; g.WS = (uint8_t*)wsc.p; g.ws_rows = Np;
        if (launch_gemm_mxfp8(EPI_F32, g, s)) return 1;
        HIP_TRY(hipStreamSynchronize(s));
        return 0;
    }
    if (precision == SYLBER_SPLIT16) {
        // both operands as hi / lo half planes, three MFMA passes into one fp32 accumulator
        TmpBuf ab, wb;
        const long xp = (((long)M + 128) * K + 255) & ~255L, wp = (((long)N + 128) * K + 255) & ~255L;
        if (ab.alloc((size_t)xp * 4) || wb.alloc((size_t)wp * 4)) { syl_set_error("sylber_op_linear", "alloc"); return 1; }
        HIP_TRY(hipMemsetAsync(ab.p, 0, (size_t)xp * 4, s)); HIP_TRY(hipMemsetAsync(wb.p, 0, (size_t)wp * 4, s));
        if (launch_f32_to_split16(a_dev, (bf16_t*)ab.p, xp, (size_t)M * K, s)) return 1;
        if (launch_f32_to_split16(w_dev, (bf16_t*)wb.p, wp, (size_t)N * K, s)) return 1;
        GemmArgs g = {};
        g.X = (bf16_t*)ab.p; g.ldx = K; g.W = (bf16_t*)wb.p; g.M = M; g.N = N; g.K = K; g.bias = bias_dev; g.act = act;
        g.out0 = c_dev; g.ld0 = N; g.fmt = FMT_SPLIT; g.x_lo = xp; g.w_lo = wp;
        decode_tile(tile, g);
        if (launch_gemm_bf16(EPI_F32, g, s)) return 1;
        HIP_TRY(hipStreamSynchronize(s));
        return 0;
    }
    if (precision != SYLBER_BF16) { syl_set_error("sylber_op_linear", "precision must be bf16, fp8 or split16"); return 1; }
    TmpBuf ab, wb;
    if (ab.alloc(((size_t)M + 128) * K * 2) || wb.alloc(((size_t)N + 128) * K * 2)) { syl_set_error("sylber_op_linear", "alloc"); return 1; }
    if (launch_f32_to_bf16(a_dev, (bf16_t*)ab.p, (size_t)M * K, s)) return 1;
    if (launch_f32_to_bf16(w_dev, (bf16_t*)wb.p, (size_t)N * K, s)) return 1;
    GemmArgs g = {};
    g.X = (bf16_t*)ab.p; g.ldx = K; g.W = (bf16_t*)wb.p; g.M = M; g.N = N; g.K = K; g.bias = bias_dev; g.act = act;
    g.out0 = c_dev; g.ld0 = N; decode_tile(tile, g);
    if (launch_gemm_bf16(EPI_F32, g, s)) return 1;
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// the residual GEMM of an encoder block (attention out-projection, FFN2): pre[M,N] <- A W^T + bias + LayerNorm(pre) in place,
// the LayerNorm re-derived from the row statistics (mean, rstd) and affine the previous LayerNorm launch left (EPI_F32_RESLN)
extern "C" int sylber_op_linear_resln(const float* a_dev, const float* w_dev, const float* bias_dev, float* pre_dev,
                                      const float* stats_dev, const float* gamma_dev, const float* beta_dev, int32_t M, int32_t N,
                                      int32_t K, int32_t tile, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    TmpBuf ab, wb;
    if (ab.alloc(((size_t)M + 128) * K * 2) || wb.alloc(((size_t)N + 128) * K * 2)) { syl_set_error("sylber_op_linear_resln", "alloc"); return 1; }
    if (launch_f32_to_bf16(a_dev, (bf16_t*)ab.p, (size_t)M * K, s)) return 1;
    if (launch_f32_to_bf16(w_dev, (bf16_t*)wb.p, (size_t)N * K, s)) return 1;
    GemmArgs g = {};
    g.X = (bf16_t*)ab.p; g.ldx = K; g.W = (bf16_t*)wb.p; g.M = M; g.N = N; g.K = K; g.bias = bias_dev;
    g.out0 = pre_dev; g.ld0 = N; g.res = pre_dev; g.ldres = N; g.ln_stats = stats_dev; g.ln_gamma = gamma_dev; g.ln_beta = beta_dev;
    decode_tile(tile, g);
    if (launch_gemm_bf16(EPI_F32_RESLN, g, s)) return 1;
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// one 3-tap stride-2 conv layer of the feature extractor as the 16-bit forward runs it (implicit GEMM over channels-last rows in
// the chunk-major K order, GELU, 16-bit out): x [R, 512] fp32 rows (R >= 2 M + 1), w [512 out][512 in][3] fp32 (torch Conv1d
// layout), y16 [M, 512] bf16 words, y[m] = gelu(sum_{t, c} w[:, c, t] x[2 m + t, c])
extern "C" int sylber_op_conv3(const float* x_dev, const float* w_host, uint16_t* y16_dev, int32_t R, int32_t M, int32_t tile, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (M < 1 || R < 2 * M + 1) { syl_set_error("sylber_op_conv3", "need R >= 2 M + 1 input rows"); return 1; }
    TmpBuf xb, wb;
    if (xb.alloc(((size_t)R + 130) * 512 * 2) || wb.alloc((size_t)512 * 1536 * 2)) { syl_set_error("sylber_op_conv3", "alloc"); return 1; }
    HIP_TRY(hipMemsetAsync(xb.p, 0, ((size_t)R + 130) * 512 * 2, s));
    if (launch_f32_to_bf16(x_dev, (bf16_t*)xb.p, (size_t)R * 512, s)) return 1;
    std::vector<bf16_t> wp((size_t)512 * 1536);
    for (int o = 0; o < 512; ++o)
        for (int pos = 0; pos < 1536; ++pos) {
            const int e = tap3_offset(pos * 2) / 2, t = e / 512, cc = e % 512;     // operand-row element = (tap t, channel cc)
            wp[(size_t)o * 1536 + pos] = f2bf(w_host[((size_t)o * 512 + cc) * 3 + t]);
        }
    HIP_TRY(hipMemcpyAsync(wb.p, wp.data(), wp.size() * 2, hipMemcpyHostToDevice, s));
    GemmArgs g = {};
    g.X = (bf16_t*)xb.p; g.ldx = 1024; g.W = (bf16_t*)wb.p; g.M = M; g.N = 512; g.K = 1536; g.act = ACT_GELU_FAST; g.kpat = 1;
    g.out0 = y16_dev; g.ld0 = 512; decode_tile(tile, g);
    if (launch_gemm_bf16(EPI_BF16, g, s)) return 1;
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// the same GEMM with its 16-bit output epilogue (EPI_BF16: what the conv layers and FFN1 run): C16 = bf16 / fp16 words
extern "C" int sylber_op_linear16(const float* a_dev, const float* w_dev, const float* bias_dev, uint16_t* c16_dev, int32_t M,
                                  int32_t N, int32_t K, int32_t act, int32_t precision, int32_t tile, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (precision != SYLBER_BF16 && precision != SYLBER_FP16) { syl_set_error("sylber_op_linear16", "precision must be bf16 or fp16"); return 1; }
    if (precision == SYLBER_FP16) { syl_set_error("sylber_op_linear16", "fp16 operands are packed by sylber_create only"); return 1; }
    TmpBuf ab, wb;
    if (ab.alloc(((size_t)M + 128) * K * 2) || wb.alloc(((size_t)N + 128) * K * 2)) { syl_set_error("sylber_op_linear16", "alloc"); return 1; }
    if (launch_f32_to_bf16(a_dev, (bf16_t*)ab.p, (size_t)M * K, s)) return 1;
    if (launch_f32_to_bf16(w_dev, (bf16_t*)wb.p, (size_t)N * K, s)) return 1;
    GemmArgs g = {};
    g.X = (bf16_t*)ab.p; g.ldx = K; g.W = (bf16_t*)wb.p; g.M = M; g.N = N; g.K = K; g.bias = bias_dev; g.act = act;
    g.out0 = c16_dev; g.ld0 = N; decode_tile(tile, g);
    if (launch_gemm_bf16(EPI_BF16, g, s)) return 1;
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

extern "C" int sylber_op_mx_quantize(const float* x_dev, int32_t R, int32_t K, uint8_t* data_dev, uint8_t* scale_dev, void* stream) {
    if (!x_dev || !data_dev || !scale_dev) { syl_set_error("sylber_op_mx_quantize", "null argument"); return 1; }
    return launch_mx_quant_rows(x_dev, K, data_dev, K, scale_dev, R, R, K, (hipStream_t)stream);
}

extern "C" int sylber_op_layernorm(const float* x_dev, const float* res_dev, const float* g_dev, const float* b_dev,
                                   float* y_dev, int32_t M, int32_t D, void* stream) {
    LnArgs a = {};
    a.in = x_dev; a.in_bf16 = 0; a.ld_in = D; a.res = res_dev; a.ld_res = D; a.gamma = g_dev; a.beta = b_dev;
    a.out_f32 = y_dev; a.ld_f32 = D; a.M = M; a.D = D;
    return launch_layernorm(a, (hipStream_t)stream);
}

// q,k,v [B,T,768] f32 -> bf16 head-major q (x SYL_Q_SCALE = log2(e) / 8), k and key-permuted V^T
__global__ void pack_qkv_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                bf16_t* __restrict__ qo, bf16_t* __restrict__ ko, bf16_t* __restrict__ vto, int T, int Tp, int Tpv) {
    const int b = blockIdx.y, t = blockIdx.x;
    for (int c = threadIdx.x; c < 768; c += 256) {
        const int head = c >> 6, d = c & 63;
        const size_t src = ((size_t)b * T + t) * 768 + c;
        const size_t hm = (((size_t)b * 12 + head) * Tp + t) * 64 + d;
        qo[hm] = f2bf(q[src] * SYL_Q_SCALE);
        ko[hm] = f2bf(k[src]);
        const int pos = (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1);
        vto[(((size_t)b * 12 + head) * 64 + d) * Tpv + pos] = f2bf(v[src]);
    }
}

// The layer tap SYLBER_LTAP_QKV (forward.hip): what EPI_QK left in the workspace, back in natural order and widened exactly.  q / k
// [B][12][Tp][64] head-major, V^T [B][12][64][Tpv] with bits 2 and 3 of the key index swapped (attention.hip) -> out [B][T][2304] =
// q | k | v of frames [0, T); FMT_SPLIT adds the lo planes lo_qk / lo_vt elements on.  pos < Tp: the swap stays inside a 16-key group
// and Tp is a multiple of 32.
__global__ __launch_bounds__(256) void tap_qkv_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ vt,
                                                      float* __restrict__ out, int T, int Tp, int Tpv, int fmt, long lo_qk, long lo_vt) {
    const int b = blockIdx.y, t = blockIdx.x;
    const int pos = (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1);
    float* dst = out + ((size_t)b * T + t) * (3 * SYL_HIDDEN);
    for (int c = threadIdx.x; c < SYL_HIDDEN; c += 256) {
        const int head = c >> 6, d = c & 63;
        const size_t hm = (((size_t)b * SYL_HEADS + head) * Tp + t) * 64 + d;
        const size_t vi = (((size_t)b * SYL_HEADS + head) * 64 + d) * Tpv + pos;
        if (fmt == FMT_SPLIT) {
            dst[c] = H16<FMT_F16>::up(q[hm]) + H16<FMT_F16>::up(q[lo_qk + hm]);
            dst[SYL_HIDDEN + c] = H16<FMT_F16>::up(k[hm]) + H16<FMT_F16>::up(k[lo_qk + hm]);
            dst[2 * SYL_HIDDEN + c] = H16<FMT_F16>::up(vt[vi]) + H16<FMT_F16>::up(vt[lo_vt + vi]);
        } else if (fmt == FMT_F16) {
            dst[c] = H16<FMT_F16>::up(q[hm]); dst[SYL_HIDDEN + c] = H16<FMT_F16>::up(k[hm]); dst[2 * SYL_HIDDEN + c] = H16<FMT_F16>::up(vt[vi]);
        } else {
            dst[c] = bf2f(q[hm]); dst[SYL_HIDDEN + c] = bf2f(k[hm]); dst[2 * SYL_HIDDEN + c] = bf2f(vt[vi]);
        }
    }
}
int launch_tap_qkv(const bf16_t* q, const bf16_t* k, const bf16_t* vt, float* out, int B, int T, int Tp, int Tpv, hipStream_t s, int fmt, long lo_qk, long lo_vt) {
    if (T < 1 || T > Tp || Tp % 32 != 0 || Tpv < Tp) { syl_set_error("launch_tap_qkv", "need 1 <= T <= Tp, Tp % 32 == 0, Tpv >= Tp"); return 1; }
    hipLaunchKernelGGL(tap_qkv_kernel, dim3(T, B), dim3(256), 0, s, q, k, vt, out, T, Tp, Tpv, fmt, lo_qk, lo_vt);
    HIP_TRY(hipGetLastError());
    return 0;
}

// q,k [B,T,768] f32 -> MXFP8 head-major q (x0.125), k: e4m3 [B,H,Tp,64] + one E8M0 scale per 32 features [B,H,Tp,2].
// One 32-lane group per (token, head, 32-feature block).
__global__ void pack_qk_f8_kernel(const float* __restrict__ q, const float* __restrict__ k, uint8_t* __restrict__ q8, uint8_t* __restrict__ qs,
                                  uint8_t* __restrict__ k8, uint8_t* __restrict__ ks, int T, int Tp) {
    const int b = blockIdx.y, t = blockIdx.x;
    for (int c = threadIdx.x; c < 768; c += 256) {
        const int head = c >> 6, d = c & 63;
        const size_t src = ((size_t)b * T + t) * 768 + c;
        const size_t row = ((size_t)b * 12 + head) * Tp + t;
        const float v[2] = {q[src] * 0.125f, k[src]};
        uint8_t* dst[2] = {q8, k8};
        uint8_t* sc[2] = {qs, ks};
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            float amax = fabsf(v[w]);
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
            const unsigned e = mx_e8m0(amax);
            dst[w][row * 64 + d] = (uint8_t)(pack_fp8x4(v[w] * mx_inv_scale(e), 0.f, 0.f, 0.f) & 0xffu);
            if ((d & 31) == 0) sc[w][row * 2 + (d >> 5)] = (uint8_t)e;
        }
    }
}
// v [B,T,768] f32 -> V^T MXFP8: e4m3 [B,H,64,Tpv] (natural key order) + one E8M0 scale per 32 keys [B,H,64,Tpv/32]; keys >= T are zero.
// One thread per (feature, 32-key block).
__global__ void pack_vt_f8_kernel(const float* __restrict__ v, uint8_t* __restrict__ v8, uint8_t* __restrict__ vs, int T, int Tpv) {
    const int b = blockIdx.y, kb = blockIdx.x;           // 32-key block
    for (int c = threadIdx.x; c < 768; c += 256) {
        const int head = c >> 6, d = c & 63;
        float x[32];
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int t = kb * 32 + i;
            x[i] = t < T ? v[((size_t)b * T + t) * 768 + c] : 0.f;
            amax = fmaxf(amax, fabsf(x[i]));
        }
        const unsigned e = mx_e8m0(amax);
        const float inv = mx_inv_scale(e);
        const size_t row = ((size_t)b * 12 + head) * 64 + d;
        unsigned* dst = (unsigned*)(v8 + row * Tpv + kb * 32);
#pragma unroll
        for (int i = 0; i < 8; ++i) dst[i] = pack_fp8x4(x[4 * i] * inv, x[4 * i + 1] * inv, x[4 * i + 2] * inv, x[4 * i + 3] * inv);
        vs[row * (Tpv / 32) + kb] = (uint8_t)e;
    }
}

struct AttnF8Bufs {
    TmpBuf q8, qs, k8, ks, v8, vs, cb;
    int alloc(int B, int Tp, int Tpv) {
        const size_t n = (size_t)B * Tp * 768;
        // (k and its scales: one 64-key tile of slack, as in the bf16 path)
        return q8.alloc(n) || qs.alloc(n / 32) || k8.alloc(n + 64 * 64) || ks.alloc(n / 32 + 128) || v8.alloc((size_t)B * 768 * Tpv) ||
               vs.alloc((size_t)B * 768 * (Tpv / 32)) || cb.alloc(n * 2);
    }
    int clear(int B, int Tp, int Tpv, hipStream_t s) {
        const size_t n = (size_t)B * Tp * 768;
        HIP_TRY(hipMemsetAsync(q8.p, 0, n, s)); HIP_TRY(hipMemsetAsync(qs.p, 127, n / 32, s));
        HIP_TRY(hipMemsetAsync(k8.p, 0, n + 64 * 64, s)); HIP_TRY(hipMemsetAsync(ks.p, 127, n / 32 + 128, s));
        HIP_TRY(hipMemsetAsync(v8.p, 0, (size_t)B * 768 * Tpv, s)); HIP_TRY(hipMemsetAsync(vs.p, 127, (size_t)B * 768 * (Tpv / 32), s));
        HIP_TRY(hipMemsetAsync(cb.p, 0, n * 2, s));
        return 0;
    }
};

extern "C" int sylber_op_attention(const float* q_dev, const float* k_dev, const float* v_dev, const int32_t* valid_dev,
                                   float* o_dev, int32_t B, int32_t T, int32_t precision, int32_t queries_per_wave, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (precision != SYLBER_BF16 && precision != SYLBER_FP8) { syl_set_error("sylber_op_attention", "precision: SYLBER_BF16 or SYLBER_FP8"); return 1; }
    const int Tp = (T + 31) & ~31, Tpv = (Tp + 63) & ~63;
    if (precision == SYLBER_FP8) {
        AttnF8Bufs f;
        if (f.alloc(B, Tp, Tpv)) { syl_set_error("sylber_op_attention", "alloc"); return 1; }
        if (f.clear(B, Tp, Tpv, s)) return 1;
        hipLaunchKernelGGL(pack_qk_f8_kernel, dim3(T, B), dim3(256), 0, s, q_dev, k_dev, (uint8_t*)f.q8.p, (uint8_t*)f.qs.p, (uint8_t*)f.k8.p, (uint8_t*)f.ks.p, T, Tp);
        hipLaunchKernelGGL(pack_vt_f8_kernel, dim3(Tpv / 32, B), dim3(256), 0, s, v_dev, (uint8_t*)f.v8.p, (uint8_t*)f.vs.p, T, Tpv);
        if (launch_attention_f8((uint8_t*)f.q8.p, (uint8_t*)f.qs.p, (uint8_t*)f.k8.p, (uint8_t*)f.ks.p, (uint8_t*)f.v8.p, (uint8_t*)f.vs.p, valid_dev,
                                f.cb.p, nullptr, 0, B, T, Tp, Tpv, s)) return 1;
        if (launch_bf16_to_f32_rows((bf16_t*)f.cb.p, 768, o_dev, B, Tp, T, 768, s)) return 1;
        HIP_TRY(hipStreamSynchronize(s));
        return 0;
    }
    const int qw = queries_per_wave == 32 ? 1 : (queries_per_wave == 64 ? 2 : 0);
    TmpBuf qb, kb, vb, cb;
    const size_t n = (size_t)B * Tp * 768;
    // (k: one 64-key tile of slack -- the kernel's last K tile may start at Tp - 32 and reads 64 rows; the scores of rows >= Tp are masked)
    if (qb.alloc(n * 2) || kb.alloc(n * 2 + 64 * 64 * 2) || vb.alloc((size_t)B * 768 * Tpv * 2) || cb.alloc(n * 2)) { syl_set_error("sylber_op_attention", "alloc"); return 1; }
    HIP_TRY(hipMemsetAsync(qb.p, 0, n * 2, s)); HIP_TRY(hipMemsetAsync(kb.p, 0, n * 2 + 64 * 64 * 2, s));
    HIP_TRY(hipMemsetAsync(vb.p, 0, (size_t)B * 768 * Tpv * 2, s)); HIP_TRY(hipMemsetAsync(cb.p, 0, n * 2, s));
    hipLaunchKernelGGL(pack_qkv_kernel, dim3(T, B), dim3(256), 0, s, q_dev, k_dev, v_dev, (bf16_t*)qb.p, (bf16_t*)kb.p, (bf16_t*)vb.p, T, Tp, Tpv);
    if (launch_attention((bf16_t*)qb.p, (bf16_t*)kb.p, (bf16_t*)vb.p, valid_dev, (bf16_t*)cb.p, B, T, Tp, Tpv, qw, s)) return 1;
    if (launch_bf16_to_f32_rows((bf16_t*)cb.p, 768, o_dev, B, Tp, T, 768, s)) return 1;
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}


__global__ void fill_random_bf16(bf16_t* p, size_t n, unsigned seed);
// test aid: every byte of the handle's activation workspace becomes `byte` (0xFF: NaN patterns in every format), and the next forward
// re-runs the zeroing of the regions that are read without being written (as after a batch-shape change).  A forward that then
// returns the same bits as before reads nothing it has not written -- stale data can never leak into a result.
extern "C" int sylber_debug_poison_workspace(sylber_t c, int32_t byte) {
    if (!c) { syl_set_error("sylber_debug_poison_workspace", "null handle"); return 1; }
    GUARD_DEVICE(c->device);
    HIP_TRY(hipDeviceSynchronize());
    if (c->ws) HIP_TRY(hipMemset(c->ws, byte & 0xff, c->ws_bytes));
    if (c->seg_scratch) HIP_TRY(hipMemset(c->seg_scratch, byte & 0xff, c->seg_scratch_floats * 4));   // (long-utterance bookkeeping slab of sylber_segment)
    c->ws_B = 0; c->ws_Lmax = 0;
    graphs_clear(c);
    return 0;
}

// test aid: conv0's GroupNorm table of the handle's last forward, [B][512][2] = (a_c, b_c) with a = gamma / sqrt(var + eps) and
// b = beta - mean a (conv0_finalize_kernel), copied to the host.  It lives in the workspace and is overwritten by the next forward.
extern "C" int sylber_debug_conv0_scale_shift(sylber_t c, int32_t B, float* out_host) {
    if (!c || !out_host) { syl_set_error("sylber_debug_conv0_scale_shift", "null argument"); return 1; }
    if (!c->dbg_ss || !c->ws || B < 1 || B != c->dbg_ss_B) { syl_set_error("sylber_debug_conv0_scale_shift", "B must be the batch size of the handle's last forward"); return 1; }
    GUARD_DEVICE(c->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_host, c->dbg_ss, (size_t)B * SYL_CONV * 2 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// kernel-only timing of the attention core on random packed operands (development aid): precision SYLBER_BF16 or SYLBER_FP8
extern "C" int sylber_debug_attention_bench(int32_t B, int32_t T, int32_t precision, int32_t iters, float* ms_out) {
    const int Tp = (T + 31) & ~31, Tpv = (Tp + 63) & ~63;
    const size_t n = (size_t)B * Tp * 768;
    TmpBuf qin;
    if (qin.alloc((size_t)B * T * 768 * 4 * 3)) { syl_set_error("sylber_debug_attention_bench", "alloc"); return 1; }
    float* q = (float*)qin.p; float* k = q + (size_t)B * T * 768; float* v = k + (size_t)B * T * 768;
    const bool zero_data = iters < 0;         // iters < 0: all-zero operands (DVFS probe: the same instruction stream at lower switching power)
    if (zero_data) { iters = -iters; HIP_TRY(hipMemset(qin.p, 0, (size_t)B * T * 768 * 4 * 3)); }
    else
    {   // pseudo-random fp32 q, k, v in [-1, 1) via the bf16 filler (values irrelevant for timing beyond being finite)
        TmpBuf tmp;
        if (tmp.alloc((size_t)B * T * 768 * 3 * 2)) { syl_set_error("sylber_debug_attention_bench", "alloc"); return 1; }
        hipLaunchKernelGGL(fill_random_bf16, dim3(2048), dim3(256), 0, 0, (bf16_t*)tmp.p, (size_t)B * T * 768 * 3, 7u);
        if (launch_bf16_to_f32_rows((bf16_t*)tmp.p, 768, q, 3 * B, T, T, 768, 0)) return 1;
        HIP_TRY(hipDeviceSynchronize());
    }
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    int rc = 0;
    if (precision == SYLBER_FP8) {
        AttnF8Bufs f;
        if (f.alloc(B, Tp, Tpv) || f.clear(B, Tp, Tpv, 0)) { syl_set_error("sylber_debug_attention_bench", "alloc"); return 1; }
        hipLaunchKernelGGL(pack_qk_f8_kernel, dim3(T, B), dim3(256), 0, 0, q, k, (uint8_t*)f.q8.p, (uint8_t*)f.qs.p, (uint8_t*)f.k8.p, (uint8_t*)f.ks.p, T, Tp);
        hipLaunchKernelGGL(pack_vt_f8_kernel, dim3(Tpv / 32, B), dim3(256), 0, 0, v, (uint8_t*)f.v8.p, (uint8_t*)f.vs.p, T, Tpv);
        auto run = [&]() { return launch_attention_f8((uint8_t*)f.q8.p, (uint8_t*)f.qs.p, (uint8_t*)f.k8.p, (uint8_t*)f.ks.p, (uint8_t*)f.v8.p, (uint8_t*)f.vs.p,
                                                      nullptr, f.cb.p, nullptr, 0, B, T, Tp, Tpv, 0); };
        for (int i = 0; i < 3 && !rc; ++i) rc = run();
        hipEventRecord(e0, 0);
        for (int i = 0; i < iters && !rc; ++i) rc = run();
        hipEventRecord(e1, 0);
        hipEventSynchronize(e1);
    } else {
        TmpBuf qb, kb, vb, cb;
        if (qb.alloc(n * 2) || kb.alloc(n * 2 + 64 * 64 * 2) || vb.alloc((size_t)B * 768 * Tpv * 2) || cb.alloc(n * 2)) { syl_set_error("sylber_debug_attention_bench", "alloc"); return 1; }
        HIP_TRY(hipMemset(qb.p, 0, n * 2)); HIP_TRY(hipMemset(kb.p, 0, n * 2 + 64 * 64 * 2)); HIP_TRY(hipMemset(vb.p, 0, (size_t)B * 768 * Tpv * 2));
        hipLaunchKernelGGL(pack_qkv_kernel, dim3(T, B), dim3(256), 0, 0, q, k, v, (bf16_t*)qb.p, (bf16_t*)kb.p, (bf16_t*)vb.p, T, Tp, Tpv);
        // precision SYLBER_BF16: the default kernel (hand-scheduled key loop); 132 / 164: the compiler-scheduled kernels, 32 / 64 queries per wave
        const int qw = precision == 132 ? 1 : (precision == 164 ? 2 : (precision > 200 && precision < 220 ? precision - 100 : 0));   // 201..209: knock-out variants (experiments build)
        auto run = [&]() { return launch_attention((bf16_t*)qb.p, (bf16_t*)kb.p, (bf16_t*)vb.p, nullptr, (bf16_t*)cb.p, B, T, Tp, Tpv, qw, 0); };
        for (int i = 0; i < 3 && !rc; ++i) rc = run();
        hipEventRecord(e0, 0);
        for (int i = 0; i < iters && !rc; ++i) rc = run();
        hipEventRecord(e1, 0);
        hipEventSynchronize(e1);
    }
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    *ms_out = ms / (iters > 0 ? iters : 1);
    hipEventDestroy(e0); hipEventDestroy(e1);
    return rc;
}

// ------------------------------------------------------------------------------------------------
// GEMM micro-benchmark (development aid): times `iters` launches of the bf16 GEMM on pseudo-random
// operands with HIP events.  cfg: -1 auto, 0 = 256x128, 1 = 128x192, 2 = 128x128 tiles.
__global__ void fill_random_bf16(bf16_t* p, size_t n, unsigned seed) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        unsigned x = (unsigned)i * 2654435761u + seed;
        x ^= x >> 15; x *= 2246822519u; x ^= x >> 13; x *= 3266489917u; x ^= x >> 16;
        p[i] = f2bf(((float)(x & 0xffff) / 32768.0f - 1.0f) * 0.5f);
    }
}
__global__ void fill_random_fp8(uint8_t* p, size_t n, unsigned seed, int scale_bytes) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        unsigned x = (unsigned)i * 2654435761u + seed;
        x ^= x >> 15; x *= 2246822519u; x ^= x >> 13;
        unsigned b = x & 0xffu;
        if ((b & 0x7fu) == 0x7fu) b ^= 1u;                    // no NaN codes
        p[i] = scale_bytes ? (uint8_t)(124u + (b & 7u)) : (uint8_t)b;
    }
}

// MXFP8 leg of the micro-benchmark: cfg = 100 + tile config (0 = 128x192, 1 = 128x128, 2 = 256x256 8-wave, 3 = 256x192 8-wave); epi 0 = MXFP8 output (FFN1),
// 1 = fp32 output, 6 = fp32 residual + LayerNorm re-derivation (FFN2)
static int gemm_bench_f8(int M, int N, int K, int epi, int act, int cfg, int iters, float* ms_out) {
    TmpBuf xb, xs, wb, wsb, ob, os, bb, st;
    const long Mp = ((long)M + 255) & ~255L, Np = ((long)N + 255) & ~255L;
    if (xb.alloc((size_t)M * K) || xs.alloc((size_t)Mp * (K / 32)) || wb.alloc((size_t)N * K) || wsb.alloc((size_t)Np * (K / 32)) ||
        ob.alloc((size_t)M * N * 4) || os.alloc((size_t)Mp * (N / 32 + 2)) || bb.alloc((size_t)N * 4 * 3) || st.alloc((size_t)M * 8)) {
        syl_set_error("sylber_debug_gemm_bench", "alloc"); return 1;
    }
    hipLaunchKernelGGL(fill_random_fp8, dim3(2048), dim3(256), 0, 0, (uint8_t*)xb.p, (size_t)M * K, 1u, 0);
    hipLaunchKernelGGL(fill_random_fp8, dim3(2048), dim3(256), 0, 0, (uint8_t*)wb.p, (size_t)N * K, 2u, 0);
    hipLaunchKernelGGL(fill_random_fp8, dim3(256), dim3(256), 0, 0, (uint8_t*)xs.p, (size_t)Mp * (K / 32), 3u, 1);
    hipLaunchKernelGGL(fill_random_fp8, dim3(256), dim3(256), 0, 0, (uint8_t*)wsb.p, (size_t)Np * (K / 32), 4u, 1);
    HIP_TRY(hipMemset(bb.p, 0, (size_t)N * 12)); HIP_TRY(hipMemset(st.p, 0, (size_t)M * 8)); HIP_TRY(hipMemset(ob.p, 0, (size_t)M * N * 4));
    GemmF8Args g = {};
    g.g.M = M; g.g.N = N; g.g.K = K; g.g.bias = (float*)bb.p; g.g.act = act; g.g.out0 = ob.p; g.g.ld0 = N;
    g.g.res = (float*)ob.p; g.g.ldres = N; g.g.ln_stats = (float*)st.p; g.g.ln_gamma = (float*)bb.p + N; g.g.ln_beta = (float*)bb.p + 2 * N;
    g.X8 = (uint8_t*)xb.p; g.ldx8 = K; g.XS = (uint8_t*)xs.p; g.xs_rows = Mp; g.W8 = (uint8_t*)wb.p; g.WS = (uint8_t*)wsb.p; g.ws_rows = Np;
    g.out_scale = (uint8_t*)os.p; g.os_rows = Mp;
    const int e = epi == 0 ? EPI_MXFP8 : (epi == 6 ? EPI_F32_RESLN : EPI_F32);
    g.g.tune_cfg = cfg < 0 ? 0 : cfg + 1;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    int rc = 0;
    for (int i = 0; i < 3 && !rc; ++i) rc = launch_gemm_mxfp8(e, g, 0);
    hipEventRecord(e0, 0);
    for (int i = 0; i < iters && !rc; ++i) rc = launch_gemm_mxfp8(e, g, 0);
    hipEventRecord(e1, 0);
    hipEventSynchronize(e1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    *ms_out = ms / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
    return rc;
}

static int gemm_bench_impl(int32_t M, int32_t N, int32_t K, int32_t ldx, int32_t epi, int32_t act, int32_t cfg, int32_t iters,
                           float* ms_out, unsigned long long* g_gemm_trace_out) {
    if (cfg >= 100 && cfg < 200) return gemm_bench_f8(M, N, K, epi, act, cfg - 100, iters, ms_out);
    const bool no_h192 = act >= 10000;                    // act + 10000: the cost model without the 192-row tiles (A/B)
    act %= 10000;
    const int tail_code = act / 100;                      // act + 100 t: tail policy of the launch (GemmArgs::tune_tail)
    act %= 100;
    const bool legacy16 = cfg >= 1000000;                 // cfg + 1000000: the 16-bit-output role on the 32x32x16 kernels (GemmArgs::tune_mfma16 = -1)
    if (legacy16) cfg -= 1000000;
    const bool kpat = cfg >= 350000;                      // cfg + 400000: the 3-tap conv layers' chunk-major K order (K = 1536, ldx = 1024)
    if (kpat) cfg -= 400000;
    const bool cold = cfg >= 150000;                      // cfg + 200000: operands flushed out of the caches before every launch
    if (cold) cfg -= 200000;
    TmpBuf xb, wb, ob, rb, bb;
    const size_t xn = (size_t)(M + 8) * ldx + K, wn = (size_t)N * K;
    if (xb.alloc(xn * 2) || wb.alloc(wn * 2) || ob.alloc((size_t)M * N * 4) || rb.alloc((size_t)M * N * 4) || bb.alloc((size_t)N * 4)) {
        syl_set_error("sylber_debug_gemm_bench", "alloc"); return 1;
    }
    hipLaunchKernelGGL(fill_random_bf16, dim3(2048), dim3(256), 0, 0, (bf16_t*)xb.p, xn, 1u);
    hipLaunchKernelGGL(fill_random_bf16, dim3(2048), dim3(256), 0, 0, (bf16_t*)wb.p, wn, 2u);
    HIP_TRY(hipMemset(rb.p, 0, (size_t)M * N * 4)); HIP_TRY(hipMemset(bb.p, 0, (size_t)N * 4));
    GemmArgs g = {};
    g.X = (bf16_t*)xb.p; g.ldx = ldx; g.W = (bf16_t*)wb.p; g.M = M; g.N = N; g.K = K; g.bias = (float*)bb.p; g.act = act;
    g.out0 = ob.p; g.ld0 = N; g.res = (float*)rb.p; g.ldres = N; g.kpat = kpat ? 1 : 0;
    TmpBuf lnb;
    if (epi == EPI_F32_RESLN) {
        if (lnb.alloc((size_t)M * 8 + (size_t)N * 8)) { syl_set_error("sylber_debug_gemm_bench", "alloc"); return 1; }
        HIP_TRY(hipMemset(lnb.p, 0, (size_t)M * 8 + (size_t)N * 8));
        g.ln_stats = (float*)lnb.p; g.ln_gamma = (float*)lnb.p + (size_t)M * 2; g.ln_beta = g.ln_gamma + N;
    }
    g.Tp = 512; g.Tpv = 512; g.T = 499;               // EPI_QK: rows = (utterance, frame) at this pitch
    TmpBuf qkb;
    if (epi == EPI_QK) {
        if (qkb.alloc((size_t)(M + 512) * 768 * 2 * 3)) { syl_set_error("sylber_debug_gemm_bench", "alloc"); return 1; }
        g.out0 = qkb.p; g.out1 = (char*)qkb.p + (size_t)(M + 512) * 768 * 2; g.out2 = (char*)qkb.p + (size_t)(M + 512) * 768 * 4;
    }
    g.tune_cfg = cfg < 0 ? 0 : (cfg % 1000) + 1;
    g.tune_persist = cfg >= 9000 ? -1 : (cfg >= 1000 ? cfg / 1000 : 0);    // cfg = persist * 1000 + tile (9000 + tile: persist = -1)
    g.tune_h192 = no_h192 ? -1 : 0; g.tune_model = no_h192 ? 5 : 0;
    g.tune_mfma16 = legacy16 ? -1 : 0;
    g.tune_tail = tail_code == 0 ? 0 : (tail_code == 1 ? -1 : tail_code - 1);   // act + 100 t: t = 1 never split, t >= 2 force tail tile id t - 2
    TmpBuf trb;
    if (g_gemm_trace_out) {
        if (trb.alloc(20 * 8)) { syl_set_error("sylber_debug_gemm_bench", "alloc"); return 1; }
        HIP_TRY(hipMemset(trb.p, 0, 20 * 8));
        g.trace = (unsigned long long*)trb.p;
    }
    struct TraceFetch {
        TmpBuf& b; unsigned long long* dst;
        ~TraceFetch() { if (dst && b.p) { hipDeviceSynchronize(); hipMemcpy(dst, b.p, 20 * 8, hipMemcpyDeviceToHost); } }
    } trace_fetch{trb, g_gemm_trace_out};
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    int rc = 0;
    for (int i = 0; i < 3 && !rc; ++i) rc = launch_gemm_bf16(epi, g, 0);
    if (cold) {
        // every timed launch finds its operands COLD: 1 GiB is written between the launches (the 256 MB memory-side cache
        // and the L2s hold none of X / W / res afterwards), each launch timed by its own event pair
        TmpBuf flush;
        if (flush.alloc((size_t)1 << 30)) { syl_set_error("sylber_debug_gemm_bench", "alloc"); return 1; }
        float tot = 0.f;
        for (int i = 0; i < iters && !rc; ++i) {
            hipMemsetAsync(flush.p, i & 0xff, (size_t)1 << 30, 0);
            hipEventRecord(e0, 0);
            rc = launch_gemm_bf16(epi, g, 0);
            hipEventRecord(e1, 0);
            hipEventSynchronize(e1);
            float ms1 = 0.f;
            hipEventElapsedTime(&ms1, e0, e1);
            tot += ms1;
        }
        *ms_out = tot / iters;
        hipEventDestroy(e0); hipEventDestroy(e1);
        return rc;
    }
    hipEventRecord(e0, 0);
    for (int i = 0; i < iters && !rc; ++i) rc = launch_gemm_bf16(epi, g, 0);
    hipEventRecord(e1, 0);
    hipEventSynchronize(e1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    *ms_out = ms / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
    return rc;
}

// which tile the cost model of launch_gemm_bf16 picks (host arithmetic only; no device is touched): epi / act as GemmEpi / GemmAct, fmt 0 bf16 / 1 fp16,
// model = SYLBER_OPT_GEMM_MODEL (0: the handle owns the chip, 5: shares it), kpat = 1 for the 3-tap conv K order
extern "C" int sylber_debug_gemm_pick(int32_t M, int32_t N, int32_t K, int32_t epi, int32_t act, int32_t fmt, int32_t model, int32_t kpat) {
    GemmArgs g = {};
    g.M = M; g.N = N; g.K = K; g.act = act; g.fmt = fmt; g.tune_model = model % 100; g.kpat = kpat;
    g.tune_mfma16 = model >= 100 ? -1 : 0;               // model + 100: the 16-bit-output role on the 32x32x16 kernels
    return gemm_pick_tile(epi, g);
}

// which kernel instantiation(s) launch_gemm_bf16 resolves a launch to (gemm_plan; host arithmetic only, no device is touched): the launch as
// sylber_debug_gemm_pick describes it (fmt 2 = split16), `tile` in the encoding of the op-level entry points (decode_tile), h192 / pre / tail =
// GemmArgs::tune_h192 / tune_pre / tune_tail (tail 0: what `tile` encodes).  One line per launch of the plan goes to buf: "<first row> <end row>
// <kernel template>[<its template arguments>]".  Returns the number of launches; 0 = refused (sylber_last_error), -1 = buf too small
extern "C" int sylber_debug_gemm_resolve(int32_t M, int32_t N, int32_t K, int32_t epi, int32_t act, int32_t fmt, int32_t kpat, int32_t tile,
                                         int32_t model, int32_t h192, int32_t pre, int32_t tail, char* buf, int32_t cap) {
    GemmArgs g = {};
    g.M = M; g.N = N; g.K = K; g.act = act; g.fmt = fmt; g.kpat = kpat; g.tune_model = model; g.tune_h192 = h192; g.tune_pre = pre;
    decode_tile(tile, g);
    if (tail) g.tune_tail = tail;
    const GemmPlan p = gemm_plan(epi, g);
    int used = 0;
    for (int i = 0; i < p.n; ++i) {
        // "GemmKernel kern::<template>() [<arguments>]" (__PRETTY_FUNCTION__) -> "<template>[<arguments>]"
        const char* nm = strstr(p.k[i].name, "kern::");
        nm = nm ? nm + 6 : p.k[i].name;
        const char* par = strstr(nm, "() ");
        const int w = snprintf(buf + used, (size_t)(cap - used), "%d %d %.*s%s\n", p.a[i].m_begin, p.a[i].M, par ? (int)(par - nm) : (int)strlen(nm), nm, par ? par + 3 : "");
        if (w < 0 || w >= cap - used) return -1;
        used += w;
    }
    return p.n;
}

extern "C" int sylber_debug_gemm_bench(int32_t M, int32_t N, int32_t K, int32_t ldx, int32_t epi, int32_t act, int32_t cfg,
                                       int32_t iters, float* ms_out) {
    return gemm_bench_impl(M, N, K, ldx, epi, act, cfg, iters, ms_out, nullptr);
}

// the trace instantiation of the 8-wave kernel (tile id 30: s_memtime stamps around the phases of the K loop): one
// launch series, then the 2 x 10 cycle counters of workgroup 0's waves 0 (group 0) and 4 (group 1):
// [0] sum A (loop top -> fragments landed), [1] sum barrier after A, [2] sum B (MFMA + DMA issue), [3] sum barrier after B,
// [4] K loop total, [5] steps, [6] cost of one stamp, [7] epilogue, [8] prologue, [9] tile total
extern "C" int sylber_debug_gemm_trace(int32_t M, int32_t N, int32_t K, int32_t ldx, int32_t epi, int32_t act,
                                       unsigned long long* out20, float* ms_out) {
    if (!out20 || !ms_out) { syl_set_error("sylber_debug_gemm_trace", "null argument"); return 1; }
    // act >= 100: the trace instantiation of the UNSTAGGERED kernel (tile id 41; plain bf16 epilogue only)
    if (act >= 200) return gemm_bench_impl(M, N, K, ldx, 0, 1, 98, 3, ms_out, out20);   // asm tile 97 with phase stamps (SYLBER_EXPERIMENTS builds)
    if (act >= 100) return gemm_bench_impl(M, N, K, ldx, 0, 0, 9041, 3, ms_out, out20);
    return gemm_bench_impl(M, N, K, ldx, epi, act, 9030, 3, ms_out, out20);
}

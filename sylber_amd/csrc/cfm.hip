// Resynthesis decoder: the flow-matching Regressor of sylber/model/flowmatching.py:474-688 (8 layers, dim 512, 8 x 64 heads,
// 16 register tokens, AdaRMSNorm time conditioning) evaluated by ConditionalFlowMatcherWrapperRegressor.sample (:747-824) with
// torchdiffeq's fixed-grid midpoint rule on t = linspace(0, 1, steps).
//
// One evaluation (rows of a batch element: 16 register rows, then the Tmax frames, padded to Tp = round_up(16 + Tmax, 32)):
//   cfm_embed      xe = cond part (one GEMM per sample call, to_embed's bias and proj_in's folded in) + (to_embed o proj_in) y
//   cfm_conv       x  = [registers; gelu(dwconv31(xe)) + xe; zero rows]          (no mask: padded frames are ordinary frames, unless
//                                                                                 sylber_cfm_sample_frames bounds each row: see below)
//   per layer      h  = AdaRMSNorm(x)                     cfm_adanorm  (16-bit operand out; fp32 in the parity mode)
//                  qkv = h Wqkv^T                         GEMM, fp32 out
//                  q, k, V^T = per-head RMSNorm, rotary   cfm_qkprep   (q pre-scaled for the attention kernel)
//                  ctx = softmax(10 q.k) v                the encoder's attention kernels, 12-head layout with heads 8..11 zero
//                  x += ctx Wo^T                          GEMM, EPI_F32_RES in place
//                  h  = AdaRMSNorm(x)
//                  ff = h W1^T + b1                       GEMM, fp32 out, W1 packed [value 1408 | gate 1408] (zero rows pad)
//                  g  = gelu(gate) * value                cfm_geglu    ([M, 1408] 16-bit, columns 1365.. zero)
//                  x += g W2^T + b2                       GEMM, K = 1408, EPI_F32_RES in place
//   cfm_final      v = to_pred(RMSNorm(x)) of the frame rows, fused with the midpoint update of the sampler state
// The time conditioning (sinusoidal embedding -> Linear -> SiLU -> 16 gamma / beta vectors) depends on t only: all the times
// of one sample call are computed up front in fp32 (cfm_time_hidden, cfm_time_gb).
// sylber_cfm_sample_frames: row b has its own frame count Tb (the workspace's `valid` slots hold 16 + Tb).  cfm_conv treats frames at
// or past Tb as the zero padding at the end and writes zero rows there, attention masks keys at or past 16 + Tb, and cfm_final writes
// 0 to the output frames at or past Tb: every other launch is row-local, so row b computes what a [1, Tb] call computes.
// sylber_cfm_sample_packed: no padding to the longest clip.  The x-side buffers (x, h, qkv, ctx, ff, g, q / k / V^T) hold ONE
// pseudo-utterance of Ptot rows: clip b owns the slot [slot[b], slot[b + 1]) of round_up(16 + Tb, 64) rows (registers, its frames, zero
// rows).  The frame-side buffers (cond, xe, the sampler state, art) hold the clips' frames back to back: clip b is rows [F_b, F_b + Tb).
// The slot table (CfmLayout::o_valid, cfm_packed_table) is read by cfm_conv, cfm_qkprep (rotary positions from the slot start), the
// packed attention (keys in 64-tiles from the slot start, context rows [16 + Tb, slot end) zeroed) and cfm_final; every other launch is
// row-local and runs unchanged on M = Ptot (the GEMMs' per-row bits depend neither on M nor on the tile), so clip b computes what a
// [1, Tb] call computes.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "../../include/sylber_hip_dev.h"
#include <cmath>
#include <vector>

#define CFM_D 512
#define CFM_H 8
#define CFM_REG 16
#define CFM_OUT 14
#define CFM_COND 256
#define CFM_PROJ 64
#define CFM_TH 2048
#define CFM_FI 1365
#define CFM_FIP 1408              // FF inner width padded to a multiple of 64 (the FF-out GEMM's K)
#define CFM_KW 31
#define CFM_NORMS (2 * SYLBER_CFM_DEPTH)
#define CFM_MAX_TIMES 128         // 2 (steps - 1) <= 128
#define CFM_SLACK 256             // rows of zero slack behind every GEMM operand (tiles may read past M / N)
static const float CFM_LOG2E = 1.4426950408889634f;

struct DevGuardC {
    int prev = -1;
    explicit DevGuardC(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); }
    ~DevGuardC() { int cur = -1; if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev); }
};

struct sylber_cfm {
    int device = 0, precision = SYLBER_BF16, fmt = FMT_BF16;
    float* base = nullptr; size_t bytes = 0;       // fp32 weights
    bf16_t* base16 = nullptr; size_t bytes16 = 0;  // 16-bit GEMM operands (16-bit modes)
    // fp32 (all modes)
    float *t_w = nullptr, *t1_w = nullptr, *t1_b = nullptr;          // sinusoid weights [256], Linear(512, 2048)
    float *gb_w = nullptr, *gb_b = nullptr;                          // [16 norms][2 (gamma, beta)][512][2048], [16][2][512]
    float *wy = nullptr, *by = nullptr;                              // (to_embed[:, :64] o proj_in) [512][14], folded bias [512]
    float *conv_w = nullptr, *conv_b = nullptr, *reg = nullptr, *inv_freq = nullptr;
    float *qg = nullptr, *kg = nullptr;                              // [8 layers][8 heads][64]
    float *b1 = nullptr, *b2 = nullptr;                              // [8][2816] packed, [8][512]
    float *fin_g = nullptr, *pred_w = nullptr;                       // [512], [14][512]
    // GEMM operands: fp32 in the parity mode, else 16-bit copies (same packing, CFM_SLACK zero rows behind each)
    const void *wc = nullptr, *wqkv[SYLBER_CFM_DEPTH] = {}, *wo[SYLBER_CFM_DEPTH] = {}, *w1[SYLBER_CFM_DEPTH] = {}, *w2[SYLBER_CFM_DEPTH] = {};
    // development tap (sylber_cfm_set_tap, include/sylber_hip_dev.h): 0 = off
    int tap_stage = 0; float* tap_dev = nullptr; int64_t tap_floats = 0;
};

// ---- workspace layout ----------------------------------------------------------------------------------------------
struct CfmLayout {
    int B, T, L, Tp, Tpv; long M;
    long NF;                      // frame rows of cond / xe / the sampler state: B * T, or sum Tb (packed)
    int nclip = 0;                // packed: the clips (B = 1 and Tp = Tpv = M = Ptot for every x-side launch); 0: padded
    int total_qb = 0;             // packed: sum of ceil((16 + Tb) / 128), the attention's query blocks
    size_t o_cond, o_condx, o_xe, o_x, o_h, o_qkv, o_qkvf, o_q, o_k, o_vt, o_ctx, o_ff, o_g, o_temb, o_gb, o_y, o_valid, o_total;
};
// x-side geometry set by the callers below; ntab: ints of the per-clip tables (the last region, never cleared by cfm_prepare)
static void cfm_layout_buffers(int precision, CfmLayout& l, size_t ntab) {
    const int B = l.B;
    const size_t e = precision == SYLBER_FP32 ? 4 : 2;      // bytes of one GEMM operand element
    const size_t Ms = (size_t)l.M + CFM_SLACK;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = (o + bytes + 255) & ~(size_t)255; return r; };
    const size_t NF = (size_t)l.NF;
    l.o_cond = take((NF + CFM_SLACK) * CFM_COND * e);
    l.o_condx = take(NF * CFM_D * 4);
    l.o_xe = take(NF * CFM_D * 4);
    l.o_x = take(Ms * CFM_D * 4);
    l.o_h = take(Ms * CFM_D * e);
    l.o_qkv = take(Ms * 3 * CFM_D * 4);
    if (precision == SYLBER_FP32) {
        l.o_qkvf = take(Ms * 3 * SYL_HIDDEN * 4);            // the fp32 attention's fused [M, 2304] q | k | v (12-head layout)
        l.o_q = l.o_k = l.o_vt = 0;
    } else {
        l.o_qkvf = 0;
        const size_t nq = (size_t)B * SYL_HEADS * l.Tp * 64;
        l.o_q = take(nq * 2);
        l.o_k = take(nq * 2 + 64 * 64 * 2);                  // one 64-key tile of slack (the last K tile may start at Tp - 32)
        l.o_vt = take((size_t)B * SYL_HEADS * 64 * l.Tpv * 2);
    }
    l.o_ctx = take(Ms * SYL_HIDDEN * e);
    l.o_ff = take(Ms * 2 * CFM_FIP * 4);
    l.o_g = take(Ms * CFM_FIP * e);
    l.o_temb = take((size_t)CFM_MAX_TIMES * CFM_TH * 4);
    l.o_gb = take((size_t)CFM_MAX_TIMES * CFM_NORMS * 2 * CFM_D * 4);
    l.o_y = take(NF * CFM_OUT * 4);
    l.o_valid = take(ntab * 4);                              // sylber_cfm_sample_frames: 16 + Tb per row; packed: cfm_packed_table
    l.o_total = o;
}
static CfmLayout cfm_layout(int precision, int B, int T) {
    CfmLayout l;
    l.B = B; l.T = T; l.L = CFM_REG + T; l.Tp = (l.L + 31) & ~31; l.Tpv = (l.Tp + 63) & ~63; l.M = (long)B * l.Tp; l.NF = (long)B * T;
    cfm_layout_buffers(precision, l, (size_t)B);
    return l;
}

// packed slots: slot[b + 1] - slot[b] = round_up(16 + Tb, 64) rows.  The 64 is what the packed attention needs: its key tiles start at
// the slot start, so the last tile of a clip ends inside its own slot and never multiplies a neighbour's V.
static bool cfm_slots(const int32_t* frames, int B, std::vector<int32_t>& slot, long& nf) {
    slot.assign((size_t)B + 1, 0);
    long off = 0; nf = 0;
    for (int b = 0; b < B; ++b) {
        if (frames[b] < 1) return false;
        slot[b] = (int32_t)off;
        off += ((long)CFM_REG + frames[b] + 63) & ~63L;
        nf += frames[b];
        if (off >= (1l << 24)) return false;                 // rows of the pseudo-utterance are int in every launch
    }
    slot[B] = (int32_t)off;
    return true;
}
// the device table of a packed call: [slot offsets (B + 1) | 16 + Tb (B) | prefix of ceil((16 + Tb) / 128) (B + 1) | frame prefix F (B + 1)];
// the first 3B + 2 entries are launch_attention_packed's pk
static void cfm_packed_table(const int32_t* frames, int B, const std::vector<int32_t>& slot, std::vector<int32_t>& tab) {
    tab.assign(4 * (size_t)B + 3, 0);
    for (int b = 0; b <= B; ++b) tab[b] = slot[b];
    for (int b = 0; b < B; ++b) {
        tab[B + 1 + b] = CFM_REG + frames[b];
        tab[2 * B + 2 + b] = tab[2 * B + 1 + b] + (CFM_REG + frames[b] + 127) / 128;
        tab[3 * B + 3 + b] = tab[3 * B + 2 + b] + frames[b];
    }
}
static CfmLayout cfm_layout_packed(int precision, int nclip, int Ptot, long NF) {
    CfmLayout l;
    l.B = 1; l.T = 0; l.L = l.Tp = l.Tpv = Ptot; l.M = Ptot; l.NF = NF; l.nclip = nclip;
    cfm_layout_buffers(precision, l, 4 * (size_t)nclip + 3);
    return l;
}

// ---- development tap ---------------------------------------------------------------------------------------------------
// the buffer behind stage `stage` of a call with layout l: its bytes in the workspace, its floats (every row, no slack rows) and
// whether it holds 16-bit words.  false: no such stage in this precision
struct CfmTapBuf { size_t off; int64_t n; bool half; };
static bool cfm_tap_buf(int precision, const CfmLayout& l, int stage, CfmTapBuf& t) {
    const bool f32 = precision == SYLBER_FP32;
    const int64_t M = l.M, NF = l.NF;
    switch (stage) {
    case SYLBER_CFM_TAP_CONDX: t = {l.o_condx, NF * CFM_D, false}; return true;
    case SYLBER_CFM_TAP_GB: t = {l.o_gb, (int64_t)CFM_NORMS * 2 * CFM_D, false}; return true;
    case SYLBER_CFM_TAP_XE: t = {l.o_xe, NF * CFM_D, false}; return true;
    case SYLBER_CFM_TAP_X0: t = {l.o_x, M * CFM_D, false}; return true;
    }
    if (stage < SYLBER_CFM_TAP(0, 0) || stage >= SYLBER_CFM_TAP(SYLBER_CFM_DEPTH, 0)) return false;
    const int64_t nq = (int64_t)l.B * SYL_HEADS * l.Tp * 64;
    switch (stage & 15) {
    case SYLBER_CFM_BTAP_H_ATTN: case SYLBER_CFM_BTAP_H_FF: t = {l.o_h, M * CFM_D, !f32}; return true;
    case SYLBER_CFM_BTAP_QKV: t = {l.o_qkv, M * 3 * CFM_D, false}; return true;
    case SYLBER_CFM_BTAP_Q: t = {l.o_q, nq, true}; return !f32;
    case SYLBER_CFM_BTAP_K: t = {l.o_k, nq, true}; return !f32;
    case SYLBER_CFM_BTAP_VT: t = {l.o_vt, (int64_t)l.B * SYL_HEADS * 64 * l.Tpv, true}; return !f32;
    case SYLBER_CFM_BTAP_QKVF: t = {l.o_qkvf, M * 3 * SYL_HIDDEN, false}; return f32;
    case SYLBER_CFM_BTAP_CTX: t = {l.o_ctx, M * SYL_HIDDEN, !f32}; return true;
    case SYLBER_CFM_BTAP_X_ATTN: case SYLBER_CFM_BTAP_X_FF: t = {l.o_x, M * CFM_D, false}; return true;
    case SYLBER_CFM_BTAP_FF: t = {l.o_ff, M * 2 * CFM_FIP, false}; return true;
    case SYLBER_CFM_BTAP_G: t = {l.o_g, M * CFM_FIP, !f32}; return true;
    }
    return false;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float cfm_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

struct CfmTimes { float t[CFM_MAX_TIMES]; };

// LearnedSinusoidalPosEmb -> Linear(512, 2048) -> SiLU, one workgroup per time
__global__ __launch_bounds__(256) void cfm_time_hidden(CfmTimes times, const float* __restrict__ w, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, float* __restrict__ temb) {
    __shared__ float emb[CFM_D];
    const int i = blockIdx.x;
    const float t = times.t[i];
    for (int j = threadIdx.x; j < CFM_D / 2; j += 256) {
        const float f = __fmul_rn(__fmul_rn(__fmul_rn(t, w[j]), 2.0f), (float)M_PI);   // x * weights * 2 * pi, left to right
        emb[j] = sinf(f);
        emb[j + CFM_D / 2] = cosf(f);
    }
    __syncthreads();
    for (int n = threadIdx.x; n < CFM_TH; n += 256) {
        const float* wr = w1 + (size_t)n * CFM_D;
        float acc = 0.f;
        for (int k = 0; k < CFM_D; ++k) acc = fmaf(wr[k], emb[k], acc);
        acc += b1[n];
        temb[(size_t)i * CFM_TH + n] = acc / (1.0f + expf(-acc));
    }
}

// the 16 x 2 AdaRMSNorm gamma / beta vectors of every time: one wave per output row (its 2048 weights stay in registers
// while it walks the times)
__global__ __launch_bounds__(256) void cfm_time_gb(const float* __restrict__ temb, int ntimes, const float* __restrict__ w,
                                                   const float* __restrict__ b, float* __restrict__ gb) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= CFM_NORMS * 2 * CFM_D) return;
    float wr[CFM_TH / 64];
#pragma unroll
    for (int j = 0; j < CFM_TH / 64; ++j) wr[j] = w[(size_t)row * CFM_TH + j * 64 + lane];
    const float bias = b[row];
    for (int i = 0; i < ntimes; ++i) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < CFM_TH / 64; ++j) acc = fmaf(wr[j], temb[(size_t)i * CFM_TH + j * 64 + lane], acc);
        acc = wave_sum(acc);
        if (lane == 0) gb[(size_t)i * CFM_NORMS * 2 * CFM_D + row] = acc + bias;
    }
}

// caller's conditioning [rows, 256] fp32 -> the cond-part GEMM operand (16-bit words, or an fp32 copy)
template <int FMT>
__global__ void cfm_convert(const float* __restrict__ in, bf16_t* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = H16<FMT>::cvt(in[i]);
}

// the tap's copy of a 16-bit buffer: every word widened to fp32 (exact)
template <int FMT>
__global__ void cfm_widen(const bf16_t* __restrict__ in, float* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = H16<FMT>::up(in[i]);
}

// xe[b, t] = condx[b, t] + Wy y[b, t]   (condx holds to_embed's cond block plus every bias)
__global__ __launch_bounds__(256) void cfm_embed(const float* __restrict__ condx, const float* __restrict__ y, const float* __restrict__ wy,
                                                 float* __restrict__ xe) {
    const size_t r = blockIdx.x;
    __shared__ float yr[CFM_OUT];
    if (threadIdx.x < CFM_OUT) yr[threadIdx.x] = y ? y[r * CFM_OUT + threadIdx.x] : 0.f;
    __syncthreads();
    for (int c = threadIdx.x; c < CFM_D; c += 256) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < CFM_OUT; ++j) acc = fmaf(wy[c * CFM_OUT + j], yr[j], acc);
        xe[r * CFM_D + c] = condx[r * CFM_D + c] + acc;
    }
}

// packed calls: the clip whose entry of the ascending table tab[0 .. n) is the last one <= v (tab[0] == 0 <= v)
__device__ __forceinline__ int cfm_clip_of(const int* __restrict__ tab, int n, long v) {
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tab[mid] <= v) lo = mid; else hi = mid - 1; }
    return lo;
}

// x rows of batch element b: [registers (16); gelu(depthwise conv31(xe) + bias) + xe (T frames, zero padded at both ends);
// zero rows up to Tp]
// pk (packed, grid (Ptot, 1)): row blockIdx.x of the pseudo-utterance is row r of clip b's slot; the clip's frames are xe rows F_b ..
__global__ __launch_bounds__(256) void cfm_conv(const float* __restrict__ xe, const float* __restrict__ w, const float* __restrict__ bias,
                                                const float* __restrict__ reg, float* __restrict__ x, int T, int Tp, const int* __restrict__ valid,
                                                const int* __restrict__ pk, int nclip) {
    int r = blockIdx.x, b = blockIdx.y, Tb;
    size_t f0;                                               // xe row of the clip's frame 0
    if (pk) {
        b = cfm_clip_of(pk, nclip, r);
        r -= pk[b];
        Tb = pk[nclip + 1 + b] - CFM_REG;
        f0 = (size_t)pk[3 * nclip + 2 + b];
    } else {
        Tb = valid ? valid[b] - CFM_REG : T;                 // the row's own frames (T is the row pitch of xe)
        f0 = (size_t)b * T;
    }
    float* dst = x + (pk ? (size_t)blockIdx.x : (size_t)b * Tp + r) * CFM_D;
    for (int c = threadIdx.x; c < CFM_D; c += 256) {
        float v;
        if (r < CFM_REG) v = reg[r * CFM_D + c];
        else if (r < CFM_REG + Tb) {
            const int t = r - CFM_REG;
            const float* src = xe + f0 * CFM_D + c;
            float acc = bias[c];
            for (int k = 0; k < CFM_KW; ++k) {
                const int tt = t + k - CFM_KW / 2;
                if (tt >= 0 && tt < Tb) acc = fmaf(w[c * CFM_KW + k], src[(size_t)tt * CFM_D], acc);
            }
            v = cfm_gelu(acc) + src[(size_t)t * CFM_D];
        } else v = 0.f;
        dst[c] = v;
    }
}

// AdaRMSNorm (and the plain RMSNorm with beta == nullptr): F.normalize(x) * sqrt(512) * gamma + beta, one wave per row
template <int FMT, bool F32OUT>
__global__ __launch_bounds__(256) void cfm_adanorm(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   void* __restrict__ out, long M) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* xr = x + row * CFM_D;
    float v[8], ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { v[j] = xr[j * 64 + lane]; ss = fmaf(v[j], v[j], ss); }
    ss = wave_sum(ss);
    const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    const float sc = 22.627416997969522f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = j * 64 + lane;
        const float o = (v[j] * inv) * sc * gamma[c] + beta[c];
        if constexpr (F32OUT) ((float*)out)[row * CFM_D + c] = o;
        else ((bf16_t*)out)[row * CFM_D + c] = H16<FMT>::cvt(o);
    }
}

// per-head RMSNorm of q and k (F.normalize * gamma_h * 8), rotary (theta 50000, pairs (i, i + 32), fp32 angles pos * inv_freq,
// positions -10000 for the registers and 0.. for the frames), q scaled for the attention kernel.  One wave per (row, head).
//   16-bit modes: q, k -> [B, 12, Tp, 64], v -> V^T [B, 12, 64, Tpv] with the key axis' bits 2 and 3 swapped (attention.hip);
//                 q carries 10 * log2(e) (the 16-bit kernels take scores in log2 units)
//   fp32 mode:    the fused [M, 2304] buffer of the fp32 attention, q carrying 80 (that kernel applies the exact 1/8 itself)
//   pk (packed, B = 1, Tp = Tpv = Ptot): positions count from the row's slot start; slot starts are multiples of 64, so the key-axis
//                 bit swap of the pseudo-utterance's row is the swap within the clip's own 64-key tile
template <int FMT, bool F32>
__global__ __launch_bounds__(256) void cfm_qkprep(const float* __restrict__ qkv, const float* __restrict__ qg, const float* __restrict__ kg,
                                                  const float* __restrict__ inv_freq, bf16_t* __restrict__ q16, bf16_t* __restrict__ k16,
                                                  bf16_t* __restrict__ vt16, float* __restrict__ qkvf, int L, int Tp, int Tpv,
                                                  const int* __restrict__ pk, int nclip) {
    const int r = blockIdx.x, b = blockIdx.y, head = blockIdx.z * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const size_t row = (size_t)b * Tp + r;
    const float* src = qkv + row * 3 * CFM_D + head * 64 + lane;
    float q = src[0], k = src[CFM_D], v = src[2 * CFM_D];
    const float qn = 1.0f / fmaxf(sqrtf(wave_sum(q * q)), 1e-12f), kn = 1.0f / fmaxf(sqrtf(wave_sum(k * k)), 1e-12f);
    q = (q * qn) * qg[head * 64 + lane] * 8.0f;
    k = (k * kn) * kg[head * 64 + lane] * 8.0f;
    const int rs = pk ? r - pk[cfm_clip_of(pk, nclip, r)] : r;     // row within its slot
    const float pos = rs < CFM_REG ? -10000.0f : (float)(rs - CFM_REG);
    const float ang = __fmul_rn(pos, inv_freq[lane & 31]);
    const float cs = cosf(ang), sn = sinf(ang);
    const float qo = __shfl_xor(q, 32, 64), ko = __shfl_xor(k, 32, 64);
    // out[i] = t[i] cos - t[i + 32] sin (i < 32); out[i + 32] = t[i + 32] cos + t[i] sin
    const float qr = lane < 32 ? q * cs - qo * sn : q * cs + qo * sn;
    const float kr = lane < 32 ? k * cs - ko * sn : k * cs + ko * sn;
    if constexpr (F32) {
        float* d = qkvf + row * 3 * SYL_HIDDEN + head * 64 + lane;
        d[0] = qr * 80.0f;
        d[SYL_HIDDEN] = kr;
        d[2 * SYL_HIDDEN] = v;
    } else {
        const size_t hm = (((size_t)b * SYL_HEADS + head) * Tp + r) * 64 + lane;
        q16[hm] = H16<FMT>::cvt(qr * (10.0f * CFM_LOG2E));
        k16[hm] = H16<FMT>::cvt(kr);
        const int p = (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1);
        vt16[(((size_t)b * SYL_HEADS + head) * 64 + lane) * Tpv + p] = H16<FMT>::cvt(v);
    }
}

// GEGLU: g[m][j] = gelu(ff[m][1408 + j]) * ff[m][j], j < 1408 (the packed zero columns give exact zeros)
template <int FMT, bool F32OUT>
__global__ __launch_bounds__(256) void cfm_geglu(const float* __restrict__ ff, void* __restrict__ g, long M) {
    const long row = blockIdx.x;
    const float* src = ff + row * 2 * CFM_FIP;
    for (int j = threadIdx.x; j < CFM_FIP; j += 256) {
        const float o = cfm_gelu(src[CFM_FIP + j]) * src[j];
        if constexpr (F32OUT) ((float*)g)[row * CFM_FIP + j] = o;
        else ((bf16_t*)g)[row * CFM_FIP + j] = H16<FMT>::cvt(o);
    }
}

// final RMSNorm + to_pred of the frame rows, fused with the sampler: one wave per frame.
//   mode 0: out = v;  mode 1: ymid = y + v * hdt;  mode 2: y = y + dt * v (in place), channel 12 / pitch_amp when `last`
// (y and out may alias: each element is read and written by the same lane)
// pk (packed, B = the clips): frame fr of the state is frame t = fr - F_b of clip b, x row slot[b] + 16 + t
__global__ __launch_bounds__(256) void cfm_final(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ wp,
                                                 const float* y, float* out, long NF, int B, int T, int Tp, int mode,
                                                 float dt, int last, float pitch_amp, const int* __restrict__ valid, const int* __restrict__ pk) {
    const long fr = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (fr >= NF) return;
    size_t xrow;
    if (pk) {
        const int* F = pk + 3 * B + 2;
        const int b = cfm_clip_of(F, B, fr);
        xrow = (size_t)pk[b] + CFM_REG + (size_t)(fr - F[b]);
    } else {
        const int b = (int)(fr / T), t = (int)(fr % T);
        if (valid && t >= valid[b] - CFM_REG) {              // past the row's own frames: 0 (wave-uniform)
            if (lane < CFM_OUT) out[(size_t)fr * CFM_OUT + lane] = 0.f;
            return;
        }
        xrow = (size_t)b * Tp + CFM_REG + t;
    }
    const float* xr = x + xrow * CFM_D;
    float v[8], ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { v[j] = xr[j * 64 + lane]; ss = fmaf(v[j], v[j], ss); }
    ss = wave_sum(ss);
    const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (v[j] * inv) * 22.627416997969522f * gamma[j * 64 + lane];
    float mine = 0.f;
    for (int o = 0; o < CFM_OUT; ++o) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = fmaf(wp[o * CFM_D + j * 64 + lane], v[j], acc);
        acc = wave_sum(acc);
        if (lane == o) mine = acc;
    }
    if (lane < CFM_OUT) {
        const size_t i = (size_t)fr * CFM_OUT + lane;
        float r;
        if (mode == 0) r = mine;
        else if (mode == 1) r = __fadd_rn(y[i], __fmul_rn(mine, dt));
        else {
            r = __fadd_rn(y[i], __fmul_rn(dt, mine));
            if (last && lane == 12) r = __fdiv_rn(r, pitch_amp);
        }
        out[i] = r;
    }
}

// steps == 1 (and y0 handling): art = y0 (or zeros), channel 12 / pitch_amp when `scale`
// valid (nullable): frames t >= valid[b] - 16 of row b (T frames per row) start at, and keep, 0
__global__ void cfm_init_state(const float* __restrict__ y0, float* __restrict__ art, size_t n, int scale, float pitch_amp,
                               const int* __restrict__ valid, int T) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float v = y0 ? y0[i] : 0.f;
        if (valid) {
            const size_t fr = i / CFM_OUT;
            if ((int)(fr % T) >= valid[fr / T] - CFM_REG) v = 0.f;
        }
        if (scale && i % CFM_OUT == 12) v = __fdiv_rn(v, pitch_amp);
        art[i] = v;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static int cfm_gemm(const sylber_cfm* h, const void* X, long ldx, const void* W, int M, int N, int K, const float* bias, float* out,
                    long ld0, bool res, hipStream_t s) {
    if (h->precision == SYLBER_FP32) {
        GemmArgsF32 a = {};
        a.X = (const float*)X; a.ldx = ldx; a.W = (const float*)W; a.M = M; a.N = N; a.K = K; a.bias = bias; a.out0 = out; a.ld0 = ld0;
        if (res) { a.res = out; a.ldres = ld0; }
        a.tiled = 1;
        return launch_gemm_f32(a, s);
    }
    GemmArgs a = {};
    a.X = (const bf16_t*)X; a.ldx = ldx; a.W = (const bf16_t*)W; a.M = M; a.N = N; a.K = K; a.bias = bias; a.out0 = out; a.ld0 = ld0;
    a.fmt = h->fmt;
    if (res) { a.res = out; a.ldres = ld0; }
    return launch_gemm_bf16(res ? EPI_F32_RES : EPI_F32, a, s);
}

#define CFM_RUN(what, expr) do { if (expr) return 1; HIP_TRY(hipGetLastError()); } while (0)

// a tap is set and `stage` is it: copy the buffer behind the launch just issued to the caller's tap buffer (storage order, 16-bit words
// widened) and end the call.  CFM_TAPPED is cfm_evaluate's third result: no error, nothing further launched
enum { CFM_TAPPED = 2 };
static int cfm_tap_copy(const sylber_cfm* h, const CfmLayout& l, char* ws, int stage, int ti, hipStream_t s) {
    CfmTapBuf t;
    if (!cfm_tap_buf(h->precision, l, stage, t) || t.n > h->tap_floats) { syl_set_error("sylber_cfm tap", "tap buffer does not fit the stage"); return 1; }
    const char* src = ws + t.off + (stage == SYLBER_CFM_TAP_GB ? (size_t)ti * CFM_NORMS * 2 * CFM_D * 4 : 0);
    if (!t.half) HIP_TRY(hipMemcpyAsync(h->tap_dev, src, (size_t)t.n * 4, hipMemcpyDeviceToDevice, s));
    else if (h->fmt == FMT_F16) hipLaunchKernelGGL(cfm_widen<FMT_F16>, dim3(1024), dim3(256), 0, s, (const bf16_t*)src, h->tap_dev, (size_t)t.n);
    else hipLaunchKernelGGL(cfm_widen<FMT_BF16>, dim3(1024), dim3(256), 0, s, (const bf16_t*)src, h->tap_dev, (size_t)t.n);
    HIP_TRY(hipGetLastError());
    return CFM_TAPPED;
}
#define CFM_TAP(stage) do { if (h->tap_stage == (stage)) return cfm_tap_copy(h, l, ws, (stage), ti, s); } while (0)

// what every entry point asks before it launches anything while a tap is set
static int cfm_tap_check(const char* what, const sylber_cfm* h, const CfmLayout& l, int steps) {
    if (!h->tap_stage) return 0;
    CfmTapBuf t;
    if (!cfm_tap_buf(h->precision, l, h->tap_stage, t)) { syl_set_error(what, "the tap's stage does not exist in this precision"); return 1; }
    if (t.n > h->tap_floats) { syl_set_error(what, "the tap buffer is too small for this call (sylber_cfm_tap_floats)"); return 1; }
    if (steps < 2) { syl_set_error(what, "a tap needs an evaluation: steps >= 2"); return 1; }
    return 0;
}

// torch.linspace(0, 1, steps) on the CPU in float32: the first half counts up from 0, the second half down from 1
static void cfm_linspace(int steps, std::vector<float>& t) {
    t.resize(steps);
    if (steps == 1) { t[0] = 1.0f; return; }
    const float step = (1.0f - 0.0f) / (float)(steps - 1);
    const int half = steps / 2;
    for (int i = 0; i < steps; ++i) t[i] = i < half ? 0.0f + step * (float)i : 1.0f - step * (float)(steps - i - 1);
}

// one evaluation of the decoder at yin (fp32 [B, T, 14]) and time index ti; writes per `mode` (see cfm_final) with the
// update's base state ybase.  valid: nullptr (every row T frames) or the workspace's per-row 16 + Tb (sylber_cfm_sample_frames);
// a packed layout (l.nclip > 0) reads its table from the workspace instead (16-bit modes only)
static int cfm_evaluate(const sylber_cfm* h, const CfmLayout& l, char* ws, int ti, const float* yin, const float* ybase, float* out, int mode, float dt,
                        int last, float pitch_amp, hipStream_t s, const int* valid = nullptr) {
    const bool f32 = h->precision == SYLBER_FP32;
    const int B = l.B, T = l.T, nclip = l.nclip;
    const int* pk = nclip ? (const int*)(ws + l.o_valid) : nullptr;
    float* xe = (float*)(ws + l.o_xe); float* x = (float*)(ws + l.o_x); void* hb = ws + l.o_h;
    float* qkv = (float*)(ws + l.o_qkv); void* ctx = ws + l.o_ctx; float* ff = (float*)(ws + l.o_ff); void* g = ws + l.o_g;
    const float* gb = (const float*)(ws + l.o_gb) + (size_t)ti * CFM_NORMS * 2 * CFM_D;
    const int M = (int)l.M;
    const dim3 rows4((unsigned)((l.M + 3) / 4));
    CFM_TAP(SYLBER_CFM_TAP_CONDX);
    CFM_TAP(SYLBER_CFM_TAP_GB);
    hipLaunchKernelGGL(cfm_embed, dim3((unsigned)l.NF), dim3(256), 0, s, (const float*)(ws + l.o_condx), yin, h->wy, xe);
    CFM_RUN("embed", 0);
    CFM_TAP(SYLBER_CFM_TAP_XE);
    hipLaunchKernelGGL(cfm_conv, dim3(l.Tp, B), dim3(256), 0, s, xe, h->conv_w, h->conv_b, h->reg, x, T, l.Tp, valid, pk, nclip);
    CFM_RUN("conv", 0);
    CFM_TAP(SYLBER_CFM_TAP_X0);
    auto norm = [&](int n) {
        const float* ga = gb + (size_t)n * 2 * CFM_D;
        if (f32) hipLaunchKernelGGL((cfm_adanorm<FMT_BF16, true>), rows4, dim3(256), 0, s, x, ga, ga + CFM_D, hb, l.M);
        else if (h->fmt == FMT_F16) hipLaunchKernelGGL((cfm_adanorm<FMT_F16, false>), rows4, dim3(256), 0, s, x, ga, ga + CFM_D, hb, l.M);
        else hipLaunchKernelGGL((cfm_adanorm<FMT_BF16, false>), rows4, dim3(256), 0, s, x, ga, ga + CFM_D, hb, l.M);
    };
    for (int li = 0; li < SYLBER_CFM_DEPTH; ++li) {
        norm(2 * li);
        CFM_RUN("adanorm", 0);
        CFM_TAP(SYLBER_CFM_TAP(li, SYLBER_CFM_BTAP_H_ATTN));
        CFM_RUN("qkv", cfm_gemm(h, hb, CFM_D, h->wqkv[li], M, 3 * CFM_D, CFM_D, nullptr, qkv, 3 * CFM_D, false, s));
        CFM_TAP(SYLBER_CFM_TAP(li, SYLBER_CFM_BTAP_QKV));
        const float* qg = h->qg + li * CFM_H * 64; const float* kg = h->kg + li * CFM_H * 64;
        const dim3 gq(l.L, B, 2);
        if (f32) {
            float* qkvf = (float*)(ws + l.o_qkvf);
            hipLaunchKernelGGL((cfm_qkprep<FMT_BF16, true>), gq, dim3(256), 0, s, qkv, qg, kg, h->inv_freq, nullptr, nullptr, nullptr, qkvf, l.L, l.Tp, l.Tpv,
                               nullptr, 0);
            CFM_RUN("qkprep", 0);
            CFM_TAP(SYLBER_CFM_TAP(li, SYLBER_CFM_BTAP_QKVF));
            CFM_RUN("attention", launch_attention_f32(qkvf, qkvf + SYL_HIDDEN, qkvf + 2 * SYL_HIDDEN, valid, (float*)ctx, B, l.L, l.Tp, s));
        } else {
            bf16_t* q = (bf16_t*)(ws + l.o_q); bf16_t* k = (bf16_t*)(ws + l.o_k); bf16_t* vt = (bf16_t*)(ws + l.o_vt);
            if (h->fmt == FMT_F16) hipLaunchKernelGGL((cfm_qkprep<FMT_F16, false>), gq, dim3(256), 0, s, qkv, qg, kg, h->inv_freq, q, k, vt, nullptr, l.L, l.Tp, l.Tpv,
                                                      pk, nclip);
            else hipLaunchKernelGGL((cfm_qkprep<FMT_BF16, false>), gq, dim3(256), 0, s, qkv, qg, kg, h->inv_freq, q, k, vt, nullptr, l.L, l.Tp, l.Tpv, pk, nclip);
            CFM_RUN("qkprep", 0);
            CFM_TAP(SYLBER_CFM_TAP(li, SYLBER_CFM_BTAP_Q));
            CFM_TAP(SYLBER_CFM_TAP(li, SYLBER_CFM_BTAP_K));
            CFM_TAP(SYLBER_CFM_TAP(li, SYLBER_CFM_BTAP_VT));
            if (pk) CFM_RUN("attention", launch_attention_packed(q, k, vt, pk, nclip, l.total_qb, (bf16_t*)ctx, l.Tp, s, h->fmt));
            else CFM_RUN("attention", launch_attention(q, k, vt, valid, (bf16_t*)ctx, B, l.L, l.Tp, l.Tpv, 0, s, h->fmt));
        }
        CFM_TAP(SYLBER_CFM_TAP(li, SYLBER_CFM_BTAP_CTX));
        CFM_RUN("out", cfm_gemm(h, ctx, SYL_HIDDEN, h->wo[li], M, CFM_D, CFM_D, nullptr, x, CFM_D, true, s));
        CFM_TAP(SYLBER_CFM_TAP(li, SYLBER_CFM_BTAP_X_ATTN));
        norm(2 * li + 1);
        CFM_RUN("adanorm", 0);
        CFM_TAP(SYLBER_CFM_TAP(li, SYLBER_CFM_BTAP_H_FF));
        CFM_RUN("ff1", cfm_gemm(h, hb, CFM_D, h->w1[li], M, 2 * CFM_FIP, CFM_D, h->b1 + (size_t)li * 2 * CFM_FIP, ff, 2 * CFM_FIP, false, s));
        CFM_TAP(SYLBER_CFM_TAP(li, SYLBER_CFM_BTAP_FF));
        if (f32) hipLaunchKernelGGL((cfm_geglu<FMT_BF16, true>), dim3(M), dim3(256), 0, s, ff, g, l.M);
        else if (h->fmt == FMT_F16) hipLaunchKernelGGL((cfm_geglu<FMT_F16, false>), dim3(M), dim3(256), 0, s, ff, g, l.M);
        else hipLaunchKernelGGL((cfm_geglu<FMT_BF16, false>), dim3(M), dim3(256), 0, s, ff, g, l.M);
        CFM_RUN("geglu", 0);
        CFM_TAP(SYLBER_CFM_TAP(li, SYLBER_CFM_BTAP_G));
        CFM_RUN("ff2", cfm_gemm(h, g, CFM_FIP, h->w2[li], M, CFM_D, CFM_FIP, h->b2 + (size_t)li * CFM_D, x, CFM_D, true, s));
        CFM_TAP(SYLBER_CFM_TAP(li, SYLBER_CFM_BTAP_X_FF));
    }
    hipLaunchKernelGGL(cfm_final, dim3((unsigned)((l.NF + 3) / 4)), dim3(256), 0, s, x, h->fin_g, h->pred_w, ybase, out, l.NF, nclip ? nclip : B, T,
                       l.Tp, mode, dt, last, pitch_amp, valid, pk);
    CFM_RUN("final", 0);
    return 0;
}

// per call: clear the workspace, the conditioning GEMM (once), the time conditioning of every time of the call
static int cfm_prepare(const sylber_cfm* h, const CfmLayout& l, char* ws, const float* cond_dev, const float* times, int ntimes, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(ws, 0, l.o_valid, s));          // (everything but the per-row counts, the last region: written before this)
    const size_t n = (size_t)l.NF * CFM_COND;
    void* cb = ws + l.o_cond;
    if (h->precision == SYLBER_FP32) HIP_TRY(hipMemcpyAsync(cb, cond_dev, n * 4, hipMemcpyDeviceToDevice, s));
    else if (h->fmt == FMT_F16) hipLaunchKernelGGL(cfm_convert<FMT_F16>, dim3(1024), dim3(256), 0, s, cond_dev, (bf16_t*)cb, n);
    else hipLaunchKernelGGL(cfm_convert<FMT_BF16>, dim3(1024), dim3(256), 0, s, cond_dev, (bf16_t*)cb, n);
    CFM_RUN("convert", 0);
    CFM_RUN("cond", cfm_gemm(h, cb, CFM_COND, h->wc, (int)l.NF, CFM_D, CFM_COND, h->by, (float*)(ws + l.o_condx), CFM_D, false, s));
    CfmTimes ts = {};
    for (int i = 0; i < ntimes; ++i) ts.t[i] = times[i];
    float* temb = (float*)(ws + l.o_temb);
    hipLaunchKernelGGL(cfm_time_hidden, dim3(ntimes), dim3(256), 0, s, ts, h->t_w, h->t1_w, h->t1_b, temb);
    CFM_RUN("time", 0);
    hipLaunchKernelGGL(cfm_time_gb, dim3(CFM_NORMS * 2 * CFM_D / 4), dim3(256), 0, s, temb, ntimes, h->gb_w, h->gb_b, (float*)(ws + l.o_gb));
    CFM_RUN("time_gb", 0);
    return 0;
}

extern "C" int sylber_cfm_create(const SylberCfmWeights* w, int device, int precision, sylber_cfm_t* out) {
    if (!w || !out) { syl_set_error("sylber_cfm_create", "null argument"); return 1; }
    if (precision != SYLBER_BF16 && precision != SYLBER_FP16 && precision != SYLBER_FP32) {
        syl_set_error("sylber_cfm_create", "precision must be SYLBER_BF16, SYLBER_FP16 or SYLBER_FP32"); return 1;
    }
    const float* need[] = {w->proj_in_w, w->proj_in_b, w->time_freq, w->time_w, w->time_b, w->to_embed_w, w->to_embed_b, w->conv_w, w->conv_b,
                           w->register_tokens, w->rotary_inv_freq, w->final_gamma, w->to_pred_w};
    for (const float* p : need) if (!p) { syl_set_error("sylber_cfm_create", "missing tensor"); return 1; }
    for (int i = 0; i < SYLBER_CFM_DEPTH; ++i) {
        const SylberCfmLayer& L = w->layers[i];
        const float* ln[] = {L.attn_gamma_w, L.attn_gamma_b, L.attn_beta_w, L.attn_beta_b, L.ff_gamma_w, L.ff_gamma_b, L.ff_beta_w, L.ff_beta_b,
                             L.q_gamma, L.k_gamma, L.qkv_w, L.out_w, L.ff1_w, L.ff1_b, L.ff2_w, L.ff2_b};
        for (const float* p : ln) if (!p) { syl_set_error("sylber_cfm_create", "missing layer tensor"); return 1; }
    }
    DevGuardC dg(device);
    sylber_cfm* h = new sylber_cfm();
    h->device = device; h->precision = precision; h->fmt = precision == SYLBER_FP16 ? FMT_F16 : FMT_BF16;
    std::vector<float> host;
    auto alloc = [&](size_t n) { size_t o = (host.size() + 63) & ~(size_t)63; host.resize(o + n, 0.0f); return o; };
    auto add = [&](const float* src, size_t n) { size_t o = alloc(n); std::copy(src, src + n, host.begin() + o); return o; };
    const size_t o_tw = add(w->time_freq, CFM_D / 2), o_t1w = add(w->time_w, (size_t)CFM_TH * CFM_D), o_t1b = add(w->time_b, CFM_TH);
    const size_t o_gbw = alloc((size_t)CFM_NORMS * 2 * CFM_D * CFM_TH), o_gbb = alloc((size_t)CFM_NORMS * 2 * CFM_D);
    for (int i = 0; i < SYLBER_CFM_DEPTH; ++i) {
        const SylberCfmLayer& L = w->layers[i];
        const float* ws_[4] = {L.attn_gamma_w, L.attn_beta_w, L.ff_gamma_w, L.ff_beta_w};
        const float* bs_[4] = {L.attn_gamma_b, L.attn_beta_b, L.ff_gamma_b, L.ff_beta_b};
        for (int j = 0; j < 4; ++j) {   // row block (norm 2i + j / 2, gamma / beta j % 2)
            const size_t blk = (size_t)(2 * i + j / 2) * 2 + (j % 2);
            std::copy(ws_[j], ws_[j] + (size_t)CFM_D * CFM_TH, host.begin() + o_gbw + blk * CFM_D * CFM_TH);
            std::copy(bs_[j], bs_[j] + CFM_D, host.begin() + o_gbb + blk * CFM_D);
        }
    }
    // to_embed = [W_y (64) | W_c (256) | W_z (64)] over [proj_in(y), cond_emb, 0]: fold proj_in into the first block
    const size_t o_wy = alloc((size_t)CFM_D * CFM_OUT), o_by = alloc(CFM_D);
    const int EW = 2 * CFM_PROJ + CFM_COND;
    for (int c = 0; c < CFM_D; ++c) {
        const float* er = w->to_embed_w + (size_t)c * EW;
        double bacc = w->to_embed_b[c];
        for (int p = 0; p < CFM_PROJ; ++p) bacc += (double)er[p] * w->proj_in_b[p];
        host[o_by + c] = (float)bacc;
        for (int j = 0; j < CFM_OUT; ++j) {
            double acc = 0;
            for (int p = 0; p < CFM_PROJ; ++p) acc += (double)er[p] * w->proj_in_w[p * CFM_OUT + j];
            host[o_wy + (size_t)c * CFM_OUT + j] = (float)acc;
        }
    }
    const size_t o_cw = add(w->conv_w, (size_t)CFM_D * CFM_KW), o_cb = add(w->conv_b, CFM_D), o_reg = add(w->register_tokens, (size_t)CFM_REG * CFM_D);
    const size_t o_inv = add(w->rotary_inv_freq, 32);
    const size_t o_qg = alloc((size_t)SYLBER_CFM_DEPTH * CFM_H * 64), o_kg = alloc((size_t)SYLBER_CFM_DEPTH * CFM_H * 64);
    const size_t o_b1 = alloc((size_t)SYLBER_CFM_DEPTH * 2 * CFM_FIP), o_b2 = alloc((size_t)SYLBER_CFM_DEPTH * CFM_D);
    for (int i = 0; i < SYLBER_CFM_DEPTH; ++i) {
        const SylberCfmLayer& L = w->layers[i];
        std::copy(L.q_gamma, L.q_gamma + CFM_H * 64, host.begin() + o_qg + (size_t)i * CFM_H * 64);
        std::copy(L.k_gamma, L.k_gamma + CFM_H * 64, host.begin() + o_kg + (size_t)i * CFM_H * 64);
        for (int j = 0; j < CFM_FI; ++j) {
            host[o_b1 + (size_t)i * 2 * CFM_FIP + j] = L.ff1_b[j];
            host[o_b1 + (size_t)i * 2 * CFM_FIP + CFM_FIP + j] = L.ff1_b[CFM_FI + j];
        }
        std::copy(L.ff2_b, L.ff2_b + CFM_D, host.begin() + o_b2 + (size_t)i * CFM_D);
    }
    const size_t o_fg = add(w->final_gamma, CFM_D), o_pw = add(w->to_pred_w, (size_t)CFM_OUT * CFM_D);
    // GEMM operands (packed, CFM_SLACK zero rows each)
    const size_t o_wc = alloc((size_t)(CFM_D + CFM_SLACK) * CFM_COND);
    for (int c = 0; c < CFM_D; ++c)
        std::copy(w->to_embed_w + (size_t)c * EW + CFM_PROJ, w->to_embed_w + (size_t)c * EW + CFM_PROJ + CFM_COND, host.begin() + o_wc + (size_t)c * CFM_COND);
    size_t o_qkv[SYLBER_CFM_DEPTH], o_o[SYLBER_CFM_DEPTH], o_1[SYLBER_CFM_DEPTH], o_2[SYLBER_CFM_DEPTH];
    for (int i = 0; i < SYLBER_CFM_DEPTH; ++i) {
        const SylberCfmLayer& L = w->layers[i];
        o_qkv[i] = alloc((size_t)(3 * CFM_D + CFM_SLACK) * CFM_D);
        std::copy(L.qkv_w, L.qkv_w + (size_t)3 * CFM_D * CFM_D, host.begin() + o_qkv[i]);
        o_o[i] = alloc((size_t)(CFM_D + CFM_SLACK) * CFM_D);
        std::copy(L.out_w, L.out_w + (size_t)CFM_D * CFM_D, host.begin() + o_o[i]);
        o_1[i] = alloc((size_t)(2 * CFM_FIP + CFM_SLACK) * CFM_D);      // rows [0, 1365) value, [1408, 2773) gate, the rest zero
        std::copy(L.ff1_w, L.ff1_w + (size_t)CFM_FI * CFM_D, host.begin() + o_1[i]);
        std::copy(L.ff1_w + (size_t)CFM_FI * CFM_D, L.ff1_w + (size_t)2 * CFM_FI * CFM_D, host.begin() + o_1[i] + (size_t)CFM_FIP * CFM_D);
        o_2[i] = alloc((size_t)(CFM_D + CFM_SLACK) * CFM_FIP);           // [512][1408], columns 1365.. zero
        for (int r = 0; r < CFM_D; ++r)
            std::copy(L.ff2_w + (size_t)r * CFM_FI, L.ff2_w + (size_t)(r + 1) * CFM_FI, host.begin() + o_2[i] + (size_t)r * CFM_FIP);
    }
    const size_t gemm_begin = o_wc, gemm_end = host.size();
    h->bytes = host.size() * 4;
    if (hipMalloc((void**)&h->base, h->bytes) != hipSuccess || hipMemcpy(h->base, host.data(), h->bytes, hipMemcpyHostToDevice) != hipSuccess) {
        if (h->base) (void)hipFree(h->base);
        delete h; syl_set_error("sylber_cfm_create", "weight upload failed"); return 1;
    }
    float* B0 = h->base;
    h->t_w = B0 + o_tw; h->t1_w = B0 + o_t1w; h->t1_b = B0 + o_t1b; h->gb_w = B0 + o_gbw; h->gb_b = B0 + o_gbb;
    h->wy = B0 + o_wy; h->by = B0 + o_by; h->conv_w = B0 + o_cw; h->conv_b = B0 + o_cb; h->reg = B0 + o_reg; h->inv_freq = B0 + o_inv;
    h->qg = B0 + o_qg; h->kg = B0 + o_kg; h->b1 = B0 + o_b1; h->b2 = B0 + o_b2; h->fin_g = B0 + o_fg; h->pred_w = B0 + o_pw;
    if (precision == SYLBER_FP32) {
        h->wc = B0 + o_wc;
        for (int i = 0; i < SYLBER_CFM_DEPTH; ++i) { h->wqkv[i] = B0 + o_qkv[i]; h->wo[i] = B0 + o_o[i]; h->w1[i] = B0 + o_1[i]; h->w2[i] = B0 + o_2[i]; }
    } else {
        // 16-bit copies of the GEMM region (same offsets relative to its start)
        const size_t n16 = gemm_end - gemm_begin;
        h->bytes16 = n16 * 2;
        if (hipMalloc((void**)&h->base16, h->bytes16) != hipSuccess) { (void)hipFree(h->base); delete h; syl_set_error("sylber_cfm_create", "weight upload failed"); return 1; }
        if (h->fmt == FMT_F16) hipLaunchKernelGGL(cfm_convert<FMT_F16>, dim3(1024), dim3(256), 0, 0, B0 + gemm_begin, h->base16, n16);
        else hipLaunchKernelGGL(cfm_convert<FMT_BF16>, dim3(1024), dim3(256), 0, 0, B0 + gemm_begin, h->base16, n16);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            (void)hipFree(h->base16); (void)hipFree(h->base); delete h; syl_set_error("sylber_cfm_create", "weight conversion failed"); return 1;
        }
        bf16_t* W0 = h->base16 - gemm_begin;
        h->wc = W0 + o_wc;
        for (int i = 0; i < SYLBER_CFM_DEPTH; ++i) { h->wqkv[i] = W0 + o_qkv[i]; h->wo[i] = W0 + o_o[i]; h->w1[i] = W0 + o_1[i]; h->w2[i] = W0 + o_2[i]; }
    }
    *out = h;
    return 0;
}

extern "C" void sylber_cfm_destroy(sylber_cfm_t h) {
    if (!h) return;
    DevGuardC dg(h->device);
    if (h->base16) (void)hipFree(h->base16);
    if (h->base) (void)hipFree(h->base);
    delete h;
}

extern "C" int64_t sylber_cfm_workspace_bytes(sylber_cfm_t h, int32_t B, int32_t T) {
    if (!h || B < 1 || T < 1) { syl_set_error("sylber_cfm_workspace_bytes", "bad argument"); return -1; }
    return (int64_t)cfm_layout(h->precision, B, T).o_total;
}

static int cfm_check(const char* what, sylber_cfm_t h, const float* cond, int B, int T, const float* out, void* ws) {
    if (!h || !cond || !out || !ws) { syl_set_error(what, "null argument"); return 1; }
    if (B < 1 || T < 1 || (long)B * (CFM_REG + T + 31) > (1l << 24)) { syl_set_error(what, "need B >= 1, T >= 1 and B * (16 + T) < 2^24 rows"); return 1; }
    return 0;
}

// frames_host: nullptr (sylber_cfm_sample) or each row's own frame count (sylber_cfm_sample_frames)
static int cfm_steps(const sylber_cfm* h, const CfmLayout& l, char* ws, const float* cond_emb_dev, int steps, const float* y0_dev, float pitch_amp,
                     float* art_dev, size_t n, int T, const int* valid, hipStream_t s);

static int cfm_sample(const char* what, sylber_cfm_t h, const float* cond_emb_dev, const int32_t* frames_host, int32_t B, int32_t T, int32_t steps,
                      const float* y0_dev, float pitch_amp, float* art_dev, void* workspace_dev, void* stream) {
    if (cfm_check(what, h, cond_emb_dev, B, T, art_dev, workspace_dev)) return 1;
    if (steps < 1 || 2 * (steps - 1) > CFM_MAX_TIMES) { syl_set_error(what, "steps must be in 1..65"); return 1; }
    if (!(pitch_amp != 0.0f) || !std::isfinite(pitch_amp)) { syl_set_error(what, "pitch_amp must be finite and nonzero"); return 1; }
    if (frames_host)
        for (int b = 0; b < B; ++b)
            if (frames_host[b] < 1 || frames_host[b] > T) { syl_set_error(what, "frames must be in [1, T]"); return 1; }
    DevGuardC dg(h->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * T * CFM_OUT;
    const CfmLayout l = cfm_layout(h->precision, B, T);
    if (cfm_tap_check(what, h, l, steps)) return 1;
    char* ws = (char*)workspace_dev;
    int* valid = nullptr;
    if (frames_host) {
        valid = (int*)(ws + l.o_valid);
        if (launch_upload_ints(valid, frames_host, B, CFM_REG, s)) return 1;
    }
    return cfm_steps(h, l, ws, cond_emb_dev, steps, y0_dev, pitch_amp, art_dev, n, T, valid, s);
}

// the sampler over a prepared layout: art (n = NF * 14 floats) is the state; valid / T: cfm_init_state's masking (padded rows)
static int cfm_steps(const sylber_cfm* h, const CfmLayout& l, char* ws, const float* cond_emb_dev, int steps, const float* y0_dev, float pitch_amp,
                     float* art_dev, size_t n, int T, const int* valid, hipStream_t s) {
    // art is the sampler state; steps == 1 is a one-point grid (the state is y0) and scales channel 12 right away
    // (a tap leaves art alone: the state of its one evaluation lives in the workspace's midpoint buffer, written after cfm_prepare's clear)
    const bool tap = h->tap_stage != 0;
    float* ymid = (float*)(ws + l.o_y);
    float* state = tap ? ymid : art_dev;
    auto init = [&]() {
        hipLaunchKernelGGL(cfm_init_state, dim3(256), dim3(256), 0, s, y0_dev, state, n, steps == 1 ? 1 : 0, pitch_amp, valid, T);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    if (!tap && init()) return 1;
    if (steps == 1) return 0;
    std::vector<float> t;
    cfm_linspace(steps, t);
    std::vector<float> times;
    std::vector<float> dts;
    for (int i = 0; i + 1 < steps; ++i) {
        const float dt = t[i + 1] - t[i], half = 0.5f * dt;
        times.push_back(t[i]); times.push_back(t[i] + half); dts.push_back(dt);
    }
    if (cfm_prepare(h, l, ws, cond_emb_dev, times.data(), (int)times.size(), s)) return 1;
    if (tap) {
        if (init()) return 1;
        const int r = cfm_evaluate(h, l, ws, 0, state, state, state, 1, 0.5f * dts[0], 0, pitch_amp, s, valid);
        if (r == 0) syl_set_error("sylber_cfm tap", "the evaluation ended without reaching the tap's stage");   // (cfm_tap_check rules it out)
        return r == CFM_TAPPED ? 0 : 1;
    }
    for (int i = 0; i + 1 < steps; ++i) {
        const float dt = dts[i], half = 0.5f * dt;
        if (cfm_evaluate(h, l, ws, 2 * i, art_dev, art_dev, ymid, 1, half, 0, pitch_amp, s, valid)) return 1;
        if (cfm_evaluate(h, l, ws, 2 * i + 1, ymid, art_dev, art_dev, 2, dt, i + 2 == steps, pitch_amp, s, valid)) return 1;
    }
    return 0;
}

extern "C" int sylber_cfm_sample(sylber_cfm_t h, const float* cond_emb_dev, int32_t B, int32_t T, int32_t steps, const float* y0_dev,
                                 float pitch_amp, float* art_dev, void* workspace_dev, void* stream) {
    return cfm_sample("sylber_cfm_sample", h, cond_emb_dev, nullptr, B, T, steps, y0_dev, pitch_amp, art_dev, workspace_dev, stream);
}

extern "C" int sylber_cfm_sample_frames(sylber_cfm_t h, const float* cond_emb_dev, const int32_t* frames_host, int32_t B, int32_t T,
                                        int32_t steps, const float* y0_dev, float pitch_amp, float* art_dev, void* workspace_dev, void* stream) {
    if (!frames_host) { syl_set_error("sylber_cfm_sample_frames", "null argument"); return 1; }
    return cfm_sample("sylber_cfm_sample_frames", h, cond_emb_dev, frames_host, B, T, steps, y0_dev, pitch_amp, art_dev, workspace_dev, stream);
}

// ---- packed batches ----------------------------------------------------------------------------------------------------
extern "C" int sylber_cfm_packed_layout(const int32_t* frames_host, int32_t B, int32_t* slot_offsets) {
    if (!frames_host || !slot_offsets || B < 1) { syl_set_error("sylber_cfm_packed_layout", "need B >= 1 and non-null arrays"); return 1; }
    std::vector<int32_t> slot;
    long nf = 0;
    if (!cfm_slots(frames_host, B, slot, nf)) {
        syl_set_error("sylber_cfm_packed_layout", "every clip needs >= 1 frame, and the slots must total fewer than 2^24 rows"); return 1;
    }
    std::copy(slot.begin(), slot.end(), slot_offsets);
    return 0;
}

// the checks every packed entry point makes before it touches the device
static bool cfm_packed_check(const char* what, sylber_cfm_t h, const int32_t* frames_host, int B, std::vector<int32_t>& slot, long& nf) {
    if (!h || !frames_host) { syl_set_error(what, "null argument"); return false; }
    if (B < 1) { syl_set_error(what, "need B >= 1"); return false; }
    if (h->precision != SYLBER_BF16 && h->precision != SYLBER_FP16) {
        syl_set_error(what, "packed batches run in the bf16 and fp16 precisions only"); return false;
    }
    if (!cfm_slots(frames_host, B, slot, nf)) { syl_set_error(what, "every clip needs >= 1 frame, and the slots must total fewer than 2^24 rows"); return false; }
    return true;
}

extern "C" int64_t sylber_cfm_workspace_bytes_packed(sylber_cfm_t h, const int32_t* frames_host, int32_t B) {
    std::vector<int32_t> slot;
    long nf = 0;
    if (!cfm_packed_check("sylber_cfm_workspace_bytes_packed", h, frames_host, B, slot, nf)) return -1;
    return (int64_t)cfm_layout_packed(h->precision, B, slot[B], nf).o_total;
}

extern "C" int sylber_cfm_sample_packed(sylber_cfm_t h, const float* cond_dev, const int32_t* frames_host, int32_t B, int32_t steps,
                                        const float* y0_dev, float pitch_amp, float* art_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_cfm_sample_packed";
    std::vector<int32_t> slot;
    long nf = 0;
    if (!cfm_packed_check(what, h, frames_host, B, slot, nf)) return 1;
    if (!cond_dev || !art_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (steps < 1 || 2 * (steps - 1) > CFM_MAX_TIMES) { syl_set_error(what, "steps must be in 1..65"); return 1; }
    if (!(pitch_amp != 0.0f) || !std::isfinite(pitch_amp)) { syl_set_error(what, "pitch_amp must be finite and nonzero"); return 1; }
    std::vector<int32_t> tab;
    cfm_packed_table(frames_host, B, slot, tab);
    DevGuardC dg(h->device);
    hipStream_t s = (hipStream_t)stream;
    CfmLayout l = cfm_layout_packed(h->precision, B, slot[B], nf);
    l.total_qb = tab[3 * (size_t)B + 1];
    if (cfm_tap_check(what, h, l, steps)) return 1;
    char* ws = (char*)workspace_dev;
    if (launch_upload_ints((int*)(ws + l.o_valid), tab.data(), (int)tab.size(), 0, s)) return 1;
    return cfm_steps(h, l, ws, cond_dev, steps, y0_dev, pitch_amp, art_dev, (size_t)nf * CFM_OUT, 1, nullptr, s);
}

extern "C" int sylber_cfm_eval(sylber_cfm_t h, const float* x_dev, float t, const float* cond_emb_dev, int32_t B, int32_t T, float* v_dev,
                               void* workspace_dev, void* stream) {
    if (cfm_check("sylber_cfm_eval", h, cond_emb_dev, B, T, v_dev, workspace_dev)) return 1;
    if (!x_dev) { syl_set_error("sylber_cfm_eval", "null argument"); return 1; }
    DevGuardC dg(h->device);
    hipStream_t s = (hipStream_t)stream;
    const CfmLayout l = cfm_layout(h->precision, B, T);
    if (cfm_tap_check("sylber_cfm_eval", h, l, 2)) return 1;
    char* ws = (char*)workspace_dev;
    if (cfm_prepare(h, l, ws, cond_emb_dev, &t, 1, s)) return 1;
    const int r = cfm_evaluate(h, l, ws, 0, x_dev, x_dev, v_dev, 0, 0.f, 0, 1.f, s);
    return r == CFM_TAPPED ? 0 : r;
}

// ---- development tap (include/sylber_hip_dev.h) -------------------------------------------------------------------------------
extern "C" int sylber_cfm_set_tap(sylber_cfm_t h, int32_t stage, float* tap_dev, int64_t tap_floats) {
    if (!h) { syl_set_error("sylber_cfm_set_tap", "null handle"); return 1; }
    if (stage == 0) { h->tap_stage = 0; h->tap_dev = nullptr; h->tap_floats = 0; return 0; }
    CfmTapBuf t;
    if (!cfm_tap_buf(h->precision, cfm_layout(h->precision, 1, 1), stage, t)) {
        syl_set_error("sylber_cfm_set_tap", "unknown stage (or one this precision does not have)"); return 1;
    }
    if (!tap_dev || tap_floats < 1) { syl_set_error("sylber_cfm_set_tap", "need a tap buffer"); return 1; }
    h->tap_stage = stage; h->tap_dev = tap_dev; h->tap_floats = tap_floats;
    return 0;
}

extern "C" int64_t sylber_cfm_tap_floats(sylber_cfm_t h, int32_t stage, int32_t B, int32_t T) {
    CfmTapBuf t;
    if (!h || B < 1 || T < 1 || (long)B * (CFM_REG + T + 31) > (1l << 24)) return -1;
    return cfm_tap_buf(h->precision, cfm_layout(h->precision, B, T), stage, t) ? t.n : -1;
}

extern "C" int64_t sylber_cfm_tap_floats_packed(sylber_cfm_t h, int32_t stage, const int32_t* frames_host, int32_t B) {
    std::vector<int32_t> slot;
    long nf = 0;
    CfmTapBuf t;
    if (!cfm_packed_check("sylber_cfm_tap_floats_packed", h, frames_host, B, slot, nf)) return -1;
    return cfm_tap_buf(h->precision, cfm_layout_packed(h->precision, B, slot[B], nf), stage, t) ? t.n : -1;
}

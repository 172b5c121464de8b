// The encoder forward of libsylber_hip.so: frame arithmetic, the workspace plan of every mode, and the launch sequence of
//   sylber/model/sylber.py:122  speech_model(batch, attention_mask).last_hidden_state
// one function per stage (conv0, conv stack, feature projection, pos-conv, encoder layer), for the 16-bit / fp8 modes (Forward) and
// the fp32 parity mode (ForwardF32).  The launch names given to RUN are an interface: sylber_get_profile returns them and bench.py
// keys its FLOP counts on them.
#include "ctx.h"

extern "C" int32_t sylber_num_frames(int32_t n) {
    for (int i = 0; i < 7; ++i) n = (n - CK[i]) / CS[i] + 1;
    return n;
}

// frame pitch per utterance of the internal activation buffers: enough rows for every conv layer's valid outputs at
// its 2^(6-i) rows-per-frame pitch, rounded up to 32 (a 32-row MFMA block then never straddles two utterances, and
// 32 x 10 s = 16384 rows is a whole number of 256-row tiles)
static int frames_needed(int Lmax) {
    int n = Lmax, tp = 0;
    for (int i = 0; i < 7; ++i) {
        n = (n - CK[i]) / CS[i] + 1;
        const int f = 1 << (6 - i);
        const int need = (n + f - 1) / f;
        tp = need > tp ? need : tp;
    }
    return tp;
}
static int padded_frames(int Lmax) { return (frames_needed(Lmax) + 31) & ~31; }
extern "C" int32_t sylber_padded_frames(int32_t n_samples) { return n_samples < 400 ? 0 : padded_frames(n_samples); }

// packed batches: clip b's slot holds every conv layer's valid rows of a call of its own length (frames_needed, which can exceed its
// frame count by one or two), rounded up to whole 64-key attention tiles; the slots follow each other from frame 0
#define SYL_SLOT_ALIGN 64
extern "C" int sylber_packed_layout(const int32_t* samples_host, int32_t B, int32_t* offsets, int32_t* frames) {
    if (!samples_host || !offsets || !frames || B < 1) { syl_set_error("sylber_packed_layout", "need B >= 1 and non-null arrays"); return 1; }
    // the waveform offsets (SYL_SLOT_SAMPLES x frame offset) and the conv1 GEMM's rows (64 x frames) are 32-bit in the kernels
    const long long cap = (long long)INT32_MAX / SYL_SLOT_SAMPLES;
    long long off = 0;
    for (int b = 0; b < B; ++b) {
        if (samples_host[b] < 400) { syl_set_error("sylber_packed_layout", "every clip needs at least 400 samples (one frame)"); return 1; }
        offsets[b] = (int32_t)off;
        frames[b] = sylber_num_frames(samples_host[b]);
        off += (frames_needed(samples_host[b]) + SYL_SLOT_ALIGN - 1) & ~(SYL_SLOT_ALIGN - 1);
        if (off > cap) { syl_set_error("sylber_packed_layout", "the packed batch is too long (more than 2^31 waveform samples)"); return 1; }
    }
    offsets[B] = (int32_t)off;
    return 0;
}

// ---- workspace plans ------------------------------------------------------------------------------------------------
// One layout per mode, each built by a plan function below: make_plan (the 16-bit modes and fp8), make_plan_packed, make_plan_f32.
struct Plan {
    int B, Lmax, L[7], T, Tp, Tpv, R[7];
    size_t o_bufA, o_bufB, o_ln512, o_xf32, o_xpad, o_pre, o_stats, o_hbf16, o_q, o_k, o_vt, o_ctx, o_ffn, o_part, o_ss, o_valid,
        o_rows, o_pk, total;
    int nchunk;
    bool zero_all = false;        // zero the whole workspace on a layout change (split16: pad regions of both planes; fp32 parity plan)
    // SYLBER_SPLIT16: every 16-bit buffer holds two half planes; element offsets of the lo planes (0 otherwise)
    long lo_bufA = 0, lo_bufB = 0, lo_ln512 = 0, lo_xpad = 0, lo_hbf = 0, lo_qk = 0, lo_vt = 0, lo_ctx = 0, lo_ffn = 0;
};

// hands out 256-byte aligned offsets
struct Take {
    size_t off = 0;
    size_t operator()(size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; }
};

// valid rows of every conv layer for n samples, and the chunks of the GroupNorm partials
static void plan_conv_rows(Plan& p, int n) {
    for (int i = 0; i < 7; ++i) { n = (n - CK[i]) / CS[i] + 1; p.L[i] = n; }
    p.nchunk = (p.L[0] + 2047) / 2048;
}
// geometry of a padded batch: B utterances at a pitch of Tp frames
static void plan_padded(Plan& p, int B, int Lmax) {
    p.B = B; p.Lmax = Lmax;
    plan_conv_rows(p, Lmax);
    p.T = p.L[6];
    p.Tp = padded_frames(Lmax);
    p.Tpv = (p.Tp + 63) & ~63;
    for (int i = 0; i < 7; ++i) p.R[i] = p.Tp << (6 - i);
}
// test aid (host arithmetic only): the plan's valid rows L[7] and rows per utterance R[7] of every conv layer's output buffer
extern "C" int sylber_debug_conv_rows(int32_t n_samples, int32_t* L, int32_t* R) {
    if (!L || !R || n_samples < 400) { syl_set_error("sylber_debug_conv_rows", "need at least 400 samples and non-null arrays"); return 1; }
    Plan p = {};
    plan_padded(p, 1, n_samples);
    for (int i = 0; i < 7; ++i) { L[i] = p.L[i]; R[i] = p.R[i]; }
    return 0;
}

// the workspace offsets of a plan whose geometry is set: nb = utterances of the per-utterance tables (GroupNorm
// partials, scale / shift, valid, rows), ntab = ints of a packed batch's slot tables (0: none)
static void plan_buffers(Plan& p, int planes, int nb, int ntab) {
    const int B = p.B;
    Take take;
    const size_t M = (size_t)B * p.Tp;
    const size_t P = (size_t)planes;
    p.o_bufA = take(((size_t)B * p.R[0] + 8) * 512 * 2 * P);
    p.o_bufB = take(((size_t)B * p.R[1] + 8) * 512 * 2 * P);
    p.o_ln512 = take(M * 512 * 2 * P);
    p.o_xf32 = take(M * 768 * 4);
    p.o_xpad = take((size_t)B * (p.Tp + 128) * 768 * 2 * P);
    p.o_pre = take(M * 768 * 4);
    p.o_stats = take(M * 2 * 4);
    p.o_hbf16 = take((M + 128) * 768 * 2 * P);
    if (planes == 2) {
        p.lo_bufA = (long)(((size_t)B * p.R[0] + 8) * 512); p.lo_bufB = (long)(((size_t)B * p.R[1] + 8) * 512);
        p.lo_ln512 = (long)(M * 512); p.lo_xpad = (long)((size_t)B * (p.Tp + 128) * 768); p.lo_hbf = (long)((M + 128) * 768);
        p.lo_qk = (long)(M * 768); p.lo_vt = (long)((size_t)B * 12 * 64 * p.Tpv); p.lo_ctx = (long)((M + 128) * 768);
        p.lo_ffn = (long)((M + 128) * 3072);
        p.zero_all = true;
    }
    // q, k, V^T and the attention context are dead by the time FFN1 writes its intermediate, and that is dead before the
    // next layer's q/k/v projection: the FFN intermediate ALIASES them, which keeps a layer's working set
    // (residual stream + bf16 copy + this region + weights = ~190 MB at 32 x 10 s) inside the 256 MB Infinity Cache
    const size_t attn_begin = take.off;
    p.o_q = take(M * 768 * 2 * P);
    p.o_k = take(M * 768 * 2 * P);
    p.o_vt = take((size_t)B * 12 * 64 * p.Tpv * 2 * P);
    p.o_ctx = take((M + 128) * 768 * 2 * P);
    p.o_ffn = attn_begin;
    {
        const size_t need = (M + 128) * 3072 * 2 * P;
        if (take.off - attn_begin < need) take(need - (take.off - attn_begin));
    }
    p.o_part = take((size_t)nb * p.nchunk * 65 * 8);
    p.o_ss = take((size_t)nb * 512 * 2 * 4);
    p.o_valid = take((size_t)nb * 4);
    p.o_rows = take((size_t)nb * 4);
    p.o_pk = ntab > 0 ? take((size_t)ntab * 4) : 0;
    p.total = take.off;
}

static Plan make_plan(int B, int Lmax, int planes) {
    Plan p = {};
    plan_padded(p, B, Lmax);
    plan_buffers(p, planes, B, 0);
    return p;
}

// a packed batch (sylber_forward_packed): ONE pseudo-utterance of Ptot frames (a multiple of 64) holding `nclip` slots.  B = 1 and
// T = Tp = Tpv = Ptot for every launch that sees the whole batch; Lmax = -Ptot is the layout key of ensure_workspace (never a padded
// layout's).  L[i] = the longest clip's (nmax samples) valid rows of layer i: L[0] sizes the GroupNorm partials, each clip's own
// counts live in the slot tables.
static Plan make_plan_packed(int nclip, int Ptot, int nmax) {
    Plan p = {};
    p.B = 1; p.Lmax = -Ptot;
    plan_conv_rows(p, nmax);
    p.T = p.Tp = p.Tpv = Ptot;
    for (int i = 0; i < 7; ++i) p.R[i] = p.Tp << (6 - i);
    plan_buffers(p, 1, nclip, 3 * nclip + 2);
    return p;
}

// fp32 parity mode: the padded geometry, every tensor fp32.  o_hbf16 is the LayerNorm output h, o_q the fused [M][2304] q | k | v; there
// are no row statistics, no separate k / V^T and no slot tables (their offsets stay 0), and nothing aliases.
static Plan make_plan_f32(int B, int Lmax) {
    Plan p = {};
    plan_padded(p, B, Lmax);
    Take take;
    const size_t M = (size_t)B * p.Tp;
    p.o_bufA = take(((size_t)B * p.R[0] + 8) * 512 * 4);
    p.o_bufB = take(((size_t)B * p.R[1] + 8) * 512 * 4);
    p.o_ln512 = take(M * 512 * 4);
    p.o_xf32 = take(M * 768 * 4);
    p.o_xpad = take((size_t)B * (p.Tp + 128) * 768 * 4);
    p.o_pre = take(M * 768 * 4);
    p.o_hbf16 = take(M * 768 * 4);
    p.o_q = take(M * 2304 * 4);
    p.o_ctx = take(M * 768 * 4);
    p.o_ffn = take(M * 3072 * 4);
    p.o_part = take((size_t)B * p.nchunk * 65 * 8);
    p.o_ss = take((size_t)B * 512 * 2 * 4);
    p.o_valid = take((size_t)B * 4);
    p.o_rows = take((size_t)B * 4);
    p.total = take.off;
    p.zero_all = true;
    return p;
}

static int ensure_workspace(sylber_ctx* c, const Plan& p, hipStream_t s) {
    if (p.total > c->ws_bytes) {
        HIP_TRY(hipStreamSynchronize(s));
        if (c->ws) HIP_TRY(hipFree(c->ws));
        c->ws = nullptr; c->ws_bytes = 0;
        HIP_TRY(hipMalloc((void**)&c->ws, p.total));
        c->ws_bytes = p.total;
        c->ws_B = 0;
    }
    if (c->ws_B != p.B || c->ws_Lmax != p.Lmax) {
        // layout changed: the regions that are read but never (fully) written must read as zeros -- the pos-conv
        // input's halo rows, the V^T key tail [Tp, Tpv) and the slack rows behind the GEMM operands (which only ever
        // feed rows beyond M, but must stay finite).  Everything else is written before it is read, so a ragged
        // serving loop (new Lmax per call) pays ~60 MB of memset instead of the whole 2 GB workspace.
        const size_t M = (size_t)p.B * p.Tp;
        if (p.zero_all) HIP_TRY(hipMemsetAsync(c->ws, 0, p.total, s));
        else {
            HIP_TRY(hipMemsetAsync(c->ws + p.o_xpad, 0, (size_t)p.B * (p.Tp + 128) * 768 * 2, s));
            HIP_TRY(hipMemsetAsync(c->ws + p.o_vt, 0, (size_t)p.B * 12 * 64 * p.Tpv * 2, s));
            HIP_TRY(hipMemsetAsync(c->ws + p.o_bufA + (size_t)p.B * p.R[0] * 512 * 2, 0, 8 * 512 * 2, s));
            HIP_TRY(hipMemsetAsync(c->ws + p.o_bufB + (size_t)p.B * p.R[1] * 512 * 2, 0, 8 * 512 * 2, s));
            HIP_TRY(hipMemsetAsync(c->ws + p.o_hbf16 + M * 768 * 2, 0, 128 * 768 * 2, s));
            HIP_TRY(hipMemsetAsync(c->ws + p.o_ctx + M * 768 * 2, 0, 128 * 768 * 2, s));
            HIP_TRY(hipMemsetAsync(c->ws + p.o_ffn + M * 3072 * 2, 0, (size_t)128 * 3072 * 2, s));
        }
        c->ws_B = p.B; c->ws_Lmax = p.Lmax;
    }
    return 0;
}

// host ints -> device, without a host staging buffer: the values travel as kernel arguments (64 per
// launch), so there is no pageable hipMemcpyAsync (an implicit host synchronisation) and nothing whose lifetime
// the caller has to think about
struct ValidPack { int v[64]; };
__global__ void set_valid_kernel(int* __restrict__ dst, ValidPack p, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = p.v[threadIdx.x];
}
int launch_upload_ints(int* dst, const int32_t* vals_host, int n, int add, hipStream_t s) {
    for (int b0 = 0; b0 < n; b0 += 64) {
        ValidPack pk;
        const int k = n - b0 < 64 ? n - b0 : 64;
        for (int i = 0; i < k; ++i) pk.v[i] = vals_host[b0 + i] + add;
        hipLaunchKernelGGL(set_valid_kernel, dim3(1), dim3(64), 0, s, dst + b0, pk, k);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// what every forward call does before its first launch: the workspace of the call's plan, no captured graph left that holds another
// workspace's addresses, and the call's per-utterance tables on the device (before any capture or replay: a replayed graph reads
// this call's values).  An upload without host values is skipped.
struct Upload { size_t off; const int32_t* host; int n; };
static int begin_call(sylber_ctx* c, const Plan& p, std::initializer_list<Upload> uploads, hipStream_t s) {
    char* ws_before = c->ws;
    if (ensure_workspace(c, p, s)) return 1;
    if (c->ws != ws_before) graphs_clear(c);
    for (const Upload& u : uploads)
        if (u.host && launch_upload_ints((int*)(c->ws + u.off), u.host, u.n, 0, s)) return 1;
    return 0;
}

// ---- fp16 headroom audit --------------------------------------------------------------------------------------------
// IEEE half tops out at 65504; the fp16 modes SATURATE on conversion (H16<FMT_F16>::sat) instead of producing infinities, so a
// checkpoint whose activations outgrow the format is clamped silently.  With SYLBER_OPT_FP16_AUDIT on, every producer of a 16-bit
// activation buffer is followed by a scan of what it wrote: values AT +-65504 (0x7bff) are counted as saturated, the largest magnitude is
// kept as the stage's headroom figure.  Off (default): nothing is launched.  Synthetic weights have never come near the limit; real ones
// have never been seen by this library (the checkpoint is not obtainable offline) -- this is how a user finds out.
static const char* const AUDIT_NAMES[AUDIT_STAGES] = {"conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "ln512", "proj_xpad", "layernorm",
                                                      "q", "k", "v", "context", "ffn1"};
__global__ __launch_bounds__(256) void audit16_kernel(const unsigned short* __restrict__ buf, long rows, long cols, long pitch, unsigned* __restrict__ slot) {
    unsigned sat = 0, mx = 0;
    const long n = rows * cols;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const unsigned a = buf[(i / cols) * pitch + i % cols] & 0x7fffu;
        if (a <= 0x7c00u) mx = a > mx ? a : mx;             // (NaN patterns are not magnitudes)
        sat += a == 0x7bffu;
    }
    for (int d = 32; d >= 1; d >>= 1) { sat += __shfl_xor(sat, d, 64); const unsigned o = __shfl_xor(mx, d, 64); mx = o > mx ? o : mx; }
    if ((threadIdx.x & 63) == 0) { if (sat) atomicAdd(slot, sat); atomicMax(slot + 1, mx); }
}
static int audit16(sylber_ctx* c, int stage, const void* buf, long rows, long cols, long pitch, hipStream_t s) {
    if (!c->opt_audit16 || !c->audit_dev) return 0;
    long blocks = (rows * cols + 256L * 16 - 1) / (256L * 16);
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(audit16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const unsigned short*)buf, rows, cols, pitch, c->audit_dev + 2 * stage);
    HIP_TRY(hipGetLastError());
    return 0;
}
extern "C" int sylber_get_fp16_audit(sylber_t c, const char** names, uint32_t* saturated, float* max_abs, int32_t cap) {
    if (!c) { syl_set_error("sylber_get_fp16_audit", "null handle"); return -1; }
    if (!c->audit_dev) return 0;
    GUARD_DEVICE(c->device);
    unsigned host[AUDIT_STAGES * 2];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host, c->audit_dev, sizeof(host), hipMemcpyDeviceToHost) != hipSuccess) {
        syl_set_error("sylber_get_fp16_audit", "device read failed"); return -1;
    }
    const int n = cap < AUDIT_STAGES ? cap : AUDIT_STAGES;
    for (int i = 0; i < n; ++i) { names[i] = AUDIT_NAMES[i]; saturated[i] = host[2 * i]; max_abs[i] = h2f_host((bf16_t)host[2 * i + 1]); }
    return n;
}
// the scan of what the launch above it wrote, where the audit is on for that buffer's format (needs `c` and `s` in scope, like RUN)
#define AUDIT(on, stage, buf, rows, cols, pitch)                                                \
    do {                                                                                        \
        if ((on) && audit16(c, stage, buf, rows, cols, pitch, s)) return 1;                     \
    } while (0)

// ---- the launch sequences -------------------------------------------------------------------------------------------
// the handle's tuning options (sylber_set_option) for a GEMM launch of the encoder or the conv stack.  Every field is copied at every
// site: gemm_bf16.hip reads tune_mfma16 under EPI_BF16 only and tune_pre reaches the tile 91 loop under EPI_F32_RESLN only, so
// setting them for the other epilogues changes nothing.
static void tune_from_options(const sylber_ctx* c, GemmArgs& a) {
    a.tune_cfg = c->opt_gemm_cfg; a.tune_persist = c->opt_gemm_persist; a.tune_tail = c->opt_gemm_tail; a.tune_h192 = c->opt_gemm_h192;
    a.tune_mfma16 = c->opt_gemm_mfma16; a.tune_model = c->opt_gemm_model; a.tune_pre = c->opt_resln_pre;
}

// the workspace's typed pointers, once from the plan: T = bf16_t (16-bit modes and fp8) or float (fp32 parity mode, whose plan
// leaves stats / k / vt / pk unused)
template <class T>
struct Ws {
    T *bufA, *bufB, *ln512, *xpad, *h, *q, *k, *vt, *ctx, *ffn;
    float *xf32, *pre, *stats, *ss; double* part; int *valid, *rows;
    Ws(char* w, const Plan& p) {
        bufA = (T*)(w + p.o_bufA); bufB = (T*)(w + p.o_bufB); ln512 = (T*)(w + p.o_ln512); xpad = (T*)(w + p.o_xpad); h = (T*)(w + p.o_hbf16);
        q = (T*)(w + p.o_q); k = (T*)(w + p.o_k); vt = (T*)(w + p.o_vt); ctx = (T*)(w + p.o_ctx); ffn = (T*)(w + p.o_ffn);
        xf32 = (float*)(w + p.o_xf32); pre = (float*)(w + p.o_pre); stats = (float*)(w + p.o_stats); ss = (float*)(w + p.o_ss);
        part = (double*)(w + p.o_part); valid = (int*)(w + p.o_valid); rows = (int*)(w + p.o_rows);
    }
};

// SYLBER_FP8: the same regions as MXFP8 operands -- e4m3 bytes in front, their E8M0 block scales (row pitch Mp) behind them.  The
// LayerNorm output h, the attention context and the FFN intermediate always; q / k / V^T where the attention core runs on MXFP8
// (k: one 64-key tile of slack in between, read by the last key tile of an utterance and masked)
struct WsF8 {
    long Mp;                                            // row pitch of the activations' scale arrays
    uint8_t *h, *hs, *ctx, *ctxs, *ffn, *ffns;          // scales: 24 Mp, 24 Mp and 96 Mp bytes
    uint8_t *q, *qs, *k, *ks, *v, *vs;
    WsF8(const Ws<bf16_t>& w, const Plan& p) {
        const size_t M = (size_t)p.B * p.Tp;
        Mp = ((long)M + 255) & ~255L;
        h = (uint8_t*)w.h; hs = h + ((M * 768 + 255) & ~(size_t)255);
        ctx = (uint8_t*)w.ctx; ctxs = ctx + ((M * 768 + 255) & ~(size_t)255);
        ffn = (uint8_t*)w.ffn; ffns = ffn + ((M * 3072 + 255) & ~(size_t)255);
        q = (uint8_t*)w.q; qs = q + M * 768;
        k = (uint8_t*)w.k; ks = k + M * 768 + 4096;
        v = (uint8_t*)w.vt; vs = v + (size_t)p.B * 768 * p.Tpv;
    }
};

// a packed batch (sylber_forward_packed): its slot tables on the device (Plan::o_pk) and the host-side sizes of its launches
struct PackedCall {
    int nclip, total_samples, slot_max, tail_max, total_qb;
    const int *slot, *frames, *qb, *rows0;     // [nclip + 1], [nclip], [nclip + 1], [nclip]; slot / frames / qb contiguous (attention)
};

// the taps in front of the encoder LayerNorm (SYLBER_TAP_PROJ / SYLBER_TAP_POSCONV): frames [0, T) of every utterance of an fp32
// [B][Tp][768] workspace tensor, compacted to [B][T][768].  Copies, so a tap call is never captured into a graph (sylber_forward).
static int copy_frames_f32(const float* src, float* dst, int B, int Tp, int T, hipStream_t s, int W = SYL_HIDDEN) {
    for (int b = 0; b < B; ++b)
        HIP_TRY(hipMemcpyAsync(dst + (size_t)b * T * W, src + (size_t)b * Tp * W, (size_t)T * W * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

// the taps inside an encoder layer (SYLBER_TAP_LAYER(l, k) = -(8 (l + 1) + k)): the layer and the launch a call stops behind
struct LayerTap {
    int l = -1, k = -1;
    explicit LayerTap(int stop_stage) { if (stop_stage <= -8 && stop_stage > -1024) { l = -stop_stage / 8 - 1; k = -stop_stage % 8; } }
};
// the taps behind conv layer i = 1..6 (SYLBER_TAP_CONV(i) = -(1024 + i)): the layer a call stops behind, 0 for every other stage
static int conv_tap_layer(int stop_stage) { return (stop_stage <= SYLBER_TAP_CONV(1) && stop_stage >= SYLBER_TAP_CONV(6)) ? -stop_stage - 1024 : 0; }

// every kernel launch of the bf16 / fp16 / mixed16 / split16 / fp8 forward, in stream order; nothing else (no allocation, copy or
// synchronisation), so the sequence can be replayed from a captured hipGraph.  pk: a packed batch (bf16 / fp16), nullptr for the padded
// one; only conv0, the zeroing of the slot tails, the pos-conv and the attention read its tables.
// The one exception: with a negative stop stage (a tap) run() ends in device-to-device copies (copy_frames_f32) or a widening copy
// kernel; sylber_forward never captures such a call and sylber_forward_packed refuses it.
struct Forward {
    sylber_ctx* c; const Plan& p; const float* wav_dev; float* hidden_dev; hipStream_t s; const PackedCall* pk;
    const Ws<bf16_t> w; const WsF8 w8;
    const int B, M;
    const bool split;                                   // hi / lo half planes, erf GELU (fp32-grade decisions)
    const bool f8;                                      // the encoder layers on MXFP8 operands
    const bool aud_c, aud_e;                            // fp16 audit of the conv stack / of the encoder (never captured: graph mode is refused with it)
    const bf16_t* feats = nullptr; long feats_lo = 0;   // the conv stack's output [B*Tp][512]
    // the residual of every block is the previous LayerNorm's output; it is re-derived in the GEMM epilogue from
    // the pre-LN sum still sitting in `pre` (updated in place) + that LayerNorm's row statistics and affine
    const float *res_g = nullptr, *res_b = nullptr;
    const LayerTap tap;                                 // a tap inside a layer: layer16 / layer8 set `tapped` once they have copied it out
    const int ctap;                                     // a tap behind conv layer ctap (0: none): conv_stack sets `tapped` once it has copied it out
    bool tapped = false;

    Forward(sylber_ctx* c_, const Plan& p_, const float* wav, float* hidden, hipStream_t s_, const PackedCall* pk_)
        : c(c_), p(p_), wav_dev(wav), hidden_dev(hidden), s(s_), pk(pk_), w(c_->ws, p_), w8(w, p_), B(p_.B), M(p_.B * p_.Tp),
          split(c_->precision == SYLBER_SPLIT16), f8(c_->precision == SYLBER_FP8),
          aud_c(c_->opt_audit16 && c_->fmt_conv == FMT_F16), aud_e(c_->opt_audit16 && c_->fmt == FMT_F16), tap(c_->stop_stage),
          ctap(conv_tap_layer(c_->stop_stage)) {}

    // conv layer 0 + GroupNorm + GELU
    int conv0() {
        if (pk) {                                       // per slot: each utterance's own statistics, rows and waveform offset
            RUN("conv0_stats", launch_conv0_stats(wav_dev, pk->nclip, 0, p.L[0], w.part, p.nchunk, s, pk->rows0, pk->slot));
            RUN("conv0_finalize", launch_conv0_finalize(w.part, p.nchunk, c->conv0_w, c->gn_w, c->gn_b, pk->nclip, p.L[0], w.ss, s, pk->rows0));
            RUN("conv0_gn_gelu", launch_conv0_packed(wav_dev, pk->nclip, pk->total_samples, pk->slot_max, pk->rows0, pk->slot, c->conv0_w, w.ss, w.bufA, c->fmt_conv, s));
        } else {
            const int* rows0 = c->opt_per_utt ? w.rows : nullptr;   // per-utterance GroupNorm statistics (nullptr: padded L0)
            RUN("conv0_stats", launch_conv0_stats(wav_dev, B, p.Lmax, p.L[0], w.part, p.nchunk, s, rows0));
            RUN("conv0_finalize", launch_conv0_finalize(w.part, p.nchunk, c->conv0_w, c->gn_w, c->gn_b, B, p.L[0], w.ss, s, rows0));
            RUN("conv0_gn_gelu", launch_conv0_gn_gelu(wav_dev, B, p.Lmax, p.L[0], p.R[0], c->conv0_w, w.ss, w.bufA, 0, s, c->fmt_conv, p.lo_bufA, c->opt_conv0_valu));
        }
        AUDIT(aud_c, AUD_CONV0, w.bufA, (long)B * p.R[0], 512, 512);
        return 0;
    }

    // conv layers 1..6 as implicit GEMM (ping-pong between bufA and bufB)
    int conv_stack() {
        static const char* nm[7] = {"", "gemm_conv1", "gemm_conv2", "gemm_conv3", "gemm_conv4", "gemm_conv5", "gemm_conv6"};
        bf16_t* src = w.bufA; bf16_t* dst = w.bufB;
        long src_lo = p.lo_bufA, dst_lo = p.lo_bufB;
        for (int i = 1; i < 7; ++i) {
            GemmArgs a = {};
            a.X = src; a.ldx = (long)CS[i] * 512; a.W = c->conv_w[i]; a.M = B * p.R[i]; a.N = 512; a.K = CK[i] * 512;
            a.act = split ? ACT_GELU_ERF7 : ACT_GELU_FAST; a.out0 = dst; a.ld0 = 512; a.fmt = c->fmt_conv;
            a.x_lo = src_lo; a.w_lo = (long)512 * CK[i] * 512; a.out_lo = dst_lo;
            a.kpat = (CK[i] == 3 && c->fmt_conv != FMT_SPLIT) ? 1 : 0;      // chunk-major K order (weights packed to match at create)
            tune_from_options(c, a);
            RUN(nm[i], launch_gemm_bf16(EPI_BF16, a, s));
            AUDIT(aud_c, AUD_CONV0 + i, dst, (long)B * p.R[i], 512, 512);
            if (i == ctap) {                            // every row of the layer's output buffer, rows [L_i, R_i) included, widened exactly
                tapped = true;
                RUN("copy_out", launch_bf16_to_f32_rows(dst, 512, hidden_dev, B, p.R[i], p.R[i], 512, s, c->fmt_conv, dst_lo));
                return 0;
            }
            std::swap(src, dst); std::swap(src_lo, dst_lo);
        }
        feats = src; feats_lo = src_lo;
        return 0;
    }

    // a Linear of the encoder on 16-bit operands: X [M][K] (lo plane at x_lo), W [N][K]
    GemmArgs linear(const bf16_t* X, long x_lo, const bf16_t* W, const float* bias, int N, int K) const {
        GemmArgs g = {};
        g.X = X; g.ldx = K; g.x_lo = x_lo; g.W = W; g.w_lo = (long)N * K; g.bias = bias; g.M = M; g.N = N; g.K = K; g.fmt = c->fmt;
        return g;
    }
    // ... on MXFP8 operands
    GemmF8Args linear8(const uint8_t* X8, const uint8_t* XS, const uint8_t* W8, const uint8_t* WS, const float* bias, int N, int K) const {
        GemmF8Args g = {};
        g.g.M = M; g.g.N = N; g.g.K = K; g.g.bias = bias;
        g.X8 = X8; g.ldx8 = K; g.XS = XS; g.xs_rows = w8.Mp; g.W8 = W8; g.WS = WS; g.ws_rows = N;
        return g;
    }
    // the residual epilogue (EPI_F32_RESLN): pre <- acc + bias + LayerNorm(pre) with the statistics and affine (gamma, beta) of the LayerNorm before
    void residual(GemmArgs& g, const float* gamma, const float* beta) const {
        g.out0 = w.pre; g.ld0 = 768; g.res = w.pre; g.ldres = 768; g.ln_stats = w.stats; g.ln_gamma = gamma; g.ln_beta = beta;
    }

    // feature projection: LN(512) -> Linear(512->768), zero padded frames
    int projection() {
        LnArgs a = {};
        a.in = feats; a.in_bf16 = 1; a.ld_in = 512; a.gamma = c->fp_ln_w; a.beta = c->fp_ln_b;
        a.out_bf16 = w.ln512; a.ld_bf16 = 512; a.M = M; a.D = 512; a.fmt = c->fmt; a.fmt_in = c->fmt_conv;
        a.in_lo = feats_lo; a.out_lo = p.lo_ln512;
        RUN("ln512", launch_layernorm(a, s));
        GemmArgs g = linear(w.ln512, p.lo_ln512, c->fp_w, c->fp_b, 768, 512);     // deliberately no tune_from_options: the options never reached this launch
        g.out0 = w.xf32; g.ld0 = 768; g.out1 = w.xpad; g.Tp = p.Tp; g.T = p.T; g.valid = w.valid; g.xpad_rows = p.Tp + 128; g.out_lo = p.lo_xpad;
        RUN("gemm_proj", launch_gemm_bf16(EPI_PROJ, g, s));
        // packed: the projection sees one utterance; the frames behind each clip's own end are zeroed here instead (what valid[b] does)
        if (pk) RUN("zero_slot_tails", launch_zero_slot_tails(w.xf32, w.xpad, pk->slot, pk->frames, pk->nclip, pk->tail_max, s));
        AUDIT(aud_e, AUD_LN512, w.ln512, M, 512, 512);
        AUDIT(aud_e, AUD_XPAD, w.xpad, (long)B * (p.Tp + 128), 768, 768);
        return 0;
    }

    // positional conv + residual
    int posconv() {
        if (pk) RUN("posconv", launch_posconv_packed(w.xpad, c->pos_w, c->pos_b, w.xf32, w.pre, pk->nclip, pk->slot_max, pk->slot, pk->frames, s, c->fmt));
        else RUN("posconv", launch_posconv(w.xpad, c->pos_w, c->pos_b, w.xf32, w.pre, B, p.Tp, split ? 2 : 1, s, c->fmt, p.lo_xpad, (long)16 * 128 * 64 * 56));
        return 0;
    }

    // LayerNorm of `pre`: the last one writes the hidden states; every other one the next GEMMs' operand h (16-bit, or MXFP8 for
    // SYLBER_FP8: e4m3 + E8M0 block scales into the same buffer) and its row statistics -- no fp32 copy, see EPI_F32_RESLN
    int layernorm(const float* gam, const float* bet, bool last) {
        LnArgs a = {};
        a.in = w.pre; a.in_bf16 = 0; a.ld_in = 768; a.gamma = gam; a.beta = bet; a.M = M; a.D = 768; a.fmt = c->fmt; a.fmt_in = c->fmt;
        if (last) { a.out_f32 = hidden_dev; a.ld_f32 = 768; a.Tp = p.Tp; a.T = p.T; }
        else if (f8) { a.out_fp8 = w8.h; a.ld_fp8 = 768; a.out_scale = w8.hs; a.scale_rows = w8.Mp; a.out_stats = w.stats; }
        else { a.out_bf16 = w.h; a.ld_bf16 = 768; a.out_stats = w.stats; a.out_lo = p.lo_hbf; }
        if (launch_layernorm(a, s)) return 1;
        AUDIT(aud_e && !last && !f8, AUD_LN, w.h, M, 768, 768);
        return 0;
    }

    // a layer tap: frames [0, T) of a 16-bit workspace buffer [B][Tp][W], widened exactly, or of the fp32 pre-LayerNorm sums
    int tap_rows16(const bf16_t* buf, long lo, int W) {
        tapped = true;
        RUN("copy_out", launch_bf16_to_f32_rows(buf, W, hidden_dev, B, p.Tp, p.T, W, s, c->fmt, lo));
        return 0;
    }
    int tap_pre() { tapped = true; return copy_frames_f32(w.pre, hidden_dev, B, p.Tp, p.T, s); }

    // one post-LN encoder layer on 16-bit operands; tk: the layer tap to stop behind (-1: none)
    int layer16(const LayerDev& d, bool last, int tk) {
        // one launch for q, k and v (N = 2304): the q / k thirds leave head-major, the v third transposed (EPI_QK)
        GemmArgs g = linear(w.h, p.lo_hbf, d.wqkv, d.bqkv, 2304, 768);
        g.out0 = w.q; g.out1 = w.k; g.out2 = w.vt; g.Tp = p.Tp; g.Tpv = p.Tpv; g.T = p.T; g.out_lo = p.lo_qk; g.out2_lo = p.lo_vt;
        tune_from_options(c, g);
        RUN("gemm_qkv", launch_gemm_bf16(EPI_QK, g, s));
        AUDIT(aud_e, AUD_Q, w.q, M, 768, 768);
        AUDIT(aud_e, AUD_K, w.k, M, 768, 768);
        AUDIT(aud_e, AUD_V, w.vt, (long)B * 768, p.Tp, p.Tpv);
        if (tk == SYLBER_LTAP_QKV) {
            tapped = true;
            RUN("copy_out", launch_tap_qkv(w.q, w.k, w.vt, hidden_dev, B, p.T, p.Tp, p.Tpv, s, c->fmt, p.lo_qk, p.lo_vt));
            return 0;
        }
        if (pk) RUN("attention", launch_attention_packed(w.q, w.k, w.vt, pk->slot, pk->nclip, pk->total_qb, w.ctx, p.Tp, s, c->fmt));
        else RUN("attention", launch_attention(w.q, w.k, w.vt, w.valid, w.ctx, B, p.T, p.Tp, p.Tpv, c->opt_attn_qw, s, c->fmt, p.lo_qk, p.lo_vt, p.lo_ctx));
        AUDIT(aud_e, AUD_CTX, w.ctx, M, 768, 768);
        if (tk == SYLBER_LTAP_CTX) return tap_rows16(w.ctx, p.lo_ctx, 768);
        GemmArgs o = linear(w.ctx, p.lo_ctx, d.wo, d.bo, 768, 768);
        residual(o, res_g, res_b);
        tune_from_options(c, o);
        // out-projection + LayerNorm 1 as ONE launch on full-row tiles (gemm_rowln.hip) where the batch fills the chip
        o.out1 = w.h; o.ln_stats_out = w.stats; o.ln_gamma_out = d.ln1w; o.ln_beta_out = d.ln1b;
        if (!split && c->opt_fuse_ln > 0 && gemm_rowln_applicable(o)) {      // measured: faster as a pair, slower with two batches in flight
            RUN("gemm_out_ln", launch_gemm_rowln(o, s));
            if (tk == SYLBER_LTAP_ATTN_SUM) return tap_pre();
        } else {
            RUN("gemm_out", launch_gemm_bf16(EPI_F32_RESLN, o, s));
            if (tk == SYLBER_LTAP_ATTN_SUM) return tap_pre();
            RUN("layernorm", layernorm(d.ln1w, d.ln1b, false));
        }
        if (tk == SYLBER_LTAP_LN1) return tap_rows16(w.h, p.lo_hbf, 768);
        GemmArgs f1 = linear(w.h, p.lo_hbf, d.w1, d.b1, 3072, 768);
        f1.act = split ? ACT_GELU_ERF7 : ACT_GELU_FAST; f1.out0 = w.ffn; f1.ld0 = 3072; f1.out_lo = p.lo_ffn;
        tune_from_options(c, f1);
        RUN("gemm_ffn1", launch_gemm_bf16(EPI_BF16, f1, s));
        AUDIT(aud_e, AUD_FFN1, w.ffn, M, 3072, 3072);
        if (tk == SYLBER_LTAP_FFN1) return tap_rows16(w.ffn, p.lo_ffn, 3072);
        GemmArgs f2 = linear(w.ffn, p.lo_ffn, d.w2, d.b2, 768, 3072);
        residual(f2, d.ln1w, d.ln1b);
        tune_from_options(c, f2);
        RUN("gemm_ffn2", launch_gemm_bf16(EPI_F32_RESLN, f2, s));
        if (tk == SYLBER_LTAP_FFN2_SUM) return tap_pre();
        RUN("layernorm", layernorm(d.ln2w, d.ln2b, last));
        return 0;
    }

    // a layer tap of SYLBER_FP8: frames [0, T) of an MXFP8 workspace buffer [B][Tp][W] (K-pair-major scales, pitch w8.Mp) dequantised
    // exactly, as [B][T][2 W]: W values, then W floats holding each element's block exponent s - 127
    int tap_rows8(const uint8_t* buf, const uint8_t* scale, int W) {
        tapped = true;
        RUN("copy_out", launch_mxfp8_to_f32_rows(buf, scale, MXTAP_ROWS, w8.Mp, hidden_dev, 2L * W, 0, W, B, p.Tp, p.T, W, s));
        return 0;
    }

    // one post-LN encoder layer on MXFP8 operands (SYLBER_FP8): every GEMM reads e4m3 + block scales; FFN1 leaves its GELU output as
    // MXFP8 for FFN2; tk: the layer tap to stop behind (-1: none)
    int layer8(const LayerDev& d, bool last, int tk) {
        GemmF8Args g = linear8(w8.h, w8.hs, d.wqkvq, d.wqkvs, d.bqkv, 2304, 768);
        g.g.out0 = w.q; g.g.out1 = w.k; g.g.out2 = w.vt; g.g.Tp = p.Tp; g.g.Tpv = p.Tpv; g.g.T = p.T;
        // the attention core of the mode must not depend on the batch shape (one utterance, same hidden states alone or in a
        // batch): the q / k / v launch always runs on whole 256-row tiles -- M is padded up, the rows beyond the batch read
        // whatever follows the operand (inside the workspace: the buffer holds (M + 128) x 768 x 2 bytes) and are not stored
        GemmF8Args gq = g;
        gq.g.M = (int)w8.Mp; gq.g.M_store = M;
        if (c->opt_attn8 >= 0 && gemm_asm_f8_tile(EPI_QK8, gq) != 0) {     // attention core on MXFP8 operands
            gq.g.out0 = w8.q; gq.g.out1 = w8.k; gq.g.out2 = w8.v; gq.qs = w8.qs; gq.ks = w8.ks; gq.vs = w8.vs;
            RUN("gemm_qkv", launch_gemm_mxfp8(EPI_QK8, gq, s));
            if (tk == SYLBER_LTAP_QKV) {                // q | k | v values [0, 2304), their block exponents [2304, 4608)
                tapped = true;
                RUN("copy_out", launch_mxfp8_to_f32_rows(w8.q, w8.qs, MXTAP_HEADS, 0, hidden_dev, 4608, 0, 2304, B, p.Tp, p.T, 768, s));
                RUN("copy_out", launch_mxfp8_to_f32_rows(w8.k, w8.ks, MXTAP_HEADS, 0, hidden_dev, 4608, 768, 3072, B, p.Tp, p.T, 768, s));
                RUN("copy_out", launch_mxfp8_to_f32_rows(w8.v, w8.vs, MXTAP_VT, p.Tpv, hidden_dev, 4608, 1536, 3840, B, p.Tp, p.T, 768, s));
                return 0;
            }
            RUN("attention", launch_attention_f8(w8.q, w8.qs, w8.k, w8.ks, w8.v, w8.vs, w.valid, w8.ctx, w8.ctxs, w8.Mp, B, p.T, p.Tp, p.Tpv, s));
        } else {
            RUN("gemm_qkv", launch_gemm_mxfp8(EPI_QK, g, s));
            if (tk == SYLBER_LTAP_QKV) {                // the 16-bit buffers of EPI_QK: [B][T][2304] as in layer16
                tapped = true;
                RUN("copy_out", launch_tap_qkv(w.q, w.k, w.vt, hidden_dev, B, p.T, p.Tp, p.Tpv, s, c->fmt, p.lo_qk, p.lo_vt));
                return 0;
            }
            RUN("attention", launch_attention_f8out(w.q, w.k, w.vt, w.valid, w8.ctx, w8.ctxs, w8.Mp, B, p.T, p.Tp, p.Tpv, c->opt_attn_qw, s));
        }
        if (tk == SYLBER_LTAP_CTX) return tap_rows8(w8.ctx, w8.ctxs, 768);
        GemmF8Args o = linear8(w8.ctx, w8.ctxs, d.woq, d.wos, d.bo, 768, 768);
        residual(o.g, res_g, res_b);
        RUN("gemm_out", launch_gemm_mxfp8(EPI_F32_RESLN, o, s));
        if (tk == SYLBER_LTAP_ATTN_SUM) return tap_pre();
        RUN("layernorm", layernorm(d.ln1w, d.ln1b, false));
        if (tk == SYLBER_LTAP_LN1) return tap_rows8(w8.h, w8.hs, 768);
        GemmF8Args f1 = linear8(w8.h, w8.hs, d.w1q, d.w1s, d.b1, 3072, 768);
        f1.g.act = 1; f1.g.out0 = w8.ffn; f1.g.ld0 = 3072; f1.out_scale = w8.ffns; f1.os_rows = w8.Mp;
        RUN("gemm_ffn1", launch_gemm_mxfp8(EPI_MXFP8, f1, s));
        if (tk == SYLBER_LTAP_FFN1) return tap_rows8(w8.ffn, w8.ffns, 3072);
        GemmF8Args f2 = linear8(w8.ffn, w8.ffns, d.w2q, d.w2s, d.b2, 768, 3072);
        residual(f2.g, d.ln1w, d.ln1b);
        RUN("gemm_ffn2", launch_gemm_mxfp8(EPI_F32_RESLN, f2, s));
        if (tk == SYLBER_LTAP_FFN2_SUM) return tap_pre();
        RUN("layernorm", layernorm(d.ln2w, d.ln2b, last));
        return 0;
    }

    int run() {
        if (conv0()) return 1;
        if (c->stop_stage == SYLBER_TAP_CONV0) {        // every row of the 16-bit buffer, rows [L0, R0) included, widened exactly
            RUN("copy_out", launch_bf16_to_f32_rows(w.bufA, 512, hidden_dev, B, p.R[0], p.R[0], 512, s, c->fmt_conv, p.lo_bufA));
            return 0;
        }
        if (conv_stack()) return 1;
        if (tapped) return 0;
        if (c->stop_stage == 1) {
            RUN("copy_out", launch_bf16_to_f32_rows(feats, 512, hidden_dev, B, p.Tp, p.T, 512, s, c->fmt_conv, feats_lo));
            return 0;
        }
        if (projection()) return 1;
        if (c->stop_stage == SYLBER_TAP_PROJ) return copy_frames_f32(w.xf32, hidden_dev, B, p.Tp, p.T, s);
        if (posconv()) return 1;
        if (c->stop_stage == SYLBER_TAP_POSCONV) return copy_frames_f32(w.pre, hidden_dev, B, p.Tp, p.T, s);
        RUN("layernorm", layernorm(c->enc_ln_w, c->enc_ln_b, c->stop_stage == 2));
        if (c->stop_stage == 2) return 0;
        res_g = c->enc_ln_w; res_b = c->enc_ln_b;
        for (int l = 0; l < c->num_layers; ++l) {
            const LayerDev& d = c->L[l];
            const bool last = (l == c->num_layers - 1) || (c->stop_stage == 3 + l);
            const int tk = l == tap.l ? tap.k : -1;         // the layer tap to stop behind (-1: none)
            if (f8 ? layer8(d, last, tk) : layer16(d, last, tk)) return 1;
            if (last || tapped) break;
            res_g = d.ln2w; res_b = d.ln2b;
        }
        return 0;
    }
};

// fp32 parity mode: the same sequence, every tensor fp32 (make_plan_f32); padded batches only, never captured
struct ForwardF32 {
    sylber_ctx* c; const Plan& p; const float* wav_dev; float* hidden_dev; hipStream_t s;
    const Ws<float> w;
    const int B, M;
    const float* feats = nullptr;                       // the conv stack's output [B*Tp][512]
    const LayerTap tap;                                 // a tap inside a layer: layer() sets `tapped` once it has copied it out
    const int ctap;                                     // a tap behind conv layer ctap (0: none)
    bool tapped = false;

    ForwardF32(sylber_ctx* c_, const Plan& p_, const float* wav, float* hidden, hipStream_t s_)
        : c(c_), p(p_), wav_dev(wav), hidden_dev(hidden), s(s_), w(c_->ws, p_), B(p_.B), M(p_.B * p_.Tp), tap(c_->stop_stage),
          ctap(conv_tap_layer(c_->stop_stage)) {}

    int conv0() {
        const int* rows0 = c->opt_per_utt ? w.rows : nullptr;
        RUN("conv0_stats", launch_conv0_stats(wav_dev, B, p.Lmax, p.L[0], w.part, p.nchunk, s, rows0));
        RUN("conv0_finalize", launch_conv0_finalize(w.part, p.nchunk, c->conv0_w, c->gn_w, c->gn_b, B, p.L[0], w.ss, s, rows0));
        RUN("conv0_gn_gelu", launch_conv0_gn_gelu(wav_dev, B, p.Lmax, p.L[0], p.R[0], c->conv0_w, w.ss, w.bufA, 1, s));
        return 0;
    }

    int conv_stack() {
        float* src = w.bufA; float* dst = w.bufB;
        for (int i = 1; i < 7; ++i) {
            GemmArgsF32 a = {};
            a.X = src; a.ldx = (long)CS[i] * 512; a.W = c->conv_w32[i]; a.M = B * p.R[i]; a.N = 512; a.K = CK[i] * 512; a.act = 1;
            a.out0 = dst; a.ld0 = 512; a.tiled = 1;
            RUN("gemm_f32", launch_gemm_f32(a, s));
            if (i == ctap) {
                tapped = true;
                HIP_TRY(hipMemcpyAsync(hidden_dev, dst, (size_t)B * p.R[i] * 512 * 4, hipMemcpyDeviceToDevice, s));
                return 0;
            }
            std::swap(src, dst);
        }
        feats = src;
        return 0;
    }

    // a Linear of the encoder: X [M][K], W [N][K], out [M][N]
    GemmArgsF32 linear(const float* X, const float* W, const float* bias, float* out, int N, int K) const {
        GemmArgsF32 g = {};
        g.X = X; g.ldx = K; g.W = W; g.M = M; g.N = N; g.K = K; g.bias = bias; g.out0 = out; g.ld0 = N; g.tiled = 1;
        return g;
    }

    int projection() {
        LnArgs a = {};
        a.in = feats; a.in_bf16 = 0; a.ld_in = 512; a.gamma = c->fp_ln_w; a.beta = c->fp_ln_b; a.out_f32 = w.ln512; a.ld_f32 = 512;
        a.M = M; a.D = 512;
        RUN("ln512", launch_layernorm(a, s));
        GemmArgsF32 g = linear(w.ln512, c->fp_w32, c->fp_b, w.xf32, 768, 512);
        g.Tp = p.Tp; g.T = p.T; g.valid = w.valid; g.xpad = w.xpad; g.xpad_rows = p.Tp + 128;
        RUN("gemm_f32", launch_gemm_f32(g, s));
        return 0;
    }

    int layernorm(const float* gam, const float* bet, bool last) {
        LnArgs a = {};
        a.in = w.pre; a.in_bf16 = 0; a.ld_in = 768; a.gamma = gam; a.beta = bet; a.M = M; a.D = 768;
        if (last) { a.out_f32 = hidden_dev; a.ld_f32 = 768; a.Tp = p.Tp; a.T = p.T; }
        else { a.out_f32 = w.h; a.ld_f32 = 768; }
        return launch_layernorm(a, s);
    }

    // a layer tap: frames [0, T) of an fp32 workspace tensor [B][Tp][W] (q | k | v are stored in natural order, q unscaled)
    int tap_rows(const float* buf, int W) { tapped = true; return copy_frames_f32(buf, hidden_dev, B, p.Tp, p.T, s, W); }

    int layer(int l, bool last) {
        const LayerDev& d = c->L[l];
        const int tk = l == tap.l ? tap.k : -1;         // the layer tap to stop behind (-1: none)
        RUN("gemm_f32", launch_gemm_f32(linear(w.h, c->L32[l].wqkv, d.bqkv, w.q, 2304, 768), s));
        if (tk == SYLBER_LTAP_QKV) return tap_rows(w.q, 2304);
        RUN("attention_f32", launch_attention_f32(w.q, w.q + 768, w.q + 1536, w.valid, w.ctx, B, p.T, p.Tp, s));
        if (tk == SYLBER_LTAP_CTX) return tap_rows(w.ctx, 768);
        GemmArgsF32 o = linear(w.ctx, c->L32[l].wo, d.bo, w.pre, 768, 768);
        o.res = w.h; o.ldres = 768;
        RUN("gemm_f32", launch_gemm_f32(o, s));
        if (tk == SYLBER_LTAP_ATTN_SUM) return tap_rows(w.pre, 768);
        RUN("layernorm", layernorm(d.ln1w, d.ln1b, false));
        if (tk == SYLBER_LTAP_LN1) return tap_rows(w.h, 768);
        GemmArgsF32 f1 = linear(w.h, c->L32[l].w1, d.b1, w.ffn, 3072, 768);
        f1.act = 1;
        RUN("gemm_f32", launch_gemm_f32(f1, s));
        if (tk == SYLBER_LTAP_FFN1) return tap_rows(w.ffn, 3072);
        GemmArgsF32 f2 = linear(w.ffn, c->L32[l].w2, d.b2, w.pre, 768, 3072);
        f2.res = w.h; f2.ldres = 768;
        RUN("gemm_f32", launch_gemm_f32(f2, s));
        if (tk == SYLBER_LTAP_FFN2_SUM) return tap_rows(w.pre, 768);
        RUN("layernorm", layernorm(d.ln2w, d.ln2b, last));
        return 0;
    }

    int run() {
        if (conv0()) return 1;
        if (c->stop_stage == SYLBER_TAP_CONV0) {
            HIP_TRY(hipMemcpyAsync(hidden_dev, w.bufA, (size_t)B * p.R[0] * 512 * 4, hipMemcpyDeviceToDevice, s));
            return 0;
        }
        if (conv_stack()) return 1;
        if (tapped) return 0;
        if (c->stop_stage == 1) {
            for (int b = 0; b < B; ++b)
                HIP_TRY(hipMemcpyAsync(hidden_dev + (size_t)b * p.T * 512, feats + (size_t)b * p.Tp * 512, (size_t)p.T * 512 * 4,
                                       hipMemcpyDeviceToDevice, s));
            return 0;
        }
        if (projection()) return 1;
        if (c->stop_stage == SYLBER_TAP_PROJ) return copy_frames_f32(w.xf32, hidden_dev, B, p.Tp, p.T, s);
        RUN("posconv_f32", launch_posconv_f32(w.xpad, c->pos_w32, c->pos_b, w.xf32, w.pre, B, p.Tp, s));
        if (c->stop_stage == SYLBER_TAP_POSCONV) return copy_frames_f32(w.pre, hidden_dev, B, p.Tp, p.T, s);
        RUN("layernorm", layernorm(c->enc_ln_w, c->enc_ln_b, c->stop_stage == 2));
        if (c->stop_stage == 2) return 0;
        for (int l = 0; l < c->num_layers; ++l) {
            const bool last = (l == c->num_layers - 1) || (c->stop_stage == 3 + l);
            if (layer(l, last)) return 1;
            if (last || tapped) break;
        }
        return 0;
    }
};

// Graph mode (sylber_set_graph_mode): the first call with a new (B, Lmax, stop stage, input, output) runs eagerly (which also sets the
// kernels' attributes), the second captures the launch sequence on the caller's stream into a hipGraph, later calls replay it.  At
// most 8 graphs per handle, least recently used out first.
static int forward_graph(sylber_ctx* c, const Plan& p, const float* wav_dev, float* hidden_dev, hipStream_t s) {
    GraphEntry* e = nullptr;
    for (auto& g : c->graphs)
        if (g.B == p.B && g.Lmax == p.Lmax && g.stop_stage == c->stop_stage && g.in == wav_dev && g.out == hidden_dev) e = &g;
    if (e && e->exec) { e->stamp = ++c->graph_clock; HIP_TRY(hipGraphLaunch(e->exec, s)); return 0; }
    if (!e) {
        if (c->graphs.size() >= 8) {
            size_t v = 0;
            for (size_t i = 1; i < c->graphs.size(); ++i) if (c->graphs[i].stamp < c->graphs[v].stamp) v = i;
            if (c->graphs[v].exec) hipGraphExecDestroy(c->graphs[v].exec);
            c->graphs.erase(c->graphs.begin() + v);
        }
        c->graphs.push_back({p.B, p.Lmax, c->stop_stage, wav_dev, hidden_dev, nullptr, ++c->graph_clock});
        return Forward(c, p, wav_dev, hidden_dev, s, nullptr).run();
    }
    HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = Forward(c, p, wav_dev, hidden_dev, s, nullptr).run();
    hipGraph_t graph = nullptr;
    const hipError_t ec = hipStreamEndCapture(s, &graph);
    if (rc != 0 || ec != hipSuccess || !graph) {
        if (graph) hipGraphDestroy(graph);
        if (rc == 0) syl_set_error("sylber_forward", "hipGraph capture failed");
        return 1;
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (ei != hipSuccess) { syl_set_error("sylber_forward", "hipGraphInstantiate failed"); return 1; }
    e->exec = exec; e->stamp = ++c->graph_clock;
    HIP_TRY(hipGraphLaunch(exec, s));
    return 0;
}

extern "C" int sylber_forward(sylber_t c, const float* wav_dev, const int32_t* lengths_host, int32_t B, int32_t Lmax,
                              float* hidden_dev, void* stream) {
    if (!c || !wav_dev || !hidden_dev) { syl_set_error("sylber_forward", "null argument"); return 1; }
    if (B < 1 || Lmax < 400) { syl_set_error("sylber_forward", "need B >= 1 and at least 400 samples (one frame)"); return 1; }
    // valid frames per utterance (TP:664-689): conv-length formula of the number of valid samples; and its conv0 frames, (n_b - 10) / 5 + 1,
    // for the GroupNorm statistics of SYLBER_OPT_PER_UTTERANCE
    std::vector<int32_t> valid(B), rows0(B);
    for (int b = 0; b < B; ++b) {
        const int len = lengths_host ? lengths_host[b] : Lmax;
        if (len > Lmax || len < 400) { syl_set_error("sylber_forward", "lengths must be in [400, Lmax]"); return 1; }
        valid[b] = sylber_num_frames(len);
        rows0[b] = (len - CK[0]) / CS[0] + 1;
    }
    hipStream_t s = (hipStream_t)stream;
    GUARD_DEVICE(c->device);
    const bool f32 = c->precision == SYLBER_FP32;
    const Plan p = f32 ? make_plan_f32(B, Lmax) : make_plan(B, Lmax, c->precision == SYLBER_SPLIT16 ? 2 : 1);
    if (begin_call(c, p, {{p.o_valid, valid.data(), B}, {p.o_rows, c->opt_per_utt ? rows0.data() : nullptr, B}}, s)) return 1;
    c->dbg_ss = (const float*)(c->ws + p.o_ss); c->dbg_ss_B = B;      // sylber_debug_conv0_scale_shift
    if (f32) return ForwardF32(c, p, wav_dev, hidden_dev, s).run();
    // a tap (negative stop stage) copies workspace tensors out: always eager, never captured
    if (!c->graph_mode || c->profiling || c->opt_audit16 || s == nullptr || c->stop_stage < 0) return Forward(c, p, wav_dev, hidden_dev, s, nullptr).run();
    return forward_graph(c, p, wav_dev, hidden_dev, s);
}

// Packed batch: B clips of samples_host[b] samples, clip b at sample SYL_SLOT_SAMPLES x offsets[b] of wav_dev (sylber_packed_layout), zero
// to the end of its slot; the whole batch runs as ONE utterance of offsets[B] frames, and only the GroupNorm statistics, conv0, the
// zeroing of the frames behind each clip's end, the pos-conv and the attention read the slot tables.  hidden_dev [offsets[B]][768].
extern "C" int sylber_forward_packed(sylber_t c, const float* wav_dev, const int32_t* samples_host, int32_t B, float* hidden_dev, void* stream) {
    if (!c || !wav_dev || !samples_host || !hidden_dev) { syl_set_error("sylber_forward_packed", "null argument"); return 1; }
    if (c->precision != SYLBER_BF16 && c->precision != SYLBER_FP16) {
        syl_set_error("sylber_forward_packed", "packed batches run in the bf16 and fp16 precisions only"); return 1;
    }
    if (c->graph_mode) { syl_set_error("sylber_forward_packed", "not available in graph mode (sylber_set_graph_mode)"); return 1; }
    if (c->stop_stage != 0 || c->opt_conv0_valu != 0 || c->opt_attn_qw != 0) {
        syl_set_error("sylber_forward_packed", "not available with a stop stage, SYLBER_OPT_CONV0_VALU or SYLBER_OPT_ATTN_QUERIES_PER_WAVE"); return 1;
    }
    std::vector<int32_t> off(B > 0 ? B + 1 : 1), fr(B > 0 ? B : 1);
    if (sylber_packed_layout(samples_host, B, off.data(), fr.data())) return 1;
    const int Ptot = off[B];
    std::vector<int32_t> tab(3 * (size_t)B + 2), rows0(B);
    int slot_max = 0, tail_max = 0, nmax = 0;
    tab[2 * B + 1] = 0;
    for (int b = 0; b < B; ++b) {
        const int sl = off[b + 1] - off[b];
        slot_max = sl > slot_max ? sl : slot_max;
        tail_max = sl - fr[b] > tail_max ? sl - fr[b] : tail_max;
        rows0[b] = (samples_host[b] - CK[0]) / CS[0] + 1;
        nmax = samples_host[b] > nmax ? samples_host[b] : nmax;
        tab[B + 1 + b] = fr[b];
        tab[2 * B + 2 + b] = tab[2 * B + 1 + b] + (fr[b] + 127) / 128;
    }
    for (int b = 0; b <= B; ++b) tab[b] = off[b];
    hipStream_t s = (hipStream_t)stream;
    GUARD_DEVICE(c->device);
    const Plan p = make_plan_packed(B, Ptot, nmax);
    const int32_t one = Ptot;                           // the projection's valid[0]: no frame of the pseudo-utterance is padding to it
    if (begin_call(c, p, {{p.o_pk, tab.data(), 3 * B + 2}, {p.o_rows, rows0.data(), B}, {p.o_valid, &one, 1}}, s)) return 1;
    const int* pkd = (const int*)(c->ws + p.o_pk);
    c->dbg_ss = (const float*)(c->ws + p.o_ss); c->dbg_ss_B = B;
    const PackedCall pc = {B, SYL_SLOT_SAMPLES * Ptot, slot_max, tail_max, tab[3 * B + 1], pkd, pkd + B + 1, pkd + 2 * B + 1, (const int*)(c->ws + p.o_rows)};
    return Forward(c, p, wav_dev, hidden_dev, s, &pc).run();
}

// each clip's own rows of a packed forward's hidden states, back to back: one device-to-host copy instead of one per clip.  Up to 64
// clips per launch, their source row, destination row and frame count as kernel arguments; grid (row blocks, clips), one wave per row
struct GatherPack { int src[64], dst[64], n[64]; };
__global__ __launch_bounds__(256) void packed_gather_kernel(const float* __restrict__ in, float* __restrict__ out, GatherPack g) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < g.n[b]; r += gridDim.x * 4) {
        const float4* s = (const float4*)(in + ((size_t)g.src[b] + r) * SYL_HIDDEN);
        float4* d = (float4*)(out + ((size_t)g.dst[b] + r) * SYL_HIDDEN);
#pragma unroll
        for (int i = 0; i < 3; ++i) d[lane + 64 * i] = s[lane + 64 * i];
    }
}
extern "C" int sylber_packed_gather(const float* hidden_dev, const int32_t* samples_host, int32_t B, float* out_dev, void* stream) {
    if (!hidden_dev || !samples_host || !out_dev) { syl_set_error("sylber_packed_gather", "null argument"); return 1; }
    std::vector<int32_t> off(B > 0 ? B + 1 : 1), fr(B > 0 ? B : 1);
    if (sylber_packed_layout(samples_host, B, off.data(), fr.data())) return 1;
    int dst = 0;
    for (int b0 = 0; b0 < B; b0 += 64) {
        GatherPack g;
        const int k = B - b0 < 64 ? B - b0 : 64;
        int nmax = 1;
        for (int i = 0; i < k; ++i) {
            g.src[i] = off[b0 + i]; g.dst[i] = dst; g.n[i] = fr[b0 + i];
            dst += fr[b0 + i];
            nmax = fr[b0 + i] > nmax ? fr[b0 + i] : nmax;
        }
        const int gx = (nmax + 15) / 16;               // ~4 rows per wave
        hipLaunchKernelGGL(packed_gather_kernel, dim3(gx, k), dim3(256), 0, (hipStream_t)stream, hidden_dev, out_dev, g);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

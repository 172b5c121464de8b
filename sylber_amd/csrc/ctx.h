// The handle (sylber_ctx) and the helpers every translation unit that takes one shares: api.hip (handle, options, profiling, segment
// entry points), forward.hip (workspace plans and the encoder forward) and ops.hip (op-level and debug entry points).
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/sylber_hip.h"
#include "../../include/sylber_hip_dev.h"
#include "kernels.h"

// every entry point runs on the handle's GPU and leaves the caller's current device as it found it (a process may
// hold handles on several GPUs; sylber_destroy runs from garbage collectors at arbitrary times)
struct DeviceGuard {
    int prev = -1; bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { int cur = -1; if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev); }
};
#define GUARD_DEVICE(dev)                                                                             \
    DeviceGuard _dg(dev);                                                                             \
    if (!_dg.ok) { syl_set_error("hipSetDevice", "cannot select the handle's device"); return 1; }

// kernel widths and strides of the seven conv layers
static const int CK[7] = {10, 3, 3, 3, 3, 2, 2};
static const int CS[7] = {5, 2, 2, 2, 2, 2, 2};

struct LayerDev {
    bf16_t *wqkv, *wo, *w1, *w2;
    uint8_t *w1q = nullptr, *w1s = nullptr, *w2q = nullptr, *w2s = nullptr;   // SYLBER_FP8: MXFP8 FFN weights + E8M0 scales
    uint8_t *wqkvq = nullptr, *wqkvs = nullptr;                                // and the fused q/k/v projection
    uint8_t *woq = nullptr, *wos = nullptr;                                    // and the attention out-projection
    float *bqkv, *bo, *b1, *b2, *ln1w, *ln1b, *ln2w, *ln2b;
};

struct ProfEntry { std::string name; hipEvent_t e0, e1; };
struct GraphEntry { int B, Lmax, stop_stage; const void* in; void* out; hipGraphExec_t exec; unsigned long long stamp; };

// stages of the fp16 headroom audit (forward.hip audit16)
enum { AUD_CONV0 = 0, AUD_CONV6 = 6, AUD_LN512 = 7, AUD_XPAD = 8, AUD_LN = 9, AUD_Q = 10, AUD_K = 11, AUD_V = 12, AUD_CTX = 13, AUD_FFN1 = 14, AUDIT_STAGES = 15 };

struct sylber_ctx {
    int device = 0, precision = 0, num_layers = 9;
    int fmt = FMT_BF16;           // 16-bit operand format of the MFMA path (encoder)
    int fmt_conv = FMT_BF16;      // ... of the conv stack (differs from fmt only for SYLBER_MIXED16)
    // weights
    char* wbase = nullptr; size_t wbytes = 0;
    char* f8base = nullptr; size_t f8bytes = 0;
    float *conv0_w, *gn_w, *gn_b, *fp_ln_w, *fp_ln_b, *fp_b, *pos_b, *enc_ln_w, *enc_ln_b;
    bf16_t* conv_w[7];
    bf16_t *fp_w, *pos_w;
    LayerDev L[SYLBER_MAX_LAYERS];
    // fp32 parity mode: the same tensors kept in fp32
    float* conv_w32[7]; float *fp_w32, *pos_w32;
    struct { float *wqkv, *wo, *w1, *w2; } L32[SYLBER_MAX_LAYERS];
    // workspace
    char* ws = nullptr; size_t ws_bytes = 0;
    int ws_B = 0, ws_Lmax = 0;
    float* seg_scratch = nullptr; size_t seg_scratch_floats = 0;
    int stop_stage = 0;
    const float* dbg_ss = nullptr; int dbg_ss_B = 0;               // conv0's GroupNorm scale / shift table of the last forward (sylber_debug_conv0_scale_shift)
    int opt_gemm_cfg = 0, opt_attn_qw = 0, opt_gemm_persist = 0;   // sylber_set_option (0 = automatic)
    int opt_fuse_ln = 0;                                           // out-projection + LayerNorm in one launch: 0 auto, 1 always, -1 never
    int opt_conv0_valu = 0;                                        // 1: conv0 of the 16-bit modes on the VALU kernel (A/B switch)
    // fp16 headroom audit (SYLBER_OPT_FP16_AUDIT): per stage, how many 16-bit activations sit AT the saturation value and the largest magnitude
    int opt_audit16 = 0;
    unsigned* audit_dev = nullptr;                                 // [AUDIT_STAGES][2]: saturated count, max |x| as half bits
    int opt_segment = 0;                                           // boundary detection: 0 wide (all CUs), -1 one workgroup per utterance
    int opt_gemm_model = 0;                                        // 5: round-5 tile cost model (A/B switch)
    int opt_gemm_mfma16 = 0;                                       // -1: the 16-bit-output GEMMs on the 32x32x16 kernels (A/B switch; GemmArgs::tune_mfma16)
    int opt_gemm_h192 = 0;                                         // -1: no 192-row tiles in the cost model (A/B switch)
    int opt_gemm_tail = 0;                                         // row split of multi-round GEMM launches: 0 auto, -1 never, k + 1 = tail tile id k
    int opt_attn8 = 0;                                             // SYLBER_FP8: attention core on MXFP8 operands (0 / 1 on, -1 off)
    int opt_resln_pre = 0;                                         // residual prefetch of the out-proj / FFN2 K loops: 0 default, -1 off, 1..3 columns
    int opt_per_utt = 0;                                           // 1: conv0 GroupNorm statistics over each utterance's own frames (batch-invariant mode)
    bool graph_mode = false;
    std::vector<GraphEntry> graphs; unsigned long long graph_clock = 0;
    // profiling
    int profiling = 0;
    std::vector<ProfEntry> prof;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::string> prof_names; std::vector<float> prof_ms;
};

// destroys every captured graph of the handle (api.hip): they hold workspace addresses and the options' launch choices
void graphs_clear(sylber_ctx* c);

// one named entry of sylber_get_profile per launch (api.hip retires the events); nothing is recorded unless profiling is on
struct ProfScope {
    sylber_ctx* c; hipStream_t s; bool on;
    ProfScope(sylber_ctx* c_, hipStream_t s_, const char* name) : c(c_), s(s_), on(c_->profiling != 0) {
        if (!on) return;
        ProfEntry e; e.name = name;
        auto get = [&]() { hipEvent_t ev; if (c->ev_pool.empty()) { hipEventCreate(&ev); } else { ev = c->ev_pool.back(); c->ev_pool.pop_back(); } return ev; };
        e.e0 = get(); e.e1 = get();
        hipEventRecord(e.e0, s);
        c->prof.push_back(e);
    }
    ~ProfScope() { if (on) hipEventRecord(c->prof.back().e1, s); }
};
// (needs `c` and `s` in scope)
#define RUN(name, call)                         \
    do {                                        \
        ProfScope _ps(c, s, name);              \
        if ((call) != 0) return 1;              \
    } while (0)

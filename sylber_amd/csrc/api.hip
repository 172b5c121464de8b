// C-ABI of libsylber_hip.so (see include/sylber_hip.h): the handle (weight packing, options, profiling, graph mode) and the
// segment entry points.  The encoder forward is forward.hip, the op-level and debug entry points are ops.hip.
//   sylber/model/sylber.py:126  get_segment(...)            sylber.py:133  segment mean-pool
#include "ctx.h"

static thread_local char g_err[512] = "";
void syl_set_error(const char* what, const char* detail) { snprintf(g_err, sizeof(g_err), "%s: %s", what, detail); }
extern "C" const char* sylber_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------
struct Packer {
    std::vector<char> host;
    size_t add(size_t bytes) { size_t off = (host.size() + 255) & ~(size_t)255; host.resize(off + bytes); return off; }
    size_t add_f32(const float* src, size_t n) { size_t o = add(n * 4); memcpy(host.data() + o, src, n * 4); return o; }
    int fmt = FMT_BF16;           // 16-bit format of the MFMA operands (FMT_F16 for SYLBER_FP16)
    size_t add_bf16(const float* src, size_t n) {
        if (fmt == FMT_SPLIT) {
            // two half planes: hi = half(w) at [0, n), lo = half(w - hi) at [n, 2n)
            size_t o = add(n * 4);
            bf16_t* d = (bf16_t*)(host.data() + o);
            for (size_t i = 0; i < n; ++i) { d[i] = f2h_host(src[i]); d[n + i] = f2h_host(src[i] - h2f_host(d[i])); }
            return o;
        }
        size_t o = add(n * 2);
        bf16_t* d = (bf16_t*)(host.data() + o);
        if (fmt == FMT_F16) for (size_t i = 0; i < n; ++i) d[i] = f2h_host(src[i]);
        else for (size_t i = 0; i < n; ++i) d[i] = f2bf(src[i]);
        return o;
    }
};

extern "C" int sylber_create(const SylberWeights* w, int device, int precision, sylber_t* out) {
    if (!w || !out) { syl_set_error("sylber_create", "null argument"); return 1; }
    if (w->num_layers < 1 || w->num_layers > SYLBER_MAX_LAYERS) { syl_set_error("sylber_create", "num_layers out of range"); return 1; }
    if (precision != SYLBER_BF16 && precision != SYLBER_FP32 && precision != SYLBER_FP8 && precision != SYLBER_FP16 && precision != SYLBER_MIXED16 && precision != SYLBER_SPLIT16) { syl_set_error("sylber_create", "unknown precision"); return 1; }
    const bool f32 = precision == SYLBER_FP32;
    GUARD_DEVICE(device);
    sylber_ctx* c = new sylber_ctx();
    c->device = device; c->precision = precision; c->num_layers = w->num_layers;
    c->fmt = precision == SYLBER_FP16 ? FMT_F16 : (precision == SYLBER_SPLIT16 ? FMT_SPLIT : FMT_BF16);
    c->fmt_conv = (precision == SYLBER_FP16 || precision == SYLBER_MIXED16) ? FMT_F16 : (precision == SYLBER_SPLIT16 ? FMT_SPLIT : FMT_BF16);
    Packer P;
    P.fmt = c->fmt_conv;                                 // conv weights first
    size_t o_conv0 = P.add_f32(w->conv_w[0], 512 * 10);
    size_t o_gnw = P.add_f32(w->gn_w, 512), o_gnb = P.add_f32(w->gn_b, 512);
    size_t o_conv[7] = {0};
    for (int i = 1; i < 7; ++i) {
        // [o][c][j] -> [o][j*512 + c]: one output position's receptive field is then ONE contiguous
        // run of taps*512 channels-last activations (implicit GEMM with ldx = stride*512)
        // The 3-tap layers of the 16-bit modes are packed in the chunk-major K order every kernel walks them in (GemmArgs::kpat,
        // common.h tap3_offset): position o of a weight row holds the input element whose operand-row offset is tap3_offset(o)
        const int k = CK[i];
        const bool chunk_major = k == 3 && !f32 && c->fmt_conv != FMT_SPLIT;
        std::vector<float> tmp((size_t)512 * k * 512);
        for (int o = 0; o < 512; ++o)
            for (int cc = 0; cc < 512; ++cc)
                for (int j = 0; j < k; ++j) tmp[((size_t)o * k + j) * 512 + cc] = w->conv_w[i][((size_t)o * 512 + cc) * k + j];
        if (chunk_major) {
            std::vector<float> t2(tmp.size());
            for (int o = 0; o < 512; ++o)
                for (int pos = 0; pos < 1536; ++pos)
                    t2[(size_t)o * 1536 + pos] = tmp[(size_t)o * 1536 + tap3_offset(pos * 2) / 2];
            tmp.swap(t2);
        }
        o_conv[i] = f32 ? P.add_f32(tmp.data(), tmp.size()) : P.add_bf16(tmp.data(), tmp.size());
    }
    P.fmt = c->fmt;                                      // everything after the conv stack
    size_t o_fplw = P.add_f32(w->fp_ln_w, 512), o_fplb = P.add_f32(w->fp_ln_b, 512);
    size_t o_fpw = f32 ? P.add_f32(w->fp_w, 768 * 512) : P.add_bf16(w->fp_w, 768 * 512), o_fpb = P.add_f32(w->fp_b, 768);
    size_t o_posw;
    {
        // [768 = g*48+n][48 c][128 tap] -> [g][tap][64 n][56 c] (zero padded), 112-byte rows
        std::vector<float> tmp((size_t)16 * 128 * 64 * 56, 0.f);
        for (int g = 0; g < 16; ++g)
            for (int n = 0; n < 48; ++n)
                for (int cc = 0; cc < 48; ++cc)
                    for (int t = 0; t < 128; ++t)
                        tmp[(((size_t)g * 128 + t) * 64 + n) * 56 + cc] = w->pos_w[(((size_t)g * 48 + n) * 48 + cc) * 128 + t];
        if (!f32) o_posw = P.add_bf16(tmp.data(), tmp.size());
        else {
            // fp32 parity kernel: [g][tap][64 n][52 c] fp32, zero padded (208-byte rows, see fp32_path.hip)
            std::vector<float> t32((size_t)16 * 128 * 64 * 52, 0.f);
            for (int g = 0; g < 16; ++g)
                for (int n = 0; n < 48; ++n)
                    for (int cc = 0; cc < 48; ++cc)
                        for (int t = 0; t < 128; ++t)
                            t32[(((size_t)g * 128 + t) * 64 + n) * 52 + cc] = w->pos_w[(((size_t)g * 48 + n) * 48 + cc) * 128 + t];
            o_posw = P.add_f32(t32.data(), t32.size());
        }
    }
    size_t o_posb = P.add_f32(w->pos_b, 768);
    size_t o_elw = P.add_f32(w->enc_ln_w, 768), o_elb = P.add_f32(w->enc_ln_b, 768);
    struct LOff { size_t wqkv, bqkv, wo, bo, l1w, l1b, w1, b1, w2, b2, l2w, l2b; } lo[SYLBER_MAX_LAYERS];
    for (int l = 0; l < w->num_layers; ++l) {
        const SylberLayerWeights& lw = w->layers[l];
        std::vector<float> qkv((size_t)2304 * 768), bq(2304);
        memcpy(qkv.data(), lw.q_w, 768 * 768 * 4);
        memcpy(qkv.data() + 768 * 768, lw.k_w, 768 * 768 * 4);
        memcpy(qkv.data() + 2 * 768 * 768, lw.v_w, 768 * 768 * 4);
        memcpy(bq.data(), lw.q_b, 768 * 4); memcpy(bq.data() + 768, lw.k_b, 768 * 4); memcpy(bq.data() + 1536, lw.v_b, 768 * 4);
        lo[l].wqkv = f32 ? P.add_f32(qkv.data(), qkv.size()) : P.add_bf16(qkv.data(), qkv.size()); lo[l].bqkv = P.add_f32(bq.data(), 2304);
        lo[l].wo = f32 ? P.add_f32(lw.o_w, 768 * 768) : P.add_bf16(lw.o_w, 768 * 768); lo[l].bo = P.add_f32(lw.o_b, 768);
        lo[l].l1w = P.add_f32(lw.ln1_w, 768); lo[l].l1b = P.add_f32(lw.ln1_b, 768);
        lo[l].w1 = f32 ? P.add_f32(lw.ff1_w, (size_t)3072 * 768) : P.add_bf16(lw.ff1_w, (size_t)3072 * 768); lo[l].b1 = P.add_f32(lw.ff1_b, 3072);
        lo[l].w2 = f32 ? P.add_f32(lw.ff2_w, (size_t)768 * 3072) : P.add_bf16(lw.ff2_w, (size_t)768 * 3072); lo[l].b2 = P.add_f32(lw.ff2_b, 768);
        lo[l].l2w = P.add_f32(lw.ln2_w, 768); lo[l].l2b = P.add_f32(lw.ln2_b, 768);
    }
    c->wbytes = P.host.size();
    if (hipMalloc((void**)&c->wbase, c->wbytes) != hipSuccess) { delete c; syl_set_error("sylber_create", "hipMalloc(weights) failed"); return 1; }
    if (hipMemcpy(c->wbase, P.host.data(), c->wbytes, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(c->wbase); delete c; syl_set_error("sylber_create", "weight upload failed"); return 1;
    }
    char* b = c->wbase;
    c->conv0_w = (float*)(b + o_conv0); c->gn_w = (float*)(b + o_gnw); c->gn_b = (float*)(b + o_gnb);
    c->conv_w[0] = nullptr;
    for (int i = 1; i < 7; ++i) { c->conv_w[i] = (bf16_t*)(b + o_conv[i]); c->conv_w32[i] = (float*)(b + o_conv[i]); }
    c->fp_w32 = (float*)(b + o_fpw); c->pos_w32 = (float*)(b + o_posw);
    c->fp_ln_w = (float*)(b + o_fplw); c->fp_ln_b = (float*)(b + o_fplb);
    c->fp_w = (bf16_t*)(b + o_fpw); c->fp_b = (float*)(b + o_fpb);
    c->pos_w = (bf16_t*)(b + o_posw); c->pos_b = (float*)(b + o_posb);
    c->enc_ln_w = (float*)(b + o_elw); c->enc_ln_b = (float*)(b + o_elb);
    for (int l = 0; l < w->num_layers; ++l) {
        LayerDev& d = c->L[l];
        d.wqkv = (bf16_t*)(b + lo[l].wqkv); d.bqkv = (float*)(b + lo[l].bqkv);
        d.wo = (bf16_t*)(b + lo[l].wo); d.bo = (float*)(b + lo[l].bo);
        d.ln1w = (float*)(b + lo[l].l1w); d.ln1b = (float*)(b + lo[l].l1b);
        d.w1 = (bf16_t*)(b + lo[l].w1); d.b1 = (float*)(b + lo[l].b1);
        d.w2 = (bf16_t*)(b + lo[l].w2); d.b2 = (float*)(b + lo[l].b2);
        d.ln2w = (float*)(b + lo[l].l2w); d.ln2b = (float*)(b + lo[l].l2b);
        c->L32[l].wqkv = (float*)(b + lo[l].wqkv); c->L32[l].wo = (float*)(b + lo[l].wo);
        c->L32[l].w1 = (float*)(b + lo[l].w1); c->L32[l].w2 = (float*)(b + lo[l].w2);
    }
    if (precision == SYLBER_FP8) {
        // FFN weights once more as MXFP8 (e4m3 + one E8M0 scale per 32 input features), quantised on the device
        // from the fp32 originals with the same kernel the activations' op-level entry point uses
        const size_t per_layer = (size_t)3072 * 768 + (size_t)3072 * 24 + (size_t)768 * 3072 + (size_t)768 * 96 +
                                 (size_t)2304 * 768 + (size_t)2304 * 24 + (size_t)768 * 768 + (size_t)768 * 24;
        c->f8bytes = per_layer * w->num_layers;
        float* tmp = nullptr;
        if (hipMalloc((void**)&c->f8base, c->f8bytes) != hipSuccess || hipMalloc((void**)&tmp, (size_t)3072 * 768 * 4) != hipSuccess) {
            if (c->f8base) hipFree(c->f8base);
            hipFree(c->wbase); delete c; syl_set_error("sylber_create", "hipMalloc(fp8 weights) failed"); return 1;
        }
        int bad = 0;
        for (int l = 0; l < w->num_layers && !bad; ++l) {
            LayerDev& d = c->L[l];
            uint8_t* q = (uint8_t*)c->f8base + per_layer * l;
            d.w1q = q; d.w1s = d.w1q + (size_t)3072 * 768; d.w2q = d.w1s + (size_t)3072 * 24; d.w2s = d.w2q + (size_t)768 * 3072;
            d.wqkvq = d.w2s + (size_t)768 * 96; d.wqkvs = d.wqkvq + (size_t)2304 * 768;
            d.woq = d.wqkvs + (size_t)2304 * 24; d.wos = d.woq + (size_t)768 * 768;
            bad |= hipMemcpy(tmp, w->layers[l].o_w, (size_t)768 * 768 * 4, hipMemcpyHostToDevice) != hipSuccess;
            bad |= launch_mx_quant_rows(tmp, 768, d.woq, 768, d.wos, 768, 768, 768, nullptr);
            bad |= hipDeviceSynchronize() != hipSuccess;
            {
                const SylberLayerWeights& lw = w->layers[l];
                bad |= hipMemcpy(tmp, lw.q_w, (size_t)768 * 768 * 4, hipMemcpyHostToDevice) != hipSuccess;
                bad |= hipMemcpy(tmp + (size_t)768 * 768, lw.k_w, (size_t)768 * 768 * 4, hipMemcpyHostToDevice) != hipSuccess;
                bad |= hipMemcpy(tmp + (size_t)2 * 768 * 768, lw.v_w, (size_t)768 * 768 * 4, hipMemcpyHostToDevice) != hipSuccess;
                bad |= launch_mx_quant_rows(tmp, 768, d.wqkvq, 768, d.wqkvs, 2304, 2304, 768, nullptr);
                bad |= hipDeviceSynchronize() != hipSuccess;
            }
            bad |= hipMemcpy(tmp, w->layers[l].ff1_w, (size_t)3072 * 768 * 4, hipMemcpyHostToDevice) != hipSuccess;
            bad |= launch_mx_quant_rows(tmp, 768, d.w1q, 768, d.w1s, 3072, 3072, 768, nullptr);
            bad |= hipDeviceSynchronize() != hipSuccess;
            bad |= hipMemcpy(tmp, w->layers[l].ff2_w, (size_t)768 * 3072 * 4, hipMemcpyHostToDevice) != hipSuccess;
            bad |= launch_mx_quant_rows(tmp, 3072, d.w2q, 3072, d.w2s, 768, 768, 3072, nullptr);
            bad |= hipDeviceSynchronize() != hipSuccess;
        }
        hipFree(tmp);
        if (bad) { hipFree(c->f8base); hipFree(c->wbase); delete c; syl_set_error("sylber_create", "fp8 weight quantisation failed"); return 1; }
    }
    *out = c;
    return 0;
}

extern "C" void sylber_destroy(sylber_t c) {
    if (!c) return;
    DeviceGuard dg(c->device);
    if (c->wbase) hipFree(c->wbase);
    if (c->f8base) hipFree(c->f8base);
    if (c->ws) hipFree(c->ws);
    if (c->seg_scratch) hipFree(c->seg_scratch);
    if (c->audit_dev) hipFree(c->audit_dev);
    graphs_clear(c);
    for (auto e : c->ev_pool) hipEventDestroy(e);
    delete c;
}

extern "C" int sylber_set_stop_stage(sylber_t c, int32_t stage) {
    if (!c) return 1;
    if (stage <= SYLBER_TAP_CONV(0)) {
        // SYLBER_TAP_CONV(i) = -(1024 + i)
        if (stage == SYLBER_TAP_CONV(0) || stage < SYLBER_TAP_CONV(6)) {
            syl_set_error("sylber_set_stop_stage", "unknown tap (conv-layer taps: -(1024 + i) behind conv layer i = 1..6; conv layer 0 is stage -1)"); return 1;
        }
    } else if (stage < SYLBER_TAP_POSCONV) {
        // SYLBER_TAP_LAYER(l, k) = -(8 (l + 1) + k)
        const int n = -stage, l = n / 8 - 1, k = n % 8;
        if (l < 0 || k > SYLBER_LTAP_FFN2_SUM) {
            syl_set_error("sylber_set_stop_stage", "unknown tap (negative stages: -1 conv0, -2 projection, -3 pos-conv, -(8 (l + 1) + k) tap k = 0..5 of layer l)"); return 1;
        }
        if (l >= c->num_layers) { syl_set_error("sylber_set_stop_stage", "layer tap: the handle has no such layer"); return 1; }
    }
    c->stop_stage = stage;
    return 0;
}
extern "C" int sylber_set_option(sylber_t c, int32_t key, int32_t value) {
    if (!c) { syl_set_error("sylber_set_option", "null handle"); return 1; }
    switch (key) {
        case SYLBER_OPT_GEMM_TILE: c->opt_gemm_cfg = value < 0 ? 0 : value + 1; break;     // stored as id + 1, 0 = automatic
        case SYLBER_OPT_ATTN_QUERIES_PER_WAVE: c->opt_attn_qw = value == 32 ? 1 : (value == 64 ? 2 : 0); break;
        case SYLBER_OPT_GEMM_PERSISTENT: c->opt_gemm_persist = value; break;      // < 0: also keep the 256x256 kernel one tile per workgroup
        case SYLBER_OPT_FUSE_OUTPROJ_LN: c->opt_fuse_ln = value > 0 ? 1 : (value < 0 ? -1 : 0); break;
        case SYLBER_OPT_CONV0_VALU: c->opt_conv0_valu = value > 0 ? (value == 2 ? 2 : 1) : 0; break;     // (2: producer-only timing probe, experiments build)
        case SYLBER_OPT_RESLN_PREFETCH: c->opt_resln_pre = value < 0 ? -1 : (value <= 3 ? value : 0); break;
        case SYLBER_OPT_FP8_ATTENTION: c->opt_attn8 = value < 0 ? -1 : (value > 0 ? 1 : 0); break;
        case SYLBER_OPT_FP16_AUDIT: {
            GUARD_DEVICE(c->device);
            c->opt_audit16 = value > 0 ? 1 : 0;
            if (c->opt_audit16) {                                 // (re)start the audit from zero
                if (!c->audit_dev) HIP_TRY(hipMalloc((void**)&c->audit_dev, AUDIT_STAGES * 2 * sizeof(unsigned)));
                HIP_TRY(hipDeviceSynchronize());
                HIP_TRY(hipMemset(c->audit_dev, 0, AUDIT_STAGES * 2 * sizeof(unsigned)));
            }
            break;
        }
        case SYLBER_OPT_SEGMENT: c->opt_segment = value < 0 ? -1 : 0; break;
        case SYLBER_OPT_GEMM_MODEL: c->opt_gemm_model = value == 5 ? 5 : (value == 2 ? 2 : (value == 6 ? 6 : 0)); break;   // (6 = 0 without the lone-round rule: A/B)
        case SYLBER_OPT_GEMM_H192: c->opt_gemm_h192 = value < 0 ? -1 : 0; break;
        case SYLBER_OPT_GEMM_MFMA16: c->opt_gemm_mfma16 = value < 0 ? -1 : 0; break;
        case SYLBER_OPT_GEMM_TAIL: c->opt_gemm_tail = value < 0 ? -1 : (value > 0 ? value + 1 : 0); break;   // k > 0: tail tile id k (stored id + 1)
        case SYLBER_OPT_PER_UTTERANCE: c->opt_per_utt = value == 1 ? 1 : 0; break;
        default: syl_set_error("sylber_set_option", "unknown option key"); return 1;
    }
    if (c->graph_mode) graphs_clear(c);                   // captured launches are stale
    return 0;
}
// enabling (or re-enabling) profiling resets the accumulated per-kernel times
extern "C" int sylber_set_profiling(sylber_t c, int32_t enable) {
    if (!c) return 1;
    const char* nm[1]; float ms[1];
    sylber_get_profile(c, nm, ms, 0);   // retire pending events
    c->prof_names.clear(); c->prof_ms.clear();
    c->profiling = enable;
    return 0;
}
extern "C" int64_t sylber_workspace_bytes(sylber_t c) { return c ? (int64_t)(c->ws_bytes + c->seg_scratch_floats * 4 + c->wbytes + c->f8bytes) : 0; }

extern "C" int sylber_get_profile(sylber_t c, const char** names, float* ms, int32_t cap) {
    if (!c) return -1;
    if (!c->prof.empty()) {
        c->prof_names.clear(); c->prof_ms.clear();
        for (auto& e : c->prof) {
            hipEventSynchronize(e.e1);
            float t = 0.f;
            hipEventElapsedTime(&t, e.e0, e.e1);
            size_t i = 0;
            for (; i < c->prof_names.size(); ++i) if (c->prof_names[i] == e.name) break;
            if (i == c->prof_names.size()) { c->prof_names.push_back(e.name); c->prof_ms.push_back(0.f); }
            c->prof_ms[i] += t;
            c->ev_pool.push_back(e.e0); c->ev_pool.push_back(e.e1);
        }
        c->prof.clear();
    }
    int n = (int)c->prof_names.size();
    n = n < cap ? n : cap;
    for (int i = 0; i < n; ++i) { names[i] = c->prof_names[i].c_str(); ms[i] = c->prof_ms[i]; }
    return n;
}

// Graph mode (sylber_set_graph_mode): ~110 launches per forward are launch-latency bound for short / single
// utterances (1.5 ms for one 3 s clip with 0.4 ms of kernel work).  The second call with the same
// (B, Lmax, input, output) captures the launch sequence on the caller's stream into a hipGraph; later calls replay it
// (forward.hip forward_graph).
void graphs_clear(sylber_ctx* c) {
    for (auto& g : c->graphs) if (g.exec) hipGraphExecDestroy(g.exec);
    c->graphs.clear();
}

extern "C" int sylber_set_graph_mode(sylber_t c, int32_t enable) {
    if (!c) return 1;
    c->graph_mode = enable != 0;
    if (!enable) graphs_clear(c);
    return 0;
}

// frames_host: nullptr (sylber_segment) or each row's own frame count (sylber_segment_frames), which travels to the device as kernel
// arguments into the slots behind the wide path's slab
// row0_host (sylber_segment_packed, needs frames_host): row b's first frame is hidden row row0_host[b]
static int segment_call(const char* what, sylber_t c, const float* hidden_dev, const int32_t* frames_host, int32_t B, int32_t T, int32_t D,
                        float norm_thr, float merge_thr, int64_t* seg_dev, int32_t* nseg_dev, float* feat_dev, void* stream,
                        const int32_t* row0_host = nullptr) {
    if (!c || !hidden_dev || !seg_dev || !nseg_dev) { syl_set_error(what, "null argument"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    GUARD_DEVICE(c->device);
    // per-utterance slab of the wide path (frame norms, slot table, bookkeeping of long runs; grow-only)
    const size_t slabs = segment_scratch_floats(B, T, D);
    const size_t need = slabs + (frames_host ? (((size_t)B + 63) & ~(size_t)63) * (row0_host ? 2 : 1) : 0);
    if (need > c->seg_scratch_floats) {
        HIP_TRY(hipStreamSynchronize(s));
        if (c->seg_scratch) HIP_TRY(hipFree(c->seg_scratch));
        c->seg_scratch = nullptr; c->seg_scratch_floats = 0;
        HIP_TRY(hipMalloc((void**)&c->seg_scratch, need * 4));
        c->seg_scratch_floats = need;
    }
    int* frames_dev = nullptr;
    int* row0_dev = nullptr;
    if (frames_host) {
        frames_dev = (int*)(c->seg_scratch + slabs);
        if (launch_upload_ints(frames_dev, frames_host, B, 0, s)) return 1;
    }
    if (row0_host) {
        row0_dev = frames_dev + (((size_t)B + 63) & ~(size_t)63);
        if (launch_upload_ints(row0_dev, row0_host, B, 0, s)) return 1;
    }
    ProfScope ps(c, s, "segment");
    return launch_segment(hidden_dev, B, T, D, norm_thr, merge_thr, seg_dev, nseg_dev, feat_dev, c->seg_scratch, s, c->opt_segment, frames_dev,
                          row0_dev);
}

extern "C" int sylber_segment(sylber_t c, const float* hidden_dev, int32_t B, int32_t T, int32_t D, float norm_thr,
                              float merge_thr, int64_t* seg_dev, int32_t* nseg_dev, float* feat_dev, void* stream) {
    return segment_call("sylber_segment", c, hidden_dev, nullptr, B, T, D, norm_thr, merge_thr, seg_dev, nseg_dev, feat_dev, stream);
}

extern "C" int sylber_segment_frames(sylber_t c, const float* hidden_dev, const int32_t* frames_host, int32_t B, int32_t T, int32_t D,
                                     float norm_thr, float merge_thr, int64_t* seg_dev, int32_t* nseg_dev, float* feat_dev, void* stream) {
    if (!frames_host) { syl_set_error("sylber_segment_frames", "null argument"); return 1; }
    if (c && c->opt_segment < 0) {
        syl_set_error("sylber_segment_frames", "not available with SYLBER_OPT_SEGMENT = -1 (the one-workgroup-per-utterance kernel has no per-row bound)");
        return 1;
    }
    for (int b = 0; b < B; ++b)
        if (frames_host[b] < 1 || frames_host[b] > T) { syl_set_error("sylber_segment_frames", "frames must be in [1, T]"); return 1; }
    return segment_call("sylber_segment_frames", c, hidden_dev, frames_host, B, T, D, norm_thr, merge_thr, seg_dev, nseg_dev, feat_dev, stream);
}

// boundary detection of a packed batch (sylber_forward_packed's hidden states): clip b is segmented and pooled as its own frames
// hidden[offsets[b], offsets[b] + frames[b]) alone; tables relative to the clip's start, kcap = max frames[b] slots per clip
extern "C" int sylber_segment_packed(sylber_t c, const float* hidden_dev, const int32_t* samples_host, int32_t B, float norm_thr, float merge_thr,
                                     int64_t* seg_dev, int32_t* nseg_dev, float* feat_dev, void* stream) {
    if (!samples_host) { syl_set_error("sylber_segment_packed", "null argument"); return 1; }
    if (c && c->opt_segment < 0) {
        syl_set_error("sylber_segment_packed", "not available with SYLBER_OPT_SEGMENT = -1 (the one-workgroup-per-utterance kernel has no per-row bound)");
        return 1;
    }
    std::vector<int32_t> off(B > 0 ? B + 1 : 1), fr(B > 0 ? B : 1);
    if (sylber_packed_layout(samples_host, B, off.data(), fr.data())) return 1;
    int kcap = 0;
    for (int b = 0; b < B; ++b) kcap = fr[b] > kcap ? fr[b] : kcap;
    return segment_call("sylber_segment_packed", c, hidden_dev, fr.data(), B, kcap, SYL_HIDDEN, norm_thr, merge_thr, seg_dev, nseg_dev, feat_dev,
                        stream, off.data());
}

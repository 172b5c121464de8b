/*
 * sylber_hip_dev.h -- development aids exported by libsylber_hip.so that are NOT part of the drop-in C-ABI
 * (include/sylber_hip.h): micro-benchmarks used by tools/.  Nothing on the product path or in the parity tests
 * needs them (GPU tests use the workspace-poisoning aid and the taps), and they keep no process-global state.
 */
#ifndef SYLBER_HIP_DEV_H
#define SYLBER_HIP_DEV_H
#include <stdint.h>
#include "sylber_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
/* average ms of one launch of the bf16 GEMM kernel (M x N x K, activation row stride ldx) on pseudo-random
 * operands; epi / act as in csrc/kernels.h; cfg: -1 = automatic tile shape, else persist * 1000 + tile id;
 * cfg in [100, 200): the MXFP8 GEMM with tile configuration cfg - 100; cfg + 200000: every timed launch finds its
 * operands cold (1 GiB written between the launches, each launch timed by its own event pair) */
int sylber_debug_gemm_bench(int32_t M, int32_t N, int32_t K, int32_t ldx, int32_t epi, int32_t act, int32_t cfg,
                            int32_t iters, float* ms_out);
/* the tile id the cost model of the 16-bit GEMM launcher picks for a launch (csrc/gemm_bf16.hip TileModel): host arithmetic only, no device touched.
 * epi / act as the forward passes them (0 = 16-bit out, 3 = q,k,v, 6 = fp32 residual + LayerNorm; act 1 = GELU), fmt 0 bf16 / 1 fp16,
 * model = SYLBER_OPT_GEMM_MODEL, kpat = 1 for the 3-tap conv K order.  tests/test_abi.py pins the choices of the headline shapes. */
int sylber_debug_gemm_pick(int32_t M, int32_t N, int32_t K, int32_t epi, int32_t act, int32_t fmt, int32_t model, int32_t kpat);
/* the kernel instantiation(s) the launcher resolves that launch to (host arithmetic only): `tile` as sylber_op_linear takes it (-1 = the cost
 * model's pick; + 1000 x workgroups per CU, 9000 + id = one workgroup per tile, + 1000000 = the 16-bit-output role on the 32x32x16 kernels), fmt 2 =
 * split16, h192 / pre / tail = SYLBER_OPT_GEMM_H192 / the residual prefetch columns / the forced tail tile id + 1.  buf receives one line per launch,
 * "<first row> <end row> <kernel template>[<template arguments>]"; returns the number of launches (2 = a forced row split), 0 = refused,
 * -1 = buf too small.  tests/test_abi.py pins a grid of these against tests/golden/gemm_dispatch.txt. */
int sylber_debug_gemm_resolve(int32_t M, int32_t N, int32_t K, int32_t epi, int32_t act, int32_t fmt, int32_t kpat, int32_t tile, int32_t model,
                              int32_t h192, int32_t pre, int32_t tail, char* buf, int32_t cap);
/* the same launch through the TRACE instantiation of the 8-wave 256x256 kernel (s_memtime stamps around the phases of its K
 * loop): out20 = 2 x 10 shader-cycle counters of workgroup 0's waves 0 and 4 (csrc/api.hip sylber_debug_gemm_trace) */
int sylber_debug_gemm_trace(int32_t M, int32_t N, int32_t K, int32_t ldx, int32_t epi, int32_t act, unsigned long long* out20,
                            float* ms_out);
/* test aid: fill the handle's activation workspace with `byte` (0xFF = NaN patterns) and force the next forward to redo the zeroing it
 * does after a batch-shape change; results must not change (tests/test_gpu_encoder.py) */
int sylber_debug_poison_workspace(sylber_t h, int32_t byte);
/* test aid: conv0's GroupNorm scale / shift table of the handle's last forward (padded or packed) of B utterances, copied to
 * out_host [B][512][2]: (a, b) per channel with a = gamma / sqrt(var + 1e-5), b = beta - mean * a; synchronises the device
 * (tests/test_gpu_frontend.py checks it against float64) */
int sylber_debug_conv0_scale_shift(sylber_t h, int32_t B, float* out_host);
/* test aid (host arithmetic only, no device touched): the forward's plan for n_samples >= 400 samples per utterance -- L[i] = valid rows of
 * conv layer i = 0..6 and R[i] = rows per utterance of its output buffer (sylber_padded_frames << (6 - i)); tests/test_conv_stack_ref.py
 * checks L[i] <= R[i] and both against their restatement */
int sylber_debug_conv_rows(int32_t n_samples, int32_t* L, int32_t* R);
/* average ms of one launch of the attention core (12 heads x 64, B utterances of T frames, no key mask) on pseudo-random packed
 * operands; precision: SYLBER_BF16 (bf16 operands) or SYLBER_FP8 (MXFP8 q / k / V^T, e4m3 P) */
int sylber_debug_attention_bench(int32_t B, int32_t T, int32_t precision, int32_t iters, float* ms_out);
/* test aid: a tap inside the resynthesis decoder (csrc/cfm.hip), per handle, off by default and without effect when off.  With a stage set,
 * the next eval / sample / sample_frames / sample_packed call (steps >= 2) runs its preparation and its first evaluation (time index 0; a
 * sample call: t = 0, state y0) through the launches it always issues, up to the launch that writes the stage's buffer, copies that buffer to
 * tap_dev and returns 0; the call's own output is not written.  The copy is every row of the buffer (M = B x Tp rows, or the packed
 * call's slot rows; frame rows B x T or sum Tb for CONDX / XE) without the slack rows, in STORAGE order (no permutation undone), 16-bit
 * words widened to fp32 exactly.  The setting persists until changed; stage 0 switches it off.  Refused with an error text and no launch: an
 * unknown stage (Q / K / VT exist in the 16-bit precisions only, QKVF in fp32 only), a call whose stage needs more than tap_floats
 * floats, a sample call with steps = 1 (no evaluation).  tests/test_gpu_cfm_block.py holds every stage to float64.
 *   front stages: CONDX [NF, 512]; GB [16 norms][gamma, beta][512] of time index 0; XE [NF, 512]; X0 [M, 512] (behind cfm_conv)
 *   block li = 0..7, SYLBER_CFM_TAP(li, k): H_ATTN [M, 512]; QKV [M, 1536] fp32; Q, K [B, 12, Tp, 64]; VT [B, 12, 64, Tpv]; QKVF [M, 2304];
 *   CTX [M, 768]; X_ATTN [M, 512]; H_FF [M, 512]; FF [M, 2816] (value 1408 | gate 1408); G [M, 1408]; X_FF [M, 512] */
enum { SYLBER_CFM_TAP_CONDX = 1, SYLBER_CFM_TAP_GB = 2, SYLBER_CFM_TAP_XE = 3, SYLBER_CFM_TAP_X0 = 4 };
enum { SYLBER_CFM_BTAP_H_ATTN = 0, SYLBER_CFM_BTAP_QKV = 1, SYLBER_CFM_BTAP_Q = 2, SYLBER_CFM_BTAP_K = 3, SYLBER_CFM_BTAP_VT = 4,
       SYLBER_CFM_BTAP_QKVF = 5, SYLBER_CFM_BTAP_CTX = 6, SYLBER_CFM_BTAP_X_ATTN = 7, SYLBER_CFM_BTAP_H_FF = 8, SYLBER_CFM_BTAP_FF = 9,
       SYLBER_CFM_BTAP_G = 10, SYLBER_CFM_BTAP_X_FF = 11 };
#define SYLBER_CFM_TAP(block, k) (16 * ((block) + 1) + (k))
int sylber_cfm_set_tap(sylber_cfm_t h, int32_t stage, float* tap_dev, int64_t tap_floats);
/* floats the tap of `stage` writes for a padded [B, T] call / a packed call of B clips; -1 for an unknown stage or a bad shape */
int64_t sylber_cfm_tap_floats(sylber_cfm_t h, int32_t stage, int32_t B, int32_t T);
int64_t sylber_cfm_tap_floats_packed(sylber_cfm_t h, int32_t stage, const int32_t* frames_host, int32_t B);
/* test aid: the scalar chain behind the segmenter's threshold comparisons, as csrc/segment.hip compiles it (device pointers, launched on
 * `stream`, not synchronised).  For i < n: pow_dev[i] = the device restatement of glibc powf(x[i], .5f), sqrt_dev[i] = sqrtf(x[i]),
 * div_dev[i] = x[i] / d[i].  For wave w < nwaves and j < 768: quot_dev[768 w + j] = (c[768 w + j] * cnt[w] + m[768 w + j]) / (cnt[w] + 1),
 * the greedy scan's merge update through the scan's own function, one wave per group of 768 with its wave-wide choice between the
 * one-division form and the plain division.  Either part may be empty (n = 0 / nwaves = 0).  tests/test_gpu_segment_edges.py holds
 * all four to the host bit for bit. */
int sylber_debug_segment_scalars(const float* x_dev, const float* d_dev, int64_t n, float* pow_dev, float* sqrt_dev, float* div_dev,
                                 const float* c_dev, const float* m_dev, const int32_t* cnt_dev, int64_t nwaves, float* quot_dev,
                                 void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SYLBER_HIP_DEV_H */

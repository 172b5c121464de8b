// The two callers right behind the Segmenter path, fed with device-resident outputs
// of sylber_segment:
//   N4  k-means tokenisation of the pooled segment features: KMQuantizer.get_indices / decode
//       (sylber/model/quantizer.py:86-135; the codebook look-up itself is vector_quantize_pytorch's
//       EuclideanCodebook — a third-party dependency absent from the image — : indices = argmax_c -cdist(x, c))
//   N3  front half of SegmentSynthesis.resynthesize (sylber/model/segment_synthesis.py:103-140): every frame of a
//       segment takes the segment's mean feature, the `MLP` conditioner (Linear -> RFF -> ... -> Linear, :17-53)
//       maps it to the conditioning embedding, frames whose hidden-state norm is below the threshold are zeroed.
// Both are small next to the encoder (tens of GFLOP); they run in exact fp32 on the f32 MFMA GEMM of the parity
// mode (fp32_path.hip) so that near-ties of the arg-min and the LayerNorms see the reference's arithmetic class.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include <cstring>
#include <string>
#include <vector>

// ---- N4 ---------------------------------------------------------------------------------------------------------
// token / (||token|| + eps-under-the-root) * 6  (quantizer.py:104-105: token/(((token**2).sum(-1)+1e-8)**.5)[...,None]*6)
__global__ __launch_bounds__(256) void km_normalize_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int D) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= n) return;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) { const float v = x[(size_t)r * D + c]; s = fmaf(v, v, s); }
    s = wave_sum(s);
    const float nrm = sqrtf(s + 1e-8f);
    for (int c = lane; c < D; c += 64) y[(size_t)r * D + c] = x[(size_t)r * D + c] / nrm * 6.0f;
}
__global__ __launch_bounds__(256) void km_sqnorm_kernel(const float* __restrict__ c, float* __restrict__ out, int K, int D) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= K) return;
    float s = 0.f;
    for (int j = lane; j < D; j += 64) { const float v = c[(size_t)r * D + j]; s = fmaf(v, v, s); }
    s = wave_sum(s);
    if (lane == 0) out[r] = s;
}
// idx[r] = argmin_c (||c||^2 - 2 x.c)  (the ||x||^2 term and the square root of cdist are monotone / constant per
// row); ties -> the smallest index, like argmax over -cdist returns the first maximum.  A NaN score compares false and is never
// taken; a row whose scores are all NaN (a NaN or inf - inf token) gets index 0, which is what that argmax returns for it
__global__ __launch_bounds__(256) void km_argmin_kernel(const float* __restrict__ dots, long ld, const float* __restrict__ cn,
                                                        int32_t* __restrict__ idx, int istride, int n, int K) {
    __shared__ float bv[4]; __shared__ int bi[4];
    const int r = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float best = INFINITY; int besti = 0x7fffffff;
    for (int c = threadIdx.x; c < K; c += 256) {
        const float d = fmaf(-2.0f, dots[(size_t)r * ld + c], cn[c]);
        if (d < best || (d == best && c < besti)) { best = d; besti = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(besti, o, 64);
        if (ov < best || (ov == best && oi < besti)) { best = ov; besti = oi; }
    }
    if (lane == 0) { bv[wave] = best; bi[wave] = besti; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) if (bv[w] < best || (bv[w] == best && bi[w] < besti)) { best = bv[w]; besti = bi[w]; }
        idx[(size_t)r * istride] = besti < K ? besti : 0;
    }
}

// the same two kernels for the k-means fit (kmeans.hip): fitting on normalised rows and scoring against the squared norms with the
// quantizers' own arithmetic is what makes a fitted KMQuantizer map its training rows to the fit's labels bit for bit
int launch_km_normalize(const float* x, float* y, int n, int D, hipStream_t s) {
    hipLaunchKernelGGL(km_normalize_kernel, dim3((n + 3) / 4), dim3(256), 0, s, x, y, n, D);
    HIP_TRY(hipGetLastError());
    return 0;
}
int launch_km_sqnorm(const float* c, float* out, int K, int D, hipStream_t s) {
    hipLaunchKernelGGL(km_sqnorm_kernel, dim3((K + 3) / 4), dim3(256), 0, s, c, out, K, D);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int64_t sylber_km_workspace_floats(int32_t n, int32_t K, int32_t D) {
    if (n < 1 || K < 1 || D < 1) return -1;
    return (int64_t)n * ((K + 3) & ~3) + (int64_t)n * D + ((K + 3) & ~3) + 64;
}

// idx[r * istride] = argmin over the first K rows of cb of (||c||^2 - 2 x.c), given cn = ||c||^2: x . c on the exact-fp32 MFMA
// GEMM over the first Kc >= K rows of cb (row stride D), then km_argmin_kernel.  The GEMM's N must be a multiple of 4: with
// Kc % 4 != 0 the last (Kp - Kc) columns re-read row Kc-1.  dots: [n][Kp] floats, Kp = Kc rounded up to 4.  x: row stride ldx.
// The one arg-min rule of the library: the k-means quantizers and the residual VQ of the learned quantizer both end here.
static int km_nearest(const char* what, const float* x, long ldx, int n, const float* cb, int Kc, int K, int D, const float* cn,
                      int32_t* idx_dev, int istride, float* dots, hipStream_t s) {
    const int Kp = (Kc + 3) & ~3;
    GemmArgsF32 g = {};
    g.X = x; g.ldx = ldx; g.W = cb; g.M = n; g.N = Kc; g.K = D; g.out0 = dots; g.ld0 = Kp;
    if (Kc % 4) {
        // run the aligned part on the GEMM and leave the ragged tail to a second, 4-wide launch over the last 4 rows
        g.N = Kc & ~3;
        if (g.N > 0 && launch_gemm_f32(g, s)) return 1;
        GemmArgsF32 t = g;
        t.W = cb + (size_t)(Kc - 4 < 0 ? 0 : Kc - 4) * D; t.N = 4; t.out0 = dots + (Kc - 4 < 0 ? 0 : Kc - 4);
        if (Kc >= 4) { if (launch_gemm_f32(t, s)) return 1; }
        else { syl_set_error(what, "K < 4 with K % 4 != 0 is not supported"); return 1; }
    } else if (launch_gemm_f32(g, s)) return 1;
    hipLaunchKernelGGL(km_argmin_kernel, dim3(n), dim3(256), 0, s, dots, (long)Kp, cn, idx_dev, istride, n, K);
    HIP_TRY(hipGetLastError());
    return 0;
}

// idx_dev[r * istride] = nearest centroid of row r (istride 2: one column of the residual quantizer's [n, 2] table)
static int km_assign_impl(const char* what, const float* feats_dev, int32_t n, const float* centroids_dev, int32_t K, int32_t D,
                          int32_t normalize, int32_t* idx_dev, int istride, float* workspace_dev, hipStream_t s) {
    const int Kp = (K + 3) & ~3;
    float* dots = workspace_dev;                         // [n][Kp]
    float* xn = dots + (size_t)n * Kp;                   // [n][D] (normalised copy)
    float* cn = xn + (size_t)n * D;                      // [Kp]
    const float* x = feats_dev;
    if (normalize) {
        hipLaunchKernelGGL(km_normalize_kernel, dim3((n + 3) / 4), dim3(256), 0, s, feats_dev, xn, n, D);
        x = xn;
    }
    hipLaunchKernelGGL(km_sqnorm_kernel, dim3((K + 3) / 4), dim3(256), 0, s, centroids_dev, cn, K, D);
    HIP_TRY(hipGetLastError());
    return km_nearest(what, x, D, n, centroids_dev, K, K, D, cn, idx_dev, istride, dots, s);
}

extern "C" int sylber_km_assign(const float* feats_dev, int32_t n, const float* centroids_dev, int32_t K, int32_t D, int32_t normalize,
                                int32_t* idx_dev, float* workspace_dev, void* stream) {
    if (!feats_dev || !centroids_dev || !idx_dev || !workspace_dev) { syl_set_error("sylber_km_assign", "null argument"); return 1; }
    if (n < 1 || K < 1 || D < 16 || D % 16) { syl_set_error("sylber_km_assign", "need n, K >= 1 and D a multiple of 16"); return 1; }
    return km_assign_impl("sylber_km_assign", feats_dev, n, centroids_dev, K, D, normalize, idx_dev, 1, workspace_dev, (hipStream_t)stream);
}

// KMQuantizer.decode (quantizer.py:127-133): rows of the codebook; negative indices are clipped to 0
__global__ __launch_bounds__(256) void km_decode_kernel(const int32_t* __restrict__ idx, const float* __restrict__ c, float* __restrict__ out,
                                                        int n, int K, int D) {
    const int r = blockIdx.x;
    int i = idx[r]; i = i < 0 ? 0 : (i >= K ? K - 1 : i);
    for (int j = threadIdx.x; j < D; j += 256) out[(size_t)r * D + j] = c[(size_t)i * D + j];
}
extern "C" int sylber_km_decode(const int32_t* idx_dev, int32_t n, const float* centroids_dev, int32_t K, int32_t D, float* out_dev, void* stream) {
    if (!idx_dev || !centroids_dev || !out_dev || n < 1 || K < 1 || D < 1) { syl_set_error("sylber_km_decode", "bad argument"); return 1; }
    hipLaunchKernelGGL(km_decode_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, idx_dev, centroids_dev, out_dev, n, K, D);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ResidualKMQuantizer (quantizer.py:137-180): stage 1 is KMQuantizer(centroids).get_indices (never normalised: upstream
// builds both stages without `normalize`), stage 2 assigns token - decode(stage 1) against the second codebook
// r = x - c1[max(idx1, 0)]: one fp32 subtract per element (token - z_q); idx1 is column 0 of the [n, 2] table
__global__ __launch_bounds__(256) void km_residual_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx, const float* __restrict__ c,
                                                          float* __restrict__ r, int n, int K, int D) {
    const int row = blockIdx.x;
    int i = idx[(size_t)row * 2]; i = i < 0 ? 0 : (i >= K ? K - 1 : i);
    for (int j = threadIdx.x; j < D; j += 256) r[(size_t)row * D + j] = x[(size_t)row * D + j] - c[(size_t)i * D + j];
}

extern "C" int64_t sylber_km_residual_workspace_floats(int32_t n, int32_t K1, int32_t K2, int32_t D) {
    if (n < 1 || K1 < 1 || K2 < 1 || D < 1) return -1;
    return sylber_km_workspace_floats(n, K1 > K2 ? K1 : K2, D) + (int64_t)n * D + 64;
}

extern "C" int sylber_km_assign_residual(const float* feats_dev, int32_t n, const float* c1_dev, int32_t K1, const float* c2_dev, int32_t K2,
                                         int32_t D, int32_t* idx_dev, float* workspace_dev, void* stream) {
    static const char* what = "sylber_km_assign_residual";
    hipStream_t s = (hipStream_t)stream;
    if (!feats_dev || !c1_dev || !c2_dev || !idx_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1 || K1 < 1 || K2 < 1 || D < 16 || D % 16) { syl_set_error(what, "need n, K1, K2 >= 1 and D a multiple of 16"); return 1; }
    float* ws = workspace_dev;                                            // sylber_km_workspace_floats(n, max K, D): shared by both stages
    float* r = ws + (sylber_km_workspace_floats(n, K1 > K2 ? K1 : K2, D) + 63) / 64 * 64;   // [n][D] residual
    if (km_assign_impl(what, feats_dev, n, c1_dev, K1, D, 0, idx_dev, 2, ws, s)) return 1;
    hipLaunchKernelGGL(km_residual_kernel, dim3(n), dim3(256), 0, s, feats_dev, idx_dev, c1_dev, r, n, K1, D);
    HIP_TRY(hipGetLastError());
    return km_assign_impl(what, r, n, c2_dev, K2, D, 0, idx_dev + 1, 2, ws, s);
}

// ResidualKMQuantizer.decode (quantizer.py:174-178): z_q1 + z_q2 = c1[max(i1, 0)] + c2[max(i2, 0)], added in that order
__global__ __launch_bounds__(256) void km_decode_residual_kernel(const int32_t* __restrict__ idx, const float* __restrict__ c1, int K1,
                                                                 const float* __restrict__ c2, int K2, float* __restrict__ out, int n, int D) {
    const int r = blockIdx.x;
    int i1 = idx[(size_t)r * 2], i2 = idx[(size_t)r * 2 + 1];
    i1 = i1 < 0 ? 0 : (i1 >= K1 ? K1 - 1 : i1);
    i2 = i2 < 0 ? 0 : (i2 >= K2 ? K2 - 1 : i2);
    for (int j = threadIdx.x; j < D; j += 256) out[(size_t)r * D + j] = c1[(size_t)i1 * D + j] + c2[(size_t)i2 * D + j];
}
extern "C" int sylber_km_decode_residual(const int32_t* idx_dev, int32_t n, const float* c1_dev, int32_t K1, const float* c2_dev, int32_t K2,
                                         int32_t D, float* out_dev, void* stream) {
    if (!idx_dev || !c1_dev || !c2_dev || !out_dev || n < 1 || K1 < 1 || K2 < 1 || D < 1) {
        syl_set_error("sylber_km_decode_residual", "bad argument"); return 1;
    }
    hipLaunchKernelGGL(km_decode_residual_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, idx_dev, c1_dev, K1, c2_dev, K2, out_dev, n, D);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- learned quantizer (sylber/model/quantizer.py:6-77, 182-257: FFEncoder + two GroupedResidualVQ stacks) --------------------
// Exact fp32 like the k-means path: the encoder's Linears on the f32 MFMA GEMM (one launch per Linear, upstream's order), the
// unit norms in one kernel, the residual VQ on km_nearest (the arg-min rule above) plus a residual-update kernel per stage.
// Widths that are not multiples of 16 are zero-padded: the caller pads weights and codebooks once at load, the kernels pad the
// activations; a zero column adds fmaf(0, 0, acc) = acc to every chain, so the padded contractions are the unpadded ones.

// _unit_norm / _unit_norm_sep (quantizer.py:33-44) and the blank mask of Quantizer.forward (:217, :228-229), one wave per row:
//   y[r, c] = x[r, c] / sqrt(sum_{c' in range(c)} x[r, c']^2 + 1e-5)  for c < D (normalize; else a plain copy), the ranges being
//   [0, split) and [split, D) for 0 < split < D and [0, D) otherwise; y[r, c] = 0 for D <= c < Dy (padding);
//   the whole row 0 where !(sum_c blank[r, c]^2 > 0) (blank != nullptr: the token as it entered forward).
// Each range's sum is a lane-strided fmaf chain plus the wave's butterfly: a fixed order per row, whatever n is.  In place is allowed
// (x == y, ldx == ldy): every lane reads an element before it writes it, and the sums are complete before any write.
__global__ __launch_bounds__(256) void lq_norm_kernel(const float* x, long ldx, int n, int D, int split, int normalize,
                                                      const float* __restrict__ blank, long ldb, int Db, float* y, long ldy, int Dy) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= n) return;
    const float* xr = x + (size_t)r * ldx;
    float* yr = y + (size_t)r * ldy;
    bool zero = false;
    if (blank) {
        float b = 0.f;
        for (int c = lane; c < Db; c += 64) { const float v = blank[(size_t)r * ldb + c]; b = fmaf(v, v, b); }
        b = wave_sum(b);
        zero = !(b > 0.f);
    }
    const int sp = (split > 0 && split < D) ? split : D;
    float n0 = 1.f, n1 = 1.f;
    if (normalize) {
        float s0 = 0.f, s1 = 0.f;
        for (int c = lane; c < sp; c += 64) { const float v = xr[c]; s0 = fmaf(v, v, s0); }
        for (int c = sp + lane; c < D; c += 64) { const float v = xr[c]; s1 = fmaf(v, v, s1); }
        s0 = wave_sum(s0); s1 = wave_sum(s1);
        n0 = sqrtf(s0 + 1e-5f); n1 = sqrtf(s1 + 1e-5f);
    }
    for (int c = lane; c < Dy; c += 64) {
        float v = 0.f;
        if (c < D && !zero) { v = xr[c]; if (normalize) v = v / (c < sp ? n0 : n1); }
        yr[c] = v;
    }
}

extern "C" int sylber_lq_norm(const float* x_dev, int64_t ldx, int32_t n, int32_t D, int32_t split, int32_t normalize, const float* blank_dev,
                              int64_t ld_blank, int32_t D_blank, float* y_dev, int64_t ldy, int32_t Dy, void* stream) {
    static const char* what = "sylber_lq_norm";
    if (!x_dev || !y_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 0 || D < 1 || Dy < D || ldx < D || ldy < Dy || (blank_dev && (D_blank < 1 || ld_blank < D_blank))) {
        syl_set_error(what, "need n >= 0, D >= 1, Dy >= D, ldx >= D, ldy >= Dy (and ld_blank >= D_blank >= 1 with a blank source)"); return 1;
    }
    if (x_dev == y_dev && ldx != ldy) { syl_set_error(what, "in place needs ldx == ldy"); return 1; }
    if (n == 0) return 0;
    hipLaunchKernelGGL(lq_norm_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, x_dev, (long)ldx, n, D, split, normalize,
                       blank_dev, (long)ld_blank, D_blank, y_dev, (long)ldy, Dy);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int64_t ffenc_maxdim(int32_t num_hidden, const int32_t* dims) {
    int64_t m = 0;
    for (int i = 0; i < num_hidden; ++i) m = dims[i + 1] > m ? dims[i + 1] : m;
    return m;
}
extern "C" int64_t sylber_ffenc_workspace_floats(int32_t n, int32_t num_hidden, const int32_t* dims) {
    if (n < 1 || num_hidden < 0 || !dims) return -1;
    return 2 * (int64_t)n * ffenc_maxdim(num_hidden, dims) + 64;
}

// FFEncoder.forward (quantizer.py:15-31): per hidden dim h, Linear(in, h) -> Linear(h, h) -> ReLU -> Linear(h, h) (the FeedForward;
// Dropout is the identity in eval), then Linear(in, out).  One GEMM launch per Linear with the bias (and the ReLU) in the epilogue,
// ping-ponging between two [n][max h] buffers of the workspace.
extern "C" int sylber_ffenc(const float* x_dev, int32_t n, int32_t num_hidden, const int32_t* dims, const float* const* weights, float* y_dev,
                            float* workspace_dev, void* stream) {
    static const char* what = "sylber_ffenc";
    hipStream_t s = (hipStream_t)stream;
    if (!x_dev || !dims || !weights || !y_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1 || num_hidden < 0) { syl_set_error(what, "need n >= 1 and num_hidden >= 0"); return 1; }
    for (int i = 0; i < num_hidden + 2; ++i)
        if (dims[i] < 16 || dims[i] % 16) { syl_set_error(what, "every (padded) width must be a positive multiple of 16"); return 1; }
    for (int i = 0; i < 2 * (3 * num_hidden + 1); ++i)
        if (!weights[i]) { syl_set_error(what, "missing weight or bias"); return 1; }
    float* buf[2] = {workspace_dev, workspace_dev + (size_t)n * ffenc_maxdim(num_hidden, dims)};
    const float* cur = x_dev;
    int in = dims[0], w = 0, pp = 0;
    auto linear = [&](int out, int act, float* dst) {
        GemmArgsF32 g = {};
        g.X = cur; g.ldx = in; g.W = weights[w]; g.M = n; g.N = out; g.K = in; g.bias = weights[w + 1]; g.act = act; g.out0 = dst; g.ld0 = out;
        w += 2; cur = dst; in = out;
        return launch_gemm_f32(g, s);
    };
    for (int i = 0; i < num_hidden; ++i) {
        const int h = dims[i + 1];
        if (linear(h, 0, buf[pp])) return 1;                  // mlp.{2i}: Linear(in, h)
        pp ^= 1;
        if (linear(h, ACTF_RELU, buf[pp])) return 1;          // mlp.{2i+1}.0 + ReLU
        pp ^= 1;
        if (linear(h, 0, buf[pp])) return 1;                  // mlp.{2i+1}.3
        pp ^= 1;
    }
    return linear(dims[num_hidden + 1], 0, y_dev);             // mlp.{2H}: Linear(in, out)
}

// ||E_q[k]||^2 of every codebook row, once at load: codebooks [Q][Kp][Dp] (Kp = K rounded up to 4, Dp = D rounded up to 16, the
// padding zero), out [Q][Kp].  The same lane-strided chain as km_sqnorm_kernel (which it is): zero columns add nothing.
extern "C" int sylber_rvq_prepare(const float* codebooks_dev, int32_t Q, int32_t K, int32_t D, float* sqnorms_dev, void* stream) {
    if (!codebooks_dev || !sqnorms_dev || Q < 1 || K < 1 || D < 1) { syl_set_error("sylber_rvq_prepare", "bad argument"); return 1; }
    const int Kp = (K + 3) & ~3, Dp = (D + 15) & ~15, rows = Q * Kp;
    hipLaunchKernelGGL(km_sqnorm_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, codebooks_dev, sqnorms_dev, rows, Dp);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int64_t sylber_rvq_workspace_floats(int32_t n, int32_t K, int32_t D) {
    if (n < 1 || K < 1 || D < 1) return -1;
    return (int64_t)n * ((K + 3) & ~3) + (int64_t)n * ((D + 15) & ~15) + 64;
}

// one residual stage, one wave per row: i = idx[r * ld_idx] (already in [0, K) from the arg-min; clamped all the same), then
// r -= E_q[i] over the Dp padded columns (update_r; 0 - 0 keeps the padding 0) and z = (first ? 0 : z) + E_q[i] over D columns
// (z != nullptr): quantized_out = quantized_out + quantized, residual = residual - quantized, in stage order.
__global__ __launch_bounds__(256) void rvq_update_kernel(const int32_t* __restrict__ idx, long ld_idx, const float* __restrict__ E, int K, int D,
                                                         int Dp, float* __restrict__ res, int update_r, float* __restrict__ z, long ldz, int first, int n) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= n) return;
    int i = idx[(size_t)r * ld_idx]; i = i < 0 ? 0 : (i >= K ? K - 1 : i);
    const float* e = E + (size_t)i * Dp;
    if (update_r) for (int c = lane; c < Dp; c += 64) res[(size_t)r * Dp + c] = res[(size_t)r * Dp + c] - e[c];
    if (z) for (int c = lane; c < D; c += 64) z[(size_t)r * ldz + c] = (first ? 0.f : z[(size_t)r * ldz + c]) + e[c];
}

// ResidualVQ of one group, eval (the GroupedResidualVQ restatement): r = x; for q: i_q = argmin_k ||r - E_q[k]|| (ties: smallest k),
// z += E_q[i_q], r -= E_q[i_q].  x: rows of width D at stride ldx (a column window of the normalised encoder output), idx: column q at
// idx_dev[row * ld_idx + q], z: optional window of width D at stride ldz.  The residual lives in the workspace, zero-padded to Dp.
extern "C" int sylber_rvq_assign(const float* x_dev, int64_t ldx, int32_t n, int32_t D, const float* codebooks_dev, const float* sqnorms_dev,
                                 int32_t Q, int32_t K, int32_t* idx_dev, int64_t ld_idx, float* z_dev, int64_t ldz, float* workspace_dev,
                                 void* stream) {
    static const char* what = "sylber_rvq_assign";
    hipStream_t s = (hipStream_t)stream;
    if (!x_dev || !codebooks_dev || !sqnorms_dev || !idx_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1 || D < 1 || Q < 1 || K < 1 || ldx < D || ld_idx < Q || (z_dev && ldz < D)) {
        syl_set_error(what, "need n, D, Q, K >= 1, ldx >= D, ld_idx >= Q and ldz >= D"); return 1;
    }
    const int Kp = (K + 3) & ~3, Dp = (D + 15) & ~15;
    float* dots = workspace_dev;                              // [n][Kp]
    float* res = dots + (size_t)n * Kp;                       // [n][Dp] (16-byte aligned: Kp % 4 == 0)
    hipLaunchKernelGGL(lq_norm_kernel, dim3((n + 3) / 4), dim3(256), 0, s, x_dev, (long)ldx, n, D, 0, 0, (const float*)nullptr, 0L, 0,
                       res, (long)Dp, Dp);
    HIP_TRY(hipGetLastError());
    for (int q = 0; q < Q; ++q) {
        const float* E = codebooks_dev + (size_t)q * Kp * Dp;
        if (km_nearest(what, res, Dp, n, E, Kp, K, Dp, sqnorms_dev + (size_t)q * Kp, idx_dev + q, (int)ld_idx, dots, s)) return 1;
        const int update_r = q + 1 < Q;                         // the last stage's residual is never read
        if (!update_r && !z_dev) break;
        hipLaunchKernelGGL(rvq_update_kernel, dim3((n + 3) / 4), dim3(256), 0, s, idx_dev + q, (long)ld_idx, E, K, D, Dp, res, update_r,
                           z_dev, (long)ldz, q == 0 ? 1 : 0, n);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// get_output_from_indices of the same stack: z = sum_q E_q[clamp(i_q, 0, K-1)] in stage order (from 0, as the assignment's z),
// one wave per row.  Negative ids are upstream's clip(0); ids >= K clamp to K-1 (upstream would index out of range).
__global__ __launch_bounds__(256) void rvq_decode_kernel(const int32_t* __restrict__ idx, long ld_idx, const float* __restrict__ cb, int Q, int K,
                                                         int Kp, int D, int Dp, float* __restrict__ z, long ldz, int n) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= n) return;
    for (int c = lane; c < D; c += 64) {
        float acc = 0.f;
        for (int q = 0; q < Q; ++q) {
            int i = idx[(size_t)r * ld_idx + q]; i = i < 0 ? 0 : (i >= K ? K - 1 : i);
            acc = acc + cb[((size_t)q * Kp + i) * Dp + c];
        }
        z[(size_t)r * ldz + c] = acc;
    }
}
extern "C" int sylber_rvq_decode(const int32_t* idx_dev, int64_t ld_idx, int32_t n, const float* codebooks_dev, int32_t Q, int32_t K, int32_t D,
                                 float* z_dev, int64_t ldz, void* stream) {
    if (!idx_dev || !codebooks_dev || !z_dev || n < 0 || Q < 1 || K < 1 || D < 1 || ld_idx < Q || ldz < D) {
        syl_set_error("sylber_rvq_decode", "bad argument"); return 1;
    }
    if (n == 0) return 0;
    hipLaunchKernelGGL(rvq_decode_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, idx_dev, (long)ld_idx, codebooks_dev, Q, K,
                       (K + 3) & ~3, D, (D + 15) & ~15, z_dev, (long)ldz, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- N3 ---------------------------------------------------------------------------------------------------------
// entry points run on the handle's GPU and leave the caller's current device as they found it
struct DevGuard {
    int prev = -1;
    explicit DevGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); }
    ~DevGuard() { int cur = -1; if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev); }
};

struct sylber_mlp {
    int device = 0, input_dim = 0, output_dim = 0, num_hidden = 0, dims[SYLBER_MLP_MAX_HIDDEN] = {0};
    float* base = nullptr; size_t bytes = 0;
    struct { float *lin_w, *lin_b, *ff1_w, *ff1_b, *ff2_w, *ff2_b, *ln_w, *ln_b; } h[SYLBER_MLP_MAX_HIDDEN];
    float *out_w = nullptr, *out_b = nullptr;
};

extern "C" int sylber_mlp_create(const SylberMlpWeights* w, int device, sylber_mlp_t* out) {
    if (!w || !out) { syl_set_error("sylber_mlp_create", "null argument"); return 1; }
    if (w->num_hidden < 1 || w->num_hidden > SYLBER_MLP_MAX_HIDDEN || w->input_dim % 16 || w->output_dim % 4 || w->input_dim < 16 || w->output_dim < 4) {
        syl_set_error("sylber_mlp_create", "need 1..4 hidden layers, input_dim % 16 == 0, output_dim % 4 == 0"); return 1;
    }
    for (int i = 0; i < w->num_hidden; ++i)
        if (w->hidden_dims[i] != 512 && w->hidden_dims[i] != 768) { syl_set_error("sylber_mlp_create", "hidden dims must be 512 or 768 (LayerNorm kernel)"); return 1; }
    DevGuard dg(device);
    sylber_mlp* m = new sylber_mlp();
    m->device = device; m->input_dim = w->input_dim; m->output_dim = w->output_dim; m->num_hidden = w->num_hidden;
    std::vector<float> host;
    auto add = [&](const float* src, size_t n) { size_t o = (host.size() + 63) & ~(size_t)63; host.resize(o + n); std::copy(src, src + n, host.begin() + o); return o; };
    size_t off[SYLBER_MLP_MAX_HIDDEN][8], o_ow, o_ob;
    int in = w->input_dim;
    for (int i = 0; i < w->num_hidden; ++i) {
        const int d = w->hidden_dims[i];
        m->dims[i] = d;
        const auto& hw = w->hidden[i];
        if (!hw.lin_w || !hw.lin_b || !hw.ff1_w || !hw.ff1_b || !hw.ff2_w || !hw.ff2_b || !hw.ln_w || !hw.ln_b) { delete m; syl_set_error("sylber_mlp_create", "missing tensor"); return 1; }
        off[i][0] = add(hw.lin_w, (size_t)d * in); off[i][1] = add(hw.lin_b, d);
        off[i][2] = add(hw.ff1_w, (size_t)d * d); off[i][3] = add(hw.ff1_b, d);
        off[i][4] = add(hw.ff2_w, (size_t)d * d); off[i][5] = add(hw.ff2_b, d);
        off[i][6] = add(hw.ln_w, d); off[i][7] = add(hw.ln_b, d);
        in = d;
    }
    if (!w->out_w || !w->out_b) { delete m; syl_set_error("sylber_mlp_create", "missing tensor"); return 1; }
    o_ow = add(w->out_w, (size_t)w->output_dim * in); o_ob = add(w->out_b, w->output_dim);
    m->bytes = host.size() * 4;
    if (hipMalloc((void**)&m->base, m->bytes) != hipSuccess || hipMemcpy(m->base, host.data(), m->bytes, hipMemcpyHostToDevice) != hipSuccess) {
        if (m->base) hipFree(m->base);
        delete m; syl_set_error("sylber_mlp_create", "weight upload failed"); return 1;
    }
    for (int i = 0; i < w->num_hidden; ++i) {
        float** f[8] = {&m->h[i].lin_w, &m->h[i].lin_b, &m->h[i].ff1_w, &m->h[i].ff1_b, &m->h[i].ff2_w, &m->h[i].ff2_b, &m->h[i].ln_w, &m->h[i].ln_b};
        for (int j = 0; j < 8; ++j) *f[j] = m->base + off[i][j];
    }
    m->out_w = m->base + o_ow; m->out_b = m->base + o_ob;
    *out = m;
    return 0;
}
extern "C" void sylber_mlp_destroy(sylber_mlp_t m) {
    if (!m) return;
    DevGuard dg(m->device);
    if (m->base) hipFree(m->base);
    delete m;
}

static int mlp_maxdim(const sylber_mlp* m) {
    int d = m->input_dim > m->output_dim ? m->input_dim : m->output_dim;
    for (int i = 0; i < m->num_hidden; ++i) d = d > m->dims[i] ? d : m->dims[i];
    return d;
}
extern "C" int64_t sylber_condition_workspace_floats(sylber_mlp_t m, int32_t B, int32_t S) {
    if (!m || B < 1 || S < 1) return -1;
    const int64_t R = (int64_t)B * S + 1;
    return R * m->input_dim + 3 * R * mlp_maxdim(m) + R * m->output_dim + 256;
}

// rows (b, j < S): the pooled feature of segment j of utterance b (zeros beyond nseg[b]); row B*S: zeros (frames
// outside every segment keep averaged_target_hidden_states = 0, segment_synthesis.py:115)
__global__ __launch_bounds__(256) void cond_gather_kernel(const float* __restrict__ feat, const int32_t* __restrict__ nseg, float* __restrict__ rows,
                                                          int B, int T, int S, int D) {
    const int r = blockIdx.x;
    const bool real = r < B * S;
    const int b = real ? r / S : 0, j = real ? r - b * S : 0;
    const bool ok = real && j < nseg[b];
    for (int c = threadIdx.x; c < D; c += 256) rows[(size_t)r * D + c] = ok ? feat[((size_t)b * T + j) * D + c] : 0.f;
}

// packed batches (sylber_condition_packed / sylber_condition_units_packed): output frame f is frame t = f - F[b] of clip b, where
// pk = [F (B + 1): frame prefix | frames (B) | encoder row of each clip's frame 0 (B)] and b is the last clip with F[b] <= f
__device__ __forceinline__ int cond_clip_of(const int* __restrict__ F, int B, long f) {
    int lo = 0, hi = B - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (F[mid] <= f) lo = mid; else hi = mid - 1; }
    return lo;
}

// one wave per frame: its segment (the LAST one containing it, like the sequential slice assignment at :126), the
// hidden-state norm ((h**2).sum(-1)+1e-8)**.5 (:110), and the masked conditioning row (:138-139)
// T: the pitch of seg / feat (and of hidden and the outputs when pk is null); pk: the packed tables (frames back to back, nf of them)
__global__ __launch_bounds__(256) void cond_scatter_kernel(const float* __restrict__ hidden, const int64_t* __restrict__ seg,
                                                           const int32_t* __restrict__ nseg, const float* __restrict__ feat,
                                                           const float* __restrict__ mlp_rows, int B, int T, int S, int D, int OD, float thr,
                                                           float* __restrict__ avg_out, float* __restrict__ cond_out,
                                                           const int* __restrict__ pk, long nf) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long f = (long)blockIdx.x * 4 + wave;
    if (f >= nf) return;
    int b, t;
    size_t hrow;
    if (pk) {
        b = cond_clip_of(pk, B, f);
        t = (int)(f - pk[b]);
        hrow = (size_t)pk[2 * B + 1 + b] + t;
    } else {
        b = (int)(f / T); t = (int)(f - (long)b * T);
        hrow = (size_t)f;
    }
    const float* h = hidden + hrow * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s = fmaf(h[c], h[c], s);
    s = wave_sum(s);
    const bool silent = sqrtf(s + 1e-8f) < thr;
    int n = nseg[b]; n = n < S ? n : S;
    int j = -1;
    for (int q = lane; q < n; q += 64) {
        const int64_t s0 = seg[((size_t)b * T + q) * 2], s1 = seg[((size_t)b * T + q) * 2 + 1];
        if (t >= s0 && t < s1) j = q;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int oj = __shfl_xor(j, o, 64); j = oj > j ? oj : j; }
    const float* src = mlp_rows + (size_t)(j >= 0 ? b * S + j : B * S) * OD;
    for (int c = lane; c < OD; c += 64) cond_out[(size_t)f * OD + c] = silent ? 0.f : src[c];
    if (avg_out) for (int c = lane; c < D; c += 64) avg_out[(size_t)f * D + c] = j >= 0 ? feat[((size_t)b * T + j) * D + c] : 0.f;
}

// the `MLP` module (segment_synthesis.py:35-53) over R rows: x0 [R, input_dim] -> yo [R, output_dim]; ha/hb/hc: [R, maxdim] each
static int run_mlp(const sylber_mlp* m, const float* x0, int R, float* ha, float* hb, float* hc, float* yo, hipStream_t s) {
    const float* cur = x0; int in = m->input_dim;
    for (int i = 0; i < m->num_hidden; ++i) {
        const int d = m->dims[i];
        GemmArgsF32 g = {};
        g.X = cur; g.ldx = in; g.W = m->h[i].lin_w; g.M = R; g.N = d; g.K = in; g.bias = m->h[i].lin_b; g.out0 = ha; g.ld0 = d;
        if (launch_gemm_f32(g, s)) return 1;                                   // x = Linear(in, d)(x)
        GemmArgsF32 f1 = {};
        f1.X = ha; f1.ldx = d; f1.W = m->h[i].ff1_w; f1.M = R; f1.N = d; f1.K = d; f1.bias = m->h[i].ff1_b; f1.act = ACTF_RELU; f1.out0 = hb; f1.ld0 = d;
        if (launch_gemm_f32(f1, s)) return 1;                                  // relu(linear1(x))   (RFF, :28)
        GemmArgsF32 f2 = {};
        f2.X = hb; f2.ldx = d; f2.W = m->h[i].ff2_w; f2.M = R; f2.N = d; f2.K = d; f2.bias = m->h[i].ff2_b; f2.out0 = hc; f2.ld0 = d;
        if (launch_gemm_f32(f2, s)) return 1;                                  // x2 = linear2(.)
        LnArgs l = {};
        l.in = hc; l.in_bf16 = 0; l.ld_in = d; l.res = ha; l.ld_res = d; l.gamma = m->h[i].ln_w; l.beta = m->h[i].ln_b;
        l.out_f32 = hb; l.ld_f32 = d; l.M = R; l.D = d;
        if (launch_layernorm(l, s)) return 1;                                  // x = norm(x + x2)   (:29-30)
        // the result lives in hb: the next layer's Linear reads it into ha before hb is overwritten again
        cur = hb; in = d;
    }
    GemmArgsF32 go = {};
    go.X = cur; go.ldx = in; go.W = m->out_w; go.M = R; go.N = m->output_dim; go.K = in; go.bias = m->out_b; go.out0 = yo; go.ld0 = m->output_dim;
    return launch_gemm_f32(go, s);
}

extern "C" int sylber_condition(sylber_mlp_t m, const float* hidden_dev, const int64_t* seg_dev, const int32_t* nseg_dev, const float* feat_dev,
                                int32_t B, int32_t T, int32_t S, float norm_thr, float* avg_hidden_dev, float* cond_dev, float* workspace_dev,
                                void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!m || !hidden_dev || !seg_dev || !nseg_dev || !feat_dev || !cond_dev || !workspace_dev) { syl_set_error("sylber_condition", "null argument"); return 1; }
    if (B < 1 || T < 1 || S < 1 || S > T) { syl_set_error("sylber_condition", "need B, T >= 1 and 1 <= S <= T"); return 1; }
    DevGuard dg(m->device);
    const int D = m->input_dim, R = B * S + 1, MD = mlp_maxdim(m);
    float* x0 = workspace_dev;
    float* ha = x0 + (size_t)R * D; float* hb = ha + (size_t)R * MD; float* hc = hb + (size_t)R * MD;
    float* yo = hc + (size_t)R * MD;
    hipLaunchKernelGGL(cond_gather_kernel, dim3(R), dim3(256), 0, s, feat_dev, nseg_dev, x0, B, T, S, D);
    HIP_TRY(hipGetLastError());
    if (run_mlp(m, x0, R, ha, hb, hc, yo, s)) return 1;
    const long frames = (long)B * T;
    hipLaunchKernelGGL(cond_scatter_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, s, hidden_dev, seg_dev, nseg_dev, feat_dev, yo, B, T, S, D,
                       m->output_dim, norm_thr, avg_hidden_dev, cond_dev, nullptr, frames);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the `features is not None` branch of resynthesize (segment_synthesis.py:135-140): the caller hands in the (already
// averaged / decoded) frame features; input = MLP(features), zeroed where ((features**2).sum(-1))**.5 < 1e-4 -- NO 1e-8
// under the root here, and the threshold is the constant 1e-4 (:136-137)
__global__ __launch_bounds__(256) void cond_mask_rows_kernel(const float* __restrict__ feats, const float* __restrict__ mlp_rows, long rows, int D, int OD,
                                                             float* __restrict__ cond_out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long f = (long)blockIdx.x * 4 + wave;
    if (f >= rows) return;
    const float* h = feats + (size_t)f * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s = fmaf(h[c], h[c], s);
    s = wave_sum(s);
    const bool silent = sqrtf(s) < 1e-4f;
    for (int c = lane; c < OD; c += 64) cond_out[(size_t)f * OD + c] = silent ? 0.f : mlp_rows[(size_t)f * OD + c];
}

extern "C" int sylber_condition_features(sylber_mlp_t m, const float* features_dev, int32_t rows, float* cond_dev, float* workspace_dev,
                                         void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!m || !features_dev || !cond_dev || !workspace_dev) { syl_set_error("sylber_condition_features", "null argument"); return 1; }
    if (rows < 1) { syl_set_error("sylber_condition_features", "need rows >= 1"); return 1; }
    DevGuard dg(m->device);
    const int R = rows, MD = mlp_maxdim(m);
    float* ha = workspace_dev; float* hb = ha + (size_t)R * MD; float* hc = hb + (size_t)R * MD; float* yo = hc + (size_t)R * MD;
    if (run_mlp(m, features_dev, R, ha, hb, hc, yo, s)) return 1;
    hipLaunchKernelGGL(cond_mask_rows_kernel, dim3((unsigned)(((long)R + 3) / 4)), dim3(256), 0, s, features_dev, yo, (long)R, m->input_dim,
                       m->output_dim, cond_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- syllable units -> conditioning (the unit half of the speech <-> units loop) --------------------------------------
// Upstream turns units back into frames with expand_feature(avg_fts, durations) (flowmatching.py:873-882) and feeds the
// result to resynthesize(features=...) (segment_synthesis.py:135-140), which runs the MLP on every frame.  All frames of a
// unit carry the same row, so sylber_condition_units runs the MLP once per unit (B*S + 1 rows) and expands afterwards.
// Every MLP row is computed as in a B*T-row launch (launch_gemm_f32 picks no tile by M, the LayerNorm is row-local) and the
// silence decision uses cond_mask_rows_kernel's arithmetic on the same decoded row, so `cond` is bitwise the features path's.

enum { UNITS_BAD_COUNT = 1, UNITS_BAD_FRAMES = 2, UNITS_BAD_ID = 4, UNITS_BAD_SPAN = 8, UNITS_BAD_DURATION = 16, UNITS_BAD_SUM = 32 };

static int units_report(const char* what, const int32_t* flag_dev, hipStream_t s) {
    int32_t flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, flag_dev, sizeof(flag), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!flag) return 0;
    std::string msg;
    if (flag & UNITS_BAD_COUNT) msg += "unit counts must be in [0, S]; ";
    if (flag & UNITS_BAD_FRAMES) msg += "frame counts must be in [1, T]; ";
    if (flag & UNITS_BAD_ID) msg += "unit ids must be in [-1, K) of their codebook; ";
    if (flag & UNITS_BAD_SPAN) msg += "spans must satisfy 0 <= start < end <= T and start >= the previous unit's end; ";
    if (flag & UNITS_BAD_DURATION) msg += "durations must be >= 0; ";
    if (flag & UNITS_BAD_SUM) msg += "every row's durations must sum to T (upstream's torch.stack refuses ragged rows); ";
    msg.resize(msg.size() - 2);
    syl_set_error(what, msg.c_str());
    return 1;
}

// one block (64 lanes) per utterance: every table entry a later kernel reads is checked here first
__global__ __launch_bounds__(64) void units_check_kernel(const int32_t* __restrict__ units, int ncb, int K1, int K2,
                                                         const int32_t* __restrict__ spans, const int32_t* __restrict__ nunits,
                                                         const int32_t* __restrict__ frames, int T, int S, int32_t* __restrict__ flag) {
    const int b = blockIdx.x;
    int bad = 0;
    const int n = nunits[b];
    if (n < 0 || n > S) bad |= UNITS_BAD_COUNT;
    if (frames && (frames[b] < 1 || frames[b] > T)) bad |= UNITS_BAD_FRAMES;
    const int nn = n < 0 ? 0 : (n > S ? S : n);
    for (int j = threadIdx.x; j < nn; j += 64) {
        const size_t u = (size_t)b * S + j;
        const int i1 = units[u * ncb];
        if (i1 < -1 || i1 >= K1) bad |= UNITS_BAD_ID;
        if (ncb > 1) { const int i2 = units[u * ncb + 1]; if (i2 < -1 || i2 >= K2) bad |= UNITS_BAD_ID; }
        const int s0 = spans[u * 2], s1 = spans[u * 2 + 1];
        if (s0 < 0 || s1 <= s0 || s1 > T) bad |= UNITS_BAD_SPAN;
        if (j > 0 && s0 < spans[(u - 1) * 2 + 1]) bad |= UNITS_BAD_SPAN;
    }
    if (bad) atomicOr(flag, bad);
}

// one wave per row: row (b, j < nunits[b]) = c1[i1] (+ c2[i2]) with ids < 0 read as 0 (KMQuantizer.decode's clip), other
// rows and the trailing row B*S zero; keep[r] = !(sqrt(sum x^2) < 1e-4) in cond_mask_rows_kernel's order of operations
__global__ __launch_bounds__(256) void units_gather_kernel(const int32_t* __restrict__ units, int ncb, const float* __restrict__ c1, int K1,
                                                           const float* __restrict__ c2, int K2, const int32_t* __restrict__ nunits,
                                                           int B, int S, int D, float* __restrict__ rows, int32_t* __restrict__ keep) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r > B * S) return;
    const bool real = r < B * S;
    const int b = real ? r / S : 0, j = real ? r - b * S : 0;
    const bool ok = real && j < nunits[b];
    int i1 = ok ? units[(size_t)r * ncb] : 0, i2 = ok && c2 ? units[(size_t)r * ncb + 1] : 0;
    i1 = i1 < 0 ? 0 : (i1 >= K1 ? K1 - 1 : i1);
    i2 = i2 < 0 ? 0 : (i2 >= K2 ? K2 - 1 : i2);
    float s = 0.f;
    for (int c = lane; c < D; c += 64) {
        float v = 0.f;
        if (ok) v = c2 ? c1[(size_t)i1 * D + c] + c2[(size_t)i2 * D + c] : c1[(size_t)i1 * D + c];
        rows[(size_t)r * D + c] = v;
        s = fmaf(v, v, s);
    }
    s = wave_sum(s);
    if (lane == 0) keep[r] = ok && !(sqrtf(s) < 1e-4f);
}

// one wave per frame: the MLP row of the LAST unit whose span holds the frame; 0 where no span does, past frames[b], or
// where the unit's decoded row is silent.  pk (packed): the clips' frames back to back, nf of them (cond_clip_of)
__global__ __launch_bounds__(256) void units_expand_cond_kernel(const int32_t* __restrict__ spans, const int32_t* __restrict__ nunits,
                                                                const int32_t* __restrict__ frames, const int32_t* __restrict__ keep,
                                                                const float* __restrict__ mlp_rows, int B, int T, int S, int OD,
                                                                float* __restrict__ cond_out, const int* __restrict__ pk, long nf) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long f = (long)blockIdx.x * 4 + wave;
    if (f >= nf) return;
    int b, t;
    if (pk) { b = cond_clip_of(pk, B, f); t = (int)(f - pk[b]); }
    else { b = (int)(f / T); t = (int)(f - (long)b * T); }
    int n = nunits[b]; n = n < 0 ? 0 : (n > S ? S : n);
    int j = -1;
    for (int q = lane; q < n; q += 64) {
        const int s0 = spans[((size_t)b * S + q) * 2], s1 = spans[((size_t)b * S + q) * 2 + 1];
        if (t >= s0 && t < s1) j = q;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int oj = __shfl_xor(j, o, 64); j = oj > j ? oj : j; }
    const bool live = j >= 0 && (!frames || t < frames[b]) && keep[b * S + (j >= 0 ? j : 0)];
    const float* src = mlp_rows + (size_t)(b * S + (j >= 0 ? j : 0)) * OD;
    for (int c = lane; c < OD; c += 64) cond_out[(size_t)f * OD + c] = live ? src[c] : 0.f;
}

extern "C" int64_t sylber_condition_units_workspace_floats(sylber_mlp_t m, int32_t B, int32_t S) {
    const int64_t base = sylber_condition_workspace_floats(m, B, S);
    if (base < 0) return -1;
    return base + (int64_t)B * S + 1 + 64;
}

extern "C" int sylber_condition_units(sylber_mlp_t m, const float* c1_dev, int32_t K1, const float* c2_dev, int32_t K2, const int32_t* units_dev,
                                      const int32_t* spans_dev, const int32_t* nunits_dev, const int32_t* frames_dev, int32_t B, int32_t T,
                                      int32_t S, float* cond_dev, float* workspace_dev, void* stream) {
    static const char* what = "sylber_condition_units";
    hipStream_t s = (hipStream_t)stream;
    if (!m || !c1_dev || !units_dev || !spans_dev || !nunits_dev || !cond_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (B < 1 || T < 1 || S < 1 || K1 < 1 || (c2_dev && K2 < 1)) { syl_set_error(what, "need B, T, S, K1 >= 1 (and K2 >= 1 with a second codebook)"); return 1; }
    DevGuard dg(m->device);
    const int D = m->input_dim, R = B * S + 1, MD = mlp_maxdim(m), ncb = c2_dev ? 2 : 1;
    float* x0 = workspace_dev;
    float* ha = x0 + (size_t)R * D; float* hb = ha + (size_t)R * MD; float* hc = hb + (size_t)R * MD;
    float* yo = hc + (size_t)R * MD;
    int32_t* keep = (int32_t*)(yo + (size_t)R * m->output_dim);
    int32_t* flag = keep + R;
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(units_check_kernel, dim3(B), dim3(64), 0, s, units_dev, ncb, K1, K2, spans_dev, nunits_dev, frames_dev, T, S, flag);
    HIP_TRY(hipGetLastError());
    if (units_report(what, flag, s)) return 1;
    hipLaunchKernelGGL(units_gather_kernel, dim3((R + 3) / 4), dim3(256), 0, s, units_dev, ncb, c1_dev, K1, c2_dev, K2, nunits_dev, B, S, D,
                       x0, keep);
    HIP_TRY(hipGetLastError());
    if (run_mlp(m, x0, R, ha, hb, hc, yo, s)) return 1;
    const long frames = (long)B * T;
    hipLaunchKernelGGL(units_expand_cond_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, s, spans_dev, nunits_dev, frames_dev, keep, yo,
                       B, T, S, m->output_dim, cond_dev, nullptr, frames);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- packed batches: the conditioning of each clip's own frames, back to back --------------------------------------------
// Clip b's frame t is output row F_b + t (F_b = frames[0] + ... + frames[b - 1]), so the decoder's packed call reads `cond` as it is.
// The MLP rows and the per-frame decisions are the padded calls' (cond_gather_kernel / units_gather_kernel and run_mlp see the same
// B * S + 1 rows); only the frame -> (clip, t) map of the scatter differs, so each row is bitwise the batch-invariant call's.
extern "C" int64_t sylber_condition_packed_workspace_floats(sylber_mlp_t m, int32_t B, int32_t S) {
    const int64_t base = sylber_condition_units_workspace_floats(m, B, S);
    if (base < 0) return -1;
    return base + 3 * (int64_t)B + 1 + 64;
}

// the host checks of both packed calls and the upload of their table (at the end of the workspace); nf: the frames in all
static int cond_packed_table(const char* what, sylber_mlp_t m, const int32_t* frames_host, const int32_t* offsets_host, int B, int S,
                             float* workspace_dev, int** pk_dev, long& nf, int& fmax, hipStream_t s) {
    std::vector<int32_t> tab(3 * (size_t)B + 1, 0);
    nf = 0; fmax = 0;
    for (int b = 0; b < B; ++b) {
        const int fb = frames_host[b];
        if (fb < 1) { syl_set_error(what, "every clip needs >= 1 frame"); return 1; }
        if (offsets_host && (offsets_host[b] < 0 || (long)offsets_host[b] + fb > offsets_host[b + 1])) {
            syl_set_error(what, "clip b's frames must lie inside [offsets[b], offsets[b + 1])"); return 1;
        }
        tab[b] = (int32_t)nf;
        tab[B + 1 + b] = fb;
        tab[2 * B + 1 + b] = offsets_host ? offsets_host[b] : 0;
        nf += fb;
        fmax = fb > fmax ? fb : fmax;
        if (nf >= (1l << 31)) { syl_set_error(what, "too many frames"); return 1; }
    }
    tab[B] = (int32_t)nf;
    *pk_dev = (int*)(workspace_dev + sylber_condition_units_workspace_floats(m, B, S));
    return launch_upload_ints(*pk_dev, tab.data(), (int)tab.size(), 0, s);
}

extern "C" int sylber_condition_packed(sylber_mlp_t m, const float* hidden_dev, const int32_t* offsets_host, const int32_t* frames_host, int32_t B,
                                       const int64_t* seg_dev, const int32_t* nseg_dev, const float* feat_dev, int32_t K, int32_t S, float norm_thr,
                                       float* avg_hidden_dev, float* cond_dev, float* workspace_dev, void* stream) {
    static const char* what = "sylber_condition_packed";
    hipStream_t s = (hipStream_t)stream;
    if (!m || !hidden_dev || !offsets_host || !frames_host || !seg_dev || !nseg_dev || !feat_dev || !cond_dev || !workspace_dev) {
        syl_set_error(what, "null argument"); return 1;
    }
    if (B < 1 || K < 1 || S < 1 || S > K) { syl_set_error(what, "need B, K >= 1 and 1 <= S <= K"); return 1; }
    for (int b = 0; b < B; ++b)
        if (frames_host[b] > K) { syl_set_error(what, "frame counts must be <= K (the tables' pitch)"); return 1; }
    DevGuard dg(m->device);
    int* pk = nullptr;
    long nf = 0;
    int fmax = 0;
    if (cond_packed_table(what, m, frames_host, offsets_host, B, S, workspace_dev, &pk, nf, fmax, s)) return 1;
    const int D = m->input_dim, R = B * S + 1, MD = mlp_maxdim(m);
    float* x0 = workspace_dev;
    float* ha = x0 + (size_t)R * D; float* hb = ha + (size_t)R * MD; float* hc = hb + (size_t)R * MD;
    float* yo = hc + (size_t)R * MD;
    hipLaunchKernelGGL(cond_gather_kernel, dim3(R), dim3(256), 0, s, feat_dev, nseg_dev, x0, B, K, S, D);
    HIP_TRY(hipGetLastError());
    if (run_mlp(m, x0, R, ha, hb, hc, yo, s)) return 1;
    hipLaunchKernelGGL(cond_scatter_kernel, dim3((unsigned)((nf + 3) / 4)), dim3(256), 0, s, hidden_dev, seg_dev, nseg_dev, feat_dev, yo, B, K, S, D,
                       m->output_dim, norm_thr, avg_hidden_dev, cond_dev, pk, nf);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_condition_units_packed(sylber_mlp_t m, const float* c1_dev, int32_t K1, const float* c2_dev, int32_t K2, const int32_t* units_dev,
                                             const int32_t* spans_dev, const int32_t* nunits_dev, const int32_t* frames_host, int32_t B, int32_t S,
                                             float* cond_dev, float* workspace_dev, void* stream) {
    static const char* what = "sylber_condition_units_packed";
    hipStream_t s = (hipStream_t)stream;
    if (!m || !c1_dev || !units_dev || !spans_dev || !nunits_dev || !frames_host || !cond_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (B < 1 || S < 1 || K1 < 1 || (c2_dev && K2 < 1)) { syl_set_error(what, "need B, S, K1 >= 1 (and K2 >= 1 with a second codebook)"); return 1; }
    DevGuard dg(m->device);
    int* pk = nullptr;
    long nf = 0;
    int T = 0;                                               // the padded call's T: spans are checked against the longest clip
    if (cond_packed_table(what, m, frames_host, nullptr, B, S, workspace_dev, &pk, nf, T, s)) return 1;
    const int D = m->input_dim, R = B * S + 1, MD = mlp_maxdim(m), ncb = c2_dev ? 2 : 1;
    float* x0 = workspace_dev;
    float* ha = x0 + (size_t)R * D; float* hb = ha + (size_t)R * MD; float* hc = hb + (size_t)R * MD;
    float* yo = hc + (size_t)R * MD;
    int32_t* keep = (int32_t*)(yo + (size_t)R * m->output_dim);
    int32_t* flag = keep + R;
    const int32_t* frames_dev = pk + B + 1;
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(units_check_kernel, dim3(B), dim3(64), 0, s, units_dev, ncb, K1, K2, spans_dev, nunits_dev, frames_dev, T, S, flag);
    HIP_TRY(hipGetLastError());
    if (units_report(what, flag, s)) return 1;
    hipLaunchKernelGGL(units_gather_kernel, dim3((R + 3) / 4), dim3(256), 0, s, units_dev, ncb, c1_dev, K1, c2_dev, K2, nunits_dev, B, S, D,
                       x0, keep);
    HIP_TRY(hipGetLastError());
    if (run_mlp(m, x0, R, ha, hb, hc, yo, s)) return 1;
    hipLaunchKernelGGL(units_expand_cond_kernel, dim3((unsigned)((nf + 3) / 4)), dim3(256), 0, s, spans_dev, nunits_dev, frames_dev, keep, yo,
                       B, T, S, m->output_dim, cond_dev, pk, nf);
    HIP_TRY(hipGetLastError());
    return 0;
}

// expand_feature (flowmatching.py:873-882): row b is [feat_0]*d00 + [0]*d01 + [feat_1]*d10 + [0]*d11 + ...; starts[b*S + j]
// = the first frame of unit j, and every row must sum to T (upstream's torch.stack of the per-row results)
__global__ __launch_bounds__(64) void expand_check_kernel(const int32_t* __restrict__ dur, int S, int T, int32_t* __restrict__ starts,
                                                          int32_t* __restrict__ flag) {
    if (threadIdx.x) return;
    const int b = blockIdx.x;
    long cum = 0;
    int bad = 0;
    for (int j = 0; j < S; ++j) {
        const int d0 = dur[((size_t)b * S + j) * 2], d1 = dur[((size_t)b * S + j) * 2 + 1];
        if (d0 < 0 || d1 < 0) bad |= UNITS_BAD_DURATION;
        starts[(size_t)b * S + j] = (int32_t)(cum < 0 ? 0 : (cum > T ? T : cum));
        cum += (long)(d0 > 0 ? d0 : 0) + (d1 > 0 ? d1 : 0);
    }
    if (cum != T) bad |= UNITS_BAD_SUM;
    if (bad) atomicOr(flag, bad);
}
__global__ __launch_bounds__(256) void expand_units_kernel(const float* __restrict__ feats, const int32_t* __restrict__ dur,
                                                           const int32_t* __restrict__ starts, int B, int S, int D, int T, float* __restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long f = (long)blockIdx.x * 4 + wave;
    if (f >= (long)B * T) return;
    const int b = (int)(f / T), t = (int)(f - (long)b * T);
    int j = -1;
    for (int q = lane; q < S; q += 64) {
        const int s0 = starts[(size_t)b * S + q];
        if (t >= s0 && t < s0 + dur[((size_t)b * S + q) * 2]) j = q;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int oj = __shfl_xor(j, o, 64); j = oj > j ? oj : j; }
    const float* src = feats + ((size_t)b * S + (j >= 0 ? j : 0)) * D;
    for (int c = lane; c < D; c += 64) out[(size_t)f * D + c] = j >= 0 ? src[c] : 0.f;
}

extern "C" int sylber_expand_units(const float* feats_dev, const int32_t* durations_dev, int32_t B, int32_t S, int32_t D, int32_t T,
                                   float* out_dev, int32_t* workspace_dev, void* stream) {
    static const char* what = "sylber_expand_units";
    hipStream_t s = (hipStream_t)stream;
    if (!feats_dev || !durations_dev || !out_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (B < 1 || S < 1 || D < 1 || T < 1) { syl_set_error(what, "need B, S, D, T >= 1"); return 1; }
    int32_t* starts = workspace_dev;
    int32_t* flag = starts + (size_t)B * S;
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(expand_check_kernel, dim3(B), dim3(64), 0, s, durations_dev, S, T, starts, flag);
    HIP_TRY(hipGetLastError());
    if (units_report(what, flag, s)) return 1;
    const long frames = (long)B * T;
    hipLaunchKernelGGL(expand_units_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, s, feats_dev, durations_dev, starts, B, S, D, T,
                       out_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Fitting k-means unit codebooks on the device (sylber_amd/kmeans.py): the three steps of Lloyd's algorithm with k-means++ seeding
// that the inference kernels of downstream.hip cannot carry at corpus scale.
//   * fused assign: the exact-fp32 MFMA contraction of sylber_km_assign with a running per-row arg-min in the epilogue, so that the
//     [n, K] dot matrix is never written (at 15 M rows x 20 000 centroids it would be 1.2 TB);
//   * centroid update: fp64 sums of each cluster's rows in fixed-size pieces, added left to right, one rounding to fp32;
//   * k-means++ seeding: distance update, fp64 prefix sums and the inverse-CDF pick, all on the device (no host round trip per center).
// Every result is independent of the launch geometry: reductions run in fixed orders, and the arg-min's index tie-break does not
// depend on the order in which centroid tiles are visited.
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include <climits>

// ---- fused assign ----------------------------------------------------------------------------------------------------------------
// A workgroup owns 128 rows and walks all centroids in 128-wide tiles; 4 waves as 2 x 2, each with 2 x 2 fragments of 32 x 32.
// K step 16 through LDS.  The contraction must give the bits of gemm_f32_kernel (fp32_path.hip) that sylber_km_assign runs: there
// v_mfma_f32_32x32x2_f32 number i of a K step contracts the pair (2i, 2i + 1), lanes 0-31 supplying k = 2i and lanes 32-63 k = 2i + 1,
// i.e. an ascending fmaf chain from 0.  To feed that pair order from ds_read_b128, each LDS row holds the 16 k values of a step as
// [0 2 4 .. 14 | 1 3 5 .. 15]: a lane of half h reads eight floats from position 8 h and gets k = 2 i + h for i = 0..7.
constexpr int KA_BM = 128, KA_BN = 128, KA_BK = 16, KA_LD = 20;    // LDS row stride 20 floats (80 B: 16-byte aligned, staggered banks)

__device__ __forceinline__ bool km_better(float v, int i, float bv, int bi) { return v < bv || (v == bv && i < bi); }

__global__ __launch_bounds__(256) void km_fused_assign_kernel(const float* __restrict__ x, int n, const float* __restrict__ c, int K, int D,
                                                              const float* __restrict__ cn, const float* __restrict__ xsq,
                                                              const int32_t* __restrict__ prev, int32_t* __restrict__ idx,
                                                              float* __restrict__ dmin, double* __restrict__ part_inertia,
                                                              int* __restrict__ part_changed) {
    __shared__ __attribute__((aligned(16))) float xs[KA_BM * KA_LD];
    __shared__ __attribute__((aligned(16))) float cs[KA_BN * KA_LD];
    __shared__ float cns[KA_BN];
    __shared__ float rbv[2][KA_BM];
    __shared__ int rbi[2][KA_BM];
    __shared__ double red_d[4];
    __shared__ int red_c[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * KA_BM;
    // staging: thread -> operand row tid >> 1, k values [8 (tid & 1), 8 (tid & 1) + 8) of the step
    const int sr = tid >> 1, sh = (tid & 1) * 8;
    int xm = m0 + sr; xm = xm < n ? xm : n - 1;
    const float* xrow = x + (size_t)xm * D + sh;
    float* xdst = xs + sr * KA_LD + (sh >> 1);
    float* cdst = cs + sr * KA_LD + (sh >> 1);
    const int frow = lane & 31, fh = lane >> 5;
    const int ksteps = D / KA_BK, ntiles = (K + KA_BN - 1) / KA_BN, T = ksteps * ntiles;

    float best[2] = {INFINITY, INFINITY};
    int besti[2] = {INT_MAX, INT_MAX};
    f32x16_t acc[2][2];
    float4 xa, xb, ca, cb;
    auto fetch = [&](int t) {
        const int tile = t / ksteps, k0 = (t - tile * ksteps) * KA_BK;
        int cr = tile * KA_BN + sr; cr = cr < K ? cr : K - 1;
        const float* crow = c + (size_t)cr * D + sh + k0;
        xa = *(const float4*)(xrow + k0); xb = *(const float4*)(xrow + k0 + 4);
        ca = *(const float4*)crow; cb = *(const float4*)(crow + 4);
    };
    fetch(0);
    for (int t = 0; t < T; ++t) {
        const int tile = t / ksteps, ks = t - tile * ksteps, n0 = tile * KA_BN;
        if (ks == 0) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        }
        __syncthreads();                                   // the previous step's fragments (and the previous tile's cns) are read
        *(float4*)xdst = make_float4(xa.x, xa.z, xb.x, xb.z);
        *(float4*)(xdst + 8) = make_float4(xa.y, xa.w, xb.y, xb.w);
        *(float4*)cdst = make_float4(ca.x, ca.z, cb.x, cb.z);
        *(float4*)(cdst + 8) = make_float4(ca.y, ca.w, cb.y, cb.w);
        if (ks == 0 && tid < KA_BN) cns[tid] = n0 + tid < K ? cn[n0 + tid] : 0.f;
        __syncthreads();
        if (t + 1 < T) fetch(t + 1);                       // in flight during this step's MFMAs
        f32x4_t xf[2][2], cf[2][2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const float* xp = xs + (wm * 64 + f * 32 + frow) * KA_LD + fh * 8;
            const float* cp = cs + (wn * 64 + f * 32 + frow) * KA_LD + fh * 8;
            xf[f][0] = *(const f32x4_t*)xp; xf[f][1] = *(const f32x4_t*)(xp + 4);
            cf[f][0] = *(const f32x4_t*)cp; cf[f][1] = *(const f32x4_t*)(cp + 4);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int fm = 0; fm < 2; ++fm)
#pragma unroll
                for (int fn = 0; fn < 2; ++fn)
                    acc[fm][fn] = __builtin_amdgcn_mfma_f32_32x32x2f32(cf[fn][i >> 2][i & 3], xf[fm][i >> 2][i & 3], acc[fm][fn], 0, 0, 0);
        if (ks == ksteps - 1) {
            // epilogue of a centroid tile: lane holds row wm*64 + fm*32 + frow against centroids wn*64 + fn*32 + 8g + 4fh + e
#pragma unroll
            for (int fm = 0; fm < 2; ++fm)
#pragma unroll
                for (int fn = 0; fn < 2; ++fn)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int cl = wn * 64 + fn * 32 + 8 * g + 4 * fh + e;
                            if (n0 + cl >= K) continue;
                            const float d = fmaf(-2.0f, acc[fm][fn][4 * g + e], cns[cl]);
                            if (km_better(d, n0 + cl, best[fm], besti[fm])) { best[fm] = d; besti[fm] = n0 + cl; }
                        }
        }
    }
    // the two lane halves hold other centroids of the same rows, then the two waves wn = 0, 1
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
        const float ov = __shfl_xor(best[fm], 32, 64);
        const int oi = __shfl_xor(besti[fm], 32, 64);
        if (km_better(ov, oi, best[fm], besti[fm])) { best[fm] = ov; besti[fm] = oi; }
        if (fh == 0) { rbv[wn][wm * 64 + fm * 32 + frow] = best[fm]; rbi[wn][wm * 64 + fm * 32 + frow] = besti[fm]; }
    }
    __syncthreads();
    double v = 0.0;
    int ch = 0;
    if (tid < KA_BM && m0 + tid < n) {
        const int r = m0 + tid;
        float bv = rbv[0][tid]; int bi = rbi[0][tid];
        if (km_better(rbv[1][tid], rbi[1][tid], bv, bi)) { bv = rbv[1][tid]; bi = rbi[1][tid]; }
        idx[r] = bi;
        if (dmin) dmin[r] = bv;
        const double e = (double)xsq[r] + (double)bv;
        v = e > 0.0 ? e : 0.0;
        ch = prev ? (prev[r] != bi) : 0;
    }
    // fixed-order block sums: the wave butterfly, then waves 0..3 in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { v += __shfl_xor(v, o, 64); ch += __shfl_xor(ch, o, 64); }
    if (lane == 0) { red_d[wave] = v; red_c[wave] = ch; }
    __syncthreads();
    if (tid == 0) {
        part_inertia[blockIdx.x] = ((red_d[0] + red_d[1]) + red_d[2]) + red_d[3];
        part_changed[blockIdx.x] = red_c[0] + red_c[1] + red_c[2] + red_c[3];
    }
}

// the per-workgroup partials, summed in a fixed order: thread t sequentially over p = t, t + 256, ..., then the block in a fixed tree
__global__ __launch_bounds__(256) void km_partials_kernel(const double* __restrict__ part_inertia, const int* __restrict__ part_changed, int nb,
                                                          double* __restrict__ inertia, int64_t* __restrict__ changed) {
    __shared__ double sd[256];
    __shared__ long long sc[256];
    const int tid = threadIdx.x;
    double v = 0.0;
    long long ch = 0;
    for (int p = tid; p < nb; p += 256) { v += part_inertia[p]; ch += part_changed[p]; }
    sd[tid] = v; sc[tid] = ch;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { sd[tid] += sd[tid + s]; sc[tid] += sc[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        if (inertia) *inertia = sd[0];
        if (changed) *changed = sc[0];
    }
}

static int64_t km_blocks(int32_t n) { return ((int64_t)n + KA_BM - 1) / KA_BM; }

extern "C" int64_t sylber_kmeans_assign_workspace_floats(int32_t n, int32_t K, int32_t D) {
    if (n < 1 || K < 1 || D < 1) return -1;
    // cn [K] | xsq [n] | part_inertia [nb] doubles | part_changed [nb] ints, each piece 64-float aligned
    auto al = [](int64_t f) { return (f + 63) / 64 * 64; };
    return al(K) + al(n) + al(2 * km_blocks(n)) + al(km_blocks(n)) + 64;
}

extern "C" int sylber_kmeans_assign(const float* x_dev, int32_t n, const float* c_dev, int32_t K, int32_t D, int32_t* idx_dev, float* dmin_dev,
                                    double* inertia_dev, const int32_t* prev_idx_dev, int64_t* changed_dev, float* workspace_dev, void* stream) {
    static const char* what = "sylber_kmeans_assign";
    hipStream_t s = (hipStream_t)stream;
    if (!x_dev || !c_dev || !idx_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1 || K < 1 || D < 16 || D % 16) { syl_set_error(what, "need n, K >= 1 and D a multiple of 16"); return 1; }
    if (changed_dev && !prev_idx_dev) { syl_set_error(what, "changed_dev needs prev_idx_dev"); return 1; }
    auto al = [](int64_t f) { return (f + 63) / 64 * 64; };
    const int64_t nb = km_blocks(n);
    float* cn = workspace_dev;
    float* xsq = cn + al(K);
    double* part_inertia = (double*)(xsq + al(n));
    int* part_changed = (int*)(xsq + al(n) + al(2 * nb));
    if (launch_km_sqnorm(c_dev, cn, K, D, s) || launch_km_sqnorm(x_dev, xsq, n, D, s)) return 1;
    hipLaunchKernelGGL(km_fused_assign_kernel, dim3((unsigned)nb), dim3(256), 0, s, x_dev, n, c_dev, K, D, cn, xsq, prev_idx_dev, idx_dev,
                       dmin_dev, part_inertia, part_changed);
    HIP_TRY(hipGetLastError());
    if (inertia_dev || changed_dev) {
        hipLaunchKernelGGL(km_partials_kernel, dim3(1), dim3(256), 0, s, part_inertia, part_changed, (int)nb, inertia_dev,
                           prev_idx_dev ? changed_dev : nullptr);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" int sylber_km_normalize(const float* x_dev, int32_t n, int32_t D, float* y_dev, void* stream) {
    if (!x_dev || !y_dev || n < 1 || D < 1) { syl_set_error("sylber_km_normalize", "bad argument"); return 1; }
    return launch_km_normalize(x_dev, y_dev, n, D, (hipStream_t)stream);
}

// ---- centroid update -------------------------------------------------------------------------------------------------------------
// order[] lists the rows grouped by label, ascending within a cluster (a stable sort of the labels).  Cluster k's rows are cut into
// pieces of KU_PIECE; piece sums are fp64 in ascending row order, then each cluster adds its pieces left to right and divides once.
constexpr int KU_PIECE = 512;

__global__ __launch_bounds__(256) void km_count_kernel(const int32_t* __restrict__ idx, int n, int K, int* __restrict__ counts) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int k = idx[r];
    if (k >= 0 && k < K) atomicAdd(&counts[k], 1);        // integer atomics: the counts do not depend on their order
}

// one workgroup: offs[k] = rows before cluster k, poffs[k] = pieces before cluster k (k = 0..K), both exclusive prefix sums
__global__ __launch_bounds__(1024) void km_offsets_kernel(const int* __restrict__ counts, int K, int* __restrict__ offs, int* __restrict__ poffs) {
    __shared__ int sa[1024], sb[1024];
    const int tid = threadIdx.x, per = (K + 1023) / 1024;
    const int k0 = tid * per, k1 = k0 + per < K ? k0 + per : K;
    int a = 0, b = 0;
    for (int k = k0; k < k1; ++k) { a += counts[k]; b += (counts[k] + KU_PIECE - 1) / KU_PIECE; }
    sa[tid] = a; sb[tid] = b;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                   // inclusive Hillis-Steele scan of the per-thread totals
        const int va = tid >= o ? sa[tid - o] : 0, vb = tid >= o ? sb[tid - o] : 0;
        __syncthreads();
        sa[tid] += va; sb[tid] += vb;
        __syncthreads();
    }
    a = sa[tid] - a; b = sb[tid] - b;                      // exclusive
    for (int k = k0; k < k1; ++k) { offs[k] = a; poffs[k] = b; a += counts[k]; b += (counts[k] + KU_PIECE - 1) / KU_PIECE; }
    if (tid == 1023) { offs[K] = sa[1023]; poffs[K] = sb[1023]; }
}

// grid (pieces upper bound, ceil(D / 256)): piece p of cluster k (poffs[k] <= p < poffs[k + 1]), column j = one thread
__global__ __launch_bounds__(256) void km_piece_sum_kernel(const float* __restrict__ x, int D, const int64_t* __restrict__ order,
                                                           const int* __restrict__ offs, const int* __restrict__ poffs, int K,
                                                           double* __restrict__ part) {
    const int p = blockIdx.x;
    if (p >= poffs[K]) return;
    int lo = 0, hi = K - 1;                                // the last k with poffs[k] <= p (clusters without pieces share its poffs)
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (poffs[mid] <= p) lo = mid; else hi = mid - 1; }
    const int k = lo;
    const int start = offs[k] + (p - poffs[k]) * KU_PIECE;
    const int end = start + KU_PIECE < offs[k + 1] ? start + KU_PIECE : offs[k + 1];
    const int j = blockIdx.y * 256 + threadIdx.x;
    if (j >= D) return;
    double s = 0.0;
    for (int q = start; q < end; ++q) s += (double)x[(size_t)order[q] * D + j];
    part[(size_t)p * D + j] = s;
}

__global__ __launch_bounds__(256) void km_centroid_kernel(const double* __restrict__ part, int D, const int* __restrict__ offs,
                                                          const int* __restrict__ poffs, float* __restrict__ c) {
    const int k = blockIdx.x, j = blockIdx.y * 256 + threadIdx.x;
    const int cnt = offs[k + 1] - offs[k];
    if (cnt == 0 || j >= D) return;                        // an empty cluster keeps its centroid
    double s = 0.0;
    for (int p = poffs[k]; p < poffs[k + 1]; ++p) s += part[(size_t)p * D + j];
    c[(size_t)k * D + j] = (float)(s / (double)cnt);
}

static int64_t ku_pieces(int32_t n, int32_t K) { return ((int64_t)n + KU_PIECE - 1) / KU_PIECE + K; }

extern "C" int64_t sylber_kmeans_update_workspace_bytes(int32_t n, int32_t K, int32_t D) {
    if (n < 1 || K < 1 || D < 1) return -1;
    // offs [K + 1] | poffs [K + 1], padded to 256 B | piece sums [pieces][D] doubles
    return ((int64_t)(2 * K + 2) * 4 + 255) / 256 * 256 + ku_pieces(n, K) * D * 8;
}

extern "C" int sylber_kmeans_update(const float* x_dev, int32_t n, int32_t D, const int32_t* idx_dev, const int64_t* order_dev, int32_t K,
                                    float* c_dev, int32_t* counts_dev, void* workspace_dev, void* stream) {
    static const char* what = "sylber_kmeans_update";
    hipStream_t s = (hipStream_t)stream;
    if (!x_dev || !idx_dev || !order_dev || !c_dev || !counts_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1 || K < 1 || D < 1) { syl_set_error(what, "need n, K, D >= 1"); return 1; }
    int* offs = (int*)workspace_dev;
    int* poffs = offs + K + 1;
    double* part = (double*)((char*)workspace_dev + ((int64_t)(2 * K + 2) * 4 + 255) / 256 * 256);
    HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)K * 4, s));
    hipLaunchKernelGGL(km_count_kernel, dim3((n + 255) / 256), dim3(256), 0, s, idx_dev, n, K, counts_dev);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(km_offsets_kernel, dim3(1), dim3(1024), 0, s, counts_dev, K, offs, poffs);
    HIP_TRY(hipGetLastError());
    const unsigned cols = (unsigned)((D + 255) / 256);
    hipLaunchKernelGGL(km_piece_sum_kernel, dim3((unsigned)ku_pieces(n, K), cols), dim3(256), 0, s, x_dev, D, order_dev, offs, poffs, K, part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(km_centroid_kernel, dim3((unsigned)K, cols), dim3(256), 0, s, part, D, offs, poffs, c_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- k-means++ seeding -------------------------------------------------------------------------------------------------------------
// dist[r] = min over the chosen centers of sum_j (x_rj - c_j)^2, an fmaf chain in ascending j on the differences (duplicates give 0).
// prefix(r) = (sum of the 256-row block sums before r's block) + (inclusive scan of dist inside the block); block sums are the last
// element of that same in-block scan, so the two levels agree.  The next center is the first r with prefix(r) > u[j] * total.
constexpr int KP_B = 256;

__device__ __forceinline__ double kp_block_scan(double v, double* sh) {     // inclusive Hillis-Steele over 256 threads
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int o = 1; o < KP_B; o <<= 1) {
        const double a = tid >= o ? sh[tid - o] : 0.0;
        __syncthreads();
        sh[tid] += a;
        __syncthreads();
    }
    return sh[tid];
}

__global__ __launch_bounds__(256) void kp_init_kernel(const double* __restrict__ u, int n, int32_t* __restrict__ chosen, float* __restrict__ dist,
                                                      int32_t* __restrict__ status) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < n) dist[r] = INFINITY;
    if (r == 0) {
        long long c0 = (long long)floor(u[0] * (double)n);
        chosen[0] = (int32_t)(c0 < 0 ? 0 : (c0 >= n ? n - 1 : c0));
        *status = 0;
    }
}

// after center j - 1: update dist, write the block sums
__global__ __launch_bounds__(256) void kp_dist_kernel(const float* __restrict__ x, int n, int D, const int32_t* __restrict__ chosen, int j,
                                                      float* __restrict__ dist, double* __restrict__ bsum, const int32_t* __restrict__ status) {
    __shared__ double sh[KP_B];
    if (*status) return;
    const int r = blockIdx.x * KP_B + threadIdx.x;
    const float* cp = x + (size_t)chosen[j - 1] * D;
    float v = 0.f;
    if (r < n) {
        const float* xp = x + (size_t)r * D;
        float s = 0.f;
        for (int q = 0; q < D; q += 4) {
            const float4 a = *(const float4*)(xp + q), b = *(const float4*)(cp + q);
            float d = a.x - b.x; s = fmaf(d, d, s);
            d = a.y - b.y; s = fmaf(d, d, s);
            d = a.z - b.z; s = fmaf(d, d, s);
            d = a.w - b.w; s = fmaf(d, d, s);
        }
        v = fminf(dist[r], s);
        dist[r] = v;
    }
    const double inc = kp_block_scan((double)v, sh);
    if (threadIdx.x == KP_B - 1) bsum[blockIdx.x] = inc;
}

// one workgroup of 1024: pick center j from the block sums and the winning block's dist
__global__ __launch_bounds__(1024) void kp_select_kernel(const float* __restrict__ dist, int n, const double* __restrict__ bsum, int nb,
                                                         const double* __restrict__ u, int j, int32_t* __restrict__ chosen,
                                                         int32_t* __restrict__ status) {
    __shared__ double sh[1024];
    __shared__ int first, last;
    __shared__ double base;
    const int tid = threadIdx.x;
    if (*status) return;
    const int per = (nb + 1023) / 1024, b0 = tid * per, b1 = b0 + per < nb ? b0 + per : nb;
    double t = 0.0;
    for (int b = b0; b < b1; ++b) t += bsum[b];
    sh[tid] = t;
    if (tid == 0) { first = INT_MAX; last = -1; }
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const double a = tid >= o ? sh[tid - o] : 0.0;
        __syncthreads();
        sh[tid] += a;
        __syncthreads();
    }
    const double total = sh[1023];
    if (!(total > 0.0)) {                                  // every row coincides with a chosen center
        if (tid == 0) { *status = 1; chosen[j] = -1; }
        return;
    }
    const double thr = u[j] * total;
    double pre = sh[tid] - t;
    for (int b = b0; b < b1; ++b) {
        if (pre + bsum[b] > thr) { atomicMin(&first, b); break; }
        pre += bsum[b];
    }
    for (int b = b1 - 1; b >= b0; --b) if (bsum[b] > 0.0) { atomicMax(&last, b); break; }
    __syncthreads();
    const int blk = first != INT_MAX ? first : last;
    __syncthreads();                                       // everybody has read first / last before they are reset below
    // the prefix before block blk, in the same order as above (the owner thread's running sum)
    if (tid == blk / per) {
        double p = sh[tid] - t;
        for (int b = b0; b < blk; ++b) p += bsum[b];
        base = p;
    }
    if (tid == 0) { first = INT_MAX; last = -1; }
    __syncthreads();
    // in-block scan, the same Hillis-Steele as kp_dist_kernel's block sums (threads 0..255)
    const int r = blk * KP_B + tid;
    const double dv = (tid < KP_B && r < n) ? (double)dist[r] : 0.0;
    if (tid < KP_B) sh[tid] = dv;
    __syncthreads();
    for (int o = 1; o < KP_B; o <<= 1) {
        const double a = (tid < KP_B && tid >= o) ? sh[tid - o] : 0.0;
        __syncthreads();
        if (tid < KP_B) sh[tid] += a;
        __syncthreads();
    }
    if (tid < KP_B && r < n) {
        if (base + sh[tid] > thr) atomicMin(&first, tid);
        if (dv > 0.0) atomicMax(&last, tid);
    }
    __syncthreads();
    if (tid == 0) chosen[j] = blk * KP_B + (first != INT_MAX ? first : last);
}

extern "C" int64_t sylber_kmeans_seed_workspace_floats(int32_t n) {
    if (n < 1) return -1;
    return ((int64_t)n + 63) / 64 * 64 + 2 * (((int64_t)n + KP_B - 1) / KP_B) + 64;    // dist [n] | block sums [n / 256] doubles
}

extern "C" int sylber_kmeans_seed(const float* x_dev, int32_t n, int32_t D, int32_t K, const double* u_dev, int32_t* chosen_dev,
                                  int32_t* status_dev, float* workspace_dev, void* stream) {
    static const char* what = "sylber_kmeans_seed";
    hipStream_t s = (hipStream_t)stream;
    if (!x_dev || !u_dev || !chosen_dev || !status_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1 || K < 1 || K > n || D < 4 || D % 4) { syl_set_error(what, "need 1 <= K <= n and D a multiple of 4"); return 1; }
    const int nb = (n + KP_B - 1) / KP_B;
    float* dist = workspace_dev;
    double* bsum = (double*)(workspace_dev + ((int64_t)n + 63) / 64 * 64);
    hipLaunchKernelGGL(kp_init_kernel, dim3((n + 255) / 256), dim3(256), 0, s, u_dev, n, chosen_dev, dist, status_dev);
    HIP_TRY(hipGetLastError());
    for (int j = 1; j < K; ++j) {
        hipLaunchKernelGGL(kp_dist_kernel, dim3(nb), dim3(KP_B), 0, s, x_dev, n, D, chosen_dev, j, dist, bsum, status_dev);
        hipLaunchKernelGGL(kp_select_kernel, dim3(1), dim3(1024), 0, s, dist, n, bsum, nb, u_dev, j, chosen_dev, status_dev);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

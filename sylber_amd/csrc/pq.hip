// Product-quantized syllable search (sylber_amd/pq.py: PQSyllableIndex): a row of D floats is stored as M bytes, byte m the nearest of
// the 256 centroids of sub-space m (columns [m dsub, (m + 1) dsub), dsub = D / M); a query scores a row by M look-ups in its own
// [M, 256] table of partial scores (asymmetric distance computation).
//   * pq_encode_kernel: code[j][m] = argmin_c fmaf(-2, x_j[slice m] . C[m][c], ||C[m][c]||^2), the dot product an explicit ascending fmaf
//     chain from 0 -- the chain v_mfma_f32_32x32x2_f32 performs in km_fused_assign_kernel (kmeans.hip), so the codes are
//     sylber_kmeans_assign's labels of the sliced rows, bit for bit -- ties to the smaller c.  One launch walks all M sub-spaces of a
//     block of rows.  A sub-row without any comparable distance (a NaN in it) gets code 0 and marks its row in the byte mask.
//   * pq_lut_kernel: lut[i][m][c] = fmaf(-2, q_i[slice m] . C[m][c], cnorm[m][c] or 0), the same chain.
//   * pq_scan_kernel: a workgroup holds the tables of QB queries in LDS (M KiB each) and walks one split of the code rows, a lane per
//     row: t = the fp32 sum of the row's M table entries in ascending m, one order for every row, split and block, so t's bits are a
//     function of (query, row) alone.  Rows that beat a query's current worst go through an LDS strip into that query's sorted top
//     list (kn_insert); the per-split lists are merged with knn_lists.h.  The table gather is a random 4-byte LDS read inside a 1 KiB
//     region: bank conflicts of a few ways are part of the algorithm (any layout that avoids them changes the add order).
//   * pq_decode_kernel: out[j][slice m] = C[m][code[j][m]].
//   * ivfpq_scan_kernel (IVFPQSyllableIndex): the same t over the codes of the lists a query probes only; a workgroup holds ONE query's
//     table and walks the lists of one split of the query's probe slots; the order is (t, original id).  Its residual variant (the
//     codes are those of x_j - centroid[list of j]) keeps the one table per query -- the inner products -- and adds what the table
//     cannot hold: t = (u + a[i][slot]) + nrm_j, a = -2 q . centroid (ivfpq_list_terms_kernel, a block-uniform scalar per list) and
//     nrm_j = ||centroid + decode(code_j)||^2 (ivfpq_recon_norms_kernel, one coalesced 4-byte load per lane).
#include "kernels.h"
#include "../../include/sylber_hip.h"
#include "knn_tile.h"
#include "knn_lists.h"

constexpr int PQ_KSUB = 256;                               // centroids per sub-space: one byte per code
constexpr int PQ_MAX_M = 64;
constexpr int PQ_T = 1024;                                 // threads of a scan workgroup = code rows of a tile: four waves per SIMD keep
                                                           // the 4-byte LDS gathers in flight
constexpr int PQ_LDS = 160 * 1024;                         // LDS of a CU; one workgroup takes as many tables as fit
constexpr int PQ_LDS_FIXED = 256;                          // flags and query groups
constexpr int PQ_TARGET_BLOCKS = 512, PQ_MIN_TILES = 4;    // automatic splits: about this many workgroups, at least these tiles each
constexpr int PE_R = 32;                                   // rows of an encode workgroup

static bool pq_geometry(int D, int M) { return M >= 1 && M <= PQ_MAX_M && D >= 16 && D % M == 0 && (D / M) % 16 == 0; }

// ---- encode ----------------------------------------------------------------------------------------------------------------------
// grid ceil(n / 32): thread c owns centroid c of the current sub-space and carries 32 rows' chains; the rows' 16 values of a K step
// are staged in LDS and read as broadcasts.
__global__ __launch_bounds__(256) void pq_encode_kernel(const float* __restrict__ x, int n, int D, const float* __restrict__ cb,
                                                        const float* __restrict__ cnorm, int M, uint8_t* __restrict__ code,
                                                        uint8_t* __restrict__ bad) {
    __shared__ __attribute__((aligned(16))) float xs[PE_R][16];
    __shared__ float rv[4][PE_R];
    __shared__ int ri[4][PE_R];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r0 = blockIdx.x * PE_R, dsub = D / M;
    int xr = r0 + (tid >> 2); xr = xr < n ? xr : n - 1;
    const float* xsrc = x + (size_t)xr * D + (tid & 3) * 4;
    int isbad = 0;                                         // thread r < 32: row r0 + r has a sub-row without a code
    for (int m = 0; m < M; ++m) {
        const float* crow = cb + ((size_t)m * PQ_KSUB + tid) * dsub;
        float acc[PE_R];
#pragma unroll
        for (int r = 0; r < PE_R; ++r) acc[r] = 0.f;
        for (int k0 = 0; k0 < dsub; k0 += 16) {
            __syncthreads();                               // the previous step's xs (and the previous sub-space's rv / ri) are read
            if (tid < PE_R * 4) *(float4*)&xs[tid >> 2][(tid & 3) * 4] = *(const float4*)(xsrc + m * dsub + k0);
            float cv[16];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float4 c4 = *(const float4*)(crow + k0 + 4 * e);
                cv[4 * e] = c4.x; cv[4 * e + 1] = c4.y; cv[4 * e + 2] = c4.z; cv[4 * e + 3] = c4.w;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < PE_R; ++r) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float4 x4 = *(const float4*)&xs[r][4 * e];
                    acc[r] = __builtin_fmaf(x4.x, cv[4 * e], acc[r]);
                    acc[r] = __builtin_fmaf(x4.y, cv[4 * e + 1], acc[r]);
                    acc[r] = __builtin_fmaf(x4.z, cv[4 * e + 2], acc[r]);
                    acc[r] = __builtin_fmaf(x4.w, cv[4 * e + 3], acc[r]);
                }
            }
        }
        const float cn = cnorm[m * PQ_KSUB + tid];
#pragma unroll
        for (int r = 0; r < PE_R; ++r) {
            const float d = __builtin_fmaf(-2.0f, acc[r], cn);
            float bv = d == d ? d : INFINITY;              // a NaN distance never wins (km_better never takes it)
            int bi = d == d ? tid : INT_MAX;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (kn_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if (lane == 0) { rv[wave][r] = bv; ri[wave][r] = bi; }
        }
        __syncthreads();
        if (tid < PE_R && r0 + tid < n) {
            float bv = rv[0][tid]; int bi = ri[0][tid];
#pragma unroll
            for (int w = 1; w < 4; ++w) if (kn_better(rv[w][tid], ri[w][tid], bv, bi)) { bv = rv[w][tid]; bi = ri[w][tid]; }
            if (bi == INT_MAX) { bi = 0; isbad = 1; }
            code[(size_t)(r0 + tid) * M + m] = (uint8_t)bi;
        }
    }
    if (tid < PE_R && r0 + tid < n) bad[r0 + tid] = (uint8_t)isbad;
}

// ---- decode ----------------------------------------------------------------------------------------------------------------------
// list / cent non-null (IVF-PQ residual codes): out[j] = cent[list[j]] + that, one fp32 addition per element; a row in no list gets none.
__global__ __launch_bounds__(256) void pq_decode_kernel(const uint8_t* __restrict__ code, int64_t quads, const float* __restrict__ cb, int M,
                                                        int D, float* __restrict__ out, const int32_t* __restrict__ list,
                                                        const float* __restrict__ cent, int nlist) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;     // one float4 of the output
    if (e >= quads) return;
    const int dsub = D / M, dq = D / 4;
    const int64_t j = e / dq;
    const int col = (int)(e - j * dq) * 4, m = col / dsub;
    const int c = code[j * M + m];
    float4 v = *(const float4*)(cb + ((size_t)m * PQ_KSUB + c) * dsub + (col - m * dsub));
    if (list) {
        const int l = list[j];
        if (l >= 0 && l < nlist) {
            const float4 g = *(const float4*)(cent + (size_t)l * D + col);
            v.x = g.x + v.x; v.y = g.y + v.y; v.z = g.z + v.z; v.w = g.w + v.w;
        }
    }
    *(float4*)(out + j * D + col) = v;
}

// ---- table -----------------------------------------------------------------------------------------------------------------------
// grid n x M: workgroup (i, m), thread c.  cnorm null: the inner-product table.
__global__ __launch_bounds__(256) void pq_lut_kernel(const float* __restrict__ q, int D, const float* __restrict__ cb,
                                                     const float* __restrict__ cnorm, int M, float* __restrict__ lut) {
    const int64_t b = blockIdx.x;
    const int64_t i = b / M;
    const int m = (int)(b - i * M), c = threadIdx.x, dsub = D / M;
    const float* qr = q + i * D + (size_t)m * dsub;
    const float* cr = cb + ((size_t)m * PQ_KSUB + c) * dsub;
    float dot = 0.f;
    for (int k = 0; k < dsub; k += 4) {
        const float4 a = *(const float4*)(qr + k), v = *(const float4*)(cr + k);
        dot = __builtin_fmaf(a.x, v.x, dot);
        dot = __builtin_fmaf(a.y, v.y, dot);
        dot = __builtin_fmaf(a.z, v.z, dot);
        dot = __builtin_fmaf(a.w, v.w, dot);
    }
    lut[b * PQ_KSUB + c] = __builtin_fmaf(-2.0f, dot, cnorm ? cnorm[m * PQ_KSUB + c] : 0.f);
}

// ---- scan ------------------------------------------------------------------------------------------------------------------------
// the queries of a workgroup: the most tables that fit beside their strips and top lists
static size_t pq_lds_per_query(int M, int m) { return (size_t)M * PQ_KSUB * 4 + (size_t)PQ_T * 4 + (size_t)m * 8; }
static int pq_block_queries(int M, int m) {
    const int fit = (int)((PQ_LDS - PQ_LDS_FIXED) / pq_lds_per_query(M, m));
    for (int qb : {8, 6, 4, 3, 2}) if (fit >= qb) return qb;
    return 1;
}
static int pq_scan_splits(int64_t n, int64_t N, int QB, int64_t splits) {
    const int64_t nb = (n + QB - 1) / QB, tiles = (N + PQ_T - 1) / PQ_T;
    int64_t S = splits;
    if (S <= 0) {
        S = (PQ_TARGET_BLOCKS + nb - 1) / nb;
        const int64_t cap = tiles / PQ_MIN_TILES;
        S = S < cap ? S : cap;
    }
    S = S < tiles ? S : tiles;
    S = S < 65535 ? S : 65535;
    return (int)(S < 1 ? 1 : S);
}

template <int VEC> __device__ __forceinline__ void pq_load(const uint8_t* p, uint32_t (&w)[4]) { w[0] = *p; }
template <> __device__ __forceinline__ void pq_load<4>(const uint8_t* p, uint32_t (&w)[4]) { w[0] = *(const uint32_t*)p; }
template <> __device__ __forceinline__ void pq_load<16>(const uint8_t* p, uint32_t (&w)[4]) {
    const uint4 v = *(const uint4*)p;
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}

// grid (ceil(n / QB), S): split sp walks the tiles [sp * tiles / S, (sp + 1) * tiles / S) of PQ_T code rows.  VEC bytes of a code row
// per load (VEC divides M; 16 where M % 16 == 0).  Writes the sorted best m of every valid query over its tiles to ps / pi [n][S][m];
// entries that did not fill stay (+inf, INT_MAX).
template <int QB, int VEC>
__global__ __launch_bounds__(PQ_T) void pq_scan_kernel(const float* __restrict__ lut, int n, const uint8_t* __restrict__ code,
                                                       const uint8_t* __restrict__ bad, int N, int M, int m,
                                                       const int32_t* __restrict__ qgrp, const int32_t* __restrict__ xgrp, int S,
                                                       float* __restrict__ ps, int32_t* __restrict__ pi) {
    extern __shared__ __attribute__((aligned(16))) float pq_smem[];
    const int tsz = M * PQ_KSUB;
    float* tab = pq_smem;                                  // [QB][M][256] the queries' tables
    float* strip = tab + QB * tsz;                         // [QB][PQ_T] a tile's scores of a flagged query (NaN = not admissible)
    float* ls = strip + QB * PQ_T;                         // [QB][m] sorted scores
    int* li = (int*)(ls + QB * m);                         // [QB][m] their rows
    int* flags = li + QB * m;                              // [2][QB] by tile parity: the tile may hold a candidate of query q
    int* qgs = flags + 2 * QB;                             // [QB] the queries' groups
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int q0 = blockIdx.x * QB, sp = blockIdx.y;
    const int nq = n - q0 < QB ? n - q0 : QB;
    const int tiles = (N + PQ_T - 1) / PQ_T;
    const int tlo = (int)((int64_t)sp * tiles / S), thi = (int)((int64_t)(sp + 1) * tiles / S);
#pragma unroll
    for (int q = 0; q < QB; ++q) {                         // queries past n copy the last one: they gather, but never flag
        const float* src = lut + (size_t)(q < nq ? q0 + q : n - 1) * tsz;
        for (int e = tid * 4; e < tsz; e += PQ_T * 4) *(float4*)(tab + q * tsz + e) = *(const float4*)(src + e);
    }
    for (int e = tid; e < QB * m; e += PQ_T) { ls[e] = INFINITY; li[e] = INT_MAX; }
    if (tid < 2 * QB) flags[tid] = 0;
    if (tid < QB) qgs[tid] = qgrp ? qgrp[tid < nq ? q0 + tid : n - 1] : 0;
    __syncthreads();
    for (int tile = tlo; tile < thi; ++tile) {
        const int base = tile * PQ_T, row = base + tid;
        const int r = row < N ? row : N - 1;
        const uint8_t* cr = code + (size_t)r * M;
        float t[QB];
#pragma unroll
        for (int q = 0; q < QB; ++q) t[q] = -0.0f;         // -0 + v = v for every v, -0 included: the sum starts at its first entry
        for (int mb = 0; mb < M; mb += VEC) {
            uint32_t w[4];
            pq_load<VEC>(cr + mb, w);
#pragma unroll
            for (int b = 0; b < VEC; ++b) {
                const float* tp = tab + (mb + b) * PQ_KSUB + ((w[b >> 2] >> (8 * (b & 3))) & 255u);
#pragma unroll
                for (int q = 0; q < QB; ++q) t[q] += tp[q * tsz];
            }
        }
        const bool live = row < N && !(bad && bad[r]);
        const int g = xgrp ? xgrp[r] : 0;
        int* fl_w = flags + (tile & 1) * QB;
#pragma unroll
        for (int q = 0; q < QB; ++q) {
            const bool adm = live && q < nq && !(xgrp && g == qgs[q]);
            t[q] = adm ? t[q] : __builtin_nanf("");
            if (t[q] <= ls[q * m + m - 1]) fl_w[q] = 1;    // a superset of the exact (t, row) test; NaN never passes
        }
        __syncthreads();
        int fl = 0;
#pragma unroll
        for (int q = 0; q < QB; ++q) fl |= fl_w[q] << q;   // block-uniform; the next tile flags the other parity
        if (!fl) continue;
#pragma unroll
        for (int q = 0; q < QB; ++q) if ((fl >> q) & 1) strip[q * PQ_T + tid] = t[q];
        __syncthreads();
        if (tid < QB) fl_w[tid] = 0;
        if (wave < QB && ((fl >> wave) & 1)) {             // wave q puts the survivors of query q into its list one at a time
            float* lsr = ls + wave * m;
            int* lir = li + wave * m;
            const float* sq = strip + wave * PQ_T;
            for (int h = 0; h < PQ_T / 64; ++h) {
                uint64_t bal = __ballot(kn_better(sq[h * 64 + lane], base + h * 64 + lane, lsr[m - 1], lir[m - 1]));
                while (bal) {
                    const int c = __ffsll((unsigned long long)bal) - 1;
                    bal &= bal - 1;
                    kn_insert(lsr, lir, m, lane, sq[h * 64 + c], base + h * 64 + c);
                }
            }
        }
        __syncthreads();                                   // the lists are complete before the next tile reads its thresholds
    }
    __syncthreads();
    for (int q = 0; q < nq; ++q) {
        const size_t o = ((size_t)(q0 + q) * S + sp) * m;
        for (int e = tid; e < m; e += PQ_T) { ps[o + e] = ls[q * m + e]; pi[o + e] = li[q * m + e]; }
    }
}

// the merged lists as candidates: the (+inf, INT_MAX) fillers become (+inf, -1)
__global__ __launch_bounds__(256) void pq_cand_kernel(const float* __restrict__ ls, const int32_t* __restrict__ li, int64_t tot,
                                                      float* __restrict__ t, int32_t* __restrict__ cand) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tot) return;
    const int j = li[e];
    t[e] = j == INT_MAX ? INFINITY : ls[e];
    cand[e] = j == INT_MAX ? -1 : j;
}

template <int QB, int VEC>
static int pq_launch_scan(const float* lut, int n, const uint8_t* code, const uint8_t* bad, int N, int M, int m, const int32_t* qg,
                          const int32_t* xg, int S, float* ps, int32_t* pi, hipStream_t s) {
    static PerDeviceOnce once;
    if (once.need())
        HIP_TRY(hipFuncSetAttribute((const void*)pq_scan_kernel<QB, VEC>, hipFuncAttributeMaxDynamicSharedMemorySize, PQ_LDS));
    const size_t lds = QB * pq_lds_per_query(M, m) + PQ_LDS_FIXED;
    hipLaunchKernelGGL((pq_scan_kernel<QB, VEC>), dim3((unsigned)((n + QB - 1) / QB), (unsigned)S), dim3(PQ_T), lds, s, lut, n, code, bad, N, M,
                       m, qg, xg, S, ps, pi);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int QB, typename... A> static int pq_launch_scan_vec(int M, A... a) {
    if (M % 16 == 0) return pq_launch_scan<QB, 16>(a...);
    if (M % 4 == 0) return pq_launch_scan<QB, 4>(a...);
    return pq_launch_scan<QB, 1>(a...);
}

extern "C" int sylber_pq_encode(const float* x_dev, int32_t n, int32_t D, const float* cb_dev, const float* cnorm_dev, int32_t M,
                                uint8_t* code_dev, uint8_t* bad_dev, void* stream) {
    static const char* what = "sylber_pq_encode";
    if (!x_dev || !cb_dev || !cnorm_dev || !code_dev || !bad_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1) { syl_set_error(what, "need n >= 1"); return 1; }
    if (!pq_geometry(D, M)) { syl_set_error(what, "need 1 <= M <= 64, D % M == 0 and (D / M) % 16 == 0"); return 1; }
    hipLaunchKernelGGL(pq_encode_kernel, dim3((unsigned)((n + PE_R - 1) / PE_R)), dim3(256), 0, (hipStream_t)stream, x_dev, n, D, cb_dev,
                       cnorm_dev, M, code_dev, bad_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_pq_decode(const uint8_t* code_dev, int32_t n, const float* cb_dev, int32_t M, int32_t D, float* out_dev, void* stream) {
    static const char* what = "sylber_pq_decode";
    if (!code_dev || !cb_dev || !out_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1) { syl_set_error(what, "need n >= 1"); return 1; }
    if (!pq_geometry(D, M)) { syl_set_error(what, "need 1 <= M <= 64, D % M == 0 and (D / M) % 16 == 0"); return 1; }
    const int64_t quads = (int64_t)n * D / 4, blocks = (quads + 255) / 256;
    if (blocks > INT32_MAX) { syl_set_error(what, "n x D is too large: decode in pieces"); return 1; }
    hipLaunchKernelGGL(pq_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, code_dev, quads, cb_dev, M, D, out_dev,
                       (const int32_t*)nullptr, (const float*)nullptr, 0);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_pq_lut(const float* q_dev, int32_t n, int32_t D, const float* cb_dev, const float* cnorm_dev, int32_t M, int32_t metric,
                             float* lut_dev, void* stream) {
    static const char* what = "sylber_pq_lut";
    if (!q_dev || !cb_dev || !lut_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1) { syl_set_error(what, "need n >= 1"); return 1; }
    if (!pq_geometry(D, M)) { syl_set_error(what, "need 1 <= M <= 64, D % M == 0 and (D / M) % 16 == 0"); return 1; }
    if (metric != SYLBER_KNN_L2 && metric != SYLBER_KNN_IP) { syl_set_error(what, "unknown metric"); return 1; }
    if (metric == SYLBER_KNN_L2 && !cnorm_dev) { syl_set_error(what, "the L2 metric needs cnorm_dev"); return 1; }
    if ((int64_t)n * M > INT32_MAX) { syl_set_error(what, "n x M is too large: use smaller query chunks"); return 1; }
    hipLaunchKernelGGL(pq_lut_kernel, dim3((unsigned)((int64_t)n * M)), dim3(PQ_KSUB), 0, (hipStream_t)stream, q_dev, D, cb_dev,
                       metric == SYLBER_KNN_L2 ? cnorm_dev : nullptr, M, lut_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int64_t sylber_pq_workspace_bytes(int32_t n, int32_t N, int32_t M, int32_t m, int32_t splits) {
    if (n < 1 || N < 1 || M < 1 || M > PQ_MAX_M || m < 1 || m > KN_KMAX) return -1;
    return kn_partials_bytes(n, pq_scan_splits(n, N, pq_block_queries(M, m), splits), m);      // the S partial lists (KnPartials)
}

extern "C" int sylber_pq_scan(const float* lut_dev, int32_t n, const uint8_t* code_dev, const uint8_t* bad_dev, int32_t N, int32_t M, int32_t m,
                              const int32_t* q_group_dev, const int32_t* db_group_dev, int32_t splits, float* t_dev, int32_t* cand_dev,
                              void* workspace_dev, void* stream) {
    static const char* what = "sylber_pq_scan";
    hipStream_t s = (hipStream_t)stream;
    if (!lut_dev || !code_dev || !t_dev || !cand_dev || !workspace_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1 || N < 1) { syl_set_error(what, "need n, N >= 1"); return 1; }
    if (M < 1 || M > PQ_MAX_M) { syl_set_error(what, "need 1 <= M <= 64"); return 1; }
    if (m < 1 || m > KN_KMAX) { syl_set_error(what, "need 1 <= m <= 128"); return 1; }
    if (!q_group_dev != !db_group_dev) { syl_set_error(what, "q_group_dev and db_group_dev go together"); return 1; }
    const int QB = pq_block_queries(M, m);
    const int S = pq_scan_splits(n, N, QB, splits);
    char* w = (char*)workspace_dev;
    KnPartials p = kn_partials_carve(w, n, S, m);
    int rc = 1;
    switch (QB) {
        case 8: rc = pq_launch_scan_vec<8>(M, lut_dev, n, code_dev, bad_dev, N, M, m, q_group_dev, db_group_dev, S, p.s0, p.i0, s); break;
        case 6: rc = pq_launch_scan_vec<6>(M, lut_dev, n, code_dev, bad_dev, N, M, m, q_group_dev, db_group_dev, S, p.s0, p.i0, s); break;
        case 4: rc = pq_launch_scan_vec<4>(M, lut_dev, n, code_dev, bad_dev, N, M, m, q_group_dev, db_group_dev, S, p.s0, p.i0, s); break;
        case 3: rc = pq_launch_scan_vec<3>(M, lut_dev, n, code_dev, bad_dev, N, M, m, q_group_dev, db_group_dev, S, p.s0, p.i0, s); break;
        case 2: rc = pq_launch_scan_vec<2>(M, lut_dev, n, code_dev, bad_dev, N, M, m, q_group_dev, db_group_dev, S, p.s0, p.i0, s); break;
        default: rc = pq_launch_scan_vec<1>(M, lut_dev, n, code_dev, bad_dev, N, M, m, q_group_dev, db_group_dev, S, p.s0, p.i0, s); break;
    }
    if (rc) return rc;
    if (kn_merge_lists(p, n, S, m, s)) return 1;
    const int64_t tot = (int64_t)n * m;
    hipLaunchKernelGGL(pq_cand_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, p.s0, p.i0, tot, t_dev, cand_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- scan of the probed lists (IVF-PQ) -------------------------------------------------------------------------------------------
// One workgroup per (query, split of its probe slots): a table is fetched once per split, whatever lists the query probes, and the
// codes of lists that many queries probe come from L2 / Infinity Cache.
constexpr int IPQ_T = 512;                                 // threads = code rows of a tile.  LDS of a workgroup: the table (M KiB) + two
                                                           // strips (4 KiB) + the top list (8 m <= 1 KiB) + 16 bytes: 53 KiB at M = 48,
                                                           // three workgroups per CU (159 KiB of 160) = 24 waves, six per SIMD for
                                                           // the 4-byte gathers; 69 KiB at M = 64 (two workgroups, four waves per SIMD);
                                                           // from M <= 35 on the 32 waves of a CU allow four workgroups
constexpr int IPQ_LDS_FIXED = 16;                          // the two tile flags
constexpr int IPQ_MAX_NPROBE = 128;

static size_t ipq_lds_bytes(int M, int m) { return (size_t)M * PQ_KSUB * 4 + (size_t)IPQ_T * 8 + (size_t)m * 8 + IPQ_LDS_FIXED; }
static int ipq_splits(int64_t n, int nprobe, int splits) {
    int64_t S = splits > 0 ? splits : (PQ_TARGET_BLOCKS + n - 1) / n;
    S = S < nprobe ? S : nprobe;
    return (int)(S < 1 ? 1 : S);
}

// grid (n, S): split sp of query i walks the lists of its probe slots [sp * nprobe / S, (sp + 1) * nprobe / S), a list at a time in
// tiles of IPQ_T positions (a slot < 0 or without rows costs nothing).  code / bad / rid / xgrp are in position order (list by list,
// ascending original id within a list).  Writes the sorted best m (t, original id) of the split to ps / pi [n][S][m]; entries that
// did not fill stay (+inf, INT_MAX).  RES (residual codes): t = (u + lterm[i][slot]) + rterm[position] (rterm null: t = u + lterm),
// added before the threshold test; lterm is read once per list, rterm with the lane's own position (clamped like the code row).
template <int VEC, bool RES>
__global__ __launch_bounds__(IPQ_T) void ivfpq_scan_kernel(const float* __restrict__ lut, const int32_t* __restrict__ probe, int nprobe,
                                                          const int32_t* __restrict__ off, int nlist, const uint8_t* __restrict__ code,
                                                          const uint8_t* __restrict__ bad, const int32_t* __restrict__ rid, int NL, int M,
                                                          int m, const int32_t* __restrict__ qgrp, const int32_t* __restrict__ xgrp, int S,
                                                          const float* __restrict__ lterm, const float* __restrict__ rterm,
                                                          float* __restrict__ ps, int32_t* __restrict__ pi) {
    extern __shared__ __attribute__((aligned(16))) float ipq_smem[];
    const int tsz = M * PQ_KSUB;
    float* tab = ipq_smem;                                 // [M][256] the query's table
    float* strip = tab + tsz;                              // [IPQ_T] a flagged tile's scores (NaN = no candidate)
    int* sid = (int*)(strip + IPQ_T);                      // [IPQ_T] their original ids
    float* ls = (float*)(sid + IPQ_T);                     // [m] sorted scores
    int* li = (int*)(ls + m);                              // [m] their original ids
    int* flags = li + m;                                   // [2] by tile parity: the tile may hold a candidate
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = blockIdx.x, sp = blockIdx.y;
    const int slo = (int)((int64_t)sp * nprobe / S), shi = (int)((int64_t)(sp + 1) * nprobe / S);
    const float* src = lut + (size_t)i * tsz;
    for (int e = tid * 4; e < tsz; e += IPQ_T * 4) *(float4*)(tab + e) = *(const float4*)(src + e);
    for (int e = tid; e < m; e += IPQ_T) { ls[e] = INFINITY; li[e] = INT_MAX; }
    if (tid < 2) flags[tid] = 0;
    const int qg = qgrp ? qgrp[i] : 0;
    __syncthreads();
    int par = 0;
    for (int slot = slo; slot < shi; ++slot) {
        const int l = probe[(size_t)i * nprobe + slot];    // block-uniform
        if (l < 0 || l >= nlist) continue;
        const int lo = off[l], hi = off[l + 1];
        if (lo < 0 || hi > NL || lo >= hi) continue;
        const float a = RES ? lterm[(size_t)i * nprobe + slot] : 0.f;      // block-uniform
        for (int base = lo; base < hi; base += IPQ_T, par ^= 1) {
            const int pos = base + tid;
            const int r = pos < hi ? pos : hi - 1;
            const uint8_t* cr = code + (size_t)r * M;
            float t = -0.0f;                               // -0 + v = v for every v, -0 included: the sum starts at its first entry
            for (int mb = 0; mb < M; mb += VEC) {
                uint32_t w[4];
                pq_load<VEC>(cr + mb, w);
#pragma unroll
                for (int b = 0; b < VEC; ++b) t += tab[(mb + b) * PQ_KSUB + ((w[b >> 2] >> (8 * (b & 3))) & 255u)];
            }
            if (RES) {
                t += a;
                if (rterm) t += rterm[r];
            }
            // The order is (t, ORIGINAL id): positions ascend with the id inside a list, not across lists.  The id -- with the mask
            // and the group -- is fetched for the rows that pass the threshold only: a superset of the exact (t, id) test (NaN
            // never passes) that few rows pass once the list has filled, where a fetch for every row would add 9 bytes to the M
            // bytes of each code row.
            bool pass = pos < hi && t <= ls[m - 1];
            int id = 0;
            if (pass) {
                pass = !(bad && bad[r]) && !(xgrp && xgrp[r] == qg);
                if (pass) id = rid[r];
            }
            if (pass) flags[par] = 1;
            __syncthreads();
            if (!flags[par]) continue;                     // block-uniform; the next tile flags the other parity
            strip[tid] = pass ? t : __builtin_nanf("");
            sid[tid] = id;
            __syncthreads();
            if (tid == 0) flags[par] = 0;
            if (wave == 0) {                               // one wave puts the survivors into the list one at a time
                for (int h = 0; h < IPQ_T / 64; ++h) {
                    uint64_t bal = __ballot(kn_better(strip[h * 64 + lane], sid[h * 64 + lane], ls[m - 1], li[m - 1]));
                    while (bal) {
                        const int c = __ffsll((unsigned long long)bal) - 1;
                        bal &= bal - 1;
                        kn_insert(ls, li, m, lane, strip[h * 64 + c], sid[h * 64 + c]);
                    }
                }
            }
            __syncthreads();                               // the list is complete before the next tile reads its threshold
        }
    }
    const size_t o = ((size_t)i * S + sp) * m;
    for (int e = tid; e < m; e += IPQ_T) { ps[o + e] = ls[e]; pi[o + e] = li[e]; }
}

template <int VEC, bool RES>
static int ipq_launch_scan(const float* lut, int n, const int32_t* probe, int nprobe, const int32_t* off, int nlist, const uint8_t* code,
                           const uint8_t* bad, const int32_t* rid, int NL, int M, int m, const int32_t* qg, const int32_t* xg, int S,
                           const float* lterm, const float* rterm, float* ps, int32_t* pi, hipStream_t s) {
    static PerDeviceOnce once;
    if (once.need())
        HIP_TRY(hipFuncSetAttribute((const void*)ivfpq_scan_kernel<VEC, RES>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)ipq_lds_bytes(PQ_MAX_M, KN_KMAX)));
    hipLaunchKernelGGL((ivfpq_scan_kernel<VEC, RES>), dim3((unsigned)n, (unsigned)S), dim3(IPQ_T), ipq_lds_bytes(M, m), s, lut, probe, nprobe,
                       off, nlist, code, bad, rid, NL, M, m, qg, xg, S, lterm, rterm, ps, pi);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int64_t sylber_ivfpq_workspace_bytes(int32_t n, int32_t nprobe, int32_t m, int32_t splits) {
    if (n < 1 || nprobe < 1 || nprobe > IPQ_MAX_NPROBE || m < 1 || m > KN_KMAX || splits < 0) return -1;
    return kn_partials_bytes(n, ipq_splits(n, nprobe, splits), m);      // the S partial lists (KnPartials)
}

// the body of both scans: list_term_dev null = the codes of the rows themselves
template <bool RES>
static int ipq_scan(const char* what, const float* lut_dev, int32_t n, const int32_t* probe_dev, int32_t nprobe, const int32_t* list_offsets_dev,
                    int32_t nlist, const uint8_t* code_dev, const uint8_t* bad_dev, const int32_t* row_id_dev, int32_t N_listed, int32_t M,
                    int32_t m, const int32_t* q_group_dev, const int32_t* row_group_dev, int32_t splits, const float* list_term_dev,
                    const float* row_term_dev, float* t_dev, int32_t* cand_dev, void* workspace_dev, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!lut_dev || !probe_dev || !list_offsets_dev || !code_dev || !row_id_dev || !t_dev || !cand_dev || !workspace_dev ||
        (RES && !list_term_dev)) {
        syl_set_error(what, "null argument");
        return 1;
    }
    if (n < 1) { syl_set_error(what, "need n >= 1"); return 1; }
    if (M < 1 || M > PQ_MAX_M) { syl_set_error(what, "need 1 <= M <= 64"); return 1; }
    if (m < 1 || m > KN_KMAX) { syl_set_error(what, "need 1 <= m <= 128"); return 1; }
    if (nprobe < 1 || nprobe > IPQ_MAX_NPROBE) { syl_set_error(what, "need 1 <= nprobe <= 128"); return 1; }
    if (nlist < 1) { syl_set_error(what, "need nlist >= 1"); return 1; }
    if (N_listed < 0) { syl_set_error(what, "need N_listed >= 0"); return 1; }
    if (!q_group_dev != !row_group_dev) { syl_set_error(what, "q_group_dev and row_group_dev go together"); return 1; }
    if (splits < 0) { syl_set_error(what, "need splits >= 0"); return 1; }
    const int S = ipq_splits(n, nprobe, splits);
    char* w = (char*)workspace_dev;
    KnPartials p = kn_partials_carve(w, n, S, m);
    int rc;
    if (M % 16 == 0)
        rc = ipq_launch_scan<16, RES>(lut_dev, n, probe_dev, nprobe, list_offsets_dev, nlist, code_dev, bad_dev, row_id_dev, N_listed, M, m,
                                      q_group_dev, row_group_dev, S, list_term_dev, row_term_dev, p.s0, p.i0, s);
    else if (M % 4 == 0)
        rc = ipq_launch_scan<4, RES>(lut_dev, n, probe_dev, nprobe, list_offsets_dev, nlist, code_dev, bad_dev, row_id_dev, N_listed, M, m,
                                     q_group_dev, row_group_dev, S, list_term_dev, row_term_dev, p.s0, p.i0, s);
    else
        rc = ipq_launch_scan<1, RES>(lut_dev, n, probe_dev, nprobe, list_offsets_dev, nlist, code_dev, bad_dev, row_id_dev, N_listed, M, m,
                                     q_group_dev, row_group_dev, S, list_term_dev, row_term_dev, p.s0, p.i0, s);
    if (rc) return rc;
    if (kn_merge_lists(p, n, S, m, s)) return 1;
    const int64_t tot = (int64_t)n * m;                    // the finish of sylber_pq_scan: the (+inf, INT_MAX) fillers become (+inf, -1)
    hipLaunchKernelGGL(pq_cand_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, p.s0, p.i0, tot, t_dev, cand_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_ivfpq_scan(const float* lut_dev, int32_t n, const int32_t* probe_dev, int32_t nprobe, const int32_t* list_offsets_dev,
                                 int32_t nlist, const uint8_t* code_dev, const uint8_t* bad_dev, const int32_t* row_id_dev, int32_t N_listed,
                                 int32_t M, int32_t m, const int32_t* q_group_dev, const int32_t* row_group_dev, int32_t splits, float* t_dev,
                                 int32_t* cand_dev, void* workspace_dev, void* stream) {
    return ipq_scan<false>("sylber_ivfpq_scan", lut_dev, n, probe_dev, nprobe, list_offsets_dev, nlist, code_dev, bad_dev, row_id_dev, N_listed,
                           M, m, q_group_dev, row_group_dev, splits, nullptr, nullptr, t_dev, cand_dev, workspace_dev, stream);
}

extern "C" int sylber_ivfpq_scan_residual(const float* lut_dev, int32_t n, const int32_t* probe_dev, int32_t nprobe,
                                          const int32_t* list_offsets_dev, int32_t nlist, const uint8_t* code_dev, const uint8_t* bad_dev,
                                          const int32_t* row_id_dev, int32_t N_listed, int32_t M, int32_t m, const int32_t* q_group_dev,
                                          const int32_t* row_group_dev, int32_t splits, const float* list_term_dev, const float* row_term_dev,
                                          float* t_dev, int32_t* cand_dev, void* workspace_dev, void* stream) {
    return ipq_scan<true>("sylber_ivfpq_scan_residual", lut_dev, n, probe_dev, nprobe, list_offsets_dev, nlist, code_dev, bad_dev, row_id_dev,
                          N_listed, M, m, q_group_dev, row_group_dev, splits, list_term_dev, row_term_dev, t_dev, cand_dev, workspace_dev,
                          stream);
}

// ---- residual codes: what the one table per query cannot hold ---------------------------------------------------------------------
// thread e = pair (i, slot): a = -2 (q_i . cent[probe]), the dot product the ascending fmaf chain from 0 (knn_rerank_kernel's)
__global__ __launch_bounds__(256) void ivfpq_list_terms_kernel(const float* __restrict__ q, int64_t pairs, int D, const float* __restrict__ cent,
                                                               int nlist, const int32_t* __restrict__ probe, int nprobe,
                                                               float* __restrict__ a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= pairs) return;
    const int l = probe[e];
    float v = 0.f;
    if (l >= 0 && l < nlist) {
        const float* qr = q + (e / nprobe) * D;
        const float* cr = cent + (size_t)l * D;
        float dot = 0.f;
        for (int c = 0; c < D; c += 4) {
            const float4 x = *(const float4*)(qr + c), y = *(const float4*)(cr + c);
            dot = __builtin_fmaf(x.x, y.x, dot);
            dot = __builtin_fmaf(x.y, y.y, dot);
            dot = __builtin_fmaf(x.z, y.z, dot);
            dot = __builtin_fmaf(x.w, y.w, dot);
        }
        v = -2.0f * dot;
    }
    a[e] = v;
}

// thread j = row j: nrm = fmaf(xhat[e], xhat[e], nrm) from 0 in ascending e, xhat[e] = cent[list[j]][e] + cb[m][code[j][m]][e - m dsub]
__global__ __launch_bounds__(256) void ivfpq_recon_norms_kernel(const uint8_t* __restrict__ code, int n, const int32_t* __restrict__ list,
                                                                const float* __restrict__ cent, int nlist, const float* __restrict__ cb,
                                                                int M, int D, float* __restrict__ nrm) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int dsub = D / M, l = list[j];
    const float* gr = l >= 0 && l < nlist ? cent + (size_t)l * D : nullptr;
    float acc = 0.f;
    for (int m = 0; m < M; ++m) {
        const float* cr = cb + ((size_t)m * PQ_KSUB + code[(size_t)j * M + m]) * dsub;
        for (int k = 0; k < dsub; k += 4) {
            float4 v = *(const float4*)(cr + k);
            if (gr) {
                const float4 g = *(const float4*)(gr + m * dsub + k);
                v.x = g.x + v.x; v.y = g.y + v.y; v.z = g.z + v.z; v.w = g.w + v.w;
            }
            acc = __builtin_fmaf(v.x, v.x, acc);
            acc = __builtin_fmaf(v.y, v.y, acc);
            acc = __builtin_fmaf(v.z, v.z, acc);
            acc = __builtin_fmaf(v.w, v.w, acc);
        }
    }
    nrm[j] = acc;
}

extern "C" int sylber_ivfpq_list_terms(const float* q_dev, int32_t n, int32_t D, const float* centroid_dev, int32_t nlist,
                                       const int32_t* probe_dev, int32_t nprobe, float* list_term_dev, void* stream) {
    static const char* what = "sylber_ivfpq_list_terms";
    if (!q_dev || !centroid_dev || !probe_dev || !list_term_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1) { syl_set_error(what, "need n >= 1"); return 1; }
    if (D < 4 || D % 4) { syl_set_error(what, "need D >= 4, a multiple of 4"); return 1; }
    if (nlist < 1) { syl_set_error(what, "need nlist >= 1"); return 1; }
    if (nprobe < 1 || nprobe > IPQ_MAX_NPROBE) { syl_set_error(what, "need 1 <= nprobe <= 128"); return 1; }
    const int64_t pairs = (int64_t)n * nprobe;
    hipLaunchKernelGGL(ivfpq_list_terms_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q_dev, pairs, D,
                       centroid_dev, nlist, probe_dev, nprobe, list_term_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_ivfpq_recon_norms(const uint8_t* code_dev, int32_t n, const int32_t* list_dev, const float* centroid_dev, int32_t nlist,
                                        const float* cb_dev, int32_t M, int32_t D, float* nrm_dev, void* stream) {
    static const char* what = "sylber_ivfpq_recon_norms";
    if (!code_dev || !list_dev || !centroid_dev || !cb_dev || !nrm_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1) { syl_set_error(what, "need n >= 1"); return 1; }
    if (nlist < 1) { syl_set_error(what, "need nlist >= 1"); return 1; }
    if (!pq_geometry(D, M)) { syl_set_error(what, "need 1 <= M <= 64, D % M == 0 and (D / M) % 16 == 0"); return 1; }
    hipLaunchKernelGGL(ivfpq_recon_norms_kernel, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, code_dev, n,
                       list_dev, centroid_dev, nlist, cb_dev, M, D, nrm_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int sylber_ivfpq_decode(const uint8_t* code_dev, int32_t n, const int32_t* list_dev, const float* centroid_dev, int32_t nlist,
                                   const float* cb_dev, int32_t M, int32_t D, float* out_dev, void* stream) {
    static const char* what = "sylber_ivfpq_decode";
    if (!code_dev || !list_dev || !centroid_dev || !cb_dev || !out_dev) { syl_set_error(what, "null argument"); return 1; }
    if (n < 1) { syl_set_error(what, "need n >= 1"); return 1; }
    if (nlist < 1) { syl_set_error(what, "need nlist >= 1"); return 1; }
    if (!pq_geometry(D, M)) { syl_set_error(what, "need 1 <= M <= 64, D % M == 0 and (D / M) % 16 == 0"); return 1; }
    const int64_t quads = (int64_t)n * D / 4, blocks = (quads + 255) / 256;
    if (blocks > INT32_MAX) { syl_set_error(what, "n x D is too large: decode in pieces"); return 1; }
    hipLaunchKernelGGL(pq_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, code_dev, quads, cb_dev, M, D, out_dev,
                       list_dev, centroid_dev, nlist);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Largest error of the fp32 device math functions the resynthesis decoder calls (csrc/cfm.hip: erff in cfm_gelu, sinf / cosf in the
// rotary angles and the time embedding, expf in the time conditioning's SiLU), against the float64 function of the SAME fp32 argument
// evaluated on the device.  Exhaustive: every fp32 argument with 2^-30 <= |x| < the range's end, both signs.
//   erff   |x| < 16        absolute error, in units of u = 2^-24 (|erf| <= 1)
//   sinf   |x| < 16384     absolute error, in units of u   (the registers' rotary angle is -10000 rad)
//   cosf   |x| < 16384     absolute error, in units of u
//   expf   |x| < 64        relative error, in units of u
// tests/cfm_block_ref.py carries twice these figures as ERFF_ERR, SINCOS_ERR and EXPF_ERR.
// build: hipcc --offload-arch=gfx950 -O3 -o tools/ubench/devmath_err tools/ubench/devmath_err.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>

#define CHECK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(_e), __LINE__); return 1; } } while (0)

// worst[f] = (error in units of u as float bits) << 32 | argument bits: non-negative floats order as their bit patterns
__global__ __launch_bounds__(256) void devmath_err(int f, unsigned lo, unsigned hi, unsigned long long* worst) {
    unsigned long long mine = 0;
    const unsigned long long n = 2ull * (hi - lo);
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const unsigned bits = (lo + (unsigned)(i >> 1)) | ((unsigned)(i & 1) << 31);
        const float x = __uint_as_float(bits);
        const double xd = (double)x;
        double err;
        if (f == 0) err = fabs((double)erff(x) - erf(xd));
        else if (f == 1) err = fabs((double)sinf(x) - sin(xd));
        else if (f == 2) err = fabs((double)cosf(x) - cos(xd));
        else { const double r = exp(xd); err = fabs((double)expf(x) - r) / r; }
        const float e = (float)(err * 16777216.0);
        const unsigned long long key = ((unsigned long long)__float_as_uint(e) << 32) | bits;
        if (key > mine) mine = key;
    }
    atomicMax(worst + f, mine);
}

static unsigned bits_of(float x) { unsigned b; std::memcpy(&b, &x, 4); return b; }

int main() {
    static const char* name[4] = {"erff abs", "sinf abs", "cosf abs", "expf rel"};
    const float end[4] = {16.0f, 16384.0f, 16384.0f, 64.0f};
    unsigned long long* worst = nullptr;
    CHECK(hipMalloc((void**)&worst, 4 * sizeof(unsigned long long)));
    CHECK(hipMemset(worst, 0, 4 * sizeof(unsigned long long)));
    for (int f = 0; f < 4; ++f) {
        hipLaunchKernelGGL(devmath_err, dim3(8192), dim3(256), 0, 0, f, bits_of(ldexpf(1.0f, -30)), bits_of(end[f]), worst);
        CHECK(hipGetLastError());
    }
    CHECK(hipDeviceSynchronize());
    unsigned long long host[4];
    CHECK(hipMemcpy(host, worst, sizeof(host), hipMemcpyDeviceToHost));
    for (int f = 0; f < 4; ++f) {
        const unsigned eb = (unsigned)(host[f] >> 32), xb = (unsigned)host[f];
        float e, x;
        std::memcpy(&e, &eb, 4); std::memcpy(&x, &xb, 4);
        std::printf("%s: max error %.4f u at x = %.9g (2^-30 <= |x| < %g, every fp32 argument)\n", name[f], e, x, end[f]);
    }
    CHECK(hipFree(worst));
    return 0;
}

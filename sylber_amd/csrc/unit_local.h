// What the two local-alignment kernels on unit strings share (unit_repeats.hip: one repeat per pair; unit_repeats_all.hip: every
// repeat, round by round): the shape of a strip, the limits of the contract, the DPP exchange with the lane above, and the host's
// arithmetic on the lengths.  The loops stay in their files.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int UL_CH = 32;                                 // steps of a chunk: lanes 0 .. 31 stage its columns
constexpr int UL_RING = 128;                              // columns of the ring: a step reads back 63 columns, a chunk is staged 32 ahead
constexpr int UL_ROWS = 64;                               // rows of x in a strip: one per lane
constexpr int UL_MAX_LEN = 65536, UL_MAX_W = 8, UL_MAX_PARAM = 64;

static_assert(UL_RING >= UL_ROWS - 1 + 2 * UL_CH && (UL_RING & (UL_RING - 1)) == 0, "the ring holds a chunk's columns, the 63 behind them and the next chunk");

// lane l: v of lane l - 1 (lane 0: its own), DPP wave_shr:1
__device__ __forceinline__ int ul_lane_above(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
static inline int64_t ul_al(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
// the two rows between strips: (H, si, sj) per column, only where there is a second strip
static inline int64_t ul_rows_bytes(int64_t m, int64_t L) { return m > UL_ROWS && L > 0 ? ul_al(2 * 12 * L) : 0; }

// the host's checks of the windows' lengths -> nullptr or what is wrong
static inline const char* ul_check(const int32_t* x_win, const int32_t* y_win, int32_t n_pairs) {
    if (!x_win || !y_win) return "null argument";
    if (n_pairs < 1) return "need n_pairs >= 1";
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int64_t m = x_win[2 * (size_t)p + 1], L = y_win[2 * (size_t)p + 1];
        if (m < 0 || L < 0) return "a window has a negative number of rows";
        if (m > UL_MAX_LEN || L > UL_MAX_LEN) return "a string has at most 65536 units";
    }
    return nullptr;
}

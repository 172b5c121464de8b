// HBM -> LDS staging of the GEMM families (LDS-DMA, no VGPR round trip): the primitives, the LDS image format and the piece
// counts, stated once.  Device side only.
//
// The image.  A K step ("stage") of a tile is BM rows of the first operand followed by BN rows of the second, RB = 128 or 64
// bytes per row (the stage's K extent in bytes, whatever the element size).  An LDS-DMA instruction is lane-linear: lane l's
// 16 bytes land at M0 base + 16 l, whatever address the lane asked for.  So a stage is cut into 1-KiB PIECES (one wave
// instruction: 8 rows x 128 B or 16 rows x 64 B), wave w owns pieces w + NW i, and lane l of a piece fills position l % CPR of
// row l / CPR.  The bank swizzle therefore goes on the SOURCE: the lane asks for 16-byte chunk (l % CPR) ^ key(row) of its
// row, and the fragment read finds k-chunk q of a row at byte (q ^ key(row)) << 4.  key = (row >> 1) & 7 on 128-byte rows,
// (row >> 2) & 3 on 64-byte rows: conflict-free for ds_read_b128's 16-lane groups.  Rows past the operand's last are
// clamped to it (their products are never stored).  The per-lane source offset stays constant over the K loop: the K step,
// the split16 operand plane and the conv tap pattern ride in the scalar offset of the buffer instruction.
//
// Retirement.  LDS-DMA is a vector memory operation: a barrier (raw s_barrier or __syncthreads) does NOT wait for it.  Every
// wave counts its own pieces down with wait_vmcnt<N>() BEFORE the barrier behind which another wave reads them; N = the
// pieces (and stores) the wave issued after the ones it needs, which stay in flight across the barrier.
//
// What is shared here: the primitives, the key and the piece counts.  The per-lane voff[] / lds_off[] loops are written at each
// kernel, and nothing here checks them against the fragment reads.
#pragma once
#include "common.h"

// ---- 1. primitives ----------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* lds_vptr;
typedef const __attribute__((address_space(1))) void* glb_vptr;
typedef int i32x4_t __attribute__((ext_vector_type(4)));

// 16 bytes per lane from a flat global address
__device__ __forceinline__ void glds16(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((glb_vptr)g, (lds_vptr)l, 16, 0, 0);
}
// 16 bytes per lane through a buffer descriptor: the per-lane part of the source address is a 32-bit byte offset that stays
// CONSTANT over the K loop (and, in the persistent kernels, over the tiles), the K step / operand plane travel in the scalar
// offset, the tile's first row in the descriptor base.  Against global_load_lds with a 64-bit per-lane address (two VALU
// adds per piece and step, twice the address registers) tools/ubench/mfma_mix2.hip measures the DMA's cost beside the
// MFMAs at +16 instead of +200 issue cycles per two pieces (profiles/r03_lds_dma_cost.md).
__device__ __forceinline__ void glds16b(__amdgpu_buffer_rsrc_t rs, int voff, int soff, void* l) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_vptr)l, 16, voff, soff, 0, 0);
}
// raw buffer over everything behind `base` (no stride, no bounds: the callers clamp their rows)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)0xffffffffu, 0x00020000);
}
// the same descriptor as four scalar dwords an inline-asm statement can name
__device__ __forceinline__ i32x4_t rsrc_words(const void* base) {
    const unsigned long long p = (unsigned long long)base;
    i32x4_t r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)p);
    r.y = __builtin_amdgcn_readfirstlane((int)((unsigned)(p >> 32) & 0xffffu));
    r.z = (int)0xffffffffu;
    r.w = 0x00020000;
    return r;
}
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
#define SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)

// ---- 2. the image format ----------------------------------------------------------------------------------------------
// swizzle key of tile row `row` on RB-byte rows
template <int RB> __host__ __device__ __forceinline__ constexpr int lds_key(int row) {
    static_assert(RB == 128 || RB == 64, "LDS rows are 128 or 64 bytes");
    return RB == 128 ? (row >> 1) & 7 : (row >> 2) & 3;
}
// does the key repeat every H rows?  (Then a fragment of H rows that starts at a multiple of H sees the key of its own rows.)
template <int RB> constexpr bool lds_key_repeats(int H) {
    for (int r = 0; r < 256; ++r)
        if (lds_key<RB>(r + H) != lds_key<RB>(r)) return false;
    return true;
}
// source side: the 16-byte chunk of its row that the lane filling position `pos` asks for
template <int RB> __host__ __device__ __forceinline__ constexpr int lds_src_chunk(int row, int pos) { return pos ^ lds_key<RB>(row); }
// read side: byte offset of k-chunk q inside a row with swizzle key `key`
__host__ __device__ __forceinline__ constexpr int lds_koff(int q, int key) { return (q ^ key) << 4; }
// Fragment reads.  A lane of a 32-row (16-row) MFMA fragment reads row lane & 31 (lane & 15) of it.  Fragments start at
// multiples of their height, which is a multiple of the key's period: the key of the lane's tile row is the key of its row
// INSIDE the fragment, which is why one per-lane key serves every fragment of a wave: byte offset of k-chunk q =
// lds_koff(q, frag32_key<RB>(lane)).  (The key of row lane & 31 is the key of "row" lane: the lane's half sits above its bits.)
template <int RB> __device__ __forceinline__ int frag32_key(int lane) {
    static_assert(lds_key_repeats<RB>(32), "a 32-row fragment must span whole key periods");
    return lds_key<RB>(lane);
}
template <int RB> __device__ __forceinline__ int frag16_chunk_off(int lane, int q) {
    static_assert(lds_key_repeats<RB>(16), "a 16-row fragment must span whole key periods");
    return lds_koff(q, lds_key<RB>(lane & 15));
}

// ---- 3. the piece counts --------------------------------------------------------------------------------------------
// BM rows of the first operand ("X") at stage offset 0, BN rows of the second ("W") behind them, NW waves.  EXTRA: 1-KiB pieces
// behind the operands that are no operand rows (the MXFP8 scale piece); they take part in the split over the waves.
template <int BM, int BN, int RB, int NW, int EXTRA = 0>
struct LdsPieces {
    static constexpr int RPP = 1024 / RB;                    // rows per piece
    static constexpr int NPT = (BM + BN) / RPP, NP = NPT + EXTRA;
    // slots per wave.  NP % NW != 0: the first NP % NW waves ("hi") own one piece more than the others
    static constexpr int NPW_HI = (NP + NW - 1) / NW, NPW_LO = NP / NW, NPW = NPW_HI;
    // pieces w + NW i with i < XPW are X rows for EVERY wave: which operand (and descriptor) slot i belongs to is static
    static constexpr int XPW = BM / RPP / NW;
    static_assert(BM % RPP == 0 && BN % RPP == 0, "operand rows must fill whole pieces");
    static_assert((BM / RPP) % NW == 0, "X pieces must split evenly over the waves");
    __host__ __device__ __forceinline__ static constexpr bool is_hi(int wave) { return wave < (NP % NW == 0 ? NW : NP % NW); }
};

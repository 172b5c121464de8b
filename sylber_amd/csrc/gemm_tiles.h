// The tile ids of the 16-bit GEMM launcher (GemmArgs::tune_cfg - 1, SYLBER_OPT_GEMM_TILE): geometry, owning kernel family and the member
// of the 16x16x32 family that stands in for a forced id on that family's launches.  The cost model (gemm_bf16.hip TileModel) takes its
// geometry from here and the dispatch asks the owning family's resolver (kernels.h); a new tile = one row here + its resolver entries.
#pragma once

enum GemmFamily { FAM_HIP, FAM_ASM, FAM_ASM16 };             // gemm_bf16.hip / gemm_asm.hip / gemm_asm16.hip
struct GemmTile { int id, bm, bn, waves, per_cu, family, m16; };
constexpr int GEMM_TILE_FALLBACK = 4;                        // 128x192: what a forced id without an instantiation runs (sylber_hip.h)
constexpr int GEMM_M16_DEFAULT = 15;                         // the family's stand-in for ids without a row (and for members it lacks at this K)
constexpr GemmTile GEMM_TILES[] = {
    {0, 256, 128, 4, 1, FAM_HIP, 14},   {1, 64, 64, 4, 2, FAM_HIP, 17},      {2, 64, 128, 4, 2, FAM_HIP, 15},
    {3, 128, 128, 4, 2, FAM_HIP, 15},   {4, 128, 192, 4, 2, FAM_HIP, 14},    {5, 128, 128, 8, 2, FAM_HIP, 15},
    {6, 128, 192, 8, 2, FAM_HIP, 16},   {10, 256, 256, 8, 1, FAM_HIP, 47},   {11, 256, 192, 8, 1, FAM_HIP, 14},
    {30, 256, 256, 8, 1, FAM_HIP, 47},  {40, 256, 256, 8, 1, FAM_HIP, 47},   {41, 256, 256, 8, 1, FAM_HIP, 47},     // 30 / 41: traces of 10 / 40
    {13, 128, 128, 4, 2, FAM_ASM16, 13}, {14, 128, 192, 4, 2, FAM_ASM16, 14}, {15, 128, 128, 8, 2, FAM_ASM16, 15},
    {16, 128, 192, 8, 1, FAM_ASM16, 16}, {17, 64, 64, 4, 2, FAM_ASM16, 17},   {46, 192, 256, 8, 1, FAM_ASM16, 46},
    {47, 256, 256, 8, 1, FAM_ASM16, 47},
    {51, 192, 192, 4, 1, FAM_ASM, 46},  {57, 192, 256, 8, 1, FAM_ASM, 46},   {60, 256, 256, 4, 1, FAM_ASM, 47},
    {80, 256, 256, 4, 1, FAM_ASM, 47},  {85, 256, 256, 4, 1, FAM_ASM, 47},   {86, 256, 128, 4, 1, FAM_ASM, 14},
    {90, 256, 192, 4, 1, FAM_ASM, 14},  {91, 256, 192, 4, 1, FAM_ASM, 14},   {96, 256, 192, 4, 1, FAM_ASM, 14},     // 96 = 91 without the residual prefetch
    {95, 256, 256, 8, 1, FAM_ASM, 47},  {97, 256, 256, 8, 1, FAM_ASM, 47},
#ifdef SYLBER_GEMM_ASM_EXPERIMENTS
    // timing-only variants (knock-outs, stamps) of tiles 60 (61-78), 80 (81-83), 97 (87-89, 98) and 91 (92, 93)
    {61, 256, 256, 4, 1, FAM_ASM, 15},  {62, 256, 256, 4, 1, FAM_ASM, 15},   {63, 256, 256, 4, 1, FAM_ASM, 15},   {64, 256, 256, 4, 1, FAM_ASM, 15},
    {65, 256, 256, 4, 1, FAM_ASM, 15},  {66, 256, 256, 4, 1, FAM_ASM, 15},   {67, 256, 256, 4, 1, FAM_ASM, 15},   {68, 256, 256, 4, 1, FAM_ASM, 15},
    {69, 256, 256, 4, 1, FAM_ASM, 15},  {70, 256, 256, 4, 1, FAM_ASM, 15},   {71, 256, 256, 4, 1, FAM_ASM, 15},   {72, 256, 256, 4, 1, FAM_ASM, 15},
    {73, 256, 256, 4, 1, FAM_ASM, 15},  {74, 256, 256, 4, 1, FAM_ASM, 15},   {75, 256, 256, 4, 1, FAM_ASM, 15},   {76, 256, 256, 4, 1, FAM_ASM, 15},
    {77, 256, 256, 4, 1, FAM_ASM, 15},  {78, 256, 256, 4, 1, FAM_ASM, 15},   {81, 256, 256, 4, 1, FAM_ASM, 15},   {82, 256, 256, 4, 1, FAM_ASM, 15},
    {83, 256, 256, 4, 1, FAM_ASM, 15},  {87, 256, 256, 8, 1, FAM_ASM, 15},   {88, 256, 256, 8, 1, FAM_ASM, 15},   {89, 256, 256, 8, 1, FAM_ASM, 15},
    {92, 256, 192, 4, 1, FAM_ASM, 15},  {93, 256, 192, 4, 1, FAM_ASM, 15},
#endif
    {98, 256, 256, 8, 1, FAM_ASM, 47},                       // tile 97 with phase stamps: an instantiation in experiments builds only
};
// id -> row (nullptr: no such tile); the index is built once, a lookup is one load (the dispatch asks several times per launch)
static inline const GemmTile* gemm_tile(int id) {
    struct Index {
        const GemmTile* at[100] = {};
        Index() { for (const GemmTile& t : GEMM_TILES) at[t.id] = &t; }
    };
    static const Index index;
    return id >= 0 && id < 100 ? index.at[id] : nullptr;
}

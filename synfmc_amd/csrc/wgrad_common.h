// The pixel-/token-reduction core shared by the weight-gradient kernels (lora_wgrad.hip, conv_wgrad.hip): a slab of 128 reduction rows x 64
// columns per operand staged row-major into LDS, MFMA fragments read transposed with ds_read_b64_tr_b16 (see lora_wgrad.hip's header).
#pragma once
#include "common.h"

namespace {

constexpr int WG_BT = 128;               // tokens per staged slab
constexpr int WG_BN = 64;                // output rows (columns of A) per workgroup
constexpr int WG_BK = 64;                // output columns (columns of B) per workgroup
constexpr int WG_PITCH = 96;             // LDS row pitch in bf16: 192 B, so the 4 rows of a transposed read hit disjoint banks
constexpr int WG_MIN_SLABS = 4;          // a split reduces at least 512 tokens
constexpr int WG_TARGET = 512;           // workgroups a problem is split towards (two per CU)
constexpr size_t WG_LDS = 4 * 4 * 16 * 64 * sizeof(float);    // 64 KiB: the cross-wave reduction (the two staged slabs, 48 KiB, alias it)

typedef short __attribute__((ext_vector_type(4))) wg_s4;
__device__ __forceinline__ wg_s4 lds_tr16(const bf16_t* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) wg_s4*)(p));
}

__device__ __forceinline__ void store_slab(bf16_t* __restrict__ dst, const u32x4 (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = threadIdx.x + 256 * i;
        *reinterpret_cast<u32x4*>(dst + (e >> 3) * WG_PITCH + 8 * (e & 7)) = r[i];
    }
}

// operand fragment of the 32 columns [col0, col0 + 32) over tokens 8h .. 8h+7 of the wave's 16-token k-step at row t0
__device__ __forceinline__ bf16x8 frag(const bf16_t* __restrict__ s, int t0, int col0, int lane) {
    const int g = lane >> 4, i = lane & 15;
    const bf16_t* p = s + (t0 + 8 * (g >> 1) + (i >> 2)) * WG_PITCH + col0 + 16 * (g & 1) + 4 * (i & 3);
    union { bf16x8 v; wg_s4 h[2]; } r;
    r.h[0] = lds_tr16(p);                    // tokens +0..3
    r.h[1] = lds_tr16(p + 4 * WG_PITCH);     // tokens +4..7
    return r.v;
}

// one staged slab: wave w reduces tokens 32w .. 32w+31 of it into the whole 64 x 64 tile (every fragment read feeds two MFMAs)
__device__ __forceinline__ void slab_mfma(const bf16_t* __restrict__ sa, const bf16_t* __restrict__ sb, int wave, int lane, f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int t0 = 32 * wave + 16 * ks;
        const bf16x8 fa0 = frag(sa, t0, 0, lane), fa1 = frag(sa, t0, 32, lane);
        const bf16x8 fb0 = frag(sb, t0, 0, lane), fb1 = frag(sb, t0, 32, lane);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa0, fb0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa0, fb1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa1, fb0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa1, fb1, acc[1][1], 0, 0, 0);
    }
}

// the four waves' partial tiles -> LDS [wave][i * 2 + j][reg][lane]; element e of the tile is then ((red[e] + red[4096 + e]) + ...) in wave order
__device__ __forceinline__ void spill_tiles(float* __restrict__ red, int wave, int lane, const f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) red[((wave * 4 + i * 2 + j) * 16 + r) * 64 + lane] = acc[i][j][r];
}

// splits / slabs per split of a reduction of `rows` rows into `tiles` output tiles: a function of the shape alone
inline void wg_split_plan(int64_t rows, int64_t tiles, int& splits, int& chunk_slabs) {
    const int64_t slabs = (rows + WG_BT - 1) / WG_BT;
    int64_t s = (WG_TARGET + tiles - 1) / tiles;
    if (s > slabs / WG_MIN_SLABS) s = slabs / WG_MIN_SLABS;
    if (s < 1) s = 1;
    chunk_slabs = (int)((slabs + s - 1) / s);
    splits = (int)((slabs + chunk_slabs - 1) / chunk_slabs);
}

}  // namespace

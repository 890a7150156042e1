// MXFP8 feed-forward GEMMs (opt-in, hip_ops.FP8_FF): OCP e4m3fn elements with one E8M0 scale byte per 32 consecutive elements of the reduction axis, multiplied
// on the block-scaled matrix instruction v_mfma_scale_f32_32x32x64_f8f6f4 (twice the bf16 rate per clock at half the operand bytes).  Three pieces:
//   * fmc_mxfp8_pack_weight:    w [N, K] bf16 -> e4m3 rows + scales, for the GEGLU form with value and gate rows interleaved in 32-row blocks;
//   * fmc_layernorm_mxfp8_fwd:  LayerNorm (fp32 statistics, as layernorm_g_kernel) and quantisation in one pass over h; gamma == NULL: quantisation alone;
//   * fmc_linear_mxfp8:         out = dq(xq, xs) dq(wq, ws)^T + bias (+ residual) -> bf16, or the GEGLU product -> MXFP8 (bytes + scales) for the next GEMM.
//
// Number format.  A block's scale byte is clamp(floor(log2 amax) - 8 + 127, 0, 254) (0 for an all-zero block); its elements are x * 2^(127 - byte) clamped to
// +-448 and rounded to nearest even to e4m3 (the scaled amax lies in [256, 512): saturation is part of the format).  tests/mxfp8_common.py is the reference.
//
// Lane maps of v_mfma_scale_f32_32x32x64_f8f6f4 with both formats fp8 (cbsz = blgp = 0), measured with one-hot operands and one-hot scales on one instruction
// and pinned by the exact-integer cases of tests/test_gpu_mxfp8.py (profiles/mxfp8_ff.md):
//   A (8 VGPRs = 32 bytes per lane): lane l (r = l & 31, h = l >> 5) holds row r; bytes 0 .. 15 are k = 16 h + j of scale block 0, bytes 16 .. 31 are
//     k = 32 + 16 h + (j - 16) of scale block 1 -- a lane holds HALF of each of the row's two blocks, not one whole block;
//   B: the same with column r;
//   scale operands: byte `op_sel` of lane r's dword scales block 0 (k < 32) of row / column r, that of lane r + 32 scales block 1;
//   C/D: the shape-determined 32x32 map, column = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
// The weights are the A operand and the tokens the B operand, so a lane holds ONE token row and 16 of a 32-column output block: the GEGLU epilogue's block
// amax is a 16-register maximum and one exchange with lane ^ 32.
//
// Main loop: 128 token rows x 128 weight rows per workgroup, 4 waves = 2 x 2, each 64 x 64 as 2 x 2 matrix instructions per 64-deep k-step (K % 64 == 0
// covers every K of the model; the 16x16x128 form would need a tail at K = 320).  A k-step is 16 one-KiB LDS-DMA pieces (128 + 128 rows of 64 bytes, the
// 16-byte chunks XOR-swizzled through the SOURCE address) and four 64-row pieces of scale bytes (two per row), five requests per wave, in a ring of 4
// k-steps requested three ahead; counted vmcnt, one barrier per k-step.  A partly filled last row tile reads clamped rows and stores nothing past M.
#include "common.h"

namespace {

constexpr int BM = 128, BN = 128, NBUF = 4, LEAD = NBUF - 1;
// (an LDS-DMA load narrower than a dword still lands one DWORD per lane, zero-extended, at lane * 4: a row's two scale bytes take a dword of the stage)
constexpr int ST_X = 0, ST_W = BM * 64, ST_XS = ST_W + BN * 64, ST_WS = ST_XS + BM * 4;
constexpr int STAGE = ST_WS + BN * 4;                      // 17,408 bytes per k-step
constexpr int LDS_BYTES = NBUF * STAGE;                    // 69,632

typedef __attribute__((ext_vector_type(8))) int i32x8;

// accumulators reach VALU code only behind this fence (see TB_SETTLE in temporal_block.hip)
#define MX_SETTLE()                                               \
    do {                                                          \
        __builtin_amdgcn_sched_barrier(0);                        \
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");       \
        __builtin_amdgcn_sched_barrier(0);                        \
    } while (0)

__device__ __forceinline__ float mx_gelu(float g) {           // as gelu_erf of gemm_conv.hip
    if (!FMC_GELU_EXACT) return fmc_gelu_fast(g);
    const float x = fabsf(g) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, x, 1.f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = 1.f - p * t * __builtin_amdgcn_exp2f(-1.4426950408889634f * x * x);
    return 0.5f * g + 0.5f * fabsf(g) * e;
}

// E8M0 byte of a block with this amax (finite, >= 0) and the exact power of two that scales its elements
__device__ __forceinline__ unsigned mx_scale_byte(float amax) {
    const int eb = (int)((__float_as_uint(amax) >> 23) & 0xffu);
    return (unsigned)max(eb - 8, 0);
}
__device__ __forceinline__ float mx_inv_scale(unsigned byte) { return __uint_as_float((254u - byte) << 23); }
// four values -> four e4m3 bytes (clamped to +-448, round to nearest even)
__device__ __forceinline__ unsigned mx_pack4(float a, float b, float c, float d, float inv) {
    a = fminf(fmaxf(a * inv, -448.f), 448.f); b = fminf(fmaxf(b * inv, -448.f), 448.f);
    c = fminf(fmaxf(c * inv, -448.f), 448.f); d = fminf(fmaxf(d * inv, -448.f), 448.f);
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
    return (unsigned)r;
}

// ---- quantisers: one wave per row, a lane per 8 elements, four lanes per scale block -------------------------------------------------------------------
// source row of output row p: identity, or (geglu_inner > 0) the value / gate interleave in 32-row blocks: p = 64 t + 32 g + c <- g * inner + 32 t + c
__global__ __launch_bounds__(256) void mx_quant_rows_kernel(const bf16_t* __restrict__ x, unsigned char* __restrict__ q, unsigned char* __restrict__ s,
                                                            int64_t M, int C, int64_t ldx, int geglu_inner) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;                                    // (wave-uniform)
    int64_t src = row;
    if (geglu_inner > 0) {
        const int64_t t = row >> 6;
        const int g = (int)(row >> 5) & 1, c = (int)row & 31;
        src = (int64_t)g * geglu_inner + t * 32 + c;
    }
    const int nch = C >> 3;
    for (int ch = lane; ch < nch; ch += 64) {                // (C % 64 == 0: the four lanes of a block are in or out together)
        float v[8];
        Vec8<bf16_t>::load(x + src * ldx + ch * 8, v);
        float am = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) am = fmaxf(am, fabsf(v[i]));
        am = fmaxf(am, __shfl_xor(am, 1, 64));
        am = fmaxf(am, __shfl_xor(am, 2, 64));
        const unsigned byte = mx_scale_byte(am);
        const float inv = mx_inv_scale(byte);
        *reinterpret_cast<u32x2*>(q + row * C + ch * 8) = u32x2{mx_pack4(v[0], v[1], v[2], v[3], inv), mx_pack4(v[4], v[5], v[6], v[7], inv)};
        if ((lane & 3) == 0) s[row * (C >> 5) + (ch >> 2)] = (unsigned char)byte;
    }
}

template <int NCH>
__global__ __launch_bounds__(256) void mx_ln_quant_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          unsigned char* __restrict__ q, unsigned char* __restrict__ s, int64_t M, int C, int64_t ldx,
                                                          float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nch = C >> 3;
    float v[NCH][8];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int ch = j * 64 + lane;
        Vec8<bf16_t>::load(x + row * ldx + (ch < nch ? ch : 0) * 8, v[j]);
        if (ch >= nch) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[j][i] = 0.f;
        }
    }
    const float rc = 1.f / (float)C;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) sum += v[j][i];
    const float mean = wave_sum(sum) * rc;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const bool in = j * 64 + lane < nch;
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float d = in ? v[j][i] - mean : 0.f; sq += d * d; }
    }
    const float rs = rsqrtf(wave_sum(sq) * rc + eps);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int ch = j * 64 + lane;
        const bool in = ch < nch;
        const int chc = in ? ch : 0;
        float gm[8], bt[8], o[8];
        Vec8<float>::load(gamma + chc * 8, gm);
        Vec8<float>::load(beta + chc * 8, bt);
        float am = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { o[i] = (v[j][i] - mean) * rs * gm[i] + bt[i]; am = fmaxf(am, fabsf(o[i])); }
        am = fmaxf(am, __shfl_xor(am, 1, 64));
        am = fmaxf(am, __shfl_xor(am, 2, 64));
        const unsigned byte = mx_scale_byte(am);
        const float inv = mx_inv_scale(byte);
        if (in) {
            *reinterpret_cast<u32x2*>(q + row * C + ch * 8) = u32x2{mx_pack4(o[0], o[1], o[2], o[3], inv), mx_pack4(o[4], o[5], o[6], o[7], inv)};
            if ((lane & 3) == 0) s[row * (C >> 5) + (ch >> 2)] = (unsigned char)byte;
        }
    }
}

// ---- the GEMM ------------------------------------------------------------------------------------------------------------------------------------------
struct MxParams {
    const unsigned char* xq; const unsigned char* xs; const unsigned char* wq; const unsigned char* ws;
    const bf16_t* bias; const bf16_t* res; bf16_t* out; unsigned char* oq; unsigned char* os;
    int64_t M; int N, K;                                     // N: weight rows (GEGLU: 2 inner, packed order)
    int64_t ldres, ldo;
    int tiles_m, tiles_n;
};

template <bool GEGLU>
__global__ __launch_bounds__(256, 2)
void mxfp8_gemm_kernel(const MxParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l31 = lane & 31, h = lane >> 5;
    const int tile_m = blockIdx.x / P.tiles_n, tile_n = blockIdx.x - tile_m * P.tiles_n;
    const int64_t m0 = (int64_t)tile_m * BM;
    const int n0 = tile_n * BN;
    const int nks = P.K >> 6, kb = P.K >> 5;

    // ---- my five requests per k-step: waves 0, 1 the token pieces, waves 2, 3 the weight pieces (one pair of buffer descriptors per wave) ----
    const bool isw = wave >= 2;
    const int64_t rows = isw ? (int64_t)P.N : P.M, row00 = isw ? (int64_t)n0 : m0;
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(isw ? P.wq : P.xq), 0, (int)(rows * P.K), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc((void*)(isw ? P.ws : P.xs), 0, (int)(rows * kb), 0x00020000);
    unsigned d_vo[4], s_vo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {                            // data piece: 16 rows x 64 bytes; lane -> row lane / 4, physical chunk lane % 4
        const int r = 16 * (4 * (wave & 1) + e) + (lane >> 2);
        const int64_t rg = min(row00 + r, rows - 1);         // (rows past the end repeat the last one: reads stay inside the tensor)
        d_vo[e] = (unsigned)(rg * P.K + (((lane & 3) ^ ((r >> 2) & 3)) << 4));
    }
    {                                                        // scale piece: 64 rows x 2 bytes (a dword of LDS each)
        const int64_t rg = min(row00 + 64 * (wave & 1) + lane, rows - 1);
        s_vo = (unsigned)(rg * kb);
    }
    const int d_lds = (isw ? ST_W : ST_X) + 4096 * (wave & 1), s_lds = (isw ? ST_WS : ST_XS) + 256 * (wave & 1);
    int iss_k = 0, iss_slot = 0;
    auto issue = [&]() {
        unsigned char* stage = smem_raw + iss_slot * STAGE;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (__attribute__((address_space(3))) void*)(stage + d_lds + e * 1024), 16, (int)d_vo[e], iss_k * 64, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsc, (__attribute__((address_space(3))) void*)(stage + s_lds), 2, (int)s_vo, iss_k * 2, 0, 0);
        iss_k = iss_k + 1 == nks ? 0 : iss_k + 1;            // (past the end of K the stream wraps to valid addresses: the counts stay exact)
        iss_slot = iss_slot + 1 == NBUF ? 0 : iss_slot + 1;
    };

    f32x16 acc[2][2];                                        // [weight block][token block]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

#pragma unroll
    for (int d = 0; d < LEAD; ++d) issue();
    int rd_slot = 0;
    for (int s = 0; s < nks; ++s) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(5 * (LEAD - 1)) : "memory");        // my requests of k-step s have landed
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();                        // ... everybody's have; everybody has finished reading k-step s - 1's slot
        __builtin_amdgcn_sched_barrier(0);
        issue();                                             // k-step s + LEAD into that slot
        const unsigned char* base = smem_raw + rd_slot * STAGE;
        i32x8 wf[2], xf[2];
        int wsc[2], xsc[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int rw = wc * 64 + b * 32 + l31, rx = wr * 64 + b * 32 + l31;
            // lane half h: 16-byte chunk h of scale block 0, then chunk 2 + h of scale block 1 (the instruction's k order, see the header)
            const int c0w = h ^ ((rw >> 2) & 3), c1w = (2 + h) ^ ((rw >> 2) & 3);
            const int c0x = h ^ ((rx >> 2) & 3), c1x = (2 + h) ^ ((rx >> 2) & 3);
            union { i32x8 v; u32x4 u[2]; } t;
            t.u[0] = *reinterpret_cast<const u32x4*>(base + ST_W + rw * 64 + c0w * 16);
            t.u[1] = *reinterpret_cast<const u32x4*>(base + ST_W + rw * 64 + c1w * 16);
            wf[b] = t.v;
            t.u[0] = *reinterpret_cast<const u32x4*>(base + ST_X + rx * 64 + c0x * 16);
            t.u[1] = *reinterpret_cast<const u32x4*>(base + ST_X + rx * 64 + c1x * 16);
            xf[b] = t.v;
            wsc[b] = base[ST_WS + rw * 4 + h];
            xsc[b] = base[ST_XS + rx * 4 + h];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[a], xf[b], acc[a][b], 0, 0, 0, wsc[a], 0, xsc[b]);
        rd_slot = rd_slot + 1 == NBUF ? 0 : rd_slot + 1;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // the wrap-around requests of the tail have landed before the workgroup gives up its LDS
    MX_SETTLE();

    if constexpr (!GEGLU) {
        // out[m, n] = bf16(acc + bias[n] + residual[m, n]); a lane holds token row m and 4 consecutive n per register group
        // (bias and residual requested in one burst from clamped addresses, as the rows of layernorm_g_kernel: a load inside the store's condition is a
        //  round trip of its own)
        u32x2 bq[2][4], rq[2][2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int nc = min(n0 + wc * 64 + a * 32 + 8 * g + 4 * h, P.N - 4);
                bq[a][g] = P.bias ? *reinterpret_cast<const u32x2*>(P.bias + nc) : u32x2{0u, 0u};
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int64_t mc = min(m0 + wr * 64 + b * 32 + l31, P.M - 1);
                    rq[a][b][g] = P.res ? *reinterpret_cast<const u32x2*>(P.res + mc * P.ldres + nc) : u32x2{0u, 0u};
                }
            }
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int64_t m = m0 + wr * 64 + b * 32 + l31;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int n = n0 + wc * 64 + a * 32 + 8 * g + 4 * h;
                    float o[4] = {acc[a][b][4 * g], acc[a][b][4 * g + 1], acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]};
                    const u32x2 t = bq[a][g], u = rq[a][b][g];
                    o[0] += __uint_as_float(t[0] << 16); o[1] += __uint_as_float(t[0] & 0xffff0000u);
                    o[2] += __uint_as_float(t[1] << 16); o[3] += __uint_as_float(t[1] & 0xffff0000u);
                    o[0] += __uint_as_float(u[0] << 16); o[1] += __uint_as_float(u[0] & 0xffff0000u);
                    o[2] += __uint_as_float(u[1] << 16); o[3] += __uint_as_float(u[1] & 0xffff0000u);
                    if (m < P.M && n < P.N) *reinterpret_cast<u32x2*>(P.out + m * P.ldo + n) = u32x2{pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
                }
        }
    } else {
        // weight block 0 of a wave: 32 value rows, block 1: their gate rows (fmc_mxfp8_pack_weight); the wave's 32 output columns are ONE scale block per token
        const int inner = P.N >> 1;
        const int j0 = tile_n * 64 + wc * 32;                // first output column of the wave
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int64_t m = m0 + wr * 64 + b * 32 + l31;
            float y[16];
            float am = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int j = j0 + 8 * g + 4 * h;
                float bv[4] = {0.f, 0.f, 0.f, 0.f}, bg[4] = {0.f, 0.f, 0.f, 0.f};
                if (P.bias) {
                    const u32x2 t = *reinterpret_cast<const u32x2*>(P.bias + j), u = *reinterpret_cast<const u32x2*>(P.bias + inner + j);
                    bv[0] = __uint_as_float(t[0] << 16); bv[1] = __uint_as_float(t[0] & 0xffff0000u);
                    bv[2] = __uint_as_float(t[1] << 16); bv[3] = __uint_as_float(t[1] & 0xffff0000u);
                    bg[0] = __uint_as_float(u[0] << 16); bg[1] = __uint_as_float(u[0] & 0xffff0000u);
                    bg[2] = __uint_as_float(u[1] << 16); bg[3] = __uint_as_float(u[1] & 0xffff0000u);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    y[4 * g + i] = (acc[0][b][4 * g + i] + bv[i]) * mx_gelu(acc[1][b][4 * g + i] + bg[i]);
                    am = fmaxf(am, fabsf(y[4 * g + i]));
                }
            }
            am = fmaxf(am, __shfl_xor(am, 32, 64));
            const unsigned byte = mx_scale_byte(am);
            const float inv = mx_inv_scale(byte);
            if (m < P.M) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<unsigned*>(P.oq + m * inner + j0 + 8 * g + 4 * h) = mx_pack4(y[4 * g], y[4 * g + 1], y[4 * g + 2], y[4 * g + 3], inv);
                if (h == 0) P.os[m * (inner >> 5) + (j0 >> 5)] = (unsigned char)byte;
            }
        }
    }
}

constexpr int64_t TWO_GIB = (int64_t)1 << 31;

}  // namespace

extern "C" int fmc_mxfp8_tile_rows(void) { return BM; }
extern "C" int fmc_mxfp8_tile_cols(void) { return BN; }

extern "C" int fmc_linear_mxfp8_supported(int64_t M, int N, int K, int geglu) {
    if (M < 1 || N < 64 || K < 64 || K % 64 || N % 64) return 0;
    const int64_t rows_w = geglu ? 2 * (int64_t)N : N;      // N: output columns (GEGLU: inner)
    if (M * K >= TWO_GIB || rows_w * K >= TWO_GIB || M * (int64_t)N * (geglu ? 1 : 2) >= TWO_GIB) return 0;
    return 1;
}

/* w [N, K] bf16 (contiguous) -> wq [N, K] e4m3 + ws [N, K / 32] E8M0, scale blocks along K.  geglu_inner == 0: rows in order.  geglu_inner = inner (N == 2 inner,
 * inner % 64 == 0): packed row 64 t + 32 g + c is source row g * inner + 32 t + c, so that a wave of fmc_linear_mxfp8 meets a value column and its gate. */
extern "C" int fmc_mxfp8_pack_weight(const void* w, void* wq, void* ws, int N, int K, int geglu_inner, void* stream) {
    if (!w || !wq || !ws) FMC_FAIL(FMC_E_NULL, "mxfp8_pack_weight: NULL tensor");
    if (N < 64 || K < 64 || N % 64 || K % 64 || (int64_t)N * K >= TWO_GIB || (geglu_inner && (geglu_inner % 64 || N != 2 * geglu_inner)))
        FMC_FAIL(FMC_E_SHAPE, "mxfp8_pack_weight: need N %% 64 == 0, K %% 64 == 0, N == 2 inner, inner %% 64 == 0, N K < 2^31 (N=%d K=%d inner=%d)", N, K, geglu_inner);
    if (!fmc_aligned16(w) || !fmc_aligned16(wq) || !fmc_aligned16(ws)) FMC_FAIL(FMC_E_ALIGN, "mxfp8_pack_weight: tensors must be 16-byte aligned");
    fmc_launch<mx_quant_rows_kernel>(dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, (unsigned char*)wq, (unsigned char*)ws,
                                     (int64_t)N, K, (int64_t)K, geglu_inner);
    FMC_CHECK_LAUNCH("fmc_mxfp8_pack_weight");
    return 0;
}

/* xq [M, C] e4m3 + xs [M, C / 32] E8M0 of LayerNorm(h) (h [M, C] bf16, rows ldh apart; gamma / beta fp32; statistics in fp32), h read once.
 * gamma == NULL (then beta must be NULL too): no normalisation, the rows of h themselves are quantised -- bit for bit the reference quantiser.
 * C % 64 == 0; with gamma C <= 2048; ldh % 8 == 0; M C < 2^31. */
extern "C" int fmc_layernorm_mxfp8_fwd(const void* h, const void* gamma, const void* beta, void* xq, void* xs, int64_t M, int C, int64_t ldh, float eps,
                                       void* stream) {
    if (!h || !xq || !xs || (gamma && !beta) || (!gamma && beta)) FMC_FAIL(FMC_E_NULL, "layernorm_mxfp8_fwd: NULL tensor (gamma and beta: both or neither)");
    if (M < 1 || C < 64 || C % 64 || ldh < C || ldh % 8 || M * C >= TWO_GIB || ((M - 1) * ldh + C) * 2 >= 2 * TWO_GIB || (gamma && C > 2048))
        FMC_FAIL(FMC_E_SHAPE, "layernorm_mxfp8_fwd: need C %% 64 == 0 (<= 2048 with gamma), ldh %% 8 == 0, M C < 2^31 (M=%lld C=%d ldh=%lld)", (long long)M, C,
                 (long long)ldh);
    if (!fmc_aligned16(h) || !fmc_aligned16(xq) || !fmc_aligned16(xs) || (gamma && (!fmc_aligned16(gamma) || !fmc_aligned16(beta))))
        FMC_FAIL(FMC_E_ALIGN, "layernorm_mxfp8_fwd: tensors must be 16-byte aligned");
    const dim3 grid((unsigned)((M + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (!gamma) {
        fmc_launch<mx_quant_rows_kernel>(grid, block, 0, st, (const bf16_t*)h, (unsigned char*)xq, (unsigned char*)xs, M, C, ldh, 0);
    } else {
        const int nch = (C / 8 + 63) / 64;
#define MX_LN(NCH) fmc_launch<mx_ln_quant_kernel<NCH>>(grid, block, 0, st, (const bf16_t*)h, (const float*)gamma, (const float*)beta, (unsigned char*)xq, \
                                                       (unsigned char*)xs, M, C, ldh, eps)
        if (nch == 1) MX_LN(1); else if (nch == 2) MX_LN(2); else if (nch == 3) MX_LN(3); else MX_LN(4);
#undef MX_LN
    }
    FMC_CHECK_LAUNCH("fmc_layernorm_mxfp8_fwd");
    return 0;
}

/* geglu == 0:  out[m, n] = bf16(sum_k dq(x)[m, k] dq(w)[n, k] + bias[n] + residual[m, n])    (out rows ldo, residual rows ldres apart; bias / residual may be NULL)
 * geglu == 1:  y[m, j] = (sum_k x w_value[j] + bias[j]) * gelu(sum_k x w_gate[j] + bias[N + j]), j < N = inner, written as MXFP8: oq [M, N] e4m3 and
 *              os [M, N / 32] E8M0, the scale blocks along j; wq / ws in the packed order of fmc_mxfp8_pack_weight(geglu_inner = N); bias bf16 [2 N] in the
 *              module's order (value | gate).
 * xq [M, K] / xs [M, K / 32] and wq / ws contiguous; fp32 accumulation on v_mfma_scale_f32_32x32x64_f8f6f4.  fmc_linear_mxfp8_supported is the domain. */
extern "C" int fmc_linear_mxfp8(const void* xq, const void* xs, const void* wq, const void* ws, const void* bias, const void* residual, void* out,
                                void* out_scales, int64_t M, int N, int K, int64_t ldres, int64_t ldo, int geglu, void* stream) {
    if (!xq || !xs || !wq || !ws || !out || (geglu && !out_scales)) FMC_FAIL(FMC_E_NULL, "linear_mxfp8: NULL tensor");
    if (!fmc_linear_mxfp8_supported(M, N, K, geglu) || (!geglu && (ldo < N || ldo % 4 || (residual && (ldres < N || ldres % 4)))) || (geglu && residual))
        FMC_FAIL(FMC_E_SHAPE, "linear_mxfp8: need K %% 64 == 0, N %% 64 == 0, operands < 2 GiB, no residual with geglu (M=%lld N=%d K=%d)", (long long)M, N, K);
    if (!geglu && (((M - 1) * ldo + N) * 2 >= 2 * TWO_GIB || (residual && ((M - 1) * ldres + N) * 2 >= 2 * TWO_GIB)))
        FMC_FAIL(FMC_E_SHAPE, "linear_mxfp8: out / residual span 4 GiB or more");
    if (!fmc_aligned16(xq) || !fmc_aligned16(xs) || !fmc_aligned16(wq) || !fmc_aligned16(ws) || !fmc_aligned16(out) || (out_scales && !fmc_aligned16(out_scales)) ||
        (residual && !fmc_aligned16(residual)) || (bias && (reinterpret_cast<uintptr_t>(bias) & 7)))
        FMC_FAIL(FMC_E_ALIGN, "linear_mxfp8: tensors must be 16-byte aligned (bias 8)");
    MxParams P;
    P.xq = (const unsigned char*)xq; P.xs = (const unsigned char*)xs; P.wq = (const unsigned char*)wq; P.ws = (const unsigned char*)ws;
    P.bias = (const bf16_t*)bias; P.res = (const bf16_t*)residual; P.out = (bf16_t*)out; P.oq = (unsigned char*)out; P.os = (unsigned char*)out_scales;
    P.M = M; P.N = geglu ? 2 * N : N; P.K = K; P.ldres = ldres; P.ldo = ldo;
    P.tiles_m = (int)((M + BM - 1) / BM); P.tiles_n = (P.N + BN - 1) / BN;
    const dim3 grid((unsigned)(P.tiles_m * P.tiles_n)), block(256);
    if (geglu) fmc_launch<mxfp8_gemm_kernel<true>>(grid, block, LDS_BYTES, (hipStream_t)stream, P);
    else fmc_launch<mxfp8_gemm_kernel<false>>(grid, block, LDS_BYTES, (hipStream_t)stream, P);
    FMC_CHECK_LAUNCH("fmc_linear_mxfp8");
    return 0;
}

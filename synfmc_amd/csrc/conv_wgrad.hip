// Weight gradient of a trainable 3x3 / pad 1 / stride 1 or 2 convolution, gfx950, straight into fp32:
//     dW[co][ky][kx][ci] = alpha * sum over (n, yo, xo) of dY[n, yo, xo, co] * X[n, s yo + ky - 1, s xo + kx - 1, ci]   (+ dW)
//
// The product of lora_wgrad.hip -- out[N][K] = A^T B with the reduction index the ROW of both operands -- where A is dY as a pixel matrix
// [P = n Ho Wo][Cout] and B's row for (pixel, tap) is the input pixel under that tap, or zero outside the image: an implicit GEMM whose B
// slab is gathered instead of copied.  Everything after the loader is the shared core (wgrad_common.h): 128-pixel slabs staged row-major into
// LDS, ds_read_b64_tr_b16 fragments, v_mfma_f32_32x32x16_bf16, zero pads (the transposed read needs EXEC all ones: pad, don't mask), the four
// waves' tiles summed through LDS in wave order.
//
// Workgroup = one (tap, 64 ci, 64 co, split).  The splits are a function of the shape alone (conv_split_plan); with more than one, each writes an fp32
// partial [Cout][9][Cin] into the caller's workspace and conv_wgrad_combine_kernel adds them in split order: bit-reproducible.  Only the pass
// that writes dW (the combine, or the main kernel when there is one split) knows about alpha, accumulate and the layout of dW.
//
// Block order: the nine taps of a tile write interleaved words of the same cache lines of a [Cout][Cin][3][3] dW, so they are given block ids
// that are equal modulo 8 and within 72 of each other -- workgroups are dealt to the 8 XCDs round-robin, and the lines then fill up in one L2.
// This is placement for speed only: no result depends on it.
#include "wgrad_common.h"

namespace {

struct CwParams {
    const bf16_t* x; const bf16_t* dy; float* dw; float* ws;       // ws: [splits][Cout][9][Cin] partials (splits > 1)
    int H, W, Ho, Wo, Cin, Cout, stride, layout;
    int tiles_ci, tiles, tiles_pad, splits, chunk_slabs;            // tiles = tiles_co * tiles_ci, tiles_pad = tiles rounded up to 8
    int step_img, step_y, step_x;                                   // 128 pixels = (step_img * Ho + step_y) * Wo + step_x
    int64_t P;                                                      // n * Ho * Wo
    float alpha; int accumulate;
};

// where element (co, tap, ci) of dW lives: 0 = [Cout][Cin][3][3], 1 = [Cout][3][3][Cin]
__device__ __forceinline__ int64_t dw_index(int layout, int co, int tap, int ci, int Cin) {
    return layout == 0 ? ((int64_t)co * Cin + ci) * 9 + tap : ((int64_t)co * 9 + tap) * Cin + ci;
}

struct Pixel { int img, y, x; };        // an OUTPUT pixel (n, yo, xo)

__device__ __forceinline__ void load_dy_slab(const CwParams& P, int co0, int64_t m0, int64_t m_end, u32x4 (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = threadIdx.x + 256 * i, row = e >> 3, c = co0 + 8 * (e & 7);
        const int64_t m = m0 + row;
        r[i] = (m < m_end && c < P.Cout) ? *reinterpret_cast<const u32x4*>(P.dy + m * P.Cout + c) : u32x4{0u, 0u, 0u, 0u};
    }
}

// the B slab: slab row (threadIdx.x >> 3) + 32 i is the output pixel px[i]; its row of B is X under the tap, zero outside the image, past the
// end of the split and past Cin.  Every address formed lies inside X: the pixel is one of the P, the source row / column is checked.
__device__ __forceinline__ void load_x_slab(const CwParams& P, int ci0, int ky, int kx, int64_t m0, int64_t m_end, const Pixel (&px)[4],
                                            u32x4 (&r)[4]) {
    const int c = ci0 + 8 * (threadIdx.x & 7);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + (threadIdx.x >> 3) + 32 * i;
        const int yi = P.stride * px[i].y + ky - 1, xi = P.stride * px[i].x + kx - 1;
        const bool ok = m < m_end && c < P.Cin && yi >= 0 && yi < P.H && xi >= 0 && xi < P.W;
        r[i] = ok ? *reinterpret_cast<const u32x4*>(P.x + (((int64_t)px[i].img * P.H + yi) * P.W + xi) * P.Cin + c) : u32x4{0u, 0u, 0u, 0u};
    }
}

// 128 pixels on: each carry happens at most once because x < Wo, step_x < Wo and y < Ho, step_y < Ho
__device__ __forceinline__ void advance(const CwParams& P, Pixel (&px)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int x = px[i].x + P.step_x, y = px[i].y + P.step_y, img = px[i].img + P.step_img;
        if (x >= P.Wo) { x -= P.Wo; ++y; }
        if (y >= P.Ho) { y -= P.Ho; ++img; }
        px[i] = Pixel{img, y, x};
    }
}

__global__ void __launch_bounds__(256) conv_wgrad_kernel(const CwParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* sa = reinterpret_cast<bf16_t*>(smem);
    bf16_t* sb = sa + WG_BT * WG_PITCH;
    float* red = reinterpret_cast<float*>(smem);

    const int per_split = P.tiles_pad * 9;
    const int split = (int)blockIdx.x / per_split, r = (int)blockIdx.x % per_split;
    const int tile = (r / 72) * 8 + (r & 7), tap = (r % 72) >> 3;
    if (tile >= P.tiles) return;                                    // (the whole workgroup: no partial EXEC below)
    const int co0 = (tile / P.tiles_ci) * WG_BN, ci0 = (tile % P.tiles_ci) * WG_BK;
    const int ky = tap / 3, kx = tap % 3;
    const int64_t m_begin = (int64_t)split * P.chunk_slabs * WG_BT;
    const int64_t m_end = m_begin + (int64_t)P.chunk_slabs * WG_BT < P.P ? m_begin + (int64_t)P.chunk_slabs * WG_BT : P.P;
    const int nslabs = (int)((m_end - m_begin + WG_BT - 1) / WG_BT);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    Pixel px[4];                                                    // (a pixel past P decodes to img >= n and is never dereferenced: m < m_end fails)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned m = (unsigned)(m_begin + (threadIdx.x >> 3) + 32 * i), t = m / (unsigned)P.Wo;
        px[i] = Pixel{(int)(t / (unsigned)P.Ho), (int)(t % (unsigned)P.Ho), (int)(m % (unsigned)P.Wo)};
    }

    u32x4 ra[4], rb[4];
    load_dy_slab(P, co0, m_begin, m_end, ra);
    load_x_slab(P, ci0, ky, kx, m_begin, m_end, px, rb);
    for (int s = 0; s < nslabs; ++s) {
        store_slab(sa, ra);
        store_slab(sb, rb);
        __syncthreads();
        if (s + 1 < nslabs) {                         // next slab into registers under this slab's MFMAs
            const int64_t m1 = m_begin + (int64_t)(s + 1) * WG_BT;
            advance(P, px);
            load_dy_slab(P, co0, m1, m_end, ra);
            load_x_slab(P, ci0, ky, kx, m1, m_end, px, rb);
        }
        slab_mfma(sa, sb, wave, lane, acc);
        __syncthreads();
    }

    spill_tiles(red, wave, lane, acc);
    __syncthreads();
    const bool direct = P.splits == 1;
    float* part = direct ? nullptr : P.ws + (int64_t)split * P.Cout * 9 * P.Cin;
#pragma unroll 4
    for (int x = 0; x < 16; ++x) {
        const int e = threadIdx.x + 256 * x;
        const int l = e & 63, reg = (e >> 6) & 15, ij = e >> 10;
        const int co = co0 + 32 * (ij >> 1) + (reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5);
        const int ci = ci0 + 32 * (ij & 1) + (l & 31);
        if (co >= P.Cout || ci >= P.Cin) continue;
        const float v = ((red[e] + red[4096 + e]) + red[2 * 4096 + e]) + red[3 * 4096 + e];
        if (!direct) {
            part[dw_index(1, co, tap, ci, P.Cin)] = v;
        } else {
            float* o = P.dw + dw_index(P.layout, co, tap, ci, P.Cin);
            *o = P.accumulate ? __fmaf_rn(P.alpha, v, *o) : P.alpha * v;
        }
    }
}

// dW = alpha * sum_s ws[s] (+ dW), the splits summed in order.  One workgroup per (co, 64 ci): the 9 x 64 partial sums are read along ci and,
// for the [Cout][Cin][3][3] layout, turned through LDS so that dW is written as one run of consecutive words.
__global__ void __launch_bounds__(256) conv_wgrad_combine_kernel(const CwParams P) {
    __shared__ float turn[9 * WG_BK];
    const int co = (int)blockIdx.x / P.tiles_ci, ci0 = ((int)blockIdx.x % P.tiles_ci) * WG_BK;
    const int cw = P.Cin - ci0 < WG_BK ? P.Cin - ci0 : WG_BK;
    const int64_t plane = (int64_t)P.Cout * 9 * P.Cin;
    for (int e = threadIdx.x; e < 9 * cw; e += 256) {
        const int tap = e / cw, ci = ci0 + e % cw;
        const float* w = P.ws + dw_index(1, co, tap, ci, P.Cin);
        float s = w[0];
        for (int i = 1; i < P.splits; ++i) s += w[i * plane];
        if (P.layout == 0) {
            turn[e] = s;
        } else {
            float* o = P.dw + dw_index(1, co, tap, ci, P.Cin);
            *o = P.accumulate ? __fmaf_rn(P.alpha, s, *o) : P.alpha * s;
        }
    }
    if (P.layout != 0) return;
    __syncthreads();
    float* o = P.dw + dw_index(0, co, 0, ci0, P.Cin);                // the 9 cw words of (co, ci0 .. ci0 + cw) are consecutive
    for (int e = threadIdx.x; e < 9 * cw; e += 256) {
        const float s = turn[(e % 9) * cw + e / 9];
        o[e] = P.accumulate ? __fmaf_rn(P.alpha, s, o[e]) : P.alpha * s;
    }
}

// Splits of the pixel reduction: a function of the shape alone.  The kernel reaches its rate from about 900 workgroups on (3.5 per CU: measured
// at 675, 900, 1890 and 3510, profiles/conv_wgrad.md), and every split beyond the first writes and re-reads a [Cout][9][Cin] fp32 partial:
// the splits bring `wgs` to the nearest multiple towards CW_TARGET workgroups, and a split reduces at least WG_MIN_SLABS slabs.
constexpr int CW_TARGET = 1024;
void conv_split_plan(int64_t pixels, int64_t wgs, int& splits, int& chunk_slabs) {
    const int64_t slabs = (pixels + WG_BT - 1) / WG_BT;
    int64_t s = (CW_TARGET + wgs / 2) / wgs;
    if (s > slabs / WG_MIN_SLABS) s = slabs / WG_MIN_SLABS;
    if (s < 1) s = 1;
    chunk_slabs = (int)((slabs + s - 1) / s);
    splits = (int)((slabs + chunk_slabs - 1) / chunk_slabs);
}

bool in_domain(int n, int H, int W, int Cin, int Cout, int stride) {
    if (n < 1 || H < 1 || W < 1 || Cin < 16 || Cout < 16 || Cin % 16 || Cout % 16 || (stride != 1 && stride != 2)) return false;
    const int64_t Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const int64_t lim = (int64_t)1 << 31;
    // the pixel index and the grid are 32-bit; X, dY and dW are addressed in 64 bits
    if (n * Ho * Wo >= lim || (int64_t)Cout * 9 * Cin >= lim) return false;
    const int64_t tiles = (int64_t)((Cout + WG_BN - 1) / WG_BN) * ((Cin + WG_BK - 1) / WG_BK);
    int splits, chunk;
    conv_split_plan(n * Ho * Wo, tiles * 9, splits, chunk);
    return (tiles + 7) / 8 * 8 * 9 * splits < lim;
}

int fill(CwParams& P, int n, int H, int W, int Cin, int Cout, int stride) {
    P.H = H; P.W = W; P.Cin = Cin; P.Cout = Cout; P.stride = stride;
    P.Ho = (H - 1) / stride + 1;
    P.Wo = (W - 1) / stride + 1;
    P.P = (int64_t)n * P.Ho * P.Wo;
    P.tiles_ci = (Cin + WG_BK - 1) / WG_BK;
    P.tiles = ((Cout + WG_BN - 1) / WG_BN) * P.tiles_ci;
    P.tiles_pad = (P.tiles + 7) / 8 * 8;
    conv_split_plan(P.P, (int64_t)P.tiles * 9, P.splits, P.chunk_slabs);
    P.step_x = WG_BT % P.Wo;
    P.step_y = (WG_BT / P.Wo) % P.Ho;
    P.step_img = (WG_BT / P.Wo) / P.Ho;
    return 0;
}

int check(int n, int H, int W, int Cin, int Cout, int stride) {
    if (!in_domain(n, H, W, Cin, Cout, stride))
        FMC_FAIL(FMC_E_SHAPE, "conv3x3_wgrad_bf16: needs n, H, W >= 1, Cin %% 16 == Cout %% 16 == 0, stride 1 or 2 and fewer than 2^31 output pixels "
                              "and filter elements (n=%d H=%d W=%d Cin=%d Cout=%d stride=%d)", n, H, W, Cin, Cout, stride);
    return 0;
}

}  // namespace

extern "C" int fmc_conv3x3_wgrad_supported(int n_img, int H, int W, int Cin, int Cout, int stride) {
    return in_domain(n_img, H, W, Cin, Cout, stride) ? 1 : 0;
}

extern "C" int64_t fmc_conv3x3_wgrad_workspace_bytes(int n_img, int H, int W, int Cin, int Cout, int stride) {
    if (check(n_img, H, W, Cin, Cout, stride)) return -1;
    CwParams P{};
    fill(P, n_img, H, W, Cin, Cout, stride);
    return P.splits > 1 ? (int64_t)P.splits * Cout * 9 * Cin * 4 : 0;
}

extern "C" int fmc_conv3x3_wgrad_bf16(const void* x, const void* dy, float* dw, int n_img, int H, int W, int Cin, int Cout, int stride,
                                      int dw_layout, float alpha, int accumulate, void* workspace, int64_t ws_bytes, void* stream) {
    if (!x || !dy || !dw) FMC_FAIL(FMC_E_NULL, "conv3x3_wgrad_bf16: NULL tensor");
    if (int rc = check(n_img, H, W, Cin, Cout, stride)) return rc;
    if (dw_layout != FMC_DW_OIHW && dw_layout != FMC_DW_OHWI)
        FMC_FAIL(FMC_E_SHAPE, "conv3x3_wgrad_bf16: dw_layout is FMC_DW_OIHW (0) or FMC_DW_OHWI (1), got %d", dw_layout);
    if (!fmc_aligned16(x) || !fmc_aligned16(dy) || (reinterpret_cast<uintptr_t>(dw) & 3u))
        FMC_FAIL(FMC_E_ALIGN, "conv3x3_wgrad_bf16: x and dy must be 16-byte aligned, dw 4-byte aligned");
    CwParams P{};
    fill(P, n_img, H, W, Cin, Cout, stride);
    const int64_t need = P.splits > 1 ? (int64_t)P.splits * Cout * 9 * Cin * 4 : 0;
    if (need > 0 && !workspace) FMC_FAIL(FMC_E_NULL, "conv3x3_wgrad_bf16: the split reduction needs a workspace of %lld bytes", (long long)need);
    if (need > ws_bytes) FMC_FAIL(FMC_E_SHAPE, "conv3x3_wgrad_bf16: workspace of %lld bytes, need %lld", (long long)ws_bytes, (long long)need);
    if (need > 0 && (reinterpret_cast<uintptr_t>(workspace) & 3u)) FMC_FAIL(FMC_E_ALIGN, "conv3x3_wgrad_bf16: workspace must be 4-byte aligned");
    P.x = (const bf16_t*)x; P.dy = (const bf16_t*)dy; P.dw = dw; P.ws = need > 0 ? (float*)workspace : nullptr;
    P.layout = dw_layout; P.alpha = alpha; P.accumulate = accumulate != 0;
    hipStream_t st = (hipStream_t)stream;
    fmc_launch<conv_wgrad_kernel>(dim3((unsigned)((int64_t)P.tiles_pad * 9 * P.splits)), dim3(256), WG_LDS, st, P);
    FMC_CHECK_LAUNCH("fmc_conv3x3_wgrad_bf16");
    if (P.splits > 1) {
        hipLaunchKernelGGL(conv_wgrad_combine_kernel, dim3((unsigned)(Cout * P.tiles_ci)), dim3(256), 0, st, P);
        FMC_CHECK_LAUNCH("fmc_conv3x3_wgrad_bf16 (combine)");
    }
    return 0;
}

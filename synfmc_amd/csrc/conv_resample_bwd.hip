// Backward-data of the two resampling convolutions of the frozen U-Net (training): the 3x3 / stride-2 / pad-1 convolution of Downsample2D and
// conv3x3(nearest2x(x)) of Upsample2D.  Neither is a stride-1 convolution of dY, and neither multiplies a zero here:
//
//   stride 2:  dX[2i+py, 2j+px, ci] = sum_{(ky,di) in T[py]} sum_{(kx,dj) in T[px]} sum_co W[co][ci][ky][kx] dY[i+di, j+dj, co]
//              T[0] = {(1, 0)}, T[1] = {(2, 0), (0, +1)}: four convolutions of 1 / 2 / 2 / 4 taps, one per output parity, stored pixel-shuffled;
//   upsample:  dX[u, v, ci] = sum_{r,c = 0..3} sum_co G[co][ci][r][c] dY[2u-1+r, 2v-1+c, co]
//              rows of G from rows of W: r0 = w[2], r1 = w[1] + w[2], r2 = w[0] + w[1], r3 = w[0] (columns likewise): the transpose of the fold of
//              fmc_conv3x3_upfold_pack_weight, summed in fp32 in that routine's order and rounded to bf16 once.
//
// Both are one GEMM per tap over Cout: D[ci][pixel] += Wp[tap][ci][co] dY[source pixel of (pixel, tap)][co] on v_mfma_f32_16x16x32_bf16 with the filter as
// the A operand, so that a lane ends with 4 consecutive input channels of one pixel (one 8-byte store).  A wave owns 16 PB pixels x 16 CB channels
// (PB x CB accumulators) and takes both operands straight from global memory: the filter is packed in fragment order (a wave's load is 1 KiB
// contiguous), dY is read 16 bytes per lane with the four lanes of a pixel covering 64 contiguous bytes.  The four waves of a workgroup are neighbours
// in one flat list of tiles, channel tile fastest: they share their dY pixels in the vector cache.  No operand passes through LDS and there are no atomics: one fixed
// order of accumulation per output, bit-reproducible launch to launch.  A source pixel outside dY (or a pixel past the end of the last tile) is a ZERO
// fragment chosen by select, never a load, so nothing outside dY is read and nothing there can reach the result; a tap none of whose 16 PB pixels has a
// source is skipped by the whole wave.
//
// The stride-2 launcher picks (PB, CB) = (2, 4), (1, 4) or (1, 2), the largest whose tiles give every SIMD two waves.  The upsample launcher keeps
// (2, 4) -- every halving of the pixel tile reads the 16-tap filter once more -- and where those tiles are too few (every map of a 256 x 384 clip) it
// splits the reduction over the four rows of G among the four waves of a workgroup, added in a fixed order through LDS: 384 pixels x 1280 channels (the
// 4x6 maps of a 16-frame clip) are 960 waves.  The launches take the choice as their `tile` argument (0: this rule, what *_bwd_tile returns; stride 2: 1 / 2 / 3
// = the three tiles in that order; upsample: 1 unsplit, 2 split), so that a test can run every instantiation at any shape.
#include "common.h"

namespace {

struct ResampleBwdParams {
    const bf16_t* dy;      // [n][Hd][Wd][Cout]
    const bf16_t* wp;      // packed filter, below
    bf16_t* dx;            // [n][Ho][Wo][Cin]
    int Hd, Wd, Ho, Wo, Cin, Cout;
    int Hq, Wq;            // the pixel grid a tile index runs over: dY's (stride 2: one output per parity and dY pixel) or dX's (upsample)
    int64_t M;             // pixels of that grid over all images
    int n_ci_tiles;        // Cin / (16 CB)
    int64_t n_tiles;       // pixel tiles x channel tiles
};

// packed filter: [slot][Cin / 16][Cout / 32][64 lanes][8]; lane l of fragment (slot, cib, ks) holds W[co = 32 ks + 8 (l >> 4) + j][ci = 16 cib + (l & 15)],
// j = 0..7: the A operand of v_mfma_f32_16x16x32_bf16 as the lane wants it.  slot = 3 ky + kx (stride 2, the raw filter) or 4 r + c (upsample, G).
__global__ __launch_bounds__(256) void resample_bwd_pack_kernel(const bf16_t* __restrict__ w, bf16_t* __restrict__ dst, int cin, int cout, int up) {
    const int nks = cout >> 5, ncib = cin >> 4, slots = up ? 16 : 9;
    const int64_t total = (int64_t)slots * ncib * nks * 64;
    for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (int64_t)gridDim.x * blockDim.x) {
        int64_t t = id;
        const int lane = (int)(t & 63); t >>= 6;
        const int ks = (int)(t % nks); t /= nks;
        const int cib = (int)(t % ncib);
        const int slot = (int)(t / ncib);
        const int ci = cib * 16 + (lane & 15), co0 = ks * 32 + 8 * (lane >> 4);
        int ky0, ky1, kx0, kx1;
        if (up) {
            const int r = slot >> 2, c = slot & 3;
            ky0 = r == 0 ? 2 : (r == 1 ? 1 : 0); ky1 = r <= 1 ? 2 : (r == 2 ? 1 : 0);
            kx0 = c == 0 ? 2 : (c == 1 ? 1 : 0); kx1 = c <= 1 ? 2 : (c == 2 ? 1 : 0);
        } else {
            ky0 = ky1 = slot / 3;
            kx0 = kx1 = slot % 3;
        }
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float s = 0.f;
            for (int ky = ky0; ky <= ky1; ++ky)
                for (int kx = kx0; kx <= kx1; ++kx) s += bf2f(w[((int64_t)(co0 + j) * 9 + ky * 3 + kx) * cin + ci]);
            v[j] = s;
        }
        Vec8<bf16_t>::store(dst + id * 8, v);
    }
}

// MODE 0: stride 2 (blockIdx.y = output parity 2 py + px), 1: upsample.  SPLIT = 4 (upsample): the four waves of a workgroup share ONE tile and take one
// row of G each (4 of the 16 taps); waves 1..3 leave their accumulators in LDS and wave 0 adds them in the order 0 + 1 + 2 + 3 and stores.
template <int MODE, int PB, int CB, int SPLIT>
__global__ __launch_bounds__(256) void resample_bwd_kernel(const ResampleBwdParams p) {
    static_assert(SPLIT == 1 || (SPLIT == 4 && MODE == 1), "the split is over the four rows of G");
    __shared__ float red[SPLIT == 4 ? 3 * PB * CB * 256 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g = SPLIT == 4 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave;
    if (g >= p.n_tiles) return;                      // (SPLIT = 4: the whole workgroup)
    const int ct = (int)(g % p.n_ci_tiles);
    const int64_t pt = g / p.n_ci_tiles;
    const int l15 = lane & 15, lq = lane >> 4;
    const int py = MODE == 0 ? (int)(blockIdx.y >> 1) : 0, px = MODE == 0 ? (int)(blockIdx.y & 1) : 0;

    int pn[PB], pi[PB], pj[PB];
    bool pv[PB];
#pragma unroll
    for (int b = 0; b < PB; ++b) {
        const int64_t m = pt * (16 * PB) + b * 16 + l15;
        pv[b] = m < p.M;
        const int64_t mm = pv[b] ? m : 0;
        pj[b] = (int)(mm % p.Wq);
        pi[b] = (int)((mm / p.Wq) % p.Hq);
        pn[b] = (int)(mm / ((int64_t)p.Wq * p.Hq));
    }

    f32x4 acc[PB][CB];
#pragma unroll
    for (int b = 0; b < PB; ++b)
#pragma unroll
        for (int c = 0; c < CB; ++c) acc[b][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nks = p.Cout >> 5;
    const int ny = MODE == 0 ? 1 + py : 4, nx = MODE == 0 ? 1 + px : 4;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int ta = SPLIT == 4 ? wave : 0; ta < (SPLIT == 4 ? wave + 1 : ny); ++ta)
        for (int tb = 0; tb < nx; ++tb) {
            int slot, oy, ox;                        // source pixel = (scale * i + oy, scale * j + ox)
            if (MODE == 0) {
                const int ky = py == 0 ? 1 : (ta == 0 ? 2 : 0), kx = px == 0 ? 1 : (tb == 0 ? 2 : 0);
                slot = ky * 3 + kx;
                oy = (py == 1 && ta == 1) ? 1 : 0;
                ox = (px == 1 && tb == 1) ? 1 : 0;
            } else {
                slot = ta * 4 + tb;
                oy = ta - 1;
                ox = tb - 1;
            }
            const bf16_t* src[PB];
            bool sv[PB];
            bool any = false;
#pragma unroll
            for (int b = 0; b < PB; ++b) {
                const int sy = (MODE == 0 ? pi[b] : 2 * pi[b]) + oy, sx = (MODE == 0 ? pj[b] : 2 * pj[b]) + ox;
                sv[b] = pv[b] && sy >= 0 && sy < p.Hd && sx >= 0 && sx < p.Wd;
                src[b] = p.dy + (sv[b] ? (((int64_t)pn[b] * p.Hd + sy) * p.Wd + sx) * p.Cout + lq * 8 : 0);
                any = any || sv[b];
            }
            if (__ballot(any) == 0) continue;        // (wave-uniform)
            const bf16_t* wf = p.wp + (((int64_t)slot * (p.Cin >> 4) + (int64_t)ct * CB) * nks) * 512 + lane * 8;
            for (int ks = 0; ks < nks; ks += 2) {    // (Cout % 64 == 0: two k-steps a trip, all their loads in front of the MFMAs)
                u32x4 bfr[2][PB], afr[2][CB];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
#pragma unroll
                    for (int b = 0; b < PB; ++b) bfr[u][b] = sv[b] ? *reinterpret_cast<const u32x4*>(src[b] + (ks + u) * 32) : zero;
#pragma unroll
                    for (int c = 0; c < CB; ++c) afr[u][c] = *reinterpret_cast<const u32x4*>(wf + ((int64_t)c * nks + ks + u) * 512);
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int b = 0; b < PB; ++b)
#pragma unroll
                        for (int c = 0; c < CB; ++c)
                            acc[b][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, afr[u][c]), __builtin_bit_cast(bf16x8, bfr[u][b]),
                                                                                acc[b][c], 0, 0, 0);
            }
        }

    if constexpr (SPLIT == 4) {
        if (wave > 0) {
#pragma unroll
            for (int b = 0; b < PB; ++b)
#pragma unroll
                for (int c = 0; c < CB; ++c)
#pragma unroll
                    for (int i = 0; i < 4; ++i) red[(((wave - 1) * PB * CB + b * CB + c) * 4 + i) * 64 + lane] = acc[b][c][i];
        }
        __syncthreads();
        if (wave > 0) return;
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int b = 0; b < PB; ++b)
#pragma unroll
                for (int c = 0; c < CB; ++c)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[b][c][i] += red[((s * PB * CB + b * CB + c) * 4 + i) * 64 + lane];
    }

    // D: column = lane & 15 = pixel, row = 4 (lane >> 4) + register = input channel
#pragma unroll
    for (int b = 0; b < PB; ++b) {
        const int oy = MODE == 0 ? 2 * pi[b] + py : pi[b], ox = MODE == 0 ? 2 * pj[b] + px : pj[b];
        bf16_t* o = p.dx + (((int64_t)pn[b] * p.Ho + oy) * p.Wo + ox) * p.Cin + (ct * CB) * 16 + lq * 4;
        if (pv[b]) {
#pragma unroll
            for (int c = 0; c < CB; ++c)
                *reinterpret_cast<u32x2*>(o + c * 16) = u32x2{pack_bf2(acc[b][c][0], acc[b][c][1]), pack_bf2(acc[b][c][2], acc[b][c][3])};
        }
    }
}

const int64_t kMaxBytes = (int64_t)1 << 31;

bool resample_bwd_ok(int up, int n_img, int Hx, int Wx, int Cin, int Cout) {       // Hx x Wx: the forward's INPUT (= dX) size
    if (n_img < 1 || Cin < 64 || Cout < 64 || Cin % 64 || Cout % 64) return false;
    if (up ? (Hx < 1 || Wx < 1) : (Hx < 2 || Wx < 2 || Hx % 2 || Wx % 2)) return false;
    const int64_t px = (int64_t)n_img * Hx * Wx;
    const int64_t dx_bytes = px * Cin * 2, dy_bytes = (up ? px * 4 : px / 4) * Cout * 2;
    return dx_bytes < kMaxBytes && dy_bytes < kMaxBytes && (int64_t)(up ? 16 : 9) * Cin * Cout * 2 < kMaxBytes;
}

int pack(const char* what, int up, const void* w, void* dst, int Cin, int Cout, void* stream) {
    if (!w || !dst) FMC_FAIL(FMC_E_NULL, "%s: NULL pointer", what);
    if (Cin < 64 || Cout < 64 || Cin % 64 || Cout % 64 || (int64_t)16 * Cin * Cout * 2 >= kMaxBytes)
        FMC_FAIL(FMC_E_SHAPE, "%s: Cin %% 64, Cout %% 64 (Cin=%d Cout=%d)", what, Cin, Cout);
    if (!fmc_aligned16(w) || !fmc_aligned16(dst)) FMC_FAIL(FMC_E_ALIGN, "%s: pointers must be 16-byte aligned", what);
    const int64_t chunks = (int64_t)(up ? 16 : 9) * Cin * Cout / 8;
    const int grid = (int)((chunks + 255) / 256 < 4096 ? (chunks + 255) / 256 : 4096);
    fmc_launch<resample_bwd_pack_kernel>(dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, (bf16_t*)dst, Cin, Cout, up);
    FMC_CHECK_LAUNCH(what);
    return FMC_OK;
}

template <int MODE, int PB, int CB, int SPLIT>
void launch_tile(ResampleBwdParams p, hipStream_t st) {
    p.n_ci_tiles = p.Cin / (16 * CB);
    p.n_tiles = ((p.M + 16 * PB - 1) / (16 * PB)) * p.n_ci_tiles;
    fmc_launch<resample_bwd_kernel<MODE, PB, CB, SPLIT>>(dim3((unsigned)(SPLIT == 4 ? p.n_tiles : (p.n_tiles + 3) / 4), MODE == 0 ? 4 : 1), dim3(256), 0, st,
                                                         p);
}

// the launcher's own choice: stride 2 -> 1 / 2 / 3 = (PB, CB) (2, 4) / (1, 4) / (1, 2); upsample -> 1 = unsplit, 2 = split over the rows of G
int auto_tile(int up, int n_img, int Hx, int Wx, int Cin) {
    const int64_t M = up ? (int64_t)n_img * Hx * Wx : (int64_t)n_img * (Hx / 2) * (Wx / 2);
    const int64_t want = (int64_t)fmc_cu_count() * 8;            // two waves on every SIMD
    auto waves = [&](int pb, int cb) { return ((M + 16 * pb - 1) / (16 * pb)) * (Cin / (16 * cb)) * (up ? 1 : 4); };
    // (upsample: smaller tiles would read the filter once more per halving -- 52 MB at 1280 x 1280, the 4x6 maps are bound by it; the rows of G give the waves)
    if (up) return waves(2, 4) >= want ? 1 : 2;
    return waves(2, 4) >= want ? 1 : (waves(1, 4) >= want ? 2 : 3);
}

template <int MODE>
int launch(const char* what, const void* dy, const void* wp, void* dx, int n_img, int Hx, int Wx, int Cin, int Cout, int tile, void* stream) {
    if (!dy || !wp || !dx) FMC_FAIL(FMC_E_NULL, "%s: NULL pointer", what);
    if (!resample_bwd_ok(MODE, n_img, Hx, Wx, Cin, Cout))
        FMC_FAIL(FMC_E_SHAPE, "%s: Cin %% 64, Cout %% 64, %s, tensors below 2^31 bytes (n=%d %dx%d Cin=%d Cout=%d)", what,
                 MODE ? "Hs, Ws >= 1" : "even H, W >= 2", n_img, Hx, Wx, Cin, Cout);
    if (tile < 0 || tile > (MODE ? 2 : 3)) FMC_FAIL(FMC_E_SHAPE, "%s: tile %d (0 = the launcher's choice, 1 .. %d)", what, tile, MODE ? 2 : 3);
    if (!fmc_aligned16(dy) || !fmc_aligned16(wp) || !fmc_aligned16(dx)) FMC_FAIL(FMC_E_ALIGN, "%s: pointers must be 16-byte aligned", what);
    ResampleBwdParams p;
    p.dy = (const bf16_t*)dy; p.wp = (const bf16_t*)wp; p.dx = (bf16_t*)dx;
    p.Ho = Hx; p.Wo = Wx; p.Cin = Cin; p.Cout = Cout;
    p.Hd = MODE ? 2 * Hx : Hx / 2; p.Wd = MODE ? 2 * Wx : Wx / 2;
    p.Hq = MODE ? Hx : p.Hd; p.Wq = MODE ? Wx : p.Wd;
    p.M = (int64_t)n_img * p.Hq * p.Wq;
    p.n_ci_tiles = 0; p.n_tiles = 0;
    if (tile == 0) tile = auto_tile(MODE, n_img, Hx, Wx, Cin);
    hipStream_t st = (hipStream_t)stream;
    if constexpr (MODE == 0) {
        if (tile == 1) launch_tile<0, 2, 4, 1>(p, st);
        else if (tile == 2) launch_tile<0, 1, 4, 1>(p, st);
        else launch_tile<0, 1, 2, 1>(p, st);
    } else {
        if (tile == 1) launch_tile<1, 2, 4, 1>(p, st);
        else launch_tile<1, 2, 4, 4>(p, st);
    }
    FMC_CHECK_LAUNCH(what);
    return FMC_OK;
}

}  // namespace

extern "C" int fmc_conv3x3_down_bwd_supported(int n_img, int H, int W, int Cin, int Cout) { return resample_bwd_ok(0, n_img, H, W, Cin, Cout) ? 1 : 0; }
extern "C" int64_t fmc_conv3x3_down_bwd_packed_bytes(int Cin, int Cout) { return (int64_t)9 * Cin * Cout * 2; }
extern "C" int fmc_conv3x3_down_bwd_pack_weight(const void* w, void* dst, int Cin, int Cout, void* stream) {
    return pack("fmc_conv3x3_down_bwd_pack_weight", 0, w, dst, Cin, Cout, stream);
}
extern "C" int fmc_conv3x3_down_bwd_tile(int n_img, int H, int W, int Cin, int Cout) {
    return resample_bwd_ok(0, n_img, H, W, Cin, Cout) ? auto_tile(0, n_img, H, W, Cin) : 0;
}
extern "C" int fmc_conv3x3_down_bwd_bf16(const void* dy, const void* w_packed, void* dx, int n_img, int H, int W, int Cin, int Cout, int tile,
                                         void* stream) {
    return launch<0>("fmc_conv3x3_down_bwd_bf16", dy, w_packed, dx, n_img, H, W, Cin, Cout, tile, stream);
}

extern "C" int fmc_conv3x3_up_bwd_supported(int n_img, int Hs, int Ws, int Cin, int Cout) { return resample_bwd_ok(1, n_img, Hs, Ws, Cin, Cout) ? 1 : 0; }
extern "C" int64_t fmc_conv3x3_up_bwd_packed_bytes(int Cin, int Cout) { return (int64_t)16 * Cin * Cout * 2; }
extern "C" int fmc_conv3x3_up_bwd_pack_weight(const void* w, void* dst, int Cin, int Cout, void* stream) {
    return pack("fmc_conv3x3_up_bwd_pack_weight", 1, w, dst, Cin, Cout, stream);
}
extern "C" int fmc_conv3x3_up_bwd_tile(int n_img, int Hs, int Ws, int Cin, int Cout) {
    return resample_bwd_ok(1, n_img, Hs, Ws, Cin, Cout) ? auto_tile(1, n_img, Hs, Ws, Cin) : 0;
}
extern "C" int fmc_conv3x3_up_bwd_bf16(const void* dy, const void* w_packed, void* dx, int n_img, int Hs, int Ws, int Cin, int Cout, int tile,
                                       void* stream) {
    return launch<1>("fmc_conv3x3_up_bwd_bf16", dy, w_packed, dx, n_img, Hs, Ws, Cin, Cout, tile, stream);
}

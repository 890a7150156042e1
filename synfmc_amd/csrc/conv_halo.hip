// Implicit-GEMM 3x3 convolution for gfx950 with the INPUT HALO TILE RESIDENT IN LDS and GroupNorm + SiLU applied while it is staged
// ("GN+SiLU prologue fused into implicit-GEMM 3x3 conv, temb add + GN stats epilogue").
// Replaces, on the FMC path, conv1 / conv2 of diffusers' ResnetBlock2D together with the `nonlinearity(norm(x))` in front of them
// (ctor args fmc/models/unet_blocks.py:306-317; `InflatedConv3d` fmc/models/resnet.py:16-24, `InflatedGroupNorm` :27-37) and the conv of
// Upsample2D (unet_blocks.py:625).
//
// Why a second conv kernel.  gemm160_kernel / gemm8_kernel (gemm_conv.hip) fetch the A operand tap by tap: every input pixel travels
// L2 -> LDS NINE times, and the loop is bound by its `buffer_load ... lds` instruction stream (~15 ns per 1-KiB request and CU, serial to the
// matrix work: gemm_conv.hip, "What bounds the loop").  Here a workgroup owns 10 x 32 output pixels of ONE image x 160 output channels:
//   * the 12 x 34 input halo of a 64-channel chunk is staged ONCE (global -> registers -> LDS) and serves all 9 taps x 2 k-halves: A traffic
//     falls 9 x 320 / 408 = 7x, and because it passes through registers the consumer's GroupNorm + SiLU is applied on the way
//     (`silu(x * a[c] + b[c])`, a / b per (image, channel) from fmc_groupnorm_coef) -- the normalised tensor is never written or read;
//   * only W is streamed by LDS-DMA: 10 one-KiB requests per 32-deep sub-tile and CU instead of 30 (the tile is 320 pixels x 160 channels:
//     the cheap operand gets the long side), from a copy of the filter pre-packed in the kernel's own sub-tile order;
//   * the MFMA loop itself is gemm160_kernel's: 8 waves = 4 (pixels) x 2 (channels), a wave = 80 x 80 outputs as 5 x 5
//     v_mfma_f32_16x16x32_bf16, one 32-deep sub-tile per phase {LOAD | barrier | 25 MFMAs | barrier}, the two wave halves one barrier apart.
// LDS: halo double buffer 2 x 53,248 B ([8 sixteen-byte channel groups][416 pixels] x 16 B: a fragment read of ANY tap is conflict free,
// see halo_px_slot) + W ring 5 x 10,240 B + GroupNorm coefficients 2 x 512 B = 158,720 B.
//
// Roofline: MFMA bound.  Algorithmic flops per launch = 2 * n_img*H*W * Cout * 9*Cin; algorithmic bytes = x + w + out (+ residual).
//
// Image width: fmc_conv3x3_halo_bf16 / _sc_bf16 / _fold_bf16 take W % 32 == 0 (tiles_x = W / 32); the *_partial_* entry points (`PARTIAL`, see conv_halo_kernel) take
// any W >= 1 with tiles_x = ceil(W / 32) and a partly filled last column tile, on the same packed filters.  The whole-tile instantiations are the
// instruction streams they were (profiles/partial_tiles.md section 15); what the partial launches cost per shape is in section 17.
//
// What this kernel shares with its small-feature-map geometry (conv_halo4.hip) -- the common parameters, halo piece addressing, the W stream, the
// filter pack kernels (compiled here), the host-side checks -- is in conv_halo_common.h.
#include "conv_halo_common.h"

namespace {

using halo::IC;
constexpr int TH = 10, TW = 32, BM = TH * TW, BN = 160;
constexpr int HWID = TW + 2, HPIX = (TH + 2) * HWID;       // 34 x 12 = 408 halo pixels
constexpr int NP = 416;                                    // pixels per channel-group plane (a multiple of 16: every plane starts at the same bank)
constexpr int PLANE = NP * 16;                             // bytes
constexpr int HALO = 8 * PLANE;                            // one 64-channel chunk of the halo: 53,248 B
constexpr int NBW = 5;                                     // W ring depth: three sub-tiles in flight (requested at LOAD(s - 3))
constexpr int WSUB = BN * 64;                              // one 32-deep W sub-tile: 160 rows x 64 B
constexpr int OFF_W = 2 * HALO, OFF_COEF = OFF_W + NBW * WSUB;
constexpr int LDS_BYTES = OFF_COEF + 2 * 512;              // 158,720
constexpr int NPIECE = 7;                                  // halo pieces (16 B) per thread and chunk: 51 blocks of 8 pixels x 8 channel groups over 8 waves

struct CHParams : halo::Params {
    const float* gn_coef; int gn_act;       // [n_img, cin, 2] (scale, shift) or NULL; gn_act: SiLU behind the affine map
    float* gn_part;                         // [n_img, tiles_y * tiles_x, 32, 2] partial (sum, sum of squares) of the ROUNDED outputs, or NULL
    int tiles_y, tiles_x, tiles_n;
    int64_t x_bytes, x2_bytes, w_bytes;
};
// SC: the block's 1x1 shortcut as a centre-tap segment of the same reduction (see conv_halo_kernel)
struct CHParamsSC : CHParams {
    const bf16_t* xs; const bf16_t* xs2;    // shortcut input [n_img, H, W, cs1] (+ [n_img, H, W, cin_sc - cs1]), raw
    int cs1, cin_sc;                        // both % 64 == 0
    int64_t xs_bytes, xs2_bytes;
};

__device__ __forceinline__ float silu_fast(float z) { return z * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * z)); }

// halo staging pieces issued / written in sub-tile i of a chunk (18 sub-tiles): piece j is requested at LOAD(2 j) and written at LOAD(2 j + 3)
constexpr int nh(int i) { return (i >= 0 && i <= 12 && (i & 1) == 0) ? 1 : 0; }

// phase mode (PH): halo pieces requested in sub-tile i of a chunk of 8 sub-tiles: pieces 2 i, 2 i + 1 at LOAD(i), i = 0 .. 3, written at LOAD(i + 3)
constexpr int nhp(int i) { return (i >= 0 && i <= 3) ? (i < 3 ? 2 : 1) : 0; }

// shortcut mode (SC): the interior of a shortcut chunk is 320 pixels x 8 channel groups = NSCP pieces per thread; those of shortcut chunk 1 are
// requested in sub-tile 16 of every 3x3 chunk (nothing is fetched before the last one: the counted waits do not depend on the chunk)
constexpr int NSCP = 5;
template <bool SC> constexpr int nreq(int i) { return nh(i) + (SC && i == 16 ? NSCP : 0); }

// GN: 0 = plain convolution, 1 = operand silu(x * scale + shift), 2 = operand x * scale + shift (compile-time: the normalisation has to sit in
// the SAME basic block as the MFMAs it is interleaved with)
//
// PH: the PHASE MODE of the nearest-2x upsample convolutions.  A 3x3 convolution of a nearest-2x-upsampled image is four 2x2-tap convolutions of
// the source image, one per output parity (py, px):  out[2 i + py, 2 j + px] = sum_{a, b in {0, 1}} Wf[py][px][a][b] . src[i + py - 1 + a, j + px - 1 + b]
// (source zero-padded by one pixel; Wf = sums of the filter's rows / columns, fmc_conv3x3_halo_fold_pack_weight).  The kernel then tiles the
// SOURCE pixels (the halo is that of a plain convolution at source resolution), the channel-tile index becomes (phase, channel tile), a 64-channel
// chunk is 4 taps x 2 k-halves = 8 sub-tiles instead of 18 (2.25 x fewer MFMAs for the same outputs), and the epilogue stores pixel-shuffled.
//
// SC: the SHORTCUT MODE of a ResnetBlock2D's second convolution.  conv2(a) + Ws . [xs | xs2] + b2 + bs is one reduction over K = 9 cin + cin_sc whose
// last cin_sc channels are multiplied at the centre tap only: behind the cin / 64 chunks of 18 sub-tiles the loop walks cin_sc / 64 shortcut chunks
// of 2 sub-tiles (centre tap x 2 k-halves) on the same accumulators, fragment addresses and W ring (the packed filter carries the 1x1 filter's
// sub-tiles behind the 3x3 ones: conv_halo_sc_pack_kernel).  The shortcut product is never rounded, written or read back; the two biases meet in
// the epilogue's bias + temb sum.  Staging: shortcut chunk 0 takes the place of "the next chunk" of the last 3x3 chunk; chunk k + 1's interior
// pieces are requested in the second sub-tile of chunk k - 1 and written in the second sub-tile of chunk k into the buffer chunk k - 1 released
// -- one sub-tile ahead of their first read, so that sub-tile drains its LDS operations in front of its first barrier.
//
// PARTIAL: images of ANY width.  tiles_x = ceil(W / TW), and the last column tile of a row holds min(TW, W - x0) real columns.  The main loop needs
// nothing: a halo pixel with x >= W is outside the image and staged as zeros already (h_pix = -1, in `ups` and GroupNorm mode alike), so a pad column
// is multiplied like any other and what it accumulates is dropped.  The shortcut interior pieces, the residual burst, the output stores and the
// statistics sums ask whether their column exists; every thread runs the same barriers and counted waits as in the whole-tile form.
template <int GN, bool PH = false, bool SC = false, bool PARTIAL = false>
__global__ __launch_bounds__(512, 2)
void conv_halo_kernel(const std::conditional_t<SC, CHParamsSC, CHParams> P) {
    static_assert(!SC || (GN == 0 && !PH), "the shortcut mode is a plain 9-tap convolution");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = wave >> 2, wq = wave & 3;
    const int wc = wq & 1, wr = half * 2 + (wq >> 1);        // my 80 channels / my 80 pixels of the tile
    const int l15 = lane & 15, kq = lane >> 4;
    const bool clsA = wave < 2;                              // waves 0, 1 issue two W pieces per sub-tile, the others one

    // ---- my tile ---------------------------------------------------------------------------------------------------------------------
    int tile_p, tile_n;
    {
        const int total = P.n_img * P.tiles_y * P.tiles_x * P.tiles_n;
        const int id = blockIdx.x, q = total >> 3, r = total & 7, xcd = id & 7;
        const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);      // XCD x owns a contiguous range of tiles:
        tile_p = lin / P.tiles_n;                                                                 // the channel tiles of a pixel tile are neighbours
        tile_n = lin - tile_p * P.tiles_n;                                                        // (its halo comes from that XCD's L2 once)
    }
    const int tpi = P.tiles_y * P.tiles_x;
    const int img = tile_p / tpi, tin = tile_p - img * tpi;
    const int y0 = (tin / P.tiles_x) * TH, x0 = (tin % P.tiles_x) * TW;
    constexpr int NS = PH ? 8 : 18;                          // sub-tiles per 64-channel chunk
    const int tn1 = P.cout / BN;
    const int phase = PH ? tile_n / tn1 : 0, py = phase >> 1, px_ = phase & 1;      // (PH: W tiles are [phase][channel tile])
    const int n0 = (tile_n - phase * tn1) * BN;
    const int nchunk = P.cin >> 6;
    int nsc = 0;                                             // (SC) shortcut chunks
    if constexpr (SC) nsc = P.cin_sc >> 6;
    const int nsub = nchunk * NS + 2 * nsc;

    // ---- halo staging: my seven (pixel, channel group) pieces --------------------------------------------------------------------------
    // block b = 8 j + wave holds halo pixels 8 b .. 8 b + 7 x 8 channel groups; lane = 8 g + p takes pixel p, channel group (p + g) & 7: the eight
    // lanes of a ds_write_b128 group write eight different pixels (bank groups) of eight planes, and the wave still covers 8 whole 128-byte lines
    const int Hs = P.ups ? P.H >> 1 : P.H, Ws = P.ups ? P.W >> 1 : P.W;
    const int pp = lane & 7, pg = ((lane & 7) + (lane >> 3)) & 7;
    int h_pix[NPIECE];                                       // source pixel index (image-major), or -1: outside the image / past the halo
#pragma unroll
    for (int j = 0; j < NPIECE; ++j) {
        const int b = 8 * j + wave, px = 8 * b + pp;
        const int hy = px / HWID, hx = px - hy * HWID;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        const bool in = b < HPIX / 8 && (unsigned)y < (unsigned)P.H && (unsigned)x < (unsigned)P.W;
        const int ys = P.ups ? y >> 1 : y, xs = P.ups ? x >> 1 : x;
        h_pix[j] = in ? (img * Hs + ys) * Ws + xs : -1;
    }
    const int h_lds = pg * PLANE + (8 * wave + pp) * 16;     // + j * 1024 (+ buffer): plane of my channel group, pixel 8 (8 j + wave) + pp
    const bool last_piece = wave < HPIX / 8 - 48;            // piece 6 exists for waves 0 .. 2 only (51 blocks of 8 pixels)
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)P.x, 0, (int)P.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsX2 = __builtin_amdgcn_make_buffer_rsrc((void*)(P.x2 ? P.x2 : P.x), 0, (int)(P.x2 ? P.x2_bytes : P.x_bytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)P.w, 0, (int)P.w_bytes, 0x00020000);
    const int c2 = P.cin - P.c1;
    u32x4 hreg[2];
    // (SC) chunk indices run on through the shortcut chunks: nchunk + k is chunk k of xs | xs2
    __amdgpu_buffer_rsrc_t rsS = rsX, rsS2 = rsX;
    int cs1 = 0, cs2 = 0;
    if constexpr (SC) {
        rsS = __builtin_amdgcn_make_buffer_rsrc((void*)P.xs, 0, (int)P.xs_bytes, 0x00020000);
        rsS2 = __builtin_amdgcn_make_buffer_rsrc((void*)(P.xs2 ? P.xs2 : P.xs), 0, (int)(P.xs2 ? P.xs2_bytes : P.xs_bytes), 0x00020000);
        cs1 = P.cs1; cs2 = P.cin_sc - P.cs1;
    }
    auto halo_load = [&](int j, int ch64, u32x4& dst) {
        if constexpr (SC) {
            const bool sc = ch64 >= nchunk;
            const int k = sc ? ch64 - nchunk : ch64;
            dst = halo::piece_load(sc ? rsS : rsX, sc ? rsS2 : rsX2, sc ? cs1 : P.c1, sc ? cs2 : c2, h_pix[j], pg, k * 64, k, sc ? nsc : nchunk);
        } else {
            dst = halo::piece_load(rsX, rsX2, P.c1, c2, h_pix[j], pg, ch64 * 64, ch64, nchunk);
        }
    };
    // (SC) interior piece j of shortcut chunk k: tile pixel 64 j + 8 wave + pp = row 2 j + (wave >> 2), column 8 (wave & 3) + pp; rows past the image
    // and chunks outside [0, nsc) fetch nothing
    const int sc_row = wave >> 2;
    const int sc_pix0 = (img * P.H + y0 + sc_row) * P.W + x0 + 8 * (wave & 3) + pp;
    const int sc_lds = pg * PLANE + ((sc_row + 1) * HWID + 8 * (wave & 3) + pp + 1) * 16;      // + j * 2 * HWID * 16 (+ buffer)
    u32x4 hsc[NSCP];
    auto sc_load = [&](int j, int k, u32x4& dst) {
        int hp = (k >= 0 && y0 + sc_row + 2 * j < P.H) ? sc_pix0 + 2 * j * P.W : -1;
        if constexpr (PARTIAL) hp = x0 + 8 * (wave & 3) + pp < P.W ? hp : -1;      // a pad column fetches nothing (the word there is the next row's)
        dst = halo::piece_load(rsS, rsS2, cs1, cs2, hp, pg, k * 64, k, nsc);
    };
    auto sc_store = [&](int j, int buf, const u32x4& v) { *reinterpret_cast<u32x4*>(smem_raw + buf * HALO + sc_lds + j * (2 * HWID * 16)) = v; };
    // GroupNorm + SiLU of one staged piece, registers only (runs INSIDE an MFMA phase: its ~64 VALU instructions fill the issue slots between
    // the 25 matrix instructions instead of lengthening a LOAD phase); the 16 coefficients come from LDS ([64 channels][scale, shift] per chunk)
    auto halo_transform = [&](int j, int coefbuf, const u32x4& raw) -> u32x4 {
        if constexpr (GN == 0) return raw;
        const f32x4* src = reinterpret_cast<const f32x4*>(smem_raw + OFF_COEF + coefbuf * 512 + pg * 64);
        float f[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) { f[2 * k] = __uint_as_float(raw[k] << 16); f[2 * k + 1] = __uint_as_float(raw[k] & 0xffff0000u); }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const f32x4 t = src[k];
            const float z0 = fmaf(f[2 * k], t[0], t[1]), z1 = fmaf(f[2 * k + 1], t[2], t[3]);
            f[2 * k] = GN == 1 ? silu_fast(z0) : z0;
            f[2 * k + 1] = GN == 1 ? silu_fast(z1) : z1;
        }
        const bool in = h_pix[j] >= 0;                       // the convolution pads the NORMALISED tensor with zeros
        u32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = in ? pack_bf2(f[2 * k], f[2 * k + 1]) : 0u;
        return v;
    };
    auto halo_store = [&](int j, int buf, const u32x4& v) {
        if (j == NPIECE - 1 && !last_piece) return;          // (wave-uniform)
        *reinterpret_cast<u32x4*>(smem_raw + buf * HALO + h_lds + j * 1024) = v;
    };
    // GroupNorm coefficients of chunk `ch64`: 128 floats, every thread fetches one (4 x redundant: identical per-wave VMEM counts)
    auto coef_fetch = [&](int ch64) -> float {
        const int cc = ch64 < nchunk ? ch64 : nchunk - 1;
        const float* src = GN ? P.gn_coef + ((size_t)img * P.cin + cc * 64) * 2 + (tid & 127) : reinterpret_cast<const float*>(P.w);
        return *src;
    };

    // ---- W stream ------------------------------------------------------------------------------------------------------------------------
    // packed filter: [tiles_n][sub-tile s = (chunk, tap, half)][160 rows][32] with the LDS chunk swizzle already applied: piece p = KiB p of the block
    // waves 0, 1 take pieces 0 .. 3 (two neighbours each), the others pieces 4 .. 9
    const int my_piece = clsA ? 2 * wave : wave + 2;
    const unsigned w_vo0 = (unsigned)(lane * 16 + my_piece * 1024);
    const int w_dst0 = OFF_W + my_piece * 1024;             // (the ring offset with my piece folded in: the address arithmetic of the loop as it was)
    halo::WStream<NBW, WSUB, 1024> ws;
    ws.start(tile_n * nsub * WSUB, nsub);
    auto w_issue = [&](auto cls) { ws.template issue<decltype(cls)::value>(smem_raw, rsW, w_vo0, w_dst0, 0, tile_n * nsub * WSUB, nsub); };

    // ---- fragments -----------------------------------------------------------------------------------------------------------------------
    f32x4 acc[5][5];
    bf16x8 wf[5], af[5];
    const int wfrag = OFF_W + ((wc * 80 + l15) * 32 + (kq ^ (3 * ((l15 >> 3) & 1))) * 8) * 2;     // + slot * WSUB + nb * 1024
    int afrag[5];                                            // + buf * HALO + half * 4 * PLANE + (ky * 34 + kx) * 16
#pragma unroll
    for (int mb = 0; mb < 5; ++mb) {
        const int idx = wr * 80 + mb * 16 + l15, ty = idx >> 5, tx = idx & 31;
        afrag[mb] = kq * PLANE + (ty * HWID + tx) * 16 + (PH ? (py * HWID + px_) * 16 : 0);      // (PH: tap (a, b) of phase (py, px) reads halo pixel + (py + a, px + b))
    }

    // ---- prologue: halo chunk 0, GroupNorm coefficients of chunks 0 and 1 ---------------------------------------------------------------------
    {
        u32x4 t[NPIECE];
#pragma unroll
        for (int j = 0; j < NPIECE; ++j) halo_load(j, 0, t[j]);
        const float c0v = coef_fetch(0), c1v = coef_fetch(1);
        if (tid < 128) {
            *reinterpret_cast<float*>(smem_raw + OFF_COEF + tid * 4) = c0v;
            *reinterpret_cast<float*>(smem_raw + OFF_COEF + 512 + tid * 4) = c1v;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NPIECE; ++j) halo_store(j, 0, halo_transform(j, 0, t[j]));
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

    // ---- main loop, instantiated per wave class (two / one W request per sub-tile: the counted waits differ) -----------------------------------
    auto main_loop = [&](auto cls) {
        constexpr int NW = decltype(cls)::value ? 2 : 1;
        int rd_slot = 0;
        w_issue(cls); w_issue(cls); w_issue(cls);             // W sub-tiles 0 .. 2 in flight, sub-tile 0 retired and published
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NW) : "memory");
        __builtin_amdgcn_s_barrier();
        if (half == 1) __builtin_amdgcn_s_barrier();       // wave half 1 runs one barrier behind half 0
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int b = 0; b < 5; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
        __builtin_amdgcn_sched_barrier(0);

        int cbuf = 0;                                        // halo (and coefficient) buffer of the chunk being multiplied
        float coef_next = 0.f;
        u32x4 hpk = {0u, 0u, 0u, 0u};
        u32x4 hregp[3][2];                                   // (PH) staged pieces in flight
        for (int c = 0; c < nchunk; ++c) {
            const int abase = cbuf * HALO, nbuf = cbuf ^ 1;
            if constexpr (PH) {
                // the same phases with 8 sub-tiles per chunk: the seven halo pieces of the next chunk are requested two at a time in sub-tiles 0 .. 3 and
                // written (untransformed: GN == 0) three sub-tiles later, the last ones at LOAD(6) -- one barrier pair ahead of the next chunk's first read
                static_assert(!PH || GN == 0, "the phase mode has no GroupNorm operand path");
                auto subp = [&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    constexpr int tap = i >> 1, hk = i & 1, ta = tap >> 1, tb = tap & 1;
                    constexpr int aimm = hk * 4 * PLANE + (ta * HWID + tb) * 16;
                    if constexpr (nhp(i - 3) >= 1) halo_store(2 * (i - 3), nbuf, hregp[(i - 3) % 3][0]);
                    if constexpr (nhp(i - 3) == 2) halo_store(2 * (i - 3) + 1, nbuf, hregp[(i - 3) % 3][1]);
                    {
                        const unsigned char* Wp = smem_raw + wfrag + rd_slot * WSUB;
#pragma unroll
                        for (int nb = 0; nb < 5; ++nb) wf[nb] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Wp + nb * 1024));
#pragma unroll
                        for (int mb = 0; mb < 5; ++mb)
                            af[mb] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(smem_raw + abase + afrag[mb] + aimm));
                        rd_slot = rd_slot + 1 == NBW ? 0 : rd_slot + 1;
                    }
                    if constexpr (nhp(i) >= 1) halo_load(2 * i, c + 1, hregp[i % 3][0]);
                    if constexpr (nhp(i) == 2) halo_load(2 * i + 1, c + 1, hregp[i % 3][1]);
                    w_issue(cls);
                    {   // W sub-tile s + 1 (requested two LOADs ago) and everything older -- the halo pieces of LOAD(i - 2) among it -- has landed
                        constexpr int extra = nhp(i - 1) + nhp(i);
                        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NW + extra) : "memory");
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_setprio(1);
#pragma unroll
                    for (int mb = 0; mb < 5; ++mb)
#pragma unroll
                        for (int nb = 0; nb < 5; ++nb)
                            acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nb], af[mb], acc[mb][nb], 0, 0, 0);
                    __builtin_amdgcn_s_setprio(0);
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                };
                subp(IC<0>{}); subp(IC<1>{}); subp(IC<2>{}); subp(IC<3>{}); subp(IC<4>{}); subp(IC<5>{}); subp(IC<6>{}); subp(IC<7>{});
                cbuf = nbuf;
                continue;
            }
            auto sub = [&](auto ic) {
                constexpr int i = decltype(ic)::value;
                constexpr int tap = i >> 1, hk = i & 1, ky = tap / 3, kx = tap % 3;
                constexpr int aimm = hk * 4 * PLANE + (ky * HWID + kx) * 16;
                // 1. a staged piece of the NEXT chunk's halo: requested three sub-tiles ago, normalised during the last MFMA phase
                if constexpr (i >= 3 && i <= 15 && (i & 1) == 1) halo_store((i - 3) / 2, nbuf, hpk);
                if constexpr (i == 16) {                     // coefficients of chunk c + 2 into the buffer chunk c + 1's staging just stopped using
                    if (tid < 128) *reinterpret_cast<float*>(smem_raw + OFF_COEF + cbuf * 512 + tid * 4) = coef_next;
                }
                // 2. this sub-tile's fragments
                {
                    const unsigned char* Wp = smem_raw + wfrag + rd_slot * WSUB;
#pragma unroll
                    for (int nb = 0; nb < 5; ++nb) wf[nb] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Wp + nb * 1024));
#pragma unroll
                    for (int mb = 0; mb < 5; ++mb)
                        af[mb] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(smem_raw + abase + afrag[mb] + aimm));
                    rd_slot = rd_slot + 1 == NBW ? 0 : rd_slot + 1;
                }
                // 3. requests: one halo piece of the next chunk (even sub-tiles 0 .. 12), the coefficient of chunk c + 2, W sub-tile s + 3
                if constexpr (nh(i) == 1) halo_load(i / 2, c + 1, hreg[(i / 2) & 1]);
                if constexpr (i == 13) coef_next = coef_fetch(c + 2);
                if constexpr (SC && i == 16) {
#pragma unroll
                    for (int j = 0; j < NSCP; ++j) sc_load(j, c + 2 - nchunk, hsc[j]);
                }
                w_issue(cls);
                // 4. counted wait: W sub-tile s + 1 (requested two LOADs ago) and everything older has landed
                {
                    constexpr int extra = nreq<SC>(i - 1) + nreq<SC>(i) + (i == 13 || i == 14 ? 1 : 0);
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NW + extra) : "memory");
                }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_setprio(1);
                // (piece j = (i - 2) / 2 was requested at LOAD(i - 2) in front of that phase's W request, which the wait above retired: it is here)
                if constexpr (i >= 2 && i <= 14 && (i & 1) == 0) hpk = halo_transform((i - 2) / 2, nbuf, hreg[((i - 2) / 2) & 1]);
#pragma unroll
                for (int mb = 0; mb < 5; ++mb)
#pragma unroll
                    for (int nb = 0; nb < 5; ++nb)
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nb], af[mb], acc[mb][nb], 0, 0, 0);
                if constexpr (GN != 0 && i >= 2 && i <= 14 && (i & 1) == 0) {      // one matrix instruction, then three of the piece's VALU / LDS-read instructions
#pragma unroll
                    for (int k = 0; k < 25; ++k) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x102, 3, 0);
                    }
                }
                __builtin_amdgcn_s_setprio(0);
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
            };
            sub(IC<0>{}); sub(IC<1>{}); sub(IC<2>{}); sub(IC<3>{}); sub(IC<4>{}); sub(IC<5>{});
            sub(IC<6>{}); sub(IC<7>{}); sub(IC<8>{}); sub(IC<9>{}); sub(IC<10>{}); sub(IC<11>{});
            sub(IC<12>{}); sub(IC<13>{}); sub(IC<14>{}); sub(IC<15>{}); sub(IC<16>{}); sub(IC<17>{});
            cbuf = nbuf;
        }
        if constexpr (SC) {
            for (int k = 0; k < nsc; ++k) {
                const int abase = cbuf * HALO, nbuf = cbuf ^ 1;
                auto subs = [&](auto ic) {
                    constexpr int hk = decltype(ic)::value;
                    constexpr int aimm = hk * 4 * PLANE + (HWID + 1) * 16;      // the centre tap
                    // 1. (second sub-tile) chunk k + 1's pieces, requested two sub-tiles ago: only the two W requests behind them may be outstanding.
                    //    nbuf was last read two sub-tiles ago
                    if constexpr (hk == 1) {
                        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NW) : "memory");
#pragma unroll
                        for (int j = 0; j < NSCP; ++j) sc_store(j, nbuf, hsc[j]);
                    }
                    {
                        const unsigned char* Wp = smem_raw + wfrag + rd_slot * WSUB;
#pragma unroll
                        for (int nb = 0; nb < 5; ++nb) wf[nb] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Wp + nb * 1024));
#pragma unroll
                        for (int mb = 0; mb < 5; ++mb)
                            af[mb] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(smem_raw + abase + afrag[mb] + aimm));
                        rd_slot = rd_slot + 1 == NBW ? 0 : rd_slot + 1;
                    }
                    if constexpr (hk == 1) {
#pragma unroll
                        for (int j = 0; j < NSCP; ++j) sc_load(j, k + 2, hsc[j]);
                    }
                    w_issue(cls);
                    // 2. counted wait: W sub-tile s + 1 and everything older has landed.  First sub-tile: the pieces of the sub-tile before stay in flight
                    //    (chunk 0 follows sub-tile 17 of a 3x3 chunk, which requested none).  Second sub-tile: its stores are read one sub-tile on, so they
                    //    (and the fragment reads) drain in front of the barrier
                    if constexpr (hk == 0) {
                        if (k == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NW) : "memory");
                        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NW + NSCP) : "memory");
                    } else {
                        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * NW + NSCP) : "memory");
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_setprio(1);
#pragma unroll
                    for (int mb = 0; mb < 5; ++mb)
#pragma unroll
                        for (int nb = 0; nb < 5; ++nb)
                            acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nb], af[mb], acc[mb][nb], 0, 0, 0);
                    __builtin_amdgcn_s_setprio(0);
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                };
                subs(IC<0>{}); subs(IC<1>{});
                cbuf = nbuf;
            }
        }
    };
    if (clsA) main_loop(std::true_type{}); else main_loop(std::false_type{});
    if (half == 0) __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the wrap-around W requests of the tail have landed: LDS is free for the epilogue
    __syncthreads();

    // ---- epilogue (gemm160_kernel's: bias / temb in registers, residual through the staging tile, whole-row 16-byte stores) ---------------
    // my outputs: acc[mb][nb][j] = (tile pixel 80 wr + 16 mb + l15, tile channel 80 wc + 16 nb + 4 kq + j)
    constexpr int OP = BN + 8;                               // bf16 pitch of the staging rows (336 B)
    bf16_t* Os = reinterpret_cast<bf16_t*>(smem_raw);        // [320][OP] = 107,520 B
    constexpr int CPR = BN / 8;                              // 20 sixteen-byte chunks per row
    const int vrows = min(TH, P.H - y0) * TW;                // (rows of a tile that hangs over the image's last row are not stored)
    const int vcols = PARTIAL ? min(TW, P.W - x0) : TW;      // (PARTIAL: nor are the columns of a tile that hangs over its right border)
    auto row_valid = [&](int r) -> bool {
        if constexpr (PARTIAL) return r < vrows && (r & 31) < vcols;
        return r < vrows;
    };
    auto row_pixel = [&](int r) -> int64_t {
        if constexpr (PH) return ((int64_t)img * (2 * P.H) + 2 * (y0 + (r >> 5)) + py) * (2 * P.W) + 2 * (x0 + (r & 31)) + px_;      // pixel shuffle
        return ((int64_t)img * P.H + y0 + (r >> 5)) * P.W + x0 + (r & 31);
    };
    {   // bias and time-embedding words of my five channel blocks: all requested before the first is used (one branch per block put each load behind its
        // own s_waitcnt vmcnt(0): ten dependent round trips)
        u32x2 bt[5], tt[5];
        if (P.bias) {
#pragma unroll
            for (int nb = 0; nb < 5; ++nb) bt[nb] = *reinterpret_cast<const u32x2*>(P.bias + n0 + wc * 80 + nb * 16 + 4 * kq);
        }
        if (P.temb) {
            const bf16_t* trow = P.temb + (int64_t)(img / P.temb_div) * P.temb_ld + n0 + wc * 80 + 4 * kq;
#pragma unroll
            for (int nb = 0; nb < 5; ++nb) tt[nb] = *reinterpret_cast<const u32x2*>(trow + nb * 16);
        }
#pragma unroll
        for (int nb = 0; nb < 5; ++nb) {
            float b4[4] = {0.f, 0.f, 0.f, 0.f};
            if (P.bias) {
                b4[0] = __uint_as_float(bt[nb][0] << 16); b4[1] = __uint_as_float(bt[nb][0] & 0xffff0000u);
                b4[2] = __uint_as_float(bt[nb][1] << 16); b4[3] = __uint_as_float(bt[nb][1] & 0xffff0000u);
            }
            if (P.temb) {
                b4[0] += __uint_as_float(tt[nb][0] << 16); b4[1] += __uint_as_float(tt[nb][0] & 0xffff0000u);
                b4[2] += __uint_as_float(tt[nb][1] << 16); b4[3] += __uint_as_float(tt[nb][1] & 0xffff0000u);
            }
#pragma unroll
            for (int mb = 0; mb < 5; ++mb)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[mb][nb][j] += b4[j];
        }
    }
    if (P.res) {
        // the residual rows in two bursts of 7 loads per thread (320 x 20 chunks = 12.5 per thread) -- rolled, the loop was load -> s_waitcnt vmcnt(0) ->
        // ds_write per iteration: thirteen dependent round trips per tile
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            u32x4 rv[7];
#pragma unroll
            for (int it = 0; it < 7; ++it) {
                const int cidx = min(tid + (7 * h + it) * 512, BM * CPR - 1), r = cidx / CPR, ch = cidx - r * CPR;
                rv[it] = *reinterpret_cast<const u32x4*>(P.res + row_pixel(row_valid(r) ? r : 0) * P.cout + n0 + ch * 8);
            }
#pragma unroll
            for (int it = 0; it < 7; ++it) {
                const int cidx = tid + (7 * h + it) * 512, r = cidx / CPR, ch = cidx - r * CPR;
                if (cidx < BM * CPR) *reinterpret_cast<u32x4*>(Os + r * OP + ch * 8) = rv[it];
            }
        }
        __syncthreads();
#pragma unroll
        for (int mb = 0; mb < 5; ++mb)
#pragma unroll
            for (int nb = 0; nb < 5; ++nb) {
                const u32x2 t = *reinterpret_cast<const u32x2*>(Os + (wr * 80 + mb * 16 + l15) * OP + wc * 80 + nb * 16 + 4 * kq);
                acc[mb][nb][0] += __uint_as_float(t[0] << 16); acc[mb][nb][1] += __uint_as_float(t[0] & 0xffff0000u);
                acc[mb][nb][2] += __uint_as_float(t[1] << 16); acc[mb][nb][3] += __uint_as_float(t[1] & 0xffff0000u);
            }
        __syncthreads();
    }
#pragma unroll
    for (int mb = 0; mb < 5; ++mb)
#pragma unroll
        for (int nb = 0; nb < 5; ++nb)
            *reinterpret_cast<u32x2*>(Os + (wr * 80 + mb * 16 + l15) * OP + wc * 80 + nb * 16 + 4 * kq) =
                u32x2{pack_bf2(acc[mb][nb][0], acc[mb][nb][1]), pack_bf2(acc[mb][nb][2], acc[mb][nb][3])};
    __syncthreads();
    // GroupNorm statistics of what I just produced (the ROUNDED values, as the consumer would read them): thread t sums group t % GT over rows
    // t / GT, t / GT + RP, ...; fixed summation order, one (sum, sum of squares) pair per (image, pixel tile, group) -- no atomics
    float gs = 0.f, gss = 0.f;
    const int cpg = P.cout >> 5, GT = BN / cpg, RP = 512 / GT;
    if (P.gn_part) {
        const int gl = tid % GT;
        for (int r = tid / GT; r < vrows; r += RP) {
            if constexpr (PARTIAL) { if ((r & 31) >= vcols) continue; }
            const unsigned* wsrc = reinterpret_cast<const unsigned*>(Os + r * OP + gl * cpg);
            for (int k = 0; k < cpg / 2; ++k) {
                const unsigned u = wsrc[k];
                const float a = __uint_as_float(u << 16), b = __uint_as_float(u & 0xffff0000u);
                gs += a + b;
                gss += a * a + b * b;
            }
        }
    }
    for (int cidx = tid; cidx < BM * CPR; cidx += 512) {
        const int r = cidx / CPR, ch = cidx - r * CPR;
        if (row_valid(r))
            *reinterpret_cast<u32x4*>(P.out + row_pixel(r) * P.cout + n0 + ch * 8) = *reinterpret_cast<const u32x4*>(Os + r * OP + ch * 8);
    }
    if (P.gn_part) {
        float* red = reinterpret_cast<float*>(smem_raw + (size_t)BM * OP * 2);
        red[2 * tid] = gs;
        red[2 * tid + 1] = gss;
        __syncthreads();
        if (tid < GT) {
            float a = 0.f, b = 0.f;
            for (int k = 0; k < RP; ++k) { a += red[2 * (tid + k * GT)]; b += red[2 * (tid + k * GT) + 1]; }
            // (PH: one split per (source tile, phase))
            float* dst = P.gn_part + ((PH ? ((int64_t)img * tpi + tin) * 4 + phase : (int64_t)img * tpi + tin) * 32 + (n0 / cpg + tid)) * 2;
            dst[0] = a;
            dst[1] = b;
        }
    }
}

// ---- filter packing, for both kernels: [Cout][3][3][Cin] (channels-last filter) -> [Cout / BN][Cin / 64][9 taps][2 halves][BN rows][32], the 16-byte
// chunks of a row already in their LDS places (physical chunk p of row r holds logical chunk p ^ (3 * ((r >> 3) & 1))); BN = 160 here and in the
// 8-wave form of conv_halo4_kernel, 80 in its 4-wave form ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_halo_pack_kernel(const bf16_t* __restrict__ w, bf16_t* __restrict__ dst, int cout, int cin, int BN) {
    const int64_t total = (int64_t)cout * 9 * cin / 8;      // 16-byte chunks
    for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (int64_t)gridDim.x * blockDim.x) {
        int64_t t = id;
        const int p = (int)(t & 3); t >>= 2;
        const int row = (int)(t % BN); t /= BN;
        const int hk = (int)(t & 1); t >>= 1;
        const int tap = (int)(t % 9); t /= 9;
        const int nchunk = cin >> 6;
        const int ch64 = (int)(t % nchunk); t /= nchunk;
        const int nt = (int)t;
        const int lc = p ^ (3 * ((row >> 3) & 1));
        const int64_t src = (((int64_t)(nt * BN + row) * 9 + tap) * cin + ch64 * 64 + hk * 32 + lc * 8);
        *reinterpret_cast<u32x4*>(dst + id * 8) = *reinterpret_cast<const u32x4*>(w + src);
    }
}

// ---- shortcut-mode filter: the 3x3 filter in the order above and, behind it in every channel tile, the 1x1 shortcut filter [Cout][Cin_sc] as
// [Cin_sc / 64][2 halves][BN rows][32] with the same chunk swizzle: [Cout / BN][(Cin / 64) * 18 + (Cin_sc / 64) * 2 sub-tiles][BN rows][32] ------------------
__global__ __launch_bounds__(256) void conv_halo_sc_pack_kernel(const bf16_t* __restrict__ w, const bf16_t* __restrict__ wsc, bf16_t* __restrict__ dst,
                                                                int cout, int cin, int cin_sc, int BN) {
    const int64_t total = (int64_t)cout * (9 * cin + cin_sc) / 8;      // 16-byte chunks
    for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (int64_t)gridDim.x * blockDim.x) {
        int from_sc;
        const int64_t src = halo::sc_pack_source(id, cin, cin_sc, BN, &from_sc);
        *reinterpret_cast<u32x4*>(dst + id * 8) = *reinterpret_cast<const u32x4*>((from_sc ? wsc : w) + src);
    }
}

// ---- phase-mode filter: fold + pack in one pass.  [Cout][3][3][Cin] -> [4 phases (py, px)][Cout / BN][Cin / 64][4 taps (a, b)][2 halves][BN rows][32],
// chunk-swizzled as above.  Wf[py][px][a][b] = sum of w[ky][kx] over ky in R(py, a), kx in R(px, b) with R(0, 0) = {0}, R(0, 1) = {1, 2},
// R(1, 0) = {0, 1}, R(1, 1) = {2}: the filter rows / columns that fall on the same source pixel.  Summed in fp32 (fixed order), rounded to bf16 once. ----
__global__ __launch_bounds__(256) void conv_upfold_pack_kernel(const bf16_t* __restrict__ w, bf16_t* __restrict__ dst, int cout, int cin, int BN) {
    const int64_t total = (int64_t)cout * 16 * cin / 8;     // 16-byte chunks
    const int nchunk = cin >> 6, tn1 = cout / BN;
    for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (int64_t)gridDim.x * blockDim.x) {
        int64_t t = id;
        const int p = (int)(t & 3); t >>= 2;
        const int row = (int)(t % BN); t /= BN;
        const int hk = (int)(t & 1); t >>= 1;
        const int tap = (int)(t & 3); t >>= 2;
        const int ch64 = (int)(t % nchunk); t /= nchunk;
        const int nt = (int)(t % tn1), phase = (int)(t / tn1);
        const int py = phase >> 1, px = phase & 1, ta = tap >> 1, tb = tap & 1;
        const int ky0 = py == 0 ? ta : 2 * ta, ky1 = py == 0 ? 2 * ta : ta + 1;      // rows ky0 .. ky1 of the filter
        const int kx0 = px == 0 ? tb : 2 * tb, kx1 = px == 0 ? 2 * tb : tb + 1;
        const int lc = p ^ (3 * ((row >> 3) & 1));
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int ky = ky0; ky <= ky1; ++ky)
            for (int kx = kx0; kx <= kx1; ++kx) {
                float f[8];
                Vec8<bf16_t>::unpack(Vec8<bf16_t>::load_raw(w + (((int64_t)(nt * BN + row) * 9 + ky * 3 + kx) * cin + ch64 * 64 + hk * 32 + lc * 8)), f);
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] += f[k];
            }
        Vec8<bf16_t>::store(dst + id * 8, v);
    }
}

// ---- GroupNorm -> per-(image, channel) affine map: partial (sum, sum of squares) per (image, split, group) -> coef[n][c] = (rstd gamma_c,
// beta_c - mean rstd gamma_c); combined in fp64 like gn_apply_fwd_kernel (norm_kernels.hip) -------------------------------------------------------
__global__ __launch_bounds__(256) void gn_coef_kernel(const float* __restrict__ part, int splits, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* __restrict__ coef, float* __restrict__ stats,
                                                      int C, int G, double count, float eps) {
    __shared__ float s_mean[64], s_rstd[64];
    const int n = blockIdx.x;
    if ((int)threadIdx.x < G) {
        double a = 0.0, b = 0.0;
        for (int s = 0; s < splits; ++s) {
            const float* p = part + (((int64_t)n * splits + s) * G + threadIdx.x) * 2;
            a += (double)p[0];
            b += (double)p[1];
        }
        const double mean = a / count;
        double var = b / count - mean * mean;
        if (var < 0.0) var = 0.0;
        const float rstd = (float)(1.0 / sqrt(var + (double)eps));
        s_mean[threadIdx.x] = (float)mean;
        s_rstd[threadIdx.x] = rstd;
        if (stats) { stats[((int64_t)n * G + threadIdx.x) * 2] = (float)mean; stats[((int64_t)n * G + threadIdx.x) * 2 + 1] = rstd; }
    }
    __syncthreads();
    const int cpg = C / G;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const int g = c / cpg;
        const float a = s_rstd[g] * gamma[c];
        coef[((int64_t)n * C + c) * 2] = a;
        coef[((int64_t)n * C + c) * 2 + 1] = beta[c] - s_mean[g] * a;
    }
}

}  // namespace

void halo::pack_filter(const bf16_t* w, bf16_t* dst, int Cin, int Cout, int bn, hipStream_t st) {
    const int64_t chunks = (int64_t)Cout * 9 * Cin / 8;
    const int grid = (int)((chunks + 255) / 256 < 4096 ? (chunks + 255) / 256 : 4096);
    hipLaunchKernelGGL(conv_halo_pack_kernel, dim3(grid), dim3(256), 0, st, w, dst, Cout, Cin, bn);
}

extern "C" int64_t fmc_conv3x3_halo_packed_bytes(int Cin, int Cout) { return (int64_t)Cout * 9 * Cin * 2; }

extern "C" int fmc_conv3x3_halo_pack_weight(const void* w, void* dst, int Cin, int Cout, void* stream) {
    if (!w || !dst) FMC_FAIL(FMC_E_NULL, "conv3x3_halo_pack_weight: NULL pointer");
    if (Cin % 64 || Cout % BN) FMC_FAIL(FMC_E_SHAPE, "conv3x3_halo_pack_weight: Cin %% 64 / Cout %% 160 (Cin=%d Cout=%d)", Cin, Cout);
    if (!fmc_aligned16(w) || !fmc_aligned16(dst)) FMC_FAIL(FMC_E_ALIGN, "conv3x3_halo_pack_weight: pointers must be 16-byte aligned");
    halo::pack_filter((const bf16_t*)w, (bf16_t*)dst, Cin, Cout, BN, (hipStream_t)stream);
    FMC_CHECK_LAUNCH("fmc_conv3x3_halo_pack_weight");
    return 0;
}

// ---- host side of the launches.  Every launch form (plain, shortcut, fold) is written once, for whole column tiles (W % 32 == 0) and, `partial`,
// for images of any width: the entry points without the width rule, tiles_x = ceil(W / 32), the PARTIAL instantiation of conv_halo_kernel.  Same packed
// filters; a whole-tile shape gives the same bits on either.  The exported pairs (fmc_hip.h) are calls of these ----------------------------------------
static int halo_shape_ok(int n_img, int H, int W, int Cin, int Cin1, int Cout, int upsample2x, bool any_width) {
    if (n_img < 1 || H < 1 || W < 1 || (!any_width && W % TW) || Cin % 64 || Cout % BN) return 0;
    if (Cin1 <= 0 || Cin1 > Cin || Cin1 % 64) return 0;
    if (upsample2x && ((H | W) & 1)) return 0;
    const int64_t hs = upsample2x ? H / 2 : H, ws = upsample2x ? W / 2 : W;
    if ((int64_t)n_img * hs * ws * Cin1 * 2 >= (1ll << 31) || (int64_t)n_img * hs * ws * (Cin - Cin1) * 2 >= (1ll << 31)) return 0;
    if ((int64_t)Cout * 9 * Cin * 2 >= (1ll << 31)) return 0;
    return 1;
}

static int halo_sc_ok(int n_img, int H, int W, int Cin, int Cout, int Cin_sc, int Cin_sc1, bool any_width) {
    if (!halo_shape_ok(n_img, H, W, Cin, Cin, Cout, 0, any_width)) return 0;      // the convolution's own conditions
    return halo::sc_sources_ok(n_img, H, W, Cin, Cout, Cin_sc, Cin_sc1);
}

static int halo_fold_ok(int n_img, int Hs, int Ws, int Cin, int Cout, bool any_width) {
    if (!halo_shape_ok(n_img, Hs, Ws, Cin, Cin, Cout, 0, any_width)) return 0;    // the source-resolution convolution's own conditions
    if ((int64_t)Cout * 16 * Cin * 2 >= (1ll << 31)) return 0;
    if ((int64_t)n_img * Hs * Ws * 4 >= (1ll << 31)) return 0;
    return 1;
}

// (whole tiles at a ragged width: the floor -- what the whole-tile count has always answered for a shape its launch refuses)
static int halo_tiles_x(int W, bool partial) { return partial ? (W + TW - 1) / TW : W / TW; }
static int halo_tiles_per_image(int H, int W, bool partial) { return ((H + TH - 1) / TH) * halo_tiles_x(W, partial); }

// the grid of a filled parameter block (`phases`: 4 in phase mode) and the choice between the whole-tile and the PARTIAL instantiation
template <int GN, bool PH, bool SC, class P_> static void halo_launch(P_& P, int phases, bool partial, void* stream) {
    P.tiles_y = (P.H + TH - 1) / TH; P.tiles_x = halo_tiles_x(P.W, partial); P.tiles_n = phases * (P.cout / BN);
    const dim3 grid((unsigned)(P.n_img * P.tiles_y * P.tiles_x * P.tiles_n));
    if (partial) fmc_launch<conv_halo_kernel<GN, PH, SC, true>>(grid, dim3(512), LDS_BYTES, (hipStream_t)stream, P);
    else fmc_launch<conv_halo_kernel<GN, PH, SC>>(grid, dim3(512), LDS_BYTES, (hipStream_t)stream, P);
}

static const char* halo_width_rule(bool partial, const char* rule) { return partial ? "" : rule; }      // (the one clause in which the pairs' messages differ)

static int halo_plain(bool partial, const void* x, const void* x2, int Cin1, const void* w_packed, const void* bias, const void* temb, const void* residual,
                      void* out, int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride, int temb_img_div, int upsample2x,
                      const float* gn_coef, int gn_act, float* gn_partials, void* stream) {
    if (!x2) Cin1 = Cin;
    if (int e = halo::check_args(partial ? "conv3x3_halo_partial" : "conv3x3_halo", true, x, x2, w_packed, bias, temb, residual, out, temb_row_stride,
                                 temb_img_div, gn_partials, Cout, BN, halo_shape_ok(n_img, H, W, Cin, Cin1, Cout, upsample2x, partial),
                                 "%s: needs %sCin %% 64 == 0 (both sources), Cout %% 160 == 0, operands < 2 GiB "
                                 "(n=%d H=%d W=%d Cin=%d+%d Cout=%d ups=%d)", halo_width_rule(partial, "W % 32 == 0, "), n_img, H, W, Cin1, Cin - Cin1, Cout,
                                 upsample2x))
        return e;
    CHParams P;
    halo::fill_params(P, x, x2, Cin1, w_packed, bias, temb, residual, out, n_img, H, W, Cin, Cout, temb_row_stride, temb_img_div, upsample2x, gn_partials, 9);
    P.gn_coef = gn_coef; P.gn_act = gn_act;
    if (!gn_coef) halo_launch<0, false, false>(P, 1, partial, stream);
    else if (gn_act) halo_launch<1, false, false>(P, 1, partial, stream);
    else halo_launch<2, false, false>(P, 1, partial, stream);
    FMC_CHECK_LAUNCH(partial ? "fmc_conv3x3_halo_partial_bf16" : "fmc_conv3x3_halo_bf16");
    return 0;
}

extern "C" int fmc_conv3x3_halo_supported(int n_img, int H, int W, int Cin, int Cin1, int Cout, int upsample2x) {
    return halo_shape_ok(n_img, H, W, Cin, Cin1, Cout, upsample2x, false);
}

extern "C" int fmc_conv3x3_halo_partial_supported(int n_img, int H, int W, int Cin, int Cin1, int Cout, int upsample2x) {
    return halo_shape_ok(n_img, H, W, Cin, Cin1, Cout, upsample2x, true);
}

extern "C" int fmc_conv3x3_halo_tiles_per_image(int H, int W) { return halo_tiles_per_image(H, W, false); }

extern "C" int fmc_conv3x3_halo_partial_tiles_per_image(int H, int W) { return halo_tiles_per_image(H, W, true); }

extern "C" int fmc_conv3x3_halo_bf16(const void* x, const void* x2, int Cin1, const void* w_packed, const void* bias, const void* temb,
                                     const void* residual, void* out, int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride,
                                     int temb_img_div, int upsample2x, const float* gn_coef, int gn_act, float* gn_partials, void* stream) {
    return halo_plain(false, x, x2, Cin1, w_packed, bias, temb, residual, out, n_img, H, W, Cin, Cout, temb_row_stride, temb_img_div, upsample2x, gn_coef,
                      gn_act, gn_partials, stream);
}

extern "C" int fmc_conv3x3_halo_partial_bf16(const void* x, const void* x2, int Cin1, const void* w_packed, const void* bias, const void* temb,
                                             const void* residual, void* out, int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride,
                                             int temb_img_div, int upsample2x, const float* gn_coef, int gn_act, float* gn_partials, void* stream) {
    return halo_plain(true, x, x2, Cin1, w_packed, bias, temb, residual, out, n_img, H, W, Cin, Cout, temb_row_stride, temb_img_div, upsample2x, gn_coef,
                      gn_act, gn_partials, stream);
}

// ---- shortcut mode: a ResnetBlock2D's conv2 with the block's 1x1 shortcut in the same reduction (see conv_halo_kernel) ------------------------------
void halo::pack_filter_sc(const bf16_t* w, const bf16_t* w_sc, bf16_t* dst, int Cin, int Cout, int Cin_sc, int bn, hipStream_t st) {
    const int64_t chunks = (int64_t)Cout * (9 * Cin + Cin_sc) / 8;
    const int grid = (int)((chunks + 255) / 256 < 4096 ? (chunks + 255) / 256 : 4096);
    hipLaunchKernelGGL(conv_halo_sc_pack_kernel, dim3(grid), dim3(256), 0, st, w, w_sc, dst, Cout, Cin, Cin_sc, bn);
}

extern "C" int64_t fmc_conv3x3_halo_sc_packed_bytes(int Cin, int Cout, int Cin_sc) { return (int64_t)Cout * (9 * Cin + Cin_sc) * 2; }

extern "C" int fmc_conv3x3_halo_sc_pack_weight(const void* w, const void* w_sc, void* dst, int Cin, int Cout, int Cin_sc, int tile_channels, void* stream) {
    if (!w || !w_sc || !dst) FMC_FAIL(FMC_E_NULL, "conv3x3_halo_sc_pack_weight: NULL pointer");
    if ((tile_channels != 80 && tile_channels != 160) || Cin < 64 || Cin % 64 || Cin_sc < 64 || Cin_sc % 64 || Cout % tile_channels)
        FMC_FAIL(FMC_E_SHAPE, "conv3x3_halo_sc_pack_weight: tile_channels 80 / 160, Cin %% 64, Cin_sc %% 64, Cout %% tile_channels (Cin=%d Cin_sc=%d Cout=%d tile=%d)",
                 Cin, Cin_sc, Cout, tile_channels);
    if (!fmc_aligned16(w) || !fmc_aligned16(w_sc) || !fmc_aligned16(dst)) FMC_FAIL(FMC_E_ALIGN, "conv3x3_halo_sc_pack_weight: pointers must be 16-byte aligned");
    halo::pack_filter_sc((const bf16_t*)w, (const bf16_t*)w_sc, (bf16_t*)dst, Cin, Cout, Cin_sc, tile_channels, (hipStream_t)stream);
    FMC_CHECK_LAUNCH("fmc_conv3x3_halo_sc_pack_weight");
    return 0;
}

extern "C" int64_t fmc_conv3x3_halo_sc_pack_source(int64_t chunk, int Cin, int Cin_sc, int tile_channels, int* from_shortcut) {
    int from_sc = 0;
    const int64_t src = halo::sc_pack_source(chunk, Cin, Cin_sc, tile_channels, &from_sc);
    if (from_shortcut) *from_shortcut = from_sc;
    return src;
}

extern "C" int fmc_conv3x3_halo_sc_supported(int n_img, int H, int W, int Cin, int Cout, int Cin_sc, int Cin_sc1) {
    return halo_sc_ok(n_img, H, W, Cin, Cout, Cin_sc, Cin_sc1, false);
}

extern "C" int fmc_conv3x3_halo_sc_partial_supported(int n_img, int H, int W, int Cin, int Cout, int Cin_sc, int Cin_sc1) {
    return halo_sc_ok(n_img, H, W, Cin, Cout, Cin_sc, Cin_sc1, true);
}

static int halo_sc(bool partial, const void* x, const void* w_packed, const void* bias, const void* temb, void* out, const void* xs, const void* xs2,
                   int Cin_sc1, int Cin_sc, int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride, int temb_img_div, float* gn_partials,
                   void* stream) {
    const char* name = partial ? "conv3x3_halo_sc_partial" : "conv3x3_halo_sc";
    if (!xs2) Cin_sc1 = Cin_sc;
    if (int e = halo::check_args(name, true, x, nullptr, w_packed, bias, temb, nullptr, out, temb_row_stride, temb_img_div, gn_partials, Cout, BN,
                                 halo_sc_ok(n_img, H, W, Cin, Cout, Cin_sc, Cin_sc1, partial),
                                 "%s: needs %sCin %% 64 == 0, shortcut channels %% 64 == 0 (both sources), Cout %% 160 == 0, operands < 2 GiB "
                                 "(n=%d H=%d W=%d Cin=%d Cout=%d shortcut=%d+%d)", halo_width_rule(partial, "W % 32 == 0, "), n_img, H, W, Cin, Cout, Cin_sc1,
                                 Cin_sc - Cin_sc1))
        return e;
    if (int e = halo::check_sc_args(name, xs, xs2)) return e;
    CHParamsSC P;
    halo::fill_params(P, x, nullptr, Cin, w_packed, bias, temb, nullptr, out, n_img, H, W, Cin, Cout, temb_row_stride, temb_img_div, 0, gn_partials, 9);
    halo::fill_params_sc(P, xs, xs2, Cin_sc1, Cin_sc);
    P.gn_coef = nullptr; P.gn_act = 0;
    halo_launch<0, false, true>(P, 1, partial, stream);
    FMC_CHECK_LAUNCH(partial ? "fmc_conv3x3_halo_sc_partial_bf16" : "fmc_conv3x3_halo_sc_bf16");
    return 0;
}

extern "C" int fmc_conv3x3_halo_sc_bf16(const void* x, const void* w_packed, const void* bias, const void* temb, void* out, const void* xs,
                                        const void* xs2, int Cin_sc1, int Cin_sc, int n_img, int H, int W, int Cin, int Cout,
                                        int64_t temb_row_stride, int temb_img_div, float* gn_partials, void* stream) {
    return halo_sc(false, x, w_packed, bias, temb, out, xs, xs2, Cin_sc1, Cin_sc, n_img, H, W, Cin, Cout, temb_row_stride, temb_img_div, gn_partials, stream);
}

extern "C" int fmc_conv3x3_halo_sc_partial_bf16(const void* x, const void* w_packed, const void* bias, const void* temb, void* out, const void* xs,
                                                const void* xs2, int Cin_sc1, int Cin_sc, int n_img, int H, int W, int Cin, int Cout,
                                                int64_t temb_row_stride, int temb_img_div, float* gn_partials, void* stream) {
    return halo_sc(true, x, w_packed, bias, temb, out, xs, xs2, Cin_sc1, Cin_sc, n_img, H, W, Cin, Cout, temb_row_stride, temb_img_div, gn_partials, stream);
}

// ---- phase mode of the nearest-2x upsample convolutions (see conv_halo_kernel) ------------------------------------------------------------------
extern "C" int64_t fmc_conv3x3_upfold_packed_bytes(int Cin, int Cout) { return (int64_t)Cout * 16 * Cin * 2; }

extern "C" int fmc_conv3x3_upfold_pack_weight(const void* w, void* dst, int Cin, int Cout, int tile_channels, void* stream) {
    if (!w || !dst) FMC_FAIL(FMC_E_NULL, "conv3x3_upfold_pack_weight: NULL pointer");
    if ((tile_channels != 80 && tile_channels != 160) || Cin % 64 || Cout % tile_channels)
        FMC_FAIL(FMC_E_SHAPE, "conv3x3_upfold_pack_weight: tile_channels 80 / 160, Cin %% 64, Cout %% tile_channels (Cin=%d Cout=%d tile=%d)", Cin, Cout, tile_channels);
    if (!fmc_aligned16(w) || !fmc_aligned16(dst)) FMC_FAIL(FMC_E_ALIGN, "conv3x3_upfold_pack_weight: pointers must be 16-byte aligned");
    const int64_t chunks = (int64_t)Cout * 16 * Cin / 8;
    const int grid = (int)((chunks + 255) / 256 < 4096 ? (chunks + 255) / 256 : 4096);
    hipLaunchKernelGGL(conv_upfold_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, (bf16_t*)dst, Cout, Cin, tile_channels);
    FMC_CHECK_LAUNCH("fmc_conv3x3_upfold_pack_weight");
    return 0;
}

extern "C" int fmc_conv3x3_halo_fold_supported(int n_img, int Hs, int Ws, int Cin, int Cout) { return halo_fold_ok(n_img, Hs, Ws, Cin, Cout, false); }

extern "C" int fmc_conv3x3_halo_fold_partial_supported(int n_img, int Hs, int Ws, int Cin, int Cout) { return halo_fold_ok(n_img, Hs, Ws, Cin, Cout, true); }

static int halo_fold(bool partial, const void* x, const void* w_folded, const void* bias, void* out, int n_img, int Hs, int Ws, int Cin, int Cout,
                     float* gn_partials, void* stream) {
    if (int e = halo::check_args(partial ? "conv3x3_halo_fold_partial" : "conv3x3_halo_fold", false, x, nullptr, w_folded, bias, nullptr, nullptr, out, 0, 1,
                                 gn_partials, Cout, BN, halo_fold_ok(n_img, Hs, Ws, Cin, Cout, partial),
                                 "%s: needs %sCin %% 64 == 0, Cout %% 160 == 0, operands < 2 GiB (n=%d Hs=%d Ws=%d Cin=%d Cout=%d)",
                                 halo_width_rule(partial, "Ws % 32 == 0, "), n_img, Hs, Ws, Cin, Cout))
        return e;
    CHParams P;
    halo::fill_params(P, x, nullptr, Cin, w_folded, bias, nullptr, nullptr, out, n_img, Hs, Ws, Cin, Cout, 0, 1, 0, gn_partials, 16);
    P.gn_coef = nullptr; P.gn_act = 0;
    halo_launch<0, true, false>(P, 4, partial, stream);
    FMC_CHECK_LAUNCH(partial ? "fmc_conv3x3_halo_fold_partial_bf16" : "fmc_conv3x3_halo_fold_bf16");
    return 0;
}

extern "C" int fmc_conv3x3_halo_fold_bf16(const void* x, const void* w_folded, const void* bias, void* out, int n_img, int Hs, int Ws, int Cin,
                                          int Cout, float* gn_partials, void* stream) {
    return halo_fold(false, x, w_folded, bias, out, n_img, Hs, Ws, Cin, Cout, gn_partials, stream);
}

extern "C" int fmc_conv3x3_halo_fold_partial_bf16(const void* x, const void* w_folded, const void* bias, void* out, int n_img, int Hs, int Ws, int Cin,
                                                  int Cout, float* gn_partials, void* stream) {
    return halo_fold(true, x, w_folded, bias, out, n_img, Hs, Ws, Cin, Cout, gn_partials, stream);
}

extern "C" int fmc_groupnorm_coef(const float* partials, int part_splits, const float* gamma, const float* beta, float* coef, float* stats,
                                  int N, int HW, int C, int G, float eps, void* stream) {
    if (!partials || !gamma || !beta || !coef) FMC_FAIL(FMC_E_NULL, "groupnorm_coef: NULL pointer");
    if (N < 1 || C < 1 || G < 1 || G > 64 || C % G || part_splits < 1) FMC_FAIL(FMC_E_SHAPE, "groupnorm_coef: N=%d C=%d G=%d splits=%d", N, C, G, part_splits);
    hipLaunchKernelGGL(gn_coef_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, partials, part_splits, gamma, beta, coef, stats, C, G,
                       (double)HW * (double)(C / G), eps);
    FMC_CHECK_LAUNCH("fmc_groupnorm_coef");
    return 0;
}

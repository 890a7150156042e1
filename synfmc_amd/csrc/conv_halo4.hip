// The halo-resident 3x3 convolution (conv_halo.hip) for the SMALL feature maps of the U-Net -- 10x16 and 5x8 pixels per image at the two inner levels
// (diffusers ResnetBlock2D / Upsample2D convs of down_blocks.2-3, mid_block, up_blocks.0-1; ctor args fmc/models/unet_blocks.py:306-317, :625).
//
// Why a second geometry.  At 1280 channels those convolutions are 32 images x 160 (or 40) pixels: M = 5120 (1280) rows against K = 11520 .. 23040.
// conv_halo_kernel's 10 x 32-pixel x 160-channel tiles do not exist there, and the ring kernel's k-lockstep stream-K pass + finishing launch ran them
// at 0.17 - 0.36 of the MFMA peak (profiles/r05d_kernel_by_grid.md: 27 launches, 3.7 ms of a 28.9 ms step).  Here
//   * a tile is 320 output pixels = NB ROW BLOCKS of TH x TW pixels (TW = 16 where the image width is a multiple of 16: two 10 x 16 blocks = two
//     whole images at the 10x16 level; TW = 8 otherwise: eight 5 x 8 blocks = eight images at the 5x8 level; wider / taller images are cut into
//     such blocks) x 80 output channels: 256 tiles at the 10x16 level = one per CU, no split, no finishing pass;
//   * the input halos of the tile's row blocks ((TH + 2) x (TW + 2) pixels each, 64 channels at a time) are staged ONCE per chunk through registers
//     into LDS planes [8 channel groups][pixels] (any tap's fragment read is conflict free for TW >= 16, 2-way for TW = 8) and serve 9 taps x 2
//     k-halves; only W is streamed by LDS-DMA: 5 one-KiB requests per 32-deep sub-tile and CU;
//   * 4 waves, one per SIMD, each 80 pixels x 80 channels (5 x 5 v_mfma_f32_16x16x32_bf16): a wave keeps its matrix pipe busy alone (a 16x16x32
//     MFMA issues every 16 cycles from one wave) by software pipelining -- the fragments of sub-tile s + 1 are read into a second register set
//     while the 25 MFMAs of sub-tile s run -- with ONE barrier per sub-tile (it publishes the W sub-tile the next reads need).
// LDS: halo double buffer 2 x 8 x NP x 16 B + W ring 5 x 5 KiB (TW = 16: 135,168 B; TW = 8: 163,840 - the ring shrinks to 4).
// Roofline: MFMA bound.  Algorithmic flops per launch = 2 * n_img*H*W * Cout * 9*Cin.
//
// Image width: fmc_conv3x3_halo4_bf16 / _fold_bf16 take W % 8 == 0 and pick TW themselves; the *_partial_* entry points (`PARTIAL`, see
// conv_halo4_kernel) take any W >= 1 at the TW the caller names (fmc_conv3x3_halo4_partial_tw: the default), tiles_x = ceil(W / TW), the last row block
// of an image row partly filled -- 4 x 6 and 8 x 12 pixels per image at the 1280-channel levels of a 256x384 clip.  The whole-tile instantiations are the
// instruction streams they were (profiles/partial_tiles.md section 15); what the partial launches cost per shape is in section 17.
//
// What this kernel shares with conv_halo_kernel -- the common parameters, halo piece addressing, the W stream, the filter pack kernels (compiled in
// conv_halo.hip), the host-side checks -- is in conv_halo_common.h.
#include "conv_halo_common.h"

namespace {

using halo::IC;
constexpr int BM = 320;

// NWV waves: 4 (one per SIMD, 320 pixels x 80 channels) or 8 (two per SIMD, 320 x 160: wave = pixel block wave % 4, channel block wave / 4)
template <int TW, int NWV> struct Geo {
    static constexpr int BN = 20 * NWV, NT = 64 * NWV;
    static constexpr int WSUB = BN * 64;                   // one 32-deep W sub-tile: BN rows x 64 B (5 / 10 KiB)
    static constexpr int WPIECES = BN / 16;                // its 1-KiB pieces: 5 / 10; wave w issues piece w, the first WPIECES - NWV waves a second one
    static constexpr int TH = TW == 8 ? 5 : 10;
    static constexpr int RB = TH * TW;                     // pixels per row block
    static constexpr int NB = BM / RB;                     // row blocks per tile: 1 / 2 / 8
    static constexpr int HW_ = TW + 2, HB = (TH + 2) * HW_;    // halo pitch / halo pixels per row block
    static constexpr int HPIX = NB * HB;                   // 408 / 432 / 560
    static constexpr int NP = (HPIX + 15) / 16 * 16;       // pixels per channel-group plane (a multiple of 16: every plane starts at the same bank)
    static constexpr int PLANE = NP * 16, HALO = 8 * PLANE;
    static constexpr int NBW = (2 * HALO + 5 * WSUB <= 163840) ? 5 : 4;      // W ring depth
    static constexpr int DW = NBW - 1;                     // W sub-tile s + DW is requested at LOAD(s), into the slot sub-tile s - 1 was read from
    static constexpr int OFF_W = 2 * HALO;
    static constexpr int LDS_BYTES = OFF_W + NBW * WSUB;
    static constexpr int NPIECE = (HPIX / 8 + NWV - 1) / NWV;      // halo pieces (16 B) per thread and chunk: blocks of 8 pixels x 8 channel groups over the waves
    static_assert(HPIX % 8 == 0 && LDS_BYTES <= 163840 && NPIECE <= 18, "geometry");
};

struct C4Params : halo::Params {                            // (w: fmc_conv3x3_halo4_pack_weight, [Cout / BN][Cin / 64][9][2][BN rows][32], chunk-swizzled)
    float* gn_part;                                         // [n_img, tiles_y, 32, 2] partial sums of the rounded outputs (one split per row block), or NULL
    int tiles_y, tiles_x, tiles_p, tiles_n;                 // row blocks per image column / per image row, pixel tiles, channel tiles
    int splits; float* ws;                                  // split-K: the 64-channel chunks are dealt to `splits` workgroups per tile, which leave fp32 partial
                                                            //   sums in ws[split][pixel][Cout]; conv_halo4_finish_kernel adds them (fixed order) and runs the epilogue
    int64_t x_bytes, x2_bytes, w_bytes;
    int xcd_pc;                                             // tile order: the 8 XCDs as xcd_pc filter-slice groups x 8 / xcd_pc pixel groups (launch_c4), 0 = contiguous ranges
};

// halo pieces requested in sub-tile i of a chunk (requested at LOAD(i), written at LOAD(i + 3)): PPS = 2 per sub-tile where a thread has more than
// 12 pieces per chunk (4 waves), else one (8 waves: fewer staging registers in flight)
// Phase mode (PH, see below: 8 sub-tiles per chunk): every piece is requested in sub-tiles 0 .. 3, so that the last is written at LOAD(6), one
// barrier ahead of the next chunk's first fragment read at LOAD(7): PPS = NPIECE / 4 rounded up (2 .. 5).
template <int NPIECE, bool PH> constexpr int pps() { return PH ? (NPIECE + 3) / 4 : (NPIECE > 12 ? 2 : 1); }
template <int NPIECE, bool PH> constexpr int nh(int i) {
    constexpr int S = pps<NPIECE, PH>();
    return (i >= 0 && S * i < NPIECE) ? (NPIECE - S * i < S ? NPIECE - S * i : S) : 0;
}

// PH: the PHASE MODE of the nearest-2x upsample convolutions, as in conv_halo_kernel (conv_halo.hip): the tile is 320 SOURCE pixels, the channel-tile
// index is (phase (py, px), channel tile), a chunk is 4 taps x 2 k-halves = 8 sub-tiles of the folded filter (fmc_conv3x3_upfold_pack_weight), and the
// epilogue stores out[2 i + py, 2 j + px].  No split-K, temb or residual there.
//
// PARTIAL: images of ANY width.  tiles_x = ceil(W / TW): the last row block of an image row holds W - xb TW real columns.  As in conv_halo_kernel the
// main loop needs nothing (a halo pixel with x >= W is staged as zeros already); the split-K partial store, the residual burst, the output stores and
// the statistics sums ask whether their column exists, and every thread runs the same barriers and counted waits as in the whole-tile form.
template <int TW, int NWV, bool PH = false, bool PARTIAL = false>
__global__ __launch_bounds__(64 * NWV, NWV / 4)
void conv_halo4_kernel(const C4Params P) {
    using G = Geo<TW, NWV>;
    constexpr int BN = G::BN, NT = G::NT, WSUB = G::WSUB;
    constexpr int TH = G::TH, RB = G::RB, NB = G::NB, HW_ = G::HW_, HB = G::HB, PLANE = G::PLANE, HALO = G::HALO, NBW = G::NBW, OFF_W = G::OFF_W;
    constexpr int NPIECE = G::NPIECE, DW = G::DW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kq = lane >> 4;
    const int wp = wave & 3, wn = wave >> 2;                 // my 80 pixels / my 80 channels of the tile
    const bool clsA = wave < G::WPIECES - NWV;               // these waves issue two W pieces per sub-tile (w and NWV + w), the others one

    // ---- my tile.  Workgroup id -> XCD id & 7 (round robin).  The filter of these levels (29.5 MB at 1280 -> 1280) is larger than the input (13 MB at
    // 10x16, 3.3 MB at 5x8) and every pixel tile streams its channel tile's slice of it, so WHICH tiles share an XCD (and its L2) decides how often the
    // filter crosses the fabric: contiguous tile ranges (two pixel tiles x all 16 channel tiles per XCD at 10x16) bring the WHOLE filter into every L2 --
    // 302 MB fetched per launch for 56 MB of operands (profiles/r06fin_step_hbm_traffic_by_kernel.md).  xcd_pc > 0: the XCDs form a grid of xcd_pc
    // filter-slice groups x 8 / xcd_pc pixel groups; launch_c4 picks the split that minimises filter * pixel groups + input * slice groups. ----------
    int tile_p, tile_n, split;
    {
        const int total = P.tiles_p * P.tiles_n * P.splits;
        const int id = blockIdx.x, xcd = id & 7;
        if (P.xcd_pc > 0) {
            const int j = id >> 3, pc = P.xcd_pc;
            const int tnl = P.tiles_n * P.splits / pc, tpl = P.tiles_p / (8 / pc);      // (filter slice = (channel tile, split)) per slice group, pixel tiles per pixel group
            const int tnv = (xcd % pc) * tnl + j % tnl;
            tile_p = (xcd / pc) * tpl + j / tnl;
            split = tnv % P.splits;
            tile_n = tnv / P.splits;
        } else {
            const int q = total >> 3, r = total & 7;
            int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
            split = lin % P.splits;                          // (the splits of a tile are neighbours)
            lin /= P.splits;
            tile_p = lin / P.tiles_n;
            tile_n = lin - tile_p * P.tiles_n;
        }
    }
    constexpr int NS = PH ? 8 : 18;                          // sub-tiles per 64-channel chunk
    const int tn1 = P.cout / BN;
    const int phase = PH ? tile_n / tn1 : 0, py = phase >> 1, px_ = phase & 1;
    const int n0 = (tile_n - phase * tn1) * BN;
    const int nchunk_all = P.cin >> 6;
    const int per = (nchunk_all + P.splits - 1) / P.splits;
    const int ck0 = split * per, nchunk = max(0, min(nchunk_all, ck0 + per) - ck0);      // my chunks ck0 .. ck0 + nchunk - 1
    const int nsub = max(nchunk, 1) * NS;
    const int tpi = P.tiles_y * P.tiles_x;                   // row blocks per image: block rb = (image rb / tpi, rows ((rb % tpi) / tiles_x) TH .., columns ((rb % tpi) % tiles_x) TW ..)
    const int rb0 = tile_p * NB, rb_total = P.n_img * tpi;   // my row blocks rb0 .. rb0 + NB - 1

    // ---- halo staging: block b = 4 j + wave holds halo pixels 8 b .. 8 b + 7 x 8 channel groups; lane = 8 g + p takes pixel p, group (p + g) & 7 -----
    const int Hs = P.ups ? P.H >> 1 : P.H, Ws = P.ups ? P.W >> 1 : P.W;
    const int pp = lane & 7, pg = ((lane & 7) + (lane >> 3)) & 7;
    int h_pix[NPIECE];                                       // source pixel index (image-major), or -1
#pragma unroll
    for (int j = 0; j < NPIECE; ++j) {
        const int b = NWV * j + wave, px = 8 * b + pp;
        const int blk = px / HB, rem = px - blk * HB;
        const int hy = rem / HW_, hx = rem - hy * HW_;
        const int rb = rb0 + blk;
        const int img = rb / tpi, rin = rb - img * tpi, yb = rin / P.tiles_x, xb = rin - yb * P.tiles_x;
        const int y = yb * TH - 1 + hy, x = xb * TW - 1 + hx;
        const bool in = px < G::HPIX && rb < rb_total && (unsigned)y < (unsigned)P.H && (unsigned)x < (unsigned)P.W;
        const int ys = P.ups ? y >> 1 : y, xs = P.ups ? x >> 1 : x;
        h_pix[j] = in ? (img * Hs + ys) * Ws + xs : -1;
    }
    const int h_lds = pg * PLANE + (8 * wave + pp) * 16;     // + j * 128 NWV (+ buffer)
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)P.x, 0, (int)P.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsX2 = __builtin_amdgcn_make_buffer_rsrc((void*)(P.x2 ? P.x2 : P.x), 0, (int)(P.x2 ? P.x2_bytes : P.x_bytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)P.w, 0, (int)P.w_bytes, 0x00020000);
    const int c2 = P.cin - P.c1;
    auto halo_load = [&](int j, int crel) -> u32x4 {             // crel: chunk relative to my range
        return halo::piece_load(rsX, rsX2, P.c1, c2, h_pix[j], pg, (ck0 + crel) * 64, crel, nchunk);
    };
    auto halo_store = [&](int j, int buf, const u32x4& v) {
        if (8 * (NWV * j + wave) < G::HPIX)                   // (wave-uniform: the last piece index exists for the first waves only)
            *reinterpret_cast<u32x4*>(smem_raw + buf * HALO + h_lds + j * (128 * NWV)) = v;
    };

    // ---- W stream: piece p = KiB p of the 5-KiB sub-tile block; wave w issues piece w, wave 0 also piece 4 --------------------------------------------
    const unsigned w_vo0 = (unsigned)(lane * 16 + wave * 1024);
    const int w_base = (tile_n * nchunk_all + ck0) * NS * WSUB;       // my first sub-tile inside the channel tile's block
    halo::WStream<NBW, WSUB, NWV * 1024> ws;
    ws.start(w_base, nsub);
    auto w_issue = [&](auto cls) { ws.template issue<decltype(cls)::value>(smem_raw, rsW, w_vo0, OFF_W, wave * 1024, w_base, nsub); };

    // ---- fragments: my 80 pixels x all 80 channels ------------------------------------------------------------------------------------------------------
    f32x4 acc[5][5];
    bf16x8 wf[2][5], af[2][5];
    const int wfrag = OFF_W + ((wn * 80 + l15) * 32 + (kq ^ (3 * ((l15 >> 3) & 1))) * 8) * 2;      // + slot * WSUB + nb * 1024
    int afrag[5];                                            // + buf * HALO + half * 4 * PLANE + (ky * HW_ + kx) * 16
#pragma unroll
    for (int mb = 0; mb < 5; ++mb) {
        const int idx = wp * 80 + mb * 16 + l15, blk = idx / RB, r = idx - blk * RB, ty = r / TW, tx = r - ty * TW;
        afrag[mb] = kq * PLANE + (blk * HB + ty * HW_ + tx) * 16 + (PH ? (py * HW_ + px_) * 16 : 0);      // (PH: tap (a, b) reads halo pixel + (py + a, px + b))
    }

    // ---- prologue: halo chunk 0 ------------------------------------------------------------------------------------------------------------------------------
    {
        u32x4 t[NPIECE];
#pragma unroll
        for (int j = 0; j < NPIECE; ++j) t[j] = halo_load(j, 0);
#pragma unroll
        for (int j = 0; j < NPIECE; ++j) halo_store(j, 0, t[j]);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

    auto main_loop = [&](auto cls) {
        constexpr int NW = decltype(cls)::value ? 2 : 1;
        constexpr int PPS = pps<NPIECE, PH>();
        u32x4 hreg[3][PPS];                                  // staged pieces in flight: requested at LOAD(i), written at LOAD(i + 3)
        // W sub-tiles 0 .. DW - 1 in flight; sub-tile 0 retired, published, its fragments (and chunk 0's halo) read into set 0
        w_issue(cls); w_issue(cls); w_issue(cls);
        if constexpr (DW == 4) w_issue(cls);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DW - 1) * NW) : "memory");
        __builtin_amdgcn_s_barrier();
        int rd_slot = 0;
        auto read_frags = [&](int set, int abase, int aimm) {
            const unsigned char* Wp = smem_raw + wfrag + rd_slot * WSUB;
#pragma unroll
            for (int nb = 0; nb < 5; ++nb) wf[set][nb] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Wp + nb * 1024));
#pragma unroll
            for (int mb = 0; mb < 5; ++mb)
                af[set][mb] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(smem_raw + abase + afrag[mb] + aimm));
            rd_slot = rd_slot + 1 == NBW ? 0 : rd_slot + 1;
        };
        read_frags(0, 0, 0);
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int b = 0; b < 5; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

        int cbuf = 0;
        for (int c = 0; c < nchunk; ++c) {
            const int abase = cbuf * HALO, nbuf = cbuf ^ 1;
            auto sub = [&](auto ic) {
                constexpr int i = decltype(ic)::value;       // sub-tile s = NS c + i: multiplied here; sub-tile s + 1's fragments are read here
                constexpr int n1 = (i + 1) % NS, tap1 = n1 >> 1, hk1 = n1 & 1;
                constexpr int aimm1 = hk1 * 4 * PLANE + (PH ? (tap1 >> 1) * HW_ + (tap1 & 1) : (tap1 / 3) * HW_ + (tap1 % 3)) * 16;
                // A. counted wait: my pieces of W sub-tile s + 1 (requested at LOAD(s + 1 - DW), behind that phase's halo requests) and everything
                //    older have landed; what I issued since may stay in flight: DW - 2 W requests and the halo pieces of those phases
                {
                    constexpr int extra = nh<NPIECE, PH>(i - 1) + (DW == 4 ? nh<NPIECE, PH>(i - 2) : 0);
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DW - 2) * NW + extra) : "memory");
                }
                __builtin_amdgcn_sched_barrier(0);
                // B. publish: every wave's pieces of W sub-tile s + 1 are in LDS; every wave has finished reading sub-tile s - 1's slot
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
                // C. the staged halo pieces requested three sub-tiles ago (retired by wait A) go to the NEXT chunk's buffer
#pragma unroll
                for (int k = 0; k < nh<NPIECE, PH>(i - 3); ++k) halo_store(PPS * (i - 3) + k, nbuf, hreg[(i + 15) % 3][k]);
                // D. sub-tile s + 1's fragments into the other register set (the first sub-tile of the next chunk reads the buffer just filled)
                read_frags((i + 1) & 1, i == NS - 1 ? nbuf * HALO : abase, aimm1);
                // E. requests: two halo pieces of the next chunk, then W sub-tile s + DW (into the slot sub-tile s - 1 was read from)
#pragma unroll
                for (int k = 0; k < nh<NPIECE, PH>(i); ++k) hreg[i % 3][k] = halo_load(PPS * i + k, c + 1);
                w_issue(cls);
                // F. 25 MFMAs of sub-tile s, with C - E in their issue shadow: a 16x16x32 MFMA occupies the matrix pipe for 16 cycles and the issue
                //    port for 4 -- the fragment reads, the staging store / loads and the W request (all independent of this sub-tile's operands) go out
                //    between the matrix instructions instead of in front of them (one wave per SIMD: nobody else would cover that time)
#pragma unroll
                for (int mb = 0; mb < 5; ++mb)
#pragma unroll
                    for (int nb = 0; nb < 5; ++nb)
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i & 1][nb], af[i & 1][mb], acc[mb][nb], 0, 0, 0);
                constexpr int NST = PH ? PPS : 2, NRQ = PH ? PPS + 2 : 4;
#pragma unroll
                for (int k = 0; k < NST; ++k) {                  // staging stores first (their data is oldest), one per matrix instruction
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                }
#pragma unroll
                for (int k = 0; k < 10; ++k) {                   // the 10 fragment reads of sub-tile s + 1
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
#pragma unroll
                for (int k = 0; k < NRQ; ++k) {                  // halo requests and the W request(s)
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 25 - 10 - NST - NRQ, 0);
                __builtin_amdgcn_sched_barrier(0);
            };
            sub(IC<0>{}); sub(IC<1>{}); sub(IC<2>{}); sub(IC<3>{}); sub(IC<4>{}); sub(IC<5>{});
            sub(IC<6>{}); sub(IC<7>{});
            if constexpr (!PH) {
                sub(IC<8>{}); sub(IC<9>{}); sub(IC<10>{}); sub(IC<11>{});
                sub(IC<12>{}); sub(IC<13>{}); sub(IC<14>{}); sub(IC<15>{}); sub(IC<16>{}); sub(IC<17>{});
            }
            cbuf = nbuf;
        }
    };
    if (clsA) main_loop(std::true_type{}); else main_loop(std::false_type{});
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // the wrap-around W requests of the tail have landed: LDS is free for the epilogue
    __syncthreads();

    // ---- epilogue: bias / temb in registers, residual through the staging tile, whole-row 16-byte stores ------------------------------------------------
    // my outputs: acc[mb][nb][j] = (tile pixel 80 wave + 16 mb + l15, tile channel 16 nb + 4 kq + j)
    if (!PH && P.splits > 1) {                               // raw fp32 partial sums of my chunks: the finishing pass owns the epilogue
        const int64_t mtot = (int64_t)P.n_img * P.H * P.W;
#pragma unroll
        for (int mb = 0; mb < 5; ++mb) {
            const int r = wp * 80 + mb * 16 + l15;
            const int blk = r / RB, q = r - blk * RB, ty = q / TW, tx = q - ty * TW;
            const int rb = rb0 + blk, img = rb / tpi, rin = rb - img * tpi, yb = rin / P.tiles_x, xb = rin - yb * P.tiles_x, y = yb * TH + ty;
            bool ok = rb < rb_total && y < P.H;
            if constexpr (PARTIAL) ok = ok && xb * TW + tx < P.W;
            if (ok) {
                float* dst = P.ws + ((int64_t)split * mtot + ((int64_t)img * P.H + y) * P.W + xb * TW + tx) * P.cout + n0 + wn * 80 + 4 * kq;
#pragma unroll
                for (int nb = 0; nb < 5; ++nb) *reinterpret_cast<f32x4*>(dst + nb * 16) = acc[mb][nb];
            }
        }
        return;
    }
    constexpr int OP = BN + 8;                               // bf16 pitch of the staging rows (176 / 336 B)
    bf16_t* Os = reinterpret_cast<bf16_t*>(smem_raw);        // [320][OP] = 56,320 B
    constexpr int CPR = BN / 8;                              // sixteen-byte chunks per row
    auto row_pixel = [&](int r, bool& ok) -> int64_t {       // tile row -> global pixel (rows past the image's last row / past the last image: not stored)
        const int blk = r / RB, q = r - blk * RB, ty = q / TW, tx = q - ty * TW;
        const int rb = rb0 + blk, img = rb / tpi, rin = rb - img * tpi, yb = rin / P.tiles_x, xb = rin - yb * P.tiles_x, y = yb * TH + ty;
        ok = rb < rb_total && y < P.H;
        if constexpr (PARTIAL) ok = ok && xb * TW + tx < P.W;
        if constexpr (PH) return ((int64_t)img * (2 * P.H) + 2 * y + py) * (2 * P.W) + 2 * (xb * TW + tx) + px_;      // pixel shuffle
        return ((int64_t)img * P.H + y) * P.W + xb * TW + tx;
    };
    {   // bias and time-embedding words of my outputs: every load of a kind issued before the first is used (one `if (P.temb)` per accumulator block put
        // a load and its own s_waitcnt vmcnt(0) in each of 25 branches: 25 dependent round trips in the epilogue of every first conv of a ResNet block)
        u32x2 bt[5], tt[5][5];
        if (P.bias) {
#pragma unroll
            for (int nb = 0; nb < 5; ++nb) bt[nb] = *reinterpret_cast<const u32x2*>(P.bias + n0 + wn * 80 + nb * 16 + 4 * kq);
        }
        if (P.temb) {                                        // (a tile spans several images: the row's own image)
#pragma unroll
            for (int mb = 0; mb < 5; ++mb) {
                const int idx = wp * 80 + mb * 16 + l15, rb = min(rb0 + idx / RB, rb_total - 1), img = rb / tpi;
                const bf16_t* trow = P.temb + (int64_t)(img / P.temb_div) * P.temb_ld + n0 + wn * 80 + 4 * kq;
#pragma unroll
                for (int nb = 0; nb < 5; ++nb) tt[mb][nb] = *reinterpret_cast<const u32x2*>(trow + nb * 16);
            }
        }
#pragma unroll
        for (int nb = 0; nb < 5; ++nb) {
            float b4[4] = {0.f, 0.f, 0.f, 0.f};
            if (P.bias) {
                b4[0] = __uint_as_float(bt[nb][0] << 16); b4[1] = __uint_as_float(bt[nb][0] & 0xffff0000u);
                b4[2] = __uint_as_float(bt[nb][1] << 16); b4[3] = __uint_as_float(bt[nb][1] & 0xffff0000u);
            }
#pragma unroll
            for (int mb = 0; mb < 5; ++mb) {
                float t4[4] = {0.f, 0.f, 0.f, 0.f};
                if (P.temb) {
                    t4[0] = __uint_as_float(tt[mb][nb][0] << 16); t4[1] = __uint_as_float(tt[mb][nb][0] & 0xffff0000u);
                    t4[2] = __uint_as_float(tt[mb][nb][1] << 16); t4[3] = __uint_as_float(tt[mb][nb][1] & 0xffff0000u);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[mb][nb][j] += b4[j] + t4[j];
            }
        }
    }
    if (P.res) {
        // the residual rows in bursts of RBU loads per thread (rows that are not stored read pixel 0: never used) -- rolled, the loop was
        // load -> s_waitcnt vmcnt(0) -> ds_write per iteration: BM * CPR / NT (12.5 at 4 waves) dependent round trips
        constexpr int NIT = (BM * CPR + NT - 1) / NT, RBU = 7;
#pragma unroll
        for (int h = 0; h < (NIT + RBU - 1) / RBU; ++h) {
            u32x4 rv[RBU];
#pragma unroll
            for (int it = 0; it < RBU; ++it) {
                const int cidx = min(tid + (h * RBU + it) * NT, BM * CPR - 1), r = cidx / CPR, ch = cidx - r * CPR;
                bool ok;
                const int64_t m = row_pixel(r, ok);
                rv[it] = *reinterpret_cast<const u32x4*>(P.res + (ok ? m : 0) * P.cout + n0 + ch * 8);
            }
#pragma unroll
            for (int it = 0; it < RBU; ++it) {
                const int cidx = tid + (h * RBU + it) * NT, r = cidx / CPR, ch = cidx - r * CPR;
                if (cidx < BM * CPR) *reinterpret_cast<u32x4*>(Os + r * OP + ch * 8) = rv[it];
            }
        }
        __syncthreads();
#pragma unroll
        for (int mb = 0; mb < 5; ++mb)
#pragma unroll
            for (int nb = 0; nb < 5; ++nb) {
                const u32x2 t = *reinterpret_cast<const u32x2*>(Os + (wp * 80 + mb * 16 + l15) * OP + wn * 80 + nb * 16 + 4 * kq);
                acc[mb][nb][0] += __uint_as_float(t[0] << 16); acc[mb][nb][1] += __uint_as_float(t[0] & 0xffff0000u);
                acc[mb][nb][2] += __uint_as_float(t[1] << 16); acc[mb][nb][3] += __uint_as_float(t[1] & 0xffff0000u);
            }
        __syncthreads();
    }
#pragma unroll
    for (int mb = 0; mb < 5; ++mb)
#pragma unroll
        for (int nb = 0; nb < 5; ++nb)
            *reinterpret_cast<u32x2*>(Os + (wp * 80 + mb * 16 + l15) * OP + wn * 80 + nb * 16 + 4 * kq) =
                u32x2{pack_bf2(acc[mb][nb][0], acc[mb][nb][1]), pack_bf2(acc[mb][nb][2], acc[mb][nb][3])};
    __syncthreads();
    for (int cidx = tid; cidx < BM * CPR; cidx += NT) {
        const int r = cidx / CPR, ch = cidx - r * CPR;
        bool ok;
        const int64_t m = row_pixel(r, ok);
        if (ok) *reinterpret_cast<u32x4*>(P.out + m * P.cout + n0 + ch * 8) = *reinterpret_cast<const u32x4*>(Os + r * OP + ch * 8);
    }
    // GroupNorm statistics of the ROUNDED outputs, one (sum, sum of squares) pair per (image, row block, group): thread t sums group t % GT over
    // rows t / GT, t / GT + RP, ... of one row block at a time; fixed summation order, no atomics
    if (P.gn_part) {
        const int cpg = P.cout >> 5, GT = BN / cpg, RP = NT / GT, gl = tid % GT;
        float* red = reinterpret_cast<float*>(smem_raw + (size_t)BM * OP * 2);
        for (int blk = 0; blk < NB; ++blk) {
            const int rb = rb0 + blk;
            if (rb >= rb_total) break;                       // (uniform)
            const int img = rb / tpi, sp = rb - img * tpi;
            const int vr = min(TH, P.H - (sp / P.tiles_x) * TH) * TW;       // rows of this block inside the image
            float gs = 0.f, gss = 0.f;
            for (int r = tid / GT; r < vr; r += RP) {
                if constexpr (PARTIAL) { if ((sp % P.tiles_x) * TW + r % TW >= P.W) continue; }
                const unsigned* wsrc = reinterpret_cast<const unsigned*>(Os + (blk * RB + r) * OP + gl * cpg);
                for (int k = 0; k < cpg / 2; ++k) {
                    const unsigned u = wsrc[k];
                    const float a = __uint_as_float(u << 16), b = __uint_as_float(u & 0xffff0000u);
                    gs += a + b;
                    gss += a * a + b * b;
                }
            }
            red[2 * tid] = gs;
            red[2 * tid + 1] = gss;
            __syncthreads();
            if (tid < GT) {
                float a = 0.f, b = 0.f;
                for (int k = 0; k < RP; ++k) { a += red[2 * (tid + k * GT)]; b += red[2 * (tid + k * GT) + 1]; }
                // (PH: one split per (source row block, phase))
                float* dst = P.gn_part + ((PH ? ((int64_t)img * tpi + sp) * 4 + phase : (int64_t)img * tpi + sp) * 32 + (n0 / cpg + tid)) * 2;
                dst[0] = a;
                dst[1] = b;
            }
            __syncthreads();
        }
    }
}

// second pass of a split launch: out = sum over the splits (fixed order) + bias + temb + residual, 8 channels of one pixel per thread
__global__ __launch_bounds__(256) void conv_halo4_finish_kernel(const C4Params P) {
    const int64_t mtot = (int64_t)P.n_img * P.H * P.W, cpr = P.cout / 8, total = mtot * cpr;
    for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = id / cpr;
        const int n = (int)(id - m * cpr) * 8;
        // every operand of the chunk requested before the first is used: bias / temb / residual words, then the partial sums four splits at a time
        // (one load -> wait -> add per split and per side operand was seven dependent round trips for a launch that moves 10 MB)
        u32x4 tb = u32x4{0u, 0u, 0u, 0u}, tt = tb, tr = tb;
        if (P.bias) tb = *reinterpret_cast<const u32x4*>(P.bias + n);
        if (P.temb) tt = *reinterpret_cast<const u32x4*>(P.temb + ((m / ((int64_t)P.H * P.W)) / P.temb_div) * P.temb_ld + n);
        if (P.res) tr = *reinterpret_cast<const u32x4*>(P.res + m * P.cout + n);
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int sp0 = 0; sp0 < P.splits; sp0 += 4) {
            f32x4 pa[4], pb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float* src = P.ws + ((int64_t)min(sp0 + k, P.splits - 1) * mtot + m) * P.cout + n;
                pa[k] = *reinterpret_cast<const f32x4*>(src);
                pb[k] = *reinterpret_cast<const f32x4*>(src + 4);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)                       // (fixed order: split 0, 1, 2, ...)
                if (sp0 + k < P.splits) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { v[j] += pa[k][j]; v[4 + j] += pb[k][j]; }
                }
        }
        const u32x4* side[3] = {&tb, &tt, &tr};
#pragma unroll
        for (int q = 0; q < 3; ++q)                           // + bias, + temb, + residual, in the order of the one-pass epilogue (absent ones add zero words)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[2 * j] += __uint_as_float((*side[q])[j] << 16);
                v[2 * j + 1] += __uint_as_float((*side[q])[j] & 0xffff0000u);
            }
        Vec8<bf16_t>::store(P.out + m * P.cout + n, v);
    }
}

// ---- host side.  Row blocks are 10 x 16 or 5 x 8 pixels (`tw` = 16 / 8), 2 / 8 of them a tile.  Whole row blocks: W % tw == 0; `partial`: images of
// any width, ceil(W / tw) row blocks per image row with a partly filled last one (PARTIAL of conv_halo4_kernel).  Written once for both ------------------
constexpr int c4_th(int tw) { return tw == 8 ? 5 : 10; }
constexpr int c4_nb(int tw) { return tw == 8 ? 8 : 2; }
int c4_tiles_y(int H, int tw) { return (H + c4_th(tw) - 1) / c4_th(tw); }
// (whole row blocks at a ragged width: the floor -- what the whole-tile counts have always answered for a shape their launch refuses)
int c4_tiles_x(int W, int tw, bool partial) { return partial ? (W + tw - 1) / tw : W / tw; }
int c4_row_blocks(int H, int W, int tw, bool partial) { return c4_tiles_y(H, tw) * c4_tiles_x(W, tw, partial); }
int c4_pixel_tiles(int n_img, int H, int W, int tw, bool partial) { return (n_img * c4_row_blocks(H, W, tw, partial) + c4_nb(tw) - 1) / c4_nb(tw); }

template <int TW, int NWV, bool PH> int launch_c4(C4Params& P, bool partial, hipStream_t st) {
    using G = Geo<TW, NWV>;
    static_assert(G::TH == c4_th(TW) && G::NB == c4_nb(TW), "the host's tile counts are the kernel's geometry");
    P.tiles_y = c4_tiles_y(P.H, TW);
    P.tiles_x = c4_tiles_x(P.W, TW, partial);
    P.tiles_p = c4_pixel_tiles(P.n_img, P.H, P.W, TW, partial);
    {   // XCD grid (see the kernel): FMC_C4_XCD = 0 contiguous ranges (rounds 5's order), 1 / 2 / 4 / 8 forced where it divides, unset = least fabric traffic
        static const int forced = fmc_env_int("FMC_C4_XCD", -1);
        const int tnv = P.tiles_n * P.splits;
        double best = 0.;
        P.xcd_pc = 0;
        if (forced != 0 && (P.tiles_p * tnv) % 8 == 0) {
            for (int pc = 1; pc <= 8; pc *= 2) {
                if (tnv % pc || P.tiles_p % (8 / pc) || (forced > 0 && pc != forced)) continue;
                const double cost = (double)P.w_bytes * (8 / pc) + (double)(P.x_bytes + P.x2_bytes) * pc;
                if (!P.xcd_pc || cost < best) { best = cost; P.xcd_pc = pc; }
            }
        }
    }
    const dim3 grid((unsigned)(P.tiles_p * P.tiles_n * P.splits));
    if (partial) fmc_launch<conv_halo4_kernel<TW, NWV, PH, true>>(grid, dim3(G::NT), G::LDS_BYTES, st, P);
    else fmc_launch<conv_halo4_kernel<TW, NWV, PH>>(grid, dim3(G::NT), G::LDS_BYTES, st, P);
    if (P.splits > 1) {
        const int64_t chunks = (int64_t)P.n_img * P.H * P.W * (P.cout / 8);
        const unsigned grid = (unsigned)((chunks + 255) / 256 < 2048 ? (chunks + 255) / 256 : 2048);
        hipLaunchKernelGGL(conv_halo4_finish_kernel, dim3(grid), dim3(256), 0, st, P);
    }
    return 0;
}

// the one choice of the instantiation: 5 x 8 row blocks on 4 waves, 10 x 16 on 4 or (wide) 8
template <bool PH> void c4_launch(C4Params& P, int tw, int wide, bool partial, void* stream) {
    if (tw == 8) launch_c4<8, 4, PH>(P, partial, (hipStream_t)stream);
    else if (wide) launch_c4<16, 8, PH>(P, partial, (hipStream_t)stream);
    else launch_c4<16, 4, PH>(P, partial, (hipStream_t)stream);
}

}  // namespace

// `wide` = 0: 4 waves, 80 output channels per tile; 1: 8 waves, 160 (16-pixel-wide row blocks only).  The packed filter differs between the two.
extern "C" int fmc_conv3x3_halo4_pack_weight(const void* w, void* dst, int Cin, int Cout, int wide, void* stream) {
    const int BN = wide ? 160 : 80;
    if (!w || !dst) FMC_FAIL(FMC_E_NULL, "conv3x3_halo4_pack_weight: NULL pointer");
    if (Cin % 64 || Cout % BN) FMC_FAIL(FMC_E_SHAPE, "conv3x3_halo4_pack_weight: Cin %% 64 / Cout %% %d (Cin=%d Cout=%d)", BN, Cin, Cout);
    if (!fmc_aligned16(w) || !fmc_aligned16(dst)) FMC_FAIL(FMC_E_ALIGN, "conv3x3_halo4_pack_weight: pointers must be 16-byte aligned");
    halo::pack_filter((const bf16_t*)w, (bf16_t*)dst, Cin, Cout, BN, (hipStream_t)stream);      // (the one pack kernel, conv_halo.hip)
    FMC_CHECK_LAUNCH("fmc_conv3x3_halo4_pack_weight");
    return 0;
}

// the whole-tile entry points pick the row blocks themselves: 10 x 16 pixels where W % 16 == 0, else 5 x 8 (W % 8 == 0); any H.  The partial ones take
// `tw` from the caller: 16 (the only one of the wide form) or 8
static int c4_tw(int W) { return W % 16 == 0 ? 16 : 8; }
static bool c4_tw_ok(int tw, int wide) { return tw == 16 || (tw == 8 && !wide); }
// (the conditions of the whole-tile and the partial entry points: the latter drop the width rule alone)
static int c4_shape_ok(int n_img, int H, int W, int Cin, int Cin1, int Cout, int upsample2x, int wide, bool any_width) {
    if (n_img < 1 || H < 1 || W < 1 || Cin % 64 || Cout % (wide ? 160 : 80)) return 0;
    if (!any_width && (W < 8 || W % 8 || (wide && W % 16))) return 0;
    if (Cin1 <= 0 || Cin1 > Cin || Cin1 % 64) return 0;
    if (upsample2x && ((H | W) & 1)) return 0;
    const int64_t hs = upsample2x ? H / 2 : H, ws = upsample2x ? W / 2 : W;
    if ((int64_t)n_img * hs * ws * Cin1 * 2 >= (1ll << 31) || (int64_t)n_img * hs * ws * (Cin - Cin1) * 2 >= (1ll << 31)) return 0;
    if ((int64_t)Cout * 9 * Cin * 2 >= (1ll << 31)) return 0;
    return 1;
}

static int c4_fold_ok(int n_img, int Hs, int Ws, int Cin, int Cout, int wide, bool any_width) {
    if (!c4_shape_ok(n_img, Hs, Ws, Cin, Cin, Cout, 0, wide, any_width)) return 0;      // the source-resolution convolution's own conditions
    if ((int64_t)Cout * 16 * Cin * 2 >= (1ll << 31)) return 0;
    if ((int64_t)n_img * Hs * Ws * 4 >= (1ll << 31)) return 0;
    return 1;
}

static int c4_tiles(int n_img, int H, int W, int Cout, int wide, int tw, bool partial) {
    return c4_pixel_tiles(n_img, H, W, tw, partial) * (Cout / (wide ? 160 : 80));
}

extern "C" int fmc_conv3x3_halo4_supported(int n_img, int H, int W, int Cin, int Cin1, int Cout, int upsample2x, int wide) {
    return c4_shape_ok(n_img, H, W, Cin, Cin1, Cout, upsample2x, wide, false);
}

extern "C" int fmc_conv3x3_halo4_partial_supported(int n_img, int H, int W, int Cin, int Cin1, int Cout, int upsample2x, int wide) {
    return c4_shape_ok(n_img, H, W, Cin, Cin1, Cout, upsample2x, wide, true);
}

extern "C" int fmc_conv3x3_halo4_row_blocks_per_image(int H, int W) { return c4_row_blocks(H, W, c4_tw(W), false); }

extern "C" int fmc_conv3x3_halo4_partial_row_blocks_per_image(int H, int W, int tw) { return c4_row_blocks(H, W, tw, true); }

extern "C" int fmc_conv3x3_halo4_tiles(int n_img, int H, int W, int Cout, int wide) { return c4_tiles(n_img, H, W, Cout, wide, c4_tw(W), false); }

extern "C" int fmc_conv3x3_halo4_partial_tiles(int n_img, int H, int W, int Cout, int wide, int tw) { return c4_tiles(n_img, H, W, Cout, wide, tw, true); }

static int64_t c4_padded_pixels(int H, int W, int tw) { return (int64_t)c4_row_blocks(H, W, tw, true) * c4_th(tw) * tw; }

// the default geometry of a partial launch: that of the whole-tile entry points where W % 8 == 0, else the one with fewer pad pixels over the image (ties: 16)
extern "C" int fmc_conv3x3_halo4_partial_tw(int H, int W, int wide) {
    if (wide) return 16;
    if (W % 8 == 0) return c4_tw(W);
    return c4_padded_pixels(H, W, 8) < c4_padded_pixels(H, W, 16) ? 8 : 16;
}

// the width clause and the tail of the shape message, the two places in which the pairs' messages differ
static const char* c4_width_rule(bool partial, const char* whole) { return partial ? "tw 16 or 8 (wide: 16)" : whole; }
struct C4TwTail {
    char s[24];
    C4TwTail(bool partial, int tw) { s[0] = 0; if (partial) snprintf(s, sizeof s, " tw=%d", tw); }
};

/* fmc_conv3x3_halo4_bf16 and fmc_conv3x3_halo4_partial_bf16 (fmc_hip.h): as fmc_conv3x3_halo_bf16 without the GroupNorm operand path; gn_partials
 * [n_img, row blocks per image, 32, 2]; w_packed = fmc_conv3x3_halo4_pack_weight.  split_k > 1: the 64-channel chunks of the reduction are dealt to
 * split_k workgroups per tile (5x8-pixel images: 64 tiles on 256 CUs otherwise), fp32 partials in `workspace` (>= split_k * n_img * H * W * Cout * 4
 * bytes), summed in a fixed order by a second launch that runs the epilogue; no statistics epilogue then. */
static int c4_plain(bool partial, int tw, const void* x, const void* x2, int Cin1, const void* w_packed, const void* bias, const void* temb,
                    const void* residual, void* out, int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride, int temb_img_div, int upsample2x,
                    float* gn_partials, int split_k, void* workspace, int64_t workspace_bytes, int wide, void* stream) {
    const char* name = partial ? "conv3x3_halo4_partial" : "conv3x3_halo4";
    const int BN = wide ? 160 : 80;
    if (!x2) Cin1 = Cin;
    if (int e = halo::check_args(name, true, x, x2, w_packed, bias, temb, residual, out, temb_row_stride, temb_img_div, gn_partials, Cout, BN,
                                 c4_shape_ok(n_img, H, W, Cin, Cin1, Cout, upsample2x, wide, partial) && c4_tw_ok(tw, wide),
                                 "%s: needs %s, Cin %% 64 == 0 (both sources), Cout %% %d == 0, operands < 2 GiB "
                                 "(n=%d H=%d W=%d Cin=%d+%d Cout=%d ups=%d%s)", c4_width_rule(partial, "W % 8 == 0 (wide: % 16)"), BN, n_img, H, W, Cin1,
                                 Cin - Cin1, Cout, upsample2x, C4TwTail(partial, tw).s))
        return e;
    if (split_k < 1) split_k = 1;
    if (split_k > Cin / 64) split_k = Cin / 64;
    if (split_k > 1) {
        if (gn_partials) FMC_FAIL(FMC_E_SHAPE, "%s: the statistics epilogue is not available with split_k > 1", name);
        if (!workspace || workspace_bytes < (int64_t)split_k * n_img * H * W * Cout * 4 || !fmc_aligned16(workspace))
            FMC_FAIL(FMC_E_SHAPE, "%s: split_k %d needs a 16-byte aligned workspace of %lld bytes", name, split_k, (long long)split_k * n_img * H * W * Cout * 4);
    }
    C4Params P;
    halo::fill_params(P, x, x2, Cin1, w_packed, bias, temb, residual, out, n_img, H, W, Cin, Cout, temb_row_stride, temb_img_div, upsample2x, gn_partials, 9);
    P.tiles_n = Cout / BN;
    P.splits = split_k; P.ws = (float*)workspace;
    c4_launch<false>(P, tw, wide, partial, stream);
    FMC_CHECK_LAUNCH(partial ? "fmc_conv3x3_halo4_partial_bf16" : "fmc_conv3x3_halo4_bf16");
    return 0;
}

extern "C" int fmc_conv3x3_halo4_bf16(const void* x, const void* x2, int Cin1, const void* w_packed, const void* bias, const void* temb,
                                      const void* residual, void* out, int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride,
                                      int temb_img_div, int upsample2x, float* gn_partials, int split_k, void* workspace, int64_t workspace_bytes,
                                      int wide, void* stream) {
    return c4_plain(false, c4_tw(W), x, x2, Cin1, w_packed, bias, temb, residual, out, n_img, H, W, Cin, Cout, temb_row_stride, temb_img_div, upsample2x,
                    gn_partials, split_k, workspace, workspace_bytes, wide, stream);
}

extern "C" int fmc_conv3x3_halo4_partial_bf16(const void* x, const void* x2, int Cin1, const void* w_packed, const void* bias, const void* temb,
                                              const void* residual, void* out, int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride,
                                              int temb_img_div, int upsample2x, float* gn_partials, int split_k, void* workspace,
                                              int64_t workspace_bytes, int wide, int tw, void* stream) {
    return c4_plain(true, tw, x, x2, Cin1, w_packed, bias, temb, residual, out, n_img, H, W, Cin, Cout, temb_row_stride, temb_img_div, upsample2x,
                    gn_partials, split_k, workspace, workspace_bytes, wide, stream);
}

// ---- phase mode of the nearest-2x upsample convolutions on the small feature maps (see conv_halo4_kernel).  Hs, Ws = SOURCE size; w_folded =
// fmc_conv3x3_upfold_pack_weight(filter, tile_channels = 160 if wide else 80) ---------------------------------------------------------------------
extern "C" int fmc_conv3x3_halo4_fold_supported(int n_img, int Hs, int Ws, int Cin, int Cout, int wide) {
    return c4_fold_ok(n_img, Hs, Ws, Cin, Cout, wide, false);
}

extern "C" int fmc_conv3x3_halo4_fold_partial_supported(int n_img, int Hs, int Ws, int Cin, int Cout, int wide) {
    return c4_fold_ok(n_img, Hs, Ws, Cin, Cout, wide, true);
}

static int c4_fold(bool partial, int tw, const void* x, const void* w_folded, const void* bias, void* out, int n_img, int Hs, int Ws, int Cin, int Cout,
                   float* gn_partials, int wide, void* stream) {
    const int BN = wide ? 160 : 80;
    if (int e = halo::check_args(partial ? "conv3x3_halo4_fold_partial" : "conv3x3_halo4_fold", false, x, nullptr, w_folded, bias, nullptr, nullptr, out, 0, 1,
                                 gn_partials, Cout, BN, c4_fold_ok(n_img, Hs, Ws, Cin, Cout, wide, partial) && c4_tw_ok(tw, wide),
                                 "%s: needs %s, Cin %% 64 == 0, Cout %% %d == 0, operands < 2 GiB (n=%d Hs=%d Ws=%d Cin=%d Cout=%d%s)",
                                 c4_width_rule(partial, "Ws % 8 == 0 (wide: % 16)"), BN, n_img, Hs, Ws, Cin, Cout, C4TwTail(partial, tw).s))
        return e;
    C4Params P;
    halo::fill_params(P, x, nullptr, Cin, w_folded, bias, nullptr, nullptr, out, n_img, Hs, Ws, Cin, Cout, 0, 1, 0, gn_partials, 16);
    P.tiles_n = 4 * (Cout / BN);
    P.splits = 1; P.ws = nullptr;
    c4_launch<true>(P, tw, wide, partial, stream);
    FMC_CHECK_LAUNCH(partial ? "fmc_conv3x3_halo4_fold_partial_bf16" : "fmc_conv3x3_halo4_fold_bf16");
    return 0;
}

extern "C" int fmc_conv3x3_halo4_fold_bf16(const void* x, const void* w_folded, const void* bias, void* out, int n_img, int Hs, int Ws, int Cin,
                                           int Cout, float* gn_partials, int wide, void* stream) {
    return c4_fold(false, c4_tw(Ws), x, w_folded, bias, out, n_img, Hs, Ws, Cin, Cout, gn_partials, wide, stream);
}

extern "C" int fmc_conv3x3_halo4_fold_partial_bf16(const void* x, const void* w_folded, const void* bias, void* out, int n_img, int Hs, int Ws, int Cin,
                                                   int Cout, float* gn_partials, int wide, int tw, void* stream) {
    return c4_fold(true, tw, x, w_folded, bias, out, n_img, Hs, Ws, Cin, Cout, gn_partials, wide, stream);
}

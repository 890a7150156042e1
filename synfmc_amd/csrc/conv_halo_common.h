// NOT in the benchmark's source-hash list: after an edit here, re-collect the conv_halo* entries of profiles/roofline_counters.json by hand.
// What the two halo-resident 3x3 convolutions share (conv_halo.hip: 10 x 32-pixel tiles of one image, 8 waves, two-barrier loop; conv_halo4.hip:
// 320 pixels of whole row blocks, 4 / 8 waves, one-barrier software-pipelined loop): the common kernel parameters, the halo piece addressing, the
// W stream, the filter pack launch, the host-side checks and parameter filling.  Every piece is written so that both kernels compile to the
// instruction streams they had with their own copies (profiles/conv_halo_shared.md; the epilogue and the tile decode did not, and stay per kernel).
#pragma once
#include <type_traits>

#include "common.h"

namespace halo {

constexpr unsigned OOB = 0x80000000u;                      // buffer offset no operand reaches (all < 2 GiB): the load returns zeros

template <int I> using IC = std::integral_constant<int, I>;

// ---- kernel parameters: what both kernels read; each adds its own fields behind (the order of the fields is the kernel-argument layout) -------
struct Params {
    const bf16_t* x; const bf16_t* x2;      // input [n_img, Hs, Ws, c1] (+ second channel block [n_img, Hs, Ws, cin - c1]: the up blocks' skip connection)
    int c1;                                 // channels [0, c1) come from x; c1 == cin without x2; c1 % 64 == 0
    const bf16_t* w;                        // packed filter (fmc_conv3x3_halo_pack_weight / _halo4_pack_weight / _upfold_pack_weight)
    const bf16_t* bias; const bf16_t* temb; const bf16_t* res; bf16_t* out;
    int n_img, H, W, cin, cout, ups;        // H, W = OUTPUT size; ups: x is [n_img, H/2, W/2, .] read through a nearest 2x upsample
                                            // (phase mode: H, W = SOURCE size, the output is [n_img, 2 H, 2 W, cout]; tiles_n = 4 * cout / BN)
    int64_t temb_ld; int temb_div;
};
// A kernel's own block is `struct XParams : halo::Params` + gn_part (statistics partials or NULL) and x_bytes / x2_bytes / w_bytes, which
// fill_params sets by name (in the base they would move every kernel argument behind them).

// ---- one 16-byte piece of the input halo: source pixel `hp` (image-major, -1: outside the image / past the halo), channel group `pg` of the 64-channel
// chunk that begins at channel `cbeg`, chunk `crel` of the workgroup's `nchunk`.  Which source, its row pitch and the channel offset inside it are
// wave-uniform; branch-free per lane.  crel >= nchunk (the staging schedule runs one chunk ahead): nothing is fetched -----------------------------------
__device__ __forceinline__ u32x4 piece_load(const __amdgpu_buffer_rsrc_t& rsX, const __amdgpu_buffer_rsrc_t& rsX2, int c1, int c2, int hp, int pg,
                                            int cbeg, int crel, int nchunk) {
    const bool second = cbeg >= c1, past = crel >= nchunk;
    const int pitch = past ? 0 : (second ? c2 : c1) * 2;
    const unsigned coff = past ? OOB : (unsigned)(((second ? cbeg - c1 : cbeg) + pg * 8) * 2);
    unsigned vo = (unsigned)(hp * pitch) + coff;
    vo = hp < 0 ? OOB : vo;
    const __amdgpu_buffer_rsrc_t rs = second ? rsX2 : rsX;
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)vo, 0, 0));
}

// ---- W stream.  The packed filter holds, per channel tile, the 32-deep sub-tiles in the order the loop multiplies them, [BN rows][32] each with the
// LDS chunk swizzle already applied: a sub-tile is WSUB bytes = 1-KiB pieces that go to LDS as they are.  A wave requests its piece of the next
// sub-tile per issue(), class-A waves (`TWO`) a second one SECOND bytes further on, into a ring of NBW slots.  Past the end the stream wraps to
// valid addresses, so that the counted waits of the tail stay exact.
// The shape of this struct (state only, member order, what is an argument, the association of the LDS address) is what compiles to the two kernels'
// former instruction streams, not what reads best: after ANY edit here re-run the assembly comparison of profiles/conv_halo_shared.md. -----------------
template <int NBW, int WSUB, int SECOND> struct WStream {
    int slot, left, soff;                   // ring slot the next sub-tile goes to, sub-tiles until the wrap, its byte offset in the packed filter
                                            // (in this order the compiler numbers the three as it did the kernels' own locals)
    __device__ __forceinline__ void start(int base, int nsub) { soff = base; left = nsub; slot = 0; }
    // vo: per lane, my 16 bytes of my piece; ring, piece: LDS offset of the ring, of my piece in a slot; base, nsub: my first sub-tile, sub-tiles until the wrap
    template <bool TWO>
    __device__ __forceinline__ void issue(unsigned char* smem_raw, const __amdgpu_buffer_rsrc_t& rs, unsigned vo, int ring, int piece, int base, int nsub) {
        unsigned char* dst = smem_raw + ring + slot * WSUB + piece;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, (int)vo, soff, 0, 0);
        if constexpr (TWO)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + SECOND), 16, (int)vo, soff + SECOND, 0, 0);
        soff += WSUB;
        if (--left == 0) { left = nsub; soff = base; }
        slot = slot + 1 == NBW ? 0 : slot + 1;
    }
};

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------------
// The filter pack kernels are compiled once, in conv_halo.hip.  [Cout][3][3][Cin] (channels-last filter) -> [Cout / bn][Cin / 64][9 taps][2 halves]
// [bn rows][32], chunk-swizzled; bn = 80 / 160 output channels per tile.
void pack_filter(const bf16_t* w, bf16_t* dst, int Cin, int Cout, int bn, hipStream_t st);
// Shortcut mode: the same order with the 1x1 filter w_sc [Cout][Cin_sc] behind it in every channel tile:
// [Cout / bn][(Cin / 64) * 18 + (Cin_sc / 64) * 2 sub-tiles][bn rows][32], the shortcut sub-tiles [Cin_sc / 64][2 halves].
void pack_filter_sc(const bf16_t* w, const bf16_t* w_sc, bf16_t* dst, int Cin, int Cout, int Cin_sc, int bn, hipStream_t st);

// The argument checks of the four launch entry points, in their order: NULL, the entry point's own shape condition (`shape_ok`; its message and
// arguments come behind), alignment, temb_img_div, the statistics-epilogue condition.  `name` heads every message.  `full`: the entry point has
// the x2 / residual / temb operands (the phase-mode ones do not, and say so in the alignment message).
template <class... A>
int check_args(const char* name, bool full, const void* x, const void* x2, const void* w, const void* bias, const void* temb, const void* residual,
               const void* out, int64_t temb_row_stride, int temb_img_div, const float* gn_partials, int Cout, int bn, bool shape_ok,
               const char* shape_fmt, A... shape_args) {
    if (!x || !w || !out) FMC_FAIL(FMC_E_NULL, "%s: NULL x / w / out", name);
    if (!shape_ok) FMC_FAIL(FMC_E_SHAPE, shape_fmt, name, shape_args...);
    if (!fmc_aligned16(x) || !fmc_aligned16(w) || !fmc_aligned16(out) || (x2 && !fmc_aligned16(x2)) || (residual && !fmc_aligned16(residual)) ||
        (bias && (reinterpret_cast<uintptr_t>(bias) & 7)) || (temb && ((reinterpret_cast<uintptr_t>(temb) & 7) || temb_row_stride % 4)))
        FMC_FAIL(FMC_E_ALIGN, full ? "%s: x / w / out / residual must be 16-byte aligned, bias / temb rows 8-byte aligned"
                                   : "%s: x / w / out must be 16-byte aligned, bias 8-byte aligned", name);
    if (temb && temb_img_div < 1) FMC_FAIL(FMC_E_SHAPE, "%s: temb_img_div %d", name, temb_img_div);
    if (gn_partials && (Cout % 64 || bn % (Cout / 32)))     // a channel tile must hold whole GroupNorm groups of an even number of channels
        FMC_FAIL(FMC_E_SHAPE, "%s: the statistics epilogue needs Cout %% 64 == 0 and %d %% (Cout / 32) == 0 (Cout=%d)", name, bn, Cout);
    return 0;
}

// The index map of that order (the pack kernel's, and fmc_conv3x3_halo_sc_pack_source's for the host): 16-byte chunk `id` of the packed filter holds the
// eight elements from `return value` on of the 3x3 filter [Cout][3][3][Cin] or (*from_sc) of the 1x1 filter [Cout][Cin_sc].
__host__ __device__ inline int64_t sc_pack_source(int64_t id, int cin, int cin_sc, int bn, int* from_sc) {
    const int n3 = (cin >> 6) * 18, nsub = n3 + (cin_sc >> 6) * 2;
    int64_t t = id;
    const int p = (int)(t & 3); t >>= 2;
    const int row = (int)(t % bn); t /= bn;
    const int sub = (int)(t % nsub), nt = (int)(t / nsub);
    const int lc = p ^ (3 * ((row >> 3) & 1));                           // physical chunk p of a row holds logical chunk lc
    const int64_t co = (int64_t)nt * bn + row;
    *from_sc = sub >= n3;
    if (sub < n3) {
        const int hk = sub & 1, tap = (sub >> 1) % 9, ch64 = sub / 18;
        return (co * 9 + tap) * cin + ch64 * 64 + hk * 32 + lc * 8;
    }
    const int hk = (sub - n3) & 1, ch64 = (sub - n3) >> 1;
    return co * cin_sc + ch64 * 64 + hk * 32 + lc * 8;
}

// Shortcut mode: the conditions on the two shortcut sources (channels % 64, each below 2 GiB, the combined filter below 2 GiB) ...
inline int sc_sources_ok(int n_img, int H, int W, int Cin, int Cout, int Cin_sc, int Cin_sc1) {
    if (Cin_sc < 64 || Cin_sc % 64 || Cin_sc1 <= 0 || Cin_sc1 > Cin_sc || Cin_sc1 % 64) return 0;
    const int64_t px = (int64_t)n_img * H * W;
    if (px * Cin_sc1 * 2 >= (1ll << 31) || px * (Cin_sc - Cin_sc1) * 2 >= (1ll << 31)) return 0;
    if ((int64_t)Cout * (9 * (int64_t)Cin + Cin_sc) * 2 >= (1ll << 31)) return 0;
    return 1;
}
// ... their pointer checks, behind check_args ...
inline int check_sc_args(const char* name, const void* xs, const void* xs2) {
    if (!xs) FMC_FAIL(FMC_E_NULL, "%s: NULL shortcut input", name);
    if (!fmc_aligned16(xs) || (xs2 && !fmc_aligned16(xs2))) FMC_FAIL(FMC_E_ALIGN, "%s: the shortcut inputs must be 16-byte aligned", name);
    return 0;
}
// ... and their part of the parameter block (behind fill_params, which sets w_bytes for the 3x3 filter alone)
template <class P_>
void fill_params_sc(P_& P, const void* xs, const void* xs2, int Cin_sc1, int Cin_sc) {
    P.xs = (const bf16_t*)xs; P.xs2 = (const bf16_t*)xs2; P.cs1 = Cin_sc1; P.cin_sc = Cin_sc;
    const int64_t px = (int64_t)P.n_img * P.H * P.W;
    P.xs_bytes = px * Cin_sc1 * 2; P.xs2_bytes = px * (Cin_sc - Cin_sc1) * 2;
    P.w_bytes += (int64_t)P.cout * Cin_sc * 2;
}

// The common part of a parameter block.  H, W as in Params (phase mode: the source size, ups = 0); taps = 9, or 16 for the folded filter.
template <class P_>
void fill_params(P_& P, const void* x, const void* x2, int Cin1, const void* w, const void* bias, const void* temb, const void* residual, void* out,
                 int n_img, int H, int W, int Cin, int Cout, int64_t temb_row_stride, int temb_img_div, int upsample2x, float* gn_partials, int taps) {
    P.x = (const bf16_t*)x; P.x2 = (const bf16_t*)x2; P.c1 = Cin1;
    P.w = (const bf16_t*)w; P.bias = (const bf16_t*)bias; P.temb = (const bf16_t*)temb; P.res = (const bf16_t*)residual; P.out = (bf16_t*)out;
    P.n_img = n_img; P.H = H; P.W = W; P.cin = Cin; P.cout = Cout; P.ups = upsample2x ? 1 : 0;
    P.temb_ld = temb_row_stride; P.temb_div = temb ? temb_img_div : 1;
    P.gn_part = gn_partials;
    const int64_t hs = upsample2x ? H / 2 : H, ws = upsample2x ? W / 2 : W;
    P.x_bytes = (int64_t)n_img * hs * ws * Cin1 * 2; P.x2_bytes = (int64_t)n_img * hs * ws * (Cin - Cin1) * 2;
    P.w_bytes = (int64_t)Cout * taps * Cin * 2;
}

}  // namespace halo

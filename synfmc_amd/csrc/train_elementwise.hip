// The small bf16 passes a training step of the Camera Encoder / OMC Adapter needs next to its GEMMs and convolutions: the 2x2 average
// pool of the ResNet blocks' downsample and its backward, ReLU and its backward, and the `h + pose` add in front of the Camera-Adapter merge.
//
//   fmc_avgpool2x2_fwd   y[n, i, j, c]  = bf16(0.25f * (((x[2i, 2j] + x[2i, 2j+1]) + x[2i+1, 2j]) + x[2i+1, 2j+1]))      NHWC, floor(H/2) x floor(W/2)
//   fmc_avgpool2x2_bwd   dx[n, h, w, c] = bf16(0.25f * dy[n, h/2, w/2, c]) where h < 2 floor(H/2) and w < 2 floor(W/2), else +0
//   fmc_relu_fwd         y = x < 0 ? +0 : x              (std::max(x, 0): -0 and NaN pass through)
//   fmc_relu_bwd         dx = y > 0 ? dy : +0
//   fmc_add_bf16         out = bf16(float(a) + float(b))
//
// Pure HBM passes.  Every element of an output is written by exactly one thread, once: no atomics, a fixed order, bit-reproducible.
//
// Layout of the flat kernels (ReLU, add), as in sampler_step.hip: `head` leading elements bring the OUTPUT to a 16-byte boundary and are done
// one by one, then runs of 8 elements per thread, then a tail of n % 8 elements.  Every stream is tested on the host for 16-byte alignment
// at the first run (one bit of `vec` each): an aligned stream moves as 16-byte vectors, any other element by element in the same thread.
// The pooling kernels move 8 channels of one pixel per thread (C % 8 == 0): a tensor whose base is 16-byte aligned moves as vectors, any
// other element by element.
//
// Aliasing: an output may be one of its inputs (a thread loads all of its elements before its first store, and no two threads share one).
#include "common.h"

namespace {

constexpr int TE_BLOCK = 256;      // threads per workgroup
constexpr int TE_PER = 8;          // elements per thread and trip
constexpr int TE_GRID_CAP = 1024;  // workgroups: 4 per CU of an MI355X; a 2M-element trip

__device__ __forceinline__ void te_ld8(const bf16_t* p, bool vec, float (&v)[8]) {
    if (vec) {
        Vec8<bf16_t>::load(p, v);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = bf2f(p[k]);
    }
}

__device__ __forceinline__ void te_st8(bf16_t* p, bool vec, const float (&v)[8]) {
    if (vec) {
        Vec8<bf16_t>::store(p, v);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = f2bf(v[k]);
    }
}

// ---- flat kernels: out[i] = Op(a[i], b[i]) ---------------------------------------------------------------------------------
struct OpRelu {
    static constexpr bool two = false;
    __device__ __forceinline__ static float f(float a, float) { return a < 0.f ? 0.f : a; }
};
struct OpReluBwd {                 // a = dy, b = y
    static constexpr bool two = true;
    __device__ __forceinline__ static float f(float a, float b) { return b > 0.f ? a : 0.f; }
};
struct OpAdd {
    static constexpr bool two = true;
    __device__ __forceinline__ static float f(float a, float b) { return a + b; }
};

struct FlatArgs {
    const bf16_t* a;
    const bf16_t* b;       // NULL for a one-input op
    bf16_t* out;
    int64_t n;
    int head;              // leading scalar elements
    unsigned vec;          // bit 0 / 1 / 2: a / b / out is 16-byte aligned at element `head`
};

template <class Op>
__device__ __forceinline__ void flat_scalar(const FlatArgs& g, int64_t i) {
    const float a = bf2f(g.a[i]);
    const float b = Op::two ? bf2f(g.b[i]) : 0.f;
    g.out[i] = f2bf(Op::f(a, b));
}

template <class Op>
__global__ __launch_bounds__(TE_BLOCK) void flat_kernel(const FlatArgs g) {
    const int64_t tid = (int64_t)blockIdx.x * TE_BLOCK + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * TE_BLOCK;
    const int64_t runs = (g.n - g.head) / TE_PER;
    const int64_t tail0 = g.head + runs * TE_PER;
    for (int64_t r = tid; r < runs; r += nthreads) {
        const int64_t i = g.head + r * TE_PER;
        float a[8], b[8], o[8];
        te_ld8(g.a + i, g.vec & 1u, a);
        if (Op::two) te_ld8(g.b + i, g.vec >> 1 & 1u, b);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = Op::f(a[k], Op::two ? b[k] : 0.f);
        te_st8(g.out + i, g.vec >> 2 & 1u, o);
    }
    // head and tail: at most 7 + 7 elements, one thread each (the first workgroup holds them all)
    if (tid < g.head) flat_scalar<Op>(g, tid);
    if (tid >= g.head && tid - g.head < TE_PER && tail0 + (tid - g.head) < g.n) flat_scalar<Op>(g, tail0 + (tid - g.head));
}

template <class Op>
int flat_launch(const char* name, const void* a, const void* b, void* out, int64_t n, void* stream) {
    if (!a || !out || (Op::two && !b)) FMC_FAIL(FMC_E_NULL, "%s: NULL argument", name);
    if (n <= 0) FMC_FAIL(FMC_E_SHAPE, "%s: bad n=%lld", name, (long long)n);
    const void* ptr[3] = {a, Op::two ? b : nullptr, out};
    for (int s = 0; s < 3; ++s)
        if (ptr[s] && reinterpret_cast<uintptr_t>(ptr[s]) % 2) FMC_FAIL(FMC_E_ALIGN, "%s: stream %d is not aligned to its element size", name, s);
    FlatArgs g;
    g.a = (const bf16_t*)a;
    g.b = Op::two ? (const bf16_t*)b : nullptr;
    g.out = (bf16_t*)out;
    g.n = n;
    int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) / 2;
    if (head > n) head = n;
    g.head = (int)head;
    g.vec = 0;
    for (int s = 0; s < 3; ++s)
        if (ptr[s] && (reinterpret_cast<uintptr_t>(ptr[s]) + (size_t)head * 2) % 16 == 0) g.vec |= 1u << s;
    int64_t blocks = ((n - head) / TE_PER + TE_BLOCK - 1) / TE_BLOCK;
    if (blocks > TE_GRID_CAP) blocks = TE_GRID_CAP;
    if (blocks < 1) blocks = 1;              // (head + tail <= 7 + 7 elements fit one workgroup)
    fmc_launch<flat_kernel<Op>>(dim3((unsigned)blocks), dim3(TE_BLOCK), 0, (hipStream_t)stream, g);
    FMC_CHECK_LAUNCH(name);
    return 0;
}

// ---- 2x2 average pool, NHWC ------------------------------------------------------------------------------------------------
struct PoolArgs {
    const bf16_t* src;     // forward: x [N, H, W, C];   backward: dy [N, Ho, Wo, C]
    bf16_t* dst;           // forward: y [N, Ho, Wo, C]; backward: dx [N, H, W, C]
    int64_t items;         // 8-channel groups of dst
    int H, W, Ho, Wo, C8;  // C8 = C / 8
    int src_vec, dst_vec;  // the tensor's base is 16-byte aligned
};

__global__ __launch_bounds__(TE_BLOCK) void avgpool2x2_fwd_kernel(const PoolArgs p) {
    const int64_t nthreads = (int64_t)gridDim.x * TE_BLOCK;
    const int64_t C = (int64_t)p.C8 * 8;
    for (int64_t t = (int64_t)blockIdx.x * TE_BLOCK + threadIdx.x; t < p.items; t += nthreads) {
        const int c8 = (int)(t % p.C8);
        int64_t r = t / p.C8;
        const int j = (int)(r % p.Wo);
        r /= p.Wo;
        const int i = (int)(r % p.Ho);
        const int64_t n = r / p.Ho;
        const bf16_t* x00 = p.src + ((n * p.H + 2 * i) * p.W + 2 * j) * C + (int64_t)c8 * 8;
        float a[8], b[8], c[8], d[8], o[8];
        te_ld8(x00, p.src_vec, a);
        te_ld8(x00 + C, p.src_vec, b);
        te_ld8(x00 + (int64_t)p.W * C, p.src_vec, c);
        te_ld8(x00 + (int64_t)p.W * C + C, p.src_vec, d);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = 0.25f * (((a[k] + b[k]) + c[k]) + d[k]);
        te_st8(p.dst + t * 8, p.dst_vec, o);
    }
}

__global__ __launch_bounds__(TE_BLOCK) void avgpool2x2_bwd_kernel(const PoolArgs p) {
    const int64_t nthreads = (int64_t)gridDim.x * TE_BLOCK;
    const int64_t C = (int64_t)p.C8 * 8;
    for (int64_t t = (int64_t)blockIdx.x * TE_BLOCK + threadIdx.x; t < p.items; t += nthreads) {
        const int c8 = (int)(t % p.C8);
        int64_t r = t / p.C8;
        const int w = (int)(r % p.W);
        r /= p.W;
        const int h = (int)(r % p.H);
        const int64_t n = r / p.H;
        float o[8];
        if (h < 2 * p.Ho && w < 2 * p.Wo) {      // (the last row / column of an odd size belongs to no window)
            float g[8];
            te_ld8(p.src + ((n * p.Ho + h / 2) * p.Wo + w / 2) * C + (int64_t)c8 * 8, p.src_vec, g);
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = 0.25f * g[k];
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = 0.f;
        }
        te_st8(p.dst + t * 8, p.dst_vec, o);
    }
}

int pool_args(const char* name, const void* src, void* dst, int n_img, int H, int W, int C, bool backward, PoolArgs& p) {
    if (n_img <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) FMC_FAIL(FMC_E_SHAPE, "%s: bad n=%d H=%d W=%d C=%d (C %% 8 == 0)", name, n_img, H, W, C);
    p.H = H;
    p.W = W;
    p.Ho = H / 2;
    p.Wo = W / 2;
    p.C8 = C / 8;
    const int64_t small = (int64_t)n_img * p.Ho * p.Wo * p.C8, large = (int64_t)n_img * H * W * p.C8;
    p.items = backward ? large : small;
    const bool src_empty = backward && small == 0;      // (an H or W of 1: dY holds nothing, dX is all zeros)
    if (!dst && p.items > 0) FMC_FAIL(FMC_E_NULL, "%s: NULL output", name);
    if (!src && p.items > 0 && !src_empty) FMC_FAIL(FMC_E_NULL, "%s: NULL input", name);
    if (reinterpret_cast<uintptr_t>(src) % 2 || reinterpret_cast<uintptr_t>(dst) % 2)
        FMC_FAIL(FMC_E_ALIGN, "%s: a tensor is not aligned to its element size", name);
    p.src = (const bf16_t*)src;
    p.dst = (bf16_t*)dst;
    p.src_vec = fmc_aligned16(src);
    p.dst_vec = fmc_aligned16(dst);
    return 0;
}

inline dim3 pool_grid(int64_t items) {
    int64_t blocks = (items + TE_BLOCK - 1) / TE_BLOCK;
    if (blocks > TE_GRID_CAP) blocks = TE_GRID_CAP;
    return dim3((unsigned)blocks);
}

}  // namespace

extern "C" int fmc_avgpool2x2_fwd(const void* x, void* y, int n_img, int H, int W, int C, void* stream) {
    PoolArgs p;
    if (int rc = pool_args("fmc_avgpool2x2_fwd", x, y, n_img, H, W, C, false, p)) return rc;
    if (p.items == 0) return 0;                         // H or W of 1: an empty output
    fmc_launch<avgpool2x2_fwd_kernel>(pool_grid(p.items), dim3(TE_BLOCK), 0, (hipStream_t)stream, p);
    FMC_CHECK_LAUNCH("fmc_avgpool2x2_fwd");
    return 0;
}

extern "C" int fmc_avgpool2x2_bwd(const void* dy, void* dx, int n_img, int H, int W, int C, void* stream) {
    PoolArgs p;
    if (int rc = pool_args("fmc_avgpool2x2_bwd", dy, dx, n_img, H, W, C, true, p)) return rc;
    fmc_launch<avgpool2x2_bwd_kernel>(pool_grid(p.items), dim3(TE_BLOCK), 0, (hipStream_t)stream, p);
    FMC_CHECK_LAUNCH("fmc_avgpool2x2_bwd");
    return 0;
}

extern "C" int fmc_relu_fwd(const void* x, void* y, int64_t n, void* stream) { return flat_launch<OpRelu>("fmc_relu_fwd", x, nullptr, y, n, stream); }

extern "C" int fmc_relu_bwd(const void* dy, const void* y, void* dx, int64_t n, void* stream) {
    return flat_launch<OpReluBwd>("fmc_relu_bwd", dy, y, dx, n, stream);
}

extern "C" int fmc_add_bf16(const void* a, const void* b, void* out, int64_t n, void* stream) {
    return flat_launch<OpAdd>("fmc_add_bf16", a, b, out, n, stream);
}

// One element-wise step kernel for every sampler of the denoising loop (schedulers.py): DDIM with eta / clipping / v-prediction,
// Euler, Euler-ancestral and DPM-Solver++ multistep are the same linear form with host-computed coefficients.  Per element, fp32:
//
//   e  = has_uncond ? eu + g (ec - eu) : e0
//   m  = m_x x + m_e e ;  m = clamp(m, -m_clamp, +m_clamp) when m_clamp > 0
//   x' = c_x x + c_e e + c_m m + sum_{j < n_hist} c_h[j] hist[j] + c_n noise
//
// and the next step's model input x_in[r] = (model dtype)(in_scale x'), r < in_reps, so that the loop needs no `cat` and no cast.
//
// A pure HBM pass: n (e_bytes (1 + has_uncond + noise) + 4 (1 + n_hist) read + 4 (1 + m_out) + in_bytes in_reps written).
//
// Layout of the work: `head` leading elements bring x to a 16-byte boundary and are done one by one, then runs of 8 elements per
// thread, then a tail of n % 8 elements.  Every stream is tested on the host for 16-byte alignment at the first run (one bit of
// `vec` each): an aligned stream moves as 16-byte vectors, any other (the conditional half of a bf16 eps_uc or the second copy of
// x_in at odd n, a view into the middle of a buffer) moves element by element in the same thread, with the same arithmetic.
//
// Aliasing: x_out may be x, m_out may be any hist[j]: a thread loads all of its elements of every input before its first store,
// and no two threads share an element; those pointers are therefore NOT __restrict__.
//
// Roundings on the longest chain (tests/sampler_common.py counts them): ec - eu, g *, eu +, m_e *, + m_x x, c_m *, the six adds of
// the sum, in_scale * -- hipcc's contraction into fma only removes some.
#include "common.h"

namespace {

constexpr int SS_BLOCK = 256;      // threads per workgroup
constexpr int SS_PER = 8;          // elements per thread and trip
constexpr int SS_GRID_CAP = 1024;  // workgroups: 4 per CU of an MI355X; a 2M-element trip

enum { S_EU = 0, S_EC, S_NOISE, S_X, S_H0, S_H1, S_H2, S_XOUT, S_MOUT, S_IN0, S_IN1, S_COUNT };

struct SamplerArgs {
    const void* eu;
    const void* ec;          // NULL: no unconditional half
    const void* noise;       // NULL: none
    const float* x;
    const float* hist[3];
    float* x_out;
    float* m_out;            // NULL: not wanted
    void* x_in[2];           // NULL: not wanted
    int64_t n;
    int head;                // leading scalar elements
    unsigned vec;            // bit s: stream s is 16-byte aligned at element `head`
    int n_hist;
    fmc_sampler_coef c;
};

template <typename T> __device__ __forceinline__ float ld_one(const T* p);
template <> __device__ __forceinline__ float ld_one<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ld_one<bf16_t>(const bf16_t* p) { return bf2f(*p); }
template <typename T> __device__ __forceinline__ void st_one(T* p, float v);
template <> __device__ __forceinline__ void st_one<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void st_one<bf16_t>(bf16_t* p, float v) { *p = f2bf(v); }

template <typename T>
__device__ __forceinline__ void ld8(const T* p, bool vec, float (&v)[8]) {
    if (vec) {
        Vec8<T>::load(p, v);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = ld_one<T>(p + k);
    }
}

template <typename T>
__device__ __forceinline__ void st8(T* p, bool vec, const float (&v)[8]) {
    if (vec) {
        Vec8<T>::store(p, v);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) st_one<T>(p + k, v[k]);
    }
}

// the update of one element; `h` holds hist[j] for j < n_hist (anything beyond is not read)
__device__ __forceinline__ float sampler_update(const fmc_sampler_coef& c, bool has_uncond, bool has_noise, int n_hist, float eu, float ec,
                                                float x, const float (&h)[3], float nz, float& m_ret) {
    const float e = has_uncond ? eu + c.g * (ec - eu) : eu;
    float m = c.m_x * x + c.m_e * e;
    if (c.m_clamp > 0.f) m = fminf(fmaxf(m, -c.m_clamp), c.m_clamp);
    float acc = c.c_x * x + c.c_e * e;
    acc += c.c_m * m;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (j < n_hist) acc += c.c_h[j] * h[j];
    if (has_noise) acc += c.c_n * nz;
    m_ret = m;
    return acc;
}

template <typename TE, typename TI>
__device__ __forceinline__ void sampler_scalar(const SamplerArgs& a, int64_t i) {
    const bool has_uncond = a.ec != nullptr, has_noise = a.noise != nullptr;
    const float eu = ld_one<TE>((const TE*)a.eu + i);
    const float ec = has_uncond ? ld_one<TE>((const TE*)a.ec + i) : 0.f;
    const float nz = has_noise ? ld_one<TE>((const TE*)a.noise + i) : 0.f;
    const float x = a.x[i];
    float h[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (j < a.n_hist) h[j] = a.hist[j][i];
    float m;
    const float xn = sampler_update(a.c, has_uncond, has_noise, a.n_hist, eu, ec, x, h, nz, m);
    a.x_out[i] = xn;
    if (a.m_out) a.m_out[i] = m;
    const float xi = a.c.in_scale * xn;
    if (a.x_in[0]) st_one<TI>((TI*)a.x_in[0] + i, xi);
    if (a.x_in[1]) st_one<TI>((TI*)a.x_in[1] + i, xi);
}

template <typename TE, typename TI>
__global__ __launch_bounds__(SS_BLOCK) void sampler_step_kernel(const SamplerArgs a) {
    const int64_t tid = (int64_t)blockIdx.x * SS_BLOCK + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * SS_BLOCK;
    const bool has_uncond = a.ec != nullptr, has_noise = a.noise != nullptr;
    const int64_t runs = (a.n - a.head) / SS_PER;
    const int64_t tail0 = a.head + runs * SS_PER;

    for (int64_t r = tid; r < runs; r += nthreads) {
        const int64_t i = a.head + r * SS_PER;
        float eu[8], ec[8], nz[8], x[8], h[3][8], xn[8], m[8], xi[8];
        ld8<TE>((const TE*)a.eu + i, a.vec >> S_EU & 1, eu);
        if (has_uncond) ld8<TE>((const TE*)a.ec + i, a.vec >> S_EC & 1, ec);
        if (has_noise) ld8<TE>((const TE*)a.noise + i, a.vec >> S_NOISE & 1, nz);
        ld8<float>(a.x + i, a.vec >> S_X & 1, x);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j < a.n_hist) {
                ld8<float>(a.hist[j] + i, a.vec >> (S_H0 + j) & 1, h[j]);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) h[j][k] = 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float hk[3] = {h[0][k], h[1][k], h[2][k]};
            xn[k] = sampler_update(a.c, has_uncond, has_noise, a.n_hist, eu[k], has_uncond ? ec[k] : 0.f, x[k], hk,
                                   has_noise ? nz[k] : 0.f, m[k]);
            xi[k] = a.c.in_scale * xn[k];
        }
        st8<float>(a.x_out + i, a.vec >> S_XOUT & 1, xn);
        if (a.m_out) st8<float>(a.m_out + i, a.vec >> S_MOUT & 1, m);
        if (a.x_in[0]) st8<TI>((TI*)a.x_in[0] + i, a.vec >> S_IN0 & 1, xi);
        if (a.x_in[1]) st8<TI>((TI*)a.x_in[1] + i, a.vec >> S_IN1 & 1, xi);
    }
    // head and tail: at most 3 + 7 elements, one thread each
    if (tid < a.head) sampler_scalar<TE, TI>(a, tid);
    if (tid >= a.head && tail0 + (tid - a.head) < a.n && tid - a.head < SS_PER) sampler_scalar<TE, TI>(a, tail0 + (tid - a.head));
}

inline size_t esize(int dtype) { return dtype == FMC_BF16 ? 2 : 4; }

// ---- sliding windows: the blend of the windows' predictions and the step, one pass over the full latents ------------------------------
// x[B][C][Ftot][hw] fp32, Ftot = W (F - overlap) + overlap, window w = frames [w stride, w stride + F), stride = F - overlap.  Per
// element (b, c, f, s), with w_lo = max(0, ceil((f - F + 1) / stride)), w_hi = min(W - 1, floor(f / stride)), cnt = w_hi - w_lo + 1:
//
//   e_w = has_uncond ? eu_w + g (ec_w - eu_w) : e0_w          (window w's own frame f - w stride)
//   e   = (sum_{w = w_lo .. w_hi, ascending} e_w) / cnt
//   x'  = sampler_update(coef, x, e, hist, noise)             (the text above, entered with the blended e and no unconditional half)
//
// and x_in[r][w][b][c][f - w stride][s] = (model dtype)(in_scale x') for every covering window and r < in_reps.  The covering windows
// come from f alone: no mask tensor, no atomics.  eps and x_in are each ONE buffer addressed by (stride_r, stride_w) in elements.
//
// A pure HBM pass: per latent element, e_bytes (cnt (1 + has_uncond) + noise) + 4 (1 + n_hist) read and 4 (1 + m_out) +
// in_bytes in_reps cnt written, cnt averaging W F / Ftot over the clip (1.6 at 2 windows of 16 overlapping by 12, 2 at 3).
//
// Layout of the work: a row is the hw elements of one (b, c, f).  Each row has a scalar head that brings x to a 16-byte boundary (at
// most 3 elements), runs of 8, and a tail; one thread takes one of them per trip.  A full run moves every stream whose address is
// 16-byte aligned THERE as a vector and any other element by element (odd hw moves the alignment from row to row, per stream).
//
// Aliasing as above: a thread loads every window's eps, x, hist and noise before its first store; a latent element belongs to one
// thread, and an x_in element (r, w, f_local) to the one thread of f = w stride + f_local.
//
// Windows that do not overlap (W = 1 among them) run on sampler_step_kernel, one launch per contiguous block (the host entry
// below): such a block is the plain step, and only the same compiled kernel gives it the plain step's bits -- hipcc fuses a
// different product of `a x + b e` into the fma in the two kernels.
//
// Roundings on the longest chain (tests/window_common.py counts them): the three of each window's CFG combine, cnt - 1 adds of the
// sum, the division, then the chain above from `m_e *` on: 11 + cnt for x', 5 + cnt for m, 12 + cnt for x_in.
struct WindowArgs {
    const void* eps;
    const void* noise;       // NULL: none
    const float* x;
    const float* hist[3];
    float* x_out;
    float* m_out;            // NULL: not wanted
    void* x_in;              // NULL: not wanted
    int64_t eps_sr, eps_sw, in_sr, in_sw;
    int F, Ftot, W, stride, hw;
    int per_row;             // work items of one row: the head, the runs, the tail (some may be empty)
    unsigned items;
    int has_uncond, n_hist, in_reps;
    fmc_sampler_coef c;
};

// N consecutive elements of one row: a run of 8 (every stream that is 16-byte aligned THERE moves as a vector, any other element by
// element) or one element of a head or a tail
template <typename T, int N>
__device__ __forceinline__ void ldn(const T* p, float (&v)[N]) {
    if constexpr (N == 8) ld8<T>(p, (reinterpret_cast<uintptr_t>(p) & 15u) == 0, v);
    else v[0] = ld_one<T>(p);
}

template <typename T, int N>
__device__ __forceinline__ void stn(T* p, const float (&v)[N]) {
    if constexpr (N == 8) st8<T>(p, (reinterpret_cast<uintptr_t>(p) & 15u) == 0, v);
    else st_one<T>(p, v[0]);
}

// elements [s, s + N) of row (bc, f), covered by windows w_lo .. w_hi
template <typename TE, typename TI, int N>
__device__ __forceinline__ void window_elems(const WindowArgs& a, int bc, int f, int w_lo, int w_hi, int s) {
    const bool has_uncond = a.has_uncond != 0, has_noise = a.noise != nullptr;
    const int64_t i = ((int64_t)bc * a.Ftot + f) * a.hw + s;
    float e[N], eu[N], ec[N], nz[N], x[N], h[3][N], xn[N], m[N], xi[N];
    // The loads and, under one window, the update and the stores are in the order and the form of sampler_step_kernel's loop body:
    // hipcc's contraction into fma depends on where the operands of `m_x x + m_e e` are defined and on what the stores are fed by.
    // This brings an element under one window (the ends of a clip of overlapping windows) to within the last bits of that kernel's
    // result, not to its bits; windows that do not overlap at all never come here (fmc_window_step).
    const TE* p0 = (const TE*)a.eps + w_lo * a.eps_sw + ((int64_t)bc * a.F + (f - w_lo * a.stride)) * a.hw + s;
    ldn<TE, N>(p0, eu);
    if (has_uncond) ldn<TE, N>(p0 + a.eps_sr, ec);
    if (has_noise) ldn<TE, N>((const TE*)a.noise + i, nz);
    ldn<float, N>(a.x + i, x);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j < a.n_hist) {
            ldn<float, N>(a.hist[j] + i, h[j]);
        } else {
#pragma unroll
            for (int q = 0; q < N; ++q) h[j][q] = 0.f;
        }
    }
    if (w_lo == w_hi) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float hk[3] = {h[0][j], h[1][j], h[2][j]};
            xn[j] = sampler_update(a.c, has_uncond, has_noise, a.n_hist, eu[j], has_uncond ? ec[j] : 0.f, x[j], hk, has_noise ? nz[j] : 0.f, m[j]);
            xi[j] = a.c.in_scale * xn[j];
        }
        stn<float, N>(a.x_out + i, xn);
        if (a.m_out) stn<float, N>(a.m_out + i, m);
        TI* q = (TI*)a.x_in + w_lo * a.in_sw + ((int64_t)bc * a.F + (f - w_lo * a.stride)) * a.hw + s;
        if (a.in_reps > 0) stn<TI, N>(q, xi);
        if (a.in_reps > 1) stn<TI, N>(q + a.in_sr, xi);
        return;
    }
    {
#pragma unroll
        for (int j = 0; j < N; ++j) e[j] = has_uncond ? eu[j] + a.c.g * (ec[j] - eu[j]) : eu[j];
        for (int w = w_lo + 1; w <= w_hi; ++w) {
            const TE* p = (const TE*)a.eps + w * a.eps_sw + ((int64_t)bc * a.F + (f - w * a.stride)) * a.hw + s;
            ldn<TE, N>(p, eu);
            if (has_uncond) ldn<TE, N>(p + a.eps_sr, ec);
#pragma unroll
            for (int j = 0; j < N; ++j) e[j] += has_uncond ? eu[j] + a.c.g * (ec[j] - eu[j]) : eu[j];
        }
        const float d = (float)(w_hi - w_lo + 1);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float hk[3] = {h[0][j], h[1][j], h[2][j]};
            xn[j] = sampler_update(a.c, false, has_noise, a.n_hist, e[j] / d, 0.f, x[j], hk, has_noise ? nz[j] : 0.f, m[j]);
            xi[j] = a.c.in_scale * xn[j];
        }
    }
    stn<float, N>(a.x_out + i, xn);
    if (a.m_out) stn<float, N>(a.m_out + i, m);
    if (a.x_in) {
        for (int w = w_lo; w <= w_hi; ++w) {
            TI* p = (TI*)a.x_in + w * a.in_sw + ((int64_t)bc * a.F + (f - w * a.stride)) * a.hw + s;
            for (int r = 0; r < a.in_reps; ++r) stn<TI, N>(p + r * a.in_sr, xi);
        }
    }
}

template <typename TE, typename TI>
__global__ __launch_bounds__(SS_BLOCK) void window_step_kernel(const WindowArgs a) {
    const unsigned nthreads = gridDim.x * SS_BLOCK;
    for (unsigned it = blockIdx.x * SS_BLOCK + threadIdx.x; it < a.items; it += nthreads) {
        const unsigned row = it / (unsigned)a.per_row;
        const int k = (int)(it - row * (unsigned)a.per_row);
        const int bc = (int)(row / (unsigned)a.Ftot), f = (int)(row - (unsigned)bc * (unsigned)a.Ftot);
        const int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(a.x + (int64_t)row * a.hw) & 15u)) & 15u) >> 2);
        int s_lo = k == 0 ? 0 : head + (k - 1) * SS_PER;
        int s_hi = k == 0 ? head : s_lo + SS_PER;
        if (s_hi > a.hw) s_hi = a.hw;
        const int w_lo = f < a.F ? 0 : (f - a.F + a.stride) / a.stride;          // ceil((f - F + 1) / stride) for f >= F
        const int w_hi = min(a.W - 1, f / a.stride);
        if (s_hi - s_lo == SS_PER) {
            window_elems<TE, TI, SS_PER>(a, bc, f, w_lo, w_hi, s_lo);
        } else {                                                                 // a head or a tail: at most 7 elements
#pragma unroll 1
            for (int s = s_lo; s < s_hi; ++s) window_elems<TE, TI, 1>(a, bc, f, w_lo, w_hi, s);
        }
    }
}

}  // namespace

extern "C" int64_t fmc_sampler_step_elems_per_trip(void) { return (int64_t)SS_GRID_CAP * SS_BLOCK * SS_PER; }

static int launch_sampler_step(const void* eu, const void* ec, const void* noise, const float* x, const float* const hist[3], float* x_out,
                               float* m_out, void* x_in0, void* x_in1, int64_t n, int n_hist, fmc_sampler_coef coef, int dtype, bool in_bf,
                               void* stream);

extern "C" int fmc_sampler_step(const void* eps_uc, const float* x, const void* noise, const float* hist0, const float* hist1,
                                const float* hist2, float* x_out, float* m_out, void* x_in, int64_t n, int has_uncond, int n_hist,
                                int in_reps, fmc_sampler_coef coef, int dtype, int in_dtype, void* stream) {
    if (!eps_uc || !x || !x_out) FMC_FAIL(FMC_E_NULL, "sampler_step: NULL argument");
    if (n <= 0 || n_hist < 0 || n_hist > 3 || in_reps < 0 || in_reps > 2)
        FMC_FAIL(FMC_E_SHAPE, "sampler_step: bad n=%lld n_hist=%d in_reps=%d", (long long)n, n_hist, in_reps);
    const float* hist[3] = {hist0, hist1, hist2};
    for (int j = 0; j < n_hist; ++j)
        if (!hist[j]) FMC_FAIL(FMC_E_NULL, "sampler_step: hist[%d] is NULL with n_hist=%d", j, n_hist);
    if (in_reps > 0 && !x_in) FMC_FAIL(FMC_E_NULL, "sampler_step: x_in is NULL with in_reps=%d", in_reps);
    if (dtype != FMC_BF16 && dtype != FMC_F32) FMC_FAIL(FMC_E_DTYPE, "sampler_step: dtype %d", dtype);
    if (in_reps > 0 && in_dtype != FMC_BF16 && in_dtype != FMC_F32) FMC_FAIL(FMC_E_DTYPE, "sampler_step: in_dtype %d", in_dtype);
    const size_t es = esize(dtype), is = esize(in_dtype == FMC_BF16 ? FMC_BF16 : FMC_F32);
    return launch_sampler_step(eps_uc, has_uncond ? (const char*)eps_uc + (size_t)n * es : nullptr, noise, x, hist, x_out, m_out,
                               in_reps > 0 ? x_in : nullptr, in_reps > 1 ? (char*)x_in + (size_t)n * is : nullptr, n, n_hist, coef, dtype,
                               in_reps > 0 ? in_dtype == FMC_BF16 : dtype == FMC_BF16, stream);
}

// the launch of sampler_step_kernel on n elements; eu / ec: the two halves of the prediction (ec NULL: no unconditional half),
// x_in0 / x_in1: the copies of the next model input (NULL: not wanted).  Arguments are checked by the callers.
static int launch_sampler_step(const void* eu, const void* ec, const void* noise, const float* x, const float* const hist[3], float* x_out,
                               float* m_out, void* x_in0, void* x_in1, int64_t n, int n_hist, fmc_sampler_coef coef, int dtype, bool in_bf,
                               void* stream) {
    const size_t es = esize(dtype), is = in_bf ? 2 : 4;
    SamplerArgs a;
    a.eu = eu;
    a.ec = ec;
    a.noise = noise;
    a.x = x;
    for (int j = 0; j < 3; ++j) a.hist[j] = j < n_hist ? hist[j] : nullptr;
    a.x_out = x_out;
    a.m_out = m_out;
    a.x_in[0] = x_in0;
    a.x_in[1] = x_in1;
    a.n = n;
    a.n_hist = n_hist;
    a.c = coef;

    const void* ptr[S_COUNT] = {a.eu, a.ec, a.noise, a.x, a.hist[0], a.hist[1], a.hist[2], a.x_out, a.m_out, a.x_in[0], a.x_in[1]};
    const size_t size[S_COUNT] = {es, es, es, 4, 4, 4, 4, 4, 4, is, is};
    for (int s = 0; s < S_COUNT; ++s)
        if (ptr[s] && reinterpret_cast<uintptr_t>(ptr[s]) % size[s])
            FMC_FAIL(FMC_E_ALIGN, "sampler_step: stream %d is not aligned to its element size", s);
    int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) / 4;
    if (head > n) head = n;
    a.head = (int)head;
    a.vec = 0;
    for (int s = 0; s < S_COUNT; ++s)
        if (ptr[s] && (reinterpret_cast<uintptr_t>(ptr[s]) + (size_t)head * size[s]) % 16 == 0) a.vec |= 1u << s;

    int64_t blocks = ((n - head) / SS_PER + SS_BLOCK - 1) / SS_BLOCK;
    if (blocks > SS_GRID_CAP) blocks = SS_GRID_CAP;
    if (blocks < 1) blocks = 1;              // (head + tail <= 3 + 7 elements fit one workgroup)
    dim3 grid((unsigned)blocks), block(SS_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == FMC_BF16) {
        if (in_bf) hipLaunchKernelGGL((sampler_step_kernel<bf16_t, bf16_t>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((sampler_step_kernel<bf16_t, float>), grid, block, 0, st, a);
    } else {
        if (in_bf) hipLaunchKernelGGL((sampler_step_kernel<float, bf16_t>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((sampler_step_kernel<float, float>), grid, block, 0, st, a);
    }
    FMC_CHECK_LAUNCH("fmc_sampler_step");
    return 0;
}

extern "C" int fmc_window_step(const void* eps, int64_t eps_stride_r, int64_t eps_stride_w, const float* x, const void* noise,
                               const float* hist0, const float* hist1, const float* hist2, float* x_out, float* m_out, void* x_in,
                               int64_t in_stride_r, int64_t in_stride_w, int BC, int F, int stride, int W, int hw, int has_uncond,
                               int n_hist, int in_reps, fmc_sampler_coef coef, int dtype, int in_dtype, void* stream) {
    if (!eps || !x || !x_out) FMC_FAIL(FMC_E_NULL, "window_step: NULL argument");
    if (BC < 1 || hw < 1 || F < 1 || W < 1 || stride < 1 || stride > F || n_hist < 0 || n_hist > 3 || in_reps < 0 || in_reps > 2)
        FMC_FAIL(FMC_E_SHAPE, "window_step: bad BC=%d hw=%d F=%d stride=%d W=%d n_hist=%d in_reps=%d", BC, hw, F, stride, W, n_hist, in_reps);
    const float* hist[3] = {hist0, hist1, hist2};
    for (int j = 0; j < n_hist; ++j)
        if (!hist[j]) FMC_FAIL(FMC_E_NULL, "window_step: hist[%d] is NULL with n_hist=%d", j, n_hist);
    if (in_reps > 0 && !x_in) FMC_FAIL(FMC_E_NULL, "window_step: x_in is NULL with in_reps=%d", in_reps);
    if (dtype != FMC_BF16 && dtype != FMC_F32) FMC_FAIL(FMC_E_DTYPE, "window_step: dtype %d", dtype);
    if (in_reps > 0 && in_dtype != FMC_BF16 && in_dtype != FMC_F32) FMC_FAIL(FMC_E_DTYPE, "window_step: in_dtype %d", in_dtype);
    const size_t es = esize(dtype), is = esize(in_dtype == FMC_BF16 ? FMC_BF16 : FMC_F32);
    // element offsets are 64-bit in the kernel; rows and work items are counted in 32 bits
    const int64_t Ftot = (int64_t)(W - 1) * stride + F;
    const int per_row = (hw + SS_PER - 1) / SS_PER + 1;
    const int64_t rows = (int64_t)BC * Ftot, items = rows * per_row;
    if (Ftot >= (1ll << 31) || items >= (1ll << 31))
        FMC_FAIL(FMC_E_SHAPE, "window_step: %lld rows of %d elements are more than one launch indexes", (long long)rows, hw);
    // Windows that do not overlap (one window among them) have nothing to blend: every (b, c, window) block of F hw elements is
    // fmc_sampler_step's problem on contiguous memory, and its kernel runs it, one launch per block (one window: one launch, the
    // blocks follow each other).  Only the shared kernel gives such a block the plain step's bits: hipcc contracts the same update
    // differently in the two kernels, lane by lane.  The bits are those of the window run alone wherever the blocks keep the lanes
    // of the 8-element runs in place (F hw a multiple of 8 on 16-byte aligned buffers: every latent size in use).
    if (W == 1 || stride == F) {
        const int64_t blk = (int64_t)F * hw, n = W == 1 ? BC * blk : blk;
        const int nb = W == 1 ? 1 : BC;
        const bool in_bf = in_reps > 0 ? in_dtype == FMC_BF16 : dtype == FMC_BF16;
        for (int w = 0; w < W; ++w)
            for (int b = 0; b < nb; ++b) {
                const int64_t xo = ((int64_t)b * W + w) * blk, eo = w * eps_stride_w + b * blk, io = w * in_stride_w + b * blk;
                const float* hs[3] = {nullptr, nullptr, nullptr};
                for (int j = 0; j < n_hist; ++j) hs[j] = hist[j] + xo;
                const char* e0 = (const char*)eps + eo * (int64_t)es;
                char* i0 = in_reps > 0 ? (char*)x_in + io * (int64_t)is : nullptr;
                const int rc = launch_sampler_step(e0, has_uncond ? e0 + eps_stride_r * (int64_t)es : nullptr,
                                                   noise ? (const char*)noise + xo * (int64_t)es : nullptr, x + xo, hs, x_out + xo,
                                                   m_out ? m_out + xo : nullptr, i0, in_reps > 1 ? i0 + in_stride_r * (int64_t)is : nullptr, n,
                                                   n_hist, coef, dtype, in_bf, stream);
                if (rc) return rc;
            }
        return 0;
    }

    WindowArgs a;
    a.eps = eps;
    a.noise = noise;
    a.x = x;
    for (int j = 0; j < 3; ++j) a.hist[j] = j < n_hist ? hist[j] : nullptr;
    a.x_out = x_out;
    a.m_out = m_out;
    a.x_in = in_reps > 0 ? x_in : nullptr;
    a.eps_sr = eps_stride_r, a.eps_sw = eps_stride_w, a.in_sr = in_stride_r, a.in_sw = in_stride_w;
    a.F = F, a.Ftot = (int)Ftot, a.W = W, a.stride = stride, a.hw = hw;
    a.per_row = per_row;
    a.items = (unsigned)items;
    a.has_uncond = has_uncond ? 1 : 0, a.n_hist = n_hist, a.in_reps = in_reps;
    a.c = coef;

    const void* ptr[8] = {eps, noise, x, a.hist[0], a.hist[1], a.hist[2], x_out, m_out};
    const size_t size[8] = {es, es, 4, 4, 4, 4, 4, 4};
    for (int s = 0; s < 8; ++s)
        if (ptr[s] && reinterpret_cast<uintptr_t>(ptr[s]) % size[s])
            FMC_FAIL(FMC_E_ALIGN, "window_step: stream %d is not aligned to its element size", s);
    if (a.x_in && reinterpret_cast<uintptr_t>(x_in) % is) FMC_FAIL(FMC_E_ALIGN, "window_step: x_in is not aligned to its element size");

    int64_t blocks = (items + SS_BLOCK - 1) / SS_BLOCK;
    if (blocks > SS_GRID_CAP) blocks = SS_GRID_CAP;
    dim3 grid((unsigned)blocks), block(SS_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    const bool in_bf = in_reps > 0 ? in_dtype == FMC_BF16 : dtype == FMC_BF16;
    if (dtype == FMC_BF16) {
        if (in_bf) hipLaunchKernelGGL((window_step_kernel<bf16_t, bf16_t>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((window_step_kernel<bf16_t, float>), grid, block, 0, st, a);
    } else {
        if (in_bf) hipLaunchKernelGGL((window_step_kernel<float, bf16_t>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((window_step_kernel<float, float>), grid, block, 0, st, a);
    }
    FMC_CHECK_LAUNCH("fmc_window_step");
    return 0;
}

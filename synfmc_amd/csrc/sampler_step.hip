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

}  // namespace

extern "C" int64_t fmc_sampler_step_elems_per_trip(void) { return (int64_t)SS_GRID_CAP * SS_BLOCK * SS_PER; }

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

    SamplerArgs a;
    a.eu = eps_uc;
    a.ec = has_uncond ? (const char*)eps_uc + (size_t)n * es : nullptr;
    a.noise = noise;
    a.x = x;
    for (int j = 0; j < 3; ++j) a.hist[j] = j < n_hist ? hist[j] : nullptr;
    a.x_out = x_out;
    a.m_out = m_out;
    a.x_in[0] = in_reps > 0 ? x_in : nullptr;
    a.x_in[1] = in_reps > 1 ? (char*)x_in + (size_t)n * is : nullptr;
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
    const bool in_bf = in_reps > 0 ? in_dtype == FMC_BF16 : dtype == FMC_BF16;
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

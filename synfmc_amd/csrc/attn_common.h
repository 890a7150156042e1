// Fragment helpers shared by the spatial attention forward / backward kernels (gfx950, v_mfma_f32_32x32x16_bf16).
// Storage type T = bf16_t: one MFMA per product; T = float: split-bf16 x3 (hi*hi + hi*lo + lo*hi), the parity mode.
#pragma once
#include "common.h"
#include <initializer_list>
#include <type_traits>

namespace {

template <typename T> struct Frag;
template <> struct Frag<bf16_t> { bf16x8 hi; };
template <> struct Frag<float> { bf16x8 hi, lo; };

__device__ __forceinline__ bf16x8 zero_frag() {
    union { bf16x8 v; u32x4 u; } z;
    z.u = u32x4{0u, 0u, 0u, 0u};
    return z.v;
}

// 8 consecutive elements (global or LDS) -> MFMA fragment(s)
template <typename T> __device__ __forceinline__ void make_frag(const T* p, Frag<T>& f);
template <> __device__ __forceinline__ void make_frag<bf16_t>(const bf16_t* p, Frag<bf16_t>& f) {
    union { bf16x8 v; u32x4 u; } r;
    r.u = *reinterpret_cast<const u32x4*>(p);
    f.hi = r.v;
}
template <> __device__ __forceinline__ void make_frag<float>(const float* p, Frag<float>& f) {
    float v[8];
    Vec8<float>::load(p, v);
    split_bf16x8(v, f.hi, f.lo);
}
// two runs of 4 consecutive elements -> fragment
template <typename T> __device__ __forceinline__ void make_frag_2x4(const T* p0, const T* p1, Frag<T>& f);
template <> __device__ __forceinline__ void make_frag_2x4<bf16_t>(const bf16_t* p0, const bf16_t* p1, Frag<bf16_t>& f) {
    union { bf16x8 v; u32x2 u[2]; } r;
    r.u[0] = *reinterpret_cast<const u32x2*>(p0);
    r.u[1] = *reinterpret_cast<const u32x2*>(p1);
    f.hi = r.v;
}
template <> __device__ __forceinline__ void make_frag_2x4<float>(const float* p0, const float* p1, Frag<float>& f) {
    f32x4 a = *reinterpret_cast<const f32x4*>(p0);
    f32x4 b = *reinterpret_cast<const f32x4*>(p1);
    float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    split_bf16x8(v, f.hi, f.lo);
}
template <typename T> __device__ __forceinline__ void zero(Frag<T>& f);
template <> __device__ __forceinline__ void zero<bf16_t>(Frag<bf16_t>& f) { f.hi = zero_frag(); }
template <> __device__ __forceinline__ void zero<float>(Frag<float>& f) { f.hi = zero_frag(); f.lo = zero_frag(); }

// acc += A * B  (bf16: one MFMA; fp32 storage: hi*hi + hi*lo + lo*hi)
__device__ __forceinline__ void mma32(const Frag<bf16_t>& a, const Frag<bf16_t>& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.hi, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma32(const Frag<float>& a, const Frag<float>& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo, b.hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.lo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.hi, acc, 0, 0, 0);
}

// 8 probabilities (fp32) -> P^T fragment(s)
__device__ __forceinline__ void p_frag(const float (&p)[8], Frag<bf16_t>& f) {
    union { bf16x8 v; unsigned u[4]; } r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.u[i] = pack_bf2(p[2 * i], p[2 * i + 1]);
    f.hi = r.v;
}
__device__ __forceinline__ void p_frag(const float (&p)[8], Frag<float>& f) { split_bf16x8(p, f.hi, f.lo); }

template <typename T> __device__ __forceinline__ void store4(T* p, float a, float b, float c, float d);
template <> __device__ __forceinline__ void store4<bf16_t>(bf16_t* p, float a, float b, float c, float d) {
    *reinterpret_cast<u32x2*>(p) = u32x2{pack_bf2(a, b), pack_bf2(c, d)};
}
template <> __device__ __forceinline__ void store4<float>(float* p, float a, float b, float c, float d) {
    *reinterpret_cast<f32x4*>(p) = f32x4{a, b, c, d};
}

// NKS: number of 16-wide k-steps of the QK^T reduction (D padded to 16*NKS); NDT = ceil(NKS/2)
}  // namespace

// ---- host side, shared by spatial_attn.hip, spatial_attn_bwd.hip, temporal_attn.hip and attn_generic.hip ----------------------------------------
namespace {

// The argument checks of an attention entry point, in the one order all of them keep: required pointers, storage type, the entry's own shape check
// (`shape`: 0, or the FMC_FAIL it made), strides, 16-byte alignment.  The first failure sets "<prefix>: <text>" and is the return value.
struct AttnStrides {
    std::initializer_list<int64_t> values;
    int multiple;
    const char* text;
};
struct AttnArgs {
    const char* prefix;
    std::initializer_list<const void*> required;
    const char* null_text;
    bool typed;                                          // false: an entry point without a dtype argument
    int dtype;
    std::initializer_list<AttnStrides> strides;
    std::initializer_list<const void*> aligned;          // a NULL among them is an optional tensor left out; empty: the entry checks no alignment
};
template <class Shape>
int fmc_attn_check(const AttnArgs& a, Shape&& shape) {
    for (const void* p : a.required)
        if (!p) FMC_FAIL(FMC_E_NULL, "%s: %s", a.prefix, a.null_text);
    if (a.typed && a.dtype != FMC_BF16 && a.dtype != FMC_F32) FMC_FAIL(FMC_E_DTYPE, "%s: dtype %d", a.prefix, a.dtype);
    if (const int rc = shape()) return rc;
    for (const AttnStrides& s : a.strides)
        for (int64_t v : s.values)
            if (v % s.multiple) FMC_FAIL(FMC_E_ALIGN, "%s: %s", a.prefix, s.text);
    for (const void* p : a.aligned)
        if (p && !fmc_aligned16(p)) FMC_FAIL(FMC_E_ALIGN, "%s: tensors must be 16-byte aligned", a.prefix);
    return 0;
}

// `go(std::integral_constant<int, n>{})` for the one N that equals n; false when none does (the caller's refusal)
template <int... N, class Go>
bool fmc_pick(int n, Go&& go) {
    return ((n == N && (go(std::integral_constant<int, N>{}), true)) || ...);
}
// the 16-wide k-steps of a head width among the built ones, for the spatial forward and backward kernels
template <class Go>
bool fmc_pick_nks(int D, Go&& go) { return fmc_pick<1, 2, 3, 4, 5, 6, 8, 10>((D + 15) / 16, go); }

}  // namespace

// Gradient clipping + AdamW over many tensors, gfx950: the update of the training step (train_cam_obj_ctrl.py:917-943).
//
// Two passes over the caller's tables (include/fmc_hip.h: fmc_optim_tensor, fmc_optim_chunk):
//   pass 1  optim_norm_kernel      one workgroup per (tensor, chunk): the fp32 sum of g^2 of the chunk, a tree of depth 13 over the
//                                  squares (8 values per lane and iteration: 3 levels, 4 iterations: 2, the wave butterfly: 6, the four
//                                  waves: 2), written to partials[workgroup].  Tensors outside every clip group are not read.
//           optim_finalize_kernel  block c < n_clip_groups adds the partials of clip group c in a fixed order in fp64 and leaves the norm
//                                  and the coefficient min(1, max_norm / (norm + 1e-6)); the remaining blocks advance each tensor's step
//                                  counter and write its bias corrections (1 - beta1^t, sqrt(1 - beta2^t), computed in fp64, powers by
//                                  repeated squaring).  No atomics: the same tables and gradients give the same bits.
//   pass 2  optim_adamw_kernel     one workgroup per (tensor, chunk), 8 consecutive elements per lane and iteration: p, m, v through
//                                  16-byte aligned accesses, g through 16-byte accesses that are only 4-byte aligned (a gradient is a view
//                                  into a flat bucket; global_load / global_store_dwordx4 need dword alignment, not their size), the bf16
//                                  shadow as one 16-byte store of 8 values.  Only the last < 8 elements of a tensor take the scalar path.
// Per element 16 bytes are read and 12 - 22 written against ~40 VALU operations (two correctly rounded divisions and a square root):
// both passes are HBM bound.
#include "common.h"

#include <vector>

namespace {

constexpr int OPT_CHUNK = 8192;          // elements per workgroup: 256 lanes x 8 elements x 4 iterations
constexpr int OPT_THREADS = 256;
constexpr int OPT_ITERS = OPT_CHUNK / (OPT_THREADS * 8);
constexpr int OPT_FIN_THREADS = 1024;
constexpr int OPT_HYPER = 8;             // floats per hyper-parameter record

typedef float __attribute__((ext_vector_type(4), aligned(4))) f32x4_a4;     // 16 bytes at a 4-byte aligned address (gradient views)

// The tensors' pointers come out of a table in memory, so the compiler cannot know their address space and would emit flat_* accesses:
// say that they are global.
#define OPT_GLOBAL __attribute__((address_space(1)))
typedef OPT_GLOBAL float gf32;
typedef OPT_GLOBAL bf16_t gbf16;
__device__ __forceinline__ gf32* glob(float* p) { return (gf32*)p; }
__device__ __forceinline__ gbf16* glob(bf16_t* p) { return (gbf16*)p; }

__device__ __forceinline__ void load8(const gf32* p, float (&o)[8]) {
    const f32x4 a = *reinterpret_cast<const OPT_GLOBAL f32x4*>(p), b = *reinterpret_cast<const OPT_GLOBAL f32x4*>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[i] = a[i]; o[4 + i] = b[i]; }
}
__device__ __forceinline__ void store8(gf32* p, const float (&v)[8]) {
    *reinterpret_cast<OPT_GLOBAL f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<OPT_GLOBAL f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
}

static inline int64_t round4(int64_t n) { return (n + 3) / 4 * 4; }

// workspace layout in floats: norms | coefficients | bias corrections (2 per tensor) | per-chunk partial sums
struct OptWs { int64_t coef, bc, partials, total; };
static inline OptWs ws_layout(int n_tensors, int n_chunks, int n_clip_groups) {
    OptWs w;
    w.coef = round4(n_clip_groups);
    w.bc = w.coef + round4(n_clip_groups);
    w.partials = w.bc + round4(2 * (int64_t)n_tensors);
    w.total = w.partials + round4(n_chunks);
    return w;
}

__device__ __forceinline__ float sq_tree8(const float (&g)[8]) {
    return ((g[0] * g[0] + g[1] * g[1]) + (g[2] * g[2] + g[3] * g[3])) + ((g[4] * g[4] + g[5] * g[5]) + (g[6] * g[6] + g[7] * g[7]));
}

__device__ __forceinline__ void load_g8(const gf32* g, float (&o)[8]) {
    const f32x4_a4 a = *reinterpret_cast<const OPT_GLOBAL f32x4_a4*>(g), b = *reinterpret_cast<const OPT_GLOBAL f32x4_a4*>(g + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[i] = a[i]; o[4 + i] = b[i]; }
}

__global__ void __launch_bounds__(OPT_THREADS) optim_norm_kernel(const fmc_optim_tensor* __restrict__ T, const fmc_optim_chunk* __restrict__ C,
                                                                 float* __restrict__ partials) {
    __shared__ float red[OPT_THREADS / 64];
    const fmc_optim_chunk ck = C[blockIdx.x];
    const fmc_optim_tensor t = T[ck.tensor];
    if (t.clip_group < 0) {                               // uniform over the workgroup
        if (threadIdx.x == 0) partials[blockIdx.x] = 0.f;
        return;
    }
    const int64_t base = (int64_t)ck.chunk * OPT_CHUNK;
    const int64_t end = base + OPT_CHUNK < t.n ? base + OPT_CHUNK : t.n;
    const gf32* tg = glob(t.g);
    float acc[OPT_ITERS];
#pragma unroll
    for (int it = 0; it < OPT_ITERS; ++it) {
        const int64_t i = base + (int64_t)(it * OPT_THREADS + threadIdx.x) * 8;
        float g[8];
        if (i + 8 <= end) {
            load_g8(tg + i, g);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) g[k] = i + k < end ? tg[i + k] : 0.f;
        }
        acc[it] = sq_tree8(g);
    }
    static_assert(OPT_ITERS == 4, "the in-chunk sum is written as a tree over 4 iterations");
    float s = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ double powi(double b, long long e) {
    double r = 1.0;
    while (e > 0) {
        if (e & 1) r *= b;
        b *= b;
        e >>= 1;
    }
    return r;
}

__global__ void __launch_bounds__(OPT_FIN_THREADS) optim_finalize_kernel(const fmc_optim_tensor* __restrict__ T, int n_tensors,
                                                                         const fmc_optim_chunk* __restrict__ C, int n_chunks,
                                                                         const float* __restrict__ hyper, int n_clip_groups, float* __restrict__ ws,
                                                                         OptWs L) {
    __shared__ double red[OPT_FIN_THREADS];
    __shared__ int first[OPT_FIN_THREADS];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < n_clip_groups) {
        const int c = blockIdx.x;
        double s = 0.0;
        int f = 0x7fffffff;
        for (int j = tid; j < n_chunks; j += OPT_FIN_THREADS) {
            if (T[C[j].tensor].clip_group == c) {
                s += (double)ws[L.partials + j];
                if (j < f) f = j;
            }
        }
        red[tid] = s;
        first[tid] = f;
        __syncthreads();
        for (int o = OPT_FIN_THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) {
                red[tid] += red[tid + o];
                if (first[tid + o] < first[tid]) first[tid] = first[tid + o];
            }
            __syncthreads();
        }
        if (tid == 0) {
            const float norm = (float)sqrt(red[0]);
            float coef = 1.f;
            if (first[0] != 0x7fffffff) {                  // the group's max_grad_norm: the record of its first tensor in chunk order
                const float max_norm = hyper[OPT_HYPER * T[C[first[0]].tensor].hyper_group + 5];
                const float q = max_norm / (norm + 1e-6f);
                coef = q > 1.f ? 1.f : q;                  // a NaN stays a NaN, as under torch.clamp(max=1)
            }
            ws[c] = norm;
            ws[L.coef + c] = coef;
        }
        return;
    }
    const int i = ((int)blockIdx.x - n_clip_groups) * OPT_FIN_THREADS + tid;
    if (i >= n_tensors) return;
    const fmc_optim_tensor t = T[i];
    const float step = *t.step + 1.f;
    *t.step = step;
    const float* h = hyper + OPT_HYPER * t.hyper_group;
    const double b1 = 1.0 - (double)h[6], b2 = 1.0 - (double)h[7];
    const long long n = (long long)step;
    ws[L.bc + 2 * i] = (float)(1.0 - powi(b1, n));
    ws[L.bc + 2 * i + 1] = (float)sqrt(1.0 - powi(b2, n));
}

struct OptConsts { float coef, decay, b2, omb1, omb2, eps, step_size, bc2s; };

__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const OptConsts& k) {
    g *= k.coef;
    p *= k.decay;
    m = m + (g - m) * k.omb1;
    v = k.b2 * v + (k.omb2 * g) * g;
    const float denom = sqrtf(v) / k.bc2s + k.eps;
    p = p - k.step_size * (m / denom);
}

__global__ void __launch_bounds__(OPT_THREADS) optim_adamw_kernel(const fmc_optim_tensor* __restrict__ T, const fmc_optim_chunk* __restrict__ C,
                                                                  const float* __restrict__ hyper, const float* __restrict__ ws, OptWs L) {
    const fmc_optim_chunk ck = C[blockIdx.x];
    const fmc_optim_tensor t = T[ck.tensor];
    const float* h = hyper + OPT_HYPER * t.hyper_group;
    OptConsts k;
    const float lr = h[0];
    k.coef = t.clip_group >= 0 ? ws[L.coef + t.clip_group] : 1.f;
    k.decay = 1.f - lr * h[4];
    k.b2 = h[2];
    k.omb1 = h[6];
    k.omb2 = h[7];
    k.eps = h[3];
    k.step_size = lr / ws[L.bc + 2 * ck.tensor];
    k.bc2s = ws[L.bc + 2 * ck.tensor + 1];
    const bool zero = (t.flags & FMC_OPTIM_ZERO_GRAD) != 0;
    gf32 *tp = glob(t.p), *tg = glob(t.g), *tm = glob(t.m), *tv = glob(t.v), *sf = glob(t.shadow_f32);
    gbf16* sb = glob(t.shadow_bf16);
    const int64_t base = (int64_t)ck.chunk * OPT_CHUNK;
    const int64_t end = base + OPT_CHUNK < t.n ? base + OPT_CHUNK : t.n;
#pragma unroll 2
    for (int it = 0; it < OPT_ITERS; ++it) {
        const int64_t i = base + (int64_t)(it * OPT_THREADS + threadIdx.x) * 8;
        if (i >= end) break;
        if (i + 8 <= end) {
            float p[8], g[8], m[8], v[8];
            load8(tp + i, p);
            load_g8(tg + i, g);
            load8(tm + i, m);
            load8(tv + i, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) adamw1(p[e], g[e], m[e], v[e], k);
            store8(tp + i, p);
            store8(tm + i, m);
            store8(tv + i, v);
            u32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = pack_bf2(p[2 * e], p[2 * e + 1]);
            if (sb) *reinterpret_cast<OPT_GLOBAL u32x4*>(sb + i) = r;
            if (sf) {
                float w[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    w[2 * e] = __uint_as_float(r[e] << 16);
                    w[2 * e + 1] = __uint_as_float(r[e] & 0xffff0000u);
                }
                store8(sf + i, w);
            }
            if (zero) {
                const f32x4_a4 z = {0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<OPT_GLOBAL f32x4_a4*>(tg + i) = z;
                *reinterpret_cast<OPT_GLOBAL f32x4_a4*>(tg + i + 4) = z;
            }
        } else {
            for (int64_t j = i; j < end; ++j) {          // the last < 8 elements of the tensor
                float p = tp[j], m = tm[j], v = tv[j];
                adamw1(p, tg[j], m, v, k);
                tp[j] = p;
                tm[j] = m;
                tv[j] = v;
                const bf16_t b = f2bf(p);
                if (sb) sb[j] = b;
                if (sf) sf[j] = bf2f(b);
                if (zero) tg[j] = 0.f;
            }
        }
    }
}

int check_launch_args(const char* what, const fmc_optim_tensor* tensors, int n_tensors, const fmc_optim_chunk* chunks, int n_chunks,
                      const float* hyper, int n_hyper, int n_clip_groups, void* workspace, int64_t workspace_bytes) {
    if (!tensors || !chunks || !hyper || !workspace) FMC_FAIL(FMC_E_NULL, "%s: NULL table, hyper-parameter record or workspace", what);
    if (n_tensors < 1 || n_chunks < n_tensors || n_hyper < 1 || n_clip_groups < 0)
        FMC_FAIL(FMC_E_SHAPE, "%s: needs n_tensors >= 1, n_chunks >= n_tensors, n_hyper >= 1, n_clip_groups >= 0 (got %d, %d, %d, %d)", what,
                 n_tensors, n_chunks, n_hyper, n_clip_groups);
    const int64_t need = ws_layout(n_tensors, n_chunks, n_clip_groups).total * 4;
    if (workspace_bytes < need) FMC_FAIL(FMC_E_SHAPE, "%s: workspace of %lld bytes, need %lld", what, (long long)workspace_bytes, (long long)need);
    if (!fmc_aligned16(workspace) || (reinterpret_cast<uintptr_t>(tensors) & 7u) || (reinterpret_cast<uintptr_t>(chunks) & 7u) ||
        (reinterpret_cast<uintptr_t>(hyper) & 3u))
        FMC_FAIL(FMC_E_ALIGN, "%s: the workspace must be 16-byte aligned, the tables 8-byte, the hyper-parameter records 4-byte", what);
    return 0;
}

}  // namespace

extern "C" int fmc_optim_chunk_elems(void) { return OPT_CHUNK; }

extern "C" int64_t fmc_optim_workspace_bytes(int n_tensors, int n_chunks, int n_clip_groups) {
    if (n_tensors < 1 || n_chunks < n_tensors || n_clip_groups < 0) {
        fmc_set_error("optim_workspace_bytes: needs n_tensors >= 1, n_chunks >= n_tensors, n_clip_groups >= 0 (got %d, %d, %d)", n_tensors, n_chunks,
                      n_clip_groups);
        return -1;
    }
    return ws_layout(n_tensors, n_chunks, n_clip_groups).total * 4;
}

extern "C" int fmc_optim_check_tables(const fmc_optim_tensor* h_tensors, int n_tensors, const fmc_optim_chunk* h_chunks, int n_chunks, int n_hyper,
                                      int n_clip_groups) {
    if (!h_tensors || !h_chunks) FMC_FAIL(FMC_E_NULL, "optim_check_tables: NULL table");
    if (n_tensors < 1 || n_chunks < n_tensors || n_hyper < 1 || n_clip_groups < 0)
        FMC_FAIL(FMC_E_SHAPE, "optim_check_tables: needs n_tensors >= 1, n_chunks >= n_tensors, n_hyper >= 1, n_clip_groups >= 0 (got %d, %d, %d, %d)",
                 n_tensors, n_chunks, n_hyper, n_clip_groups);
    std::vector<int64_t> begin(n_tensors + 1, 0);
    for (int i = 0; i < n_tensors; ++i) {
        const fmc_optim_tensor& t = h_tensors[i];
        if (!t.p || !t.g || !t.m || !t.v || !t.step) FMC_FAIL(FMC_E_NULL, "optim_check_tables: NULL p / g / m / v / step in tensor %d", i);
        if (t.n < 1) FMC_FAIL(FMC_E_SHAPE, "optim_check_tables: tensor %d has %lld elements", i, (long long)t.n);
        if (t.clip_group < -1 || t.clip_group >= n_clip_groups || t.hyper_group < 0 || t.hyper_group >= n_hyper)
            FMC_FAIL(FMC_E_SHAPE, "optim_check_tables: tensor %d names clip group %d of %d, hyper-parameter group %d of %d", i, t.clip_group,
                     n_clip_groups, t.hyper_group, n_hyper);
        if (!fmc_aligned16(t.p) || !fmc_aligned16(t.m) || !fmc_aligned16(t.v) || (t.shadow_bf16 && !fmc_aligned16(t.shadow_bf16)) ||
            (t.shadow_f32 && !fmc_aligned16(t.shadow_f32)))
            FMC_FAIL(FMC_E_ALIGN, "optim_check_tables: p, m, v and the shadows of tensor %d must be 16-byte aligned (g: 4-byte)", i);
        if ((reinterpret_cast<uintptr_t>(t.g) & 3u) || (reinterpret_cast<uintptr_t>(t.step) & 3u))
            FMC_FAIL(FMC_E_ALIGN, "optim_check_tables: g and step of tensor %d must be 4-byte aligned", i);
        begin[i + 1] = begin[i] + (t.n + OPT_CHUNK - 1) / OPT_CHUNK;
    }
    if (begin[n_tensors] != n_chunks)
        FMC_FAIL(FMC_E_SHAPE, "optim_check_tables: the tensors need %lld chunks of %d elements, the map has %d", (long long)begin[n_tensors], OPT_CHUNK,
                 n_chunks);
    std::vector<unsigned char> seen(n_chunks, 0);
    for (int j = 0; j < n_chunks; ++j) {
        const fmc_optim_chunk& c = h_chunks[j];
        if (c.tensor < 0 || c.tensor >= n_tensors || c.chunk < 0 || c.chunk >= begin[c.tensor + 1] - begin[c.tensor])
            FMC_FAIL(FMC_E_SHAPE, "optim_check_tables: map entry %d names chunk %d of tensor %d, which does not exist", j, c.chunk, c.tensor);
        unsigned char& s = seen[begin[c.tensor] + c.chunk];
        if (s) FMC_FAIL(FMC_E_SHAPE, "optim_check_tables: chunk %d of tensor %d is mapped twice (entry %d)", c.chunk, c.tensor, j);
        s = 1;
    }
    return 0;                                              // n_chunks entries, all distinct, all valid: every chunk is covered once
}

extern "C" int fmc_optim_grad_norm(const fmc_optim_tensor* tensors, int n_tensors, const fmc_optim_chunk* chunks, int n_chunks, const float* hyper,
                                   int n_hyper, int n_clip_groups, void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = check_launch_args("optim_grad_norm", tensors, n_tensors, chunks, n_chunks, hyper, n_hyper, n_clip_groups, workspace, workspace_bytes))
        return rc;
    const OptWs L = ws_layout(n_tensors, n_chunks, n_clip_groups);
    float* ws = reinterpret_cast<float*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    if (n_clip_groups > 0) {
        hipLaunchKernelGGL(optim_norm_kernel, dim3((unsigned)n_chunks), dim3(OPT_THREADS), 0, st, tensors, chunks, ws + L.partials);
        FMC_CHECK_LAUNCH("fmc_optim_grad_norm");
    }
    const unsigned blocks = (unsigned)n_clip_groups + (unsigned)((n_tensors + OPT_FIN_THREADS - 1) / OPT_FIN_THREADS);
    hipLaunchKernelGGL(optim_finalize_kernel, dim3(blocks), dim3(OPT_FIN_THREADS), 0, st, tensors, n_tensors, chunks, n_chunks, hyper, n_clip_groups, ws,
                       L);
    FMC_CHECK_LAUNCH("fmc_optim_grad_norm (finalize)");
    return 0;
}

extern "C" int fmc_optim_adamw_step(const fmc_optim_tensor* tensors, int n_tensors, const fmc_optim_chunk* chunks, int n_chunks, const float* hyper,
                                    int n_hyper, int n_clip_groups, void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = check_launch_args("optim_adamw_step", tensors, n_tensors, chunks, n_chunks, hyper, n_hyper, n_clip_groups, workspace, workspace_bytes))
        return rc;
    const OptWs L = ws_layout(n_tensors, n_chunks, n_clip_groups);
    hipLaunchKernelGGL(optim_adamw_kernel, dim3((unsigned)n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, tensors, chunks, hyper,
                       reinterpret_cast<const float*>(workspace), L);
    FMC_CHECK_LAUNCH("fmc_optim_adamw_step");
    return 0;
}

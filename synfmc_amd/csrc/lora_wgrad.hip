// Weight gradient of a token matrix, gfx950: out[N][K] (fp32) = alpha * sum_m A[m][n] * B[m][k]  (+ out).
//
// The LoRA factors of the spatial attention train on it (hip_ops.lora_linear): dU = s dY^T P and dD = s Q^T X, a reduction over the
// tens of thousands of tokens of a stage-1 batch with both operands row-major [tokens][features] -- often column slices of the fused
// [M, 3C] q | k | v tensors.  The projection GEMM (gemm_conv.hip) wants its reduction index contiguous in memory; here it is the row
// index of both operands, so the tiles are staged row-major into LDS (coalesced 16-byte loads) and the MFMA fragments come out of
// ds_read_b64_tr_b16: inside a 16-lane group lane 4q+p supplies the address of token row q, columns 4p..4p+3 of a [4 tokens][16 columns]
// block and receives column (lane & 15) of it, i.e. 4 consecutive tokens of one feature -- half of a v_mfma_f32_32x32x16_bf16 operand.
//
// Workgroup = 4 waves = one 64 (n) x 64 (k) output tile; a slab of 128 tokens is staged per step and wave w reduces tokens 32w..32w+31 of
// it into the whole tile (2 x 2 accumulators: every fragment read feeds two MFMAs).  The four partial tiles are summed through LDS in
// wave order at the end.  Tokens past the end of the workgroup's range and columns past N / K are ZERO in LDS (the transposed read needs
// EXEC all ones: pad, don't mask).  Long reductions are split over `splits` workgroups per tile (a function of the problem's shape
// only): each writes an fp32 partial into the caller's workspace, and a second kernel sums them in split order -- the result is
// bit-reproducible, and a problem gives the same bits alone or in a group.
#include "wgrad_common.h"

namespace {

constexpr int WG_MAXP = 8;               // problems per launch

struct WgProblem {
    const bf16_t* a; const bf16_t* b; float* out; float* ws;  // ws: this problem's [splits][N][K] partials (splits > 1)
    int64_t M, lda, ldb, ldo;
    int N, K, tiles_n, tiles_k, splits, chunk_slabs, wg_begin, red_begin;   // red_begin: first float4 of the reduction grid
    float alpha; int accumulate;
};
struct WgParams {
    WgProblem p[WG_MAXP];
    int n;
};

__device__ __forceinline__ void load_slab(const bf16_t* __restrict__ src, int64_t ld, int64_t m0, int64_t m_end, int c0, int ncols,
                                          u32x4 (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = threadIdx.x + 256 * i, row = e >> 3, c = c0 + 8 * (e & 7);
        const int64_t m = m0 + row;
        r[i] = (m < m_end && c < ncols) ? *reinterpret_cast<const u32x4*>(src + m * ld + c) : u32x4{0u, 0u, 0u, 0u};
    }
}

__global__ void __launch_bounds__(256) wgrad_kernel(const WgParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* sa = reinterpret_cast<bf16_t*>(smem);
    bf16_t* sb = sa + WG_BT * WG_PITCH;
    float* red = reinterpret_cast<float*>(smem);

    int pi = 0;
    for (int j = 1; j < P.n; ++j)
        if ((int)blockIdx.x >= P.p[j].wg_begin) pi = j;
    const WgProblem& pr = P.p[pi];
    const int local = (int)blockIdx.x - pr.wg_begin;
    const int tk = local % pr.tiles_k, tn = (local / pr.tiles_k) % pr.tiles_n, split = local / (pr.tiles_k * pr.tiles_n);
    const int n0 = tn * WG_BN, k0 = tk * WG_BK;
    const int64_t m_begin = (int64_t)split * pr.chunk_slabs * WG_BT;
    const int64_t m_end = m_begin + (int64_t)pr.chunk_slabs * WG_BT < pr.M ? m_begin + (int64_t)pr.chunk_slabs * WG_BT : pr.M;
    const int nslabs = (int)((m_end - m_begin + WG_BT - 1) / WG_BT);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    u32x4 ra[4], rb[4];
    load_slab(pr.a + n0, pr.lda, m_begin, m_end, 0, pr.N - n0, ra);
    load_slab(pr.b + k0, pr.ldb, m_begin, m_end, 0, pr.K - k0, rb);
    for (int s = 0; s < nslabs; ++s) {
        store_slab(sa, ra);
        store_slab(sb, rb);
        __syncthreads();
        if (s + 1 < nslabs) {                         // next slab into registers under this slab's MFMAs
            const int64_t m1 = m_begin + (int64_t)(s + 1) * WG_BT;
            load_slab(pr.a + n0, pr.lda, m1, m_end, 0, pr.N - n0, ra);
            load_slab(pr.b + k0, pr.ldb, m1, m_end, 0, pr.K - k0, rb);
        }
        slab_mfma(sa, sb, wave, lane, acc);
        __syncthreads();
    }

    spill_tiles(red, wave, lane, acc);      // [wave][i * 2 + j][reg][lane], summed in wave order below
    __syncthreads();
    const bool direct = pr.splits == 1;
    float* dst = direct ? pr.out : pr.ws + (int64_t)split * pr.N * pr.K;
    const int64_t ld = direct ? pr.ldo : pr.K;
#pragma unroll 4
    for (int x = 0; x < 16; ++x) {
        const int e = threadIdx.x + 256 * x;
        const int l = e & 63, reg = (e >> 6) & 15, ij = e >> 10;
        const int n = n0 + 32 * (ij >> 1) + (reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5);
        const int k = k0 + 32 * (ij & 1) + (l & 31);
        if (n >= pr.N || k >= pr.K) continue;
        const float v = ((red[e] + red[4096 + e]) + red[2 * 4096 + e]) + red[3 * 4096 + e];
        float* o = dst + (int64_t)n * ld + k;
        if (!direct) *o = v;
        else *o = pr.accumulate ? __fmaf_rn(pr.alpha, v, *o) : pr.alpha * v;
    }
}

// out = alpha * sum_s ws[s] (+ out), 4 consecutive columns per thread, the splits summed in order
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const WgParams P) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    int pi = -1;
    for (int j = 0; j < P.n; ++j)
        if (P.p[j].splits > 1 && idx >= P.p[j].red_begin) pi = j;
    if (pi < 0) return;
    const WgProblem& pr = P.p[pi];
    const int64_t e4 = idx - pr.red_begin, nk = (int64_t)pr.N * pr.K;
    if (e4 * 4 >= nk) return;
    const float4* w = reinterpret_cast<const float4*>(pr.ws) + e4;
    float4 s = w[0];
    for (int i = 1; i < pr.splits; ++i) {
        const float4 v = w[i * (nk / 4)];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const int64_t n = (e4 * 4) / pr.K, k = (e4 * 4) % pr.K;
    float4* o = reinterpret_cast<float4*>(pr.out + n * pr.ldo + k);
    if (pr.accumulate) {
        const float4 old = *o;
        *o = float4{__fmaf_rn(pr.alpha, s.x, old.x), __fmaf_rn(pr.alpha, s.y, old.y), __fmaf_rn(pr.alpha, s.z, old.z), __fmaf_rn(pr.alpha, s.w, old.w)};
    } else {
        *o = float4{pr.alpha * s.x, pr.alpha * s.y, pr.alpha * s.z, pr.alpha * s.w};
    }
}

// splits / tokens per split of one problem: a function of (M, N, K) alone
void plan(int64_t M, int N, int K, int& tiles_n, int& tiles_k, int& splits, int& chunk_slabs) {
    tiles_n = (N + WG_BN - 1) / WG_BN;
    tiles_k = (K + WG_BK - 1) / WG_BK;
    wg_split_plan(M, (int64_t)tiles_n * tiles_k, splits, chunk_slabs);
}

int check(const fmc_wgrad_problem* problems, int n) {
    if (!problems) FMC_FAIL(FMC_E_NULL, "linear_wgrad_bf16: NULL problem list");
    if (n < 1 || n > WG_MAXP) FMC_FAIL(FMC_E_SHAPE, "linear_wgrad_bf16: 1..%d problems per launch (got %d)", WG_MAXP, n);
    for (int i = 0; i < n; ++i) {
        const fmc_wgrad_problem& q = problems[i];
        if (!q.a || !q.b || !q.out) FMC_FAIL(FMC_E_NULL, "linear_wgrad_bf16: NULL tensor in problem %d", i);
        if (q.M < 1 || q.N < 16 || q.K < 16 || q.N % 16 || q.K % 16 || q.lda < q.N || q.ldb < q.K || q.ldo < q.K)
            FMC_FAIL(FMC_E_SHAPE, "linear_wgrad_bf16: problem %d needs M >= 1, N %% 16 == K %% 16 == 0, lda >= N, ldb >= K, ldo >= K "
                                  "(M=%lld N=%d K=%d lda=%lld ldb=%lld ldo=%lld)", i, (long long)q.M, q.N, q.K, (long long)q.lda,
                     (long long)q.ldb, (long long)q.ldo);
        if (q.lda % 8 || q.ldb % 8 || q.ldo % 4 || !fmc_aligned16(q.a) || !fmc_aligned16(q.b) || !fmc_aligned16(q.out))
            FMC_FAIL(FMC_E_ALIGN, "linear_wgrad_bf16: problem %d needs 16-byte aligned pointers, lda %% 8 == ldb %% 8 == 0, ldo %% 4 == 0", i);
    }
    return 0;
}

int64_t workspace_bytes(const fmc_wgrad_problem* problems, int n) {
    int64_t bytes = 0;
    for (int i = 0; i < n; ++i) {
        int tn, tk, s, cs;
        plan(problems[i].M, problems[i].N, problems[i].K, tn, tk, s, cs);
        if (s > 1) bytes += (int64_t)s * problems[i].N * problems[i].K * 4;
    }
    return bytes;
}

}  // namespace

extern "C" int64_t fmc_linear_wgrad_workspace_bytes(const fmc_wgrad_problem* problems, int n_problems) {
    if (check(problems, n_problems)) return -1;
    return workspace_bytes(problems, n_problems);
}

extern "C" int fmc_linear_wgrad_bf16(const fmc_wgrad_problem* problems, int n_problems, void* workspace, int64_t ws_bytes, void* stream) {
    if (int rc = check(problems, n_problems)) return rc;
    const int64_t need = workspace_bytes(problems, n_problems);
    if (need > 0 && !workspace) FMC_FAIL(FMC_E_NULL, "linear_wgrad_bf16: the split reduction needs a workspace of %lld bytes", (long long)need);
    if (need > ws_bytes) FMC_FAIL(FMC_E_SHAPE, "linear_wgrad_bf16: workspace of %lld bytes, need %lld", (long long)ws_bytes, (long long)need);
    if (need > 0 && !fmc_aligned16(workspace)) FMC_FAIL(FMC_E_ALIGN, "linear_wgrad_bf16: workspace must be 16-byte aligned");
    WgParams P{};
    P.n = n_problems;
    int64_t wgs = 0, red = 0, ws_off = 0;
    for (int i = 0; i < n_problems; ++i) {
        const fmc_wgrad_problem& q = problems[i];
        WgProblem& d = P.p[i];
        d.a = (const bf16_t*)q.a; d.b = (const bf16_t*)q.b; d.out = q.out;
        d.M = q.M; d.lda = q.lda; d.ldb = q.ldb; d.ldo = q.ldo; d.N = q.N; d.K = q.K;
        d.alpha = q.alpha; d.accumulate = q.accumulate != 0;
        plan(q.M, q.N, q.K, d.tiles_n, d.tiles_k, d.splits, d.chunk_slabs);
        d.ws = d.splits > 1 ? reinterpret_cast<float*>(workspace) + ws_off : nullptr;
        if (d.splits > 1) ws_off += (int64_t)d.splits * q.N * q.K;
        d.wg_begin = (int)wgs;
        wgs += (int64_t)d.tiles_n * d.tiles_k * d.splits;
        d.red_begin = (int)red;
        if (d.splits > 1) red += ((int64_t)q.N * q.K / 4 + 255) / 256 * 256;
    }
    if (wgs >= ((int64_t)1 << 31) || red >= ((int64_t)1 << 31)) FMC_FAIL(FMC_E_SHAPE, "linear_wgrad_bf16: launch too large");
    hipStream_t st = (hipStream_t)stream;
    fmc_launch<wgrad_kernel>(dim3((unsigned)wgs), dim3(256), WG_LDS, st, P);
    FMC_CHECK_LAUNCH("fmc_linear_wgrad_bf16");
    if (red > 0) {
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)(red / 256)), dim3(256), 0, st, P);
        FMC_CHECK_LAUNCH("fmc_linear_wgrad_bf16 (reduce)");
    }
    return 0;
}

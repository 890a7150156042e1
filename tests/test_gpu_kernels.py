"""Parity of every hand-written HIP kernel (through the C ABI) against the CPU oracle on seeded inputs.

Tolerances (rel-inf = max|a-b| / max|b|):
  * FMC_F32 storage (parity mode): 1e-5 for HBM-bound passes, 2e-5 for the split-bf16 attention kernels
    (the north-star asks for 1e-3 end to end);
  * FMC_BF16 storage: the kernel is compared with the oracle evaluated on the SAME bf16-rounded inputs, so the
    difference is the bf16 rounding of the output (2^-8 relative per element) plus, for attention, the bf16
    rounding of the probabilities: 1e-2.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conditioning as OC
from oracle import diffusers_restated as OD
from tests.conv_fwd_common import assert_bf16_close, assert_f32_close      # (the element-wise bounds; other test files import them from here)

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 1e-2}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def rel_inf(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rnd(shape, seed, dtype, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * scale + shift
    return x.to(dtype).float(), x.to(dtype).cuda()          # (oracle input = rounded values in fp32, device input)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,HW,C,act", [(2, 40, 320, True), (3, 160, 640, False), (2, 9, 1280, True),
                                        (1, 640, 960, True), (2, 7, 2560, True), (2, 33, 64, False),
                                        (2, 2560, 320, True), (1, 2560, 640, False), (2, 2499, 320, True),
                                        (1, 2560, 960, True), (1, 4096, 320, True),
                                        (1, 1024, 64, True), (1, 256, 128, False), (3, 1024, 64, True)])   # one image, single-pass kernel (the VAE decodes frame by frame)
def test_groupnorm_silu(K, dtype, N, HW, C, act):
    xo, xd = rnd((N, HW, C), 1, dtype, scale=1.5, shift=0.7)
    g = torch.Generator().manual_seed(2)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    eps = 1e-5
    ref = F.group_norm(xo.permute(0, 2, 1), 32, gamma, beta, eps)          # nn.GroupNorm on [N, C, HW]
    ref = (F.silu(ref) if act else ref).permute(0, 2, 1)
    y = K.groupnorm_silu(xd, gamma.cuda(), beta.cuda(), 32, eps, act)
    assert rel_inf(y.float(), ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_groupnorm_silu_backward(K, dtype):
    N, HW, C = 2, 48, 320
    xo, xd = rnd((N, HW, C), 3, dtype, scale=1.2, shift=-0.3)
    do, dd = rnd((N, HW, C), 4, dtype)
    g = torch.Generator().manual_seed(5)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    for act in (False, True):
        xr = xo.clone().requires_grad_(True)
        ref = F.group_norm(xr.permute(0, 2, 1), 32, gamma, beta, 1e-5)
        ref = (F.silu(ref) if act else ref).permute(0, 2, 1)
        ref.backward(do)
        xg = xd.clone().requires_grad_(True)
        y = K.groupnorm_silu(xg, gamma.cuda(), beta.cuda(), 32, 1e-5, act)
        y.backward(dd)
        assert rel_inf(xg.grad.float(), xr.grad) < (1e-4 if dtype == torch.float32 else 2e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [64, 320, 640, 1280])
def test_layernorm_and_pe(K, dtype, C):
    B, Fr, P = 2, 16, 5
    xo, xd = rnd((B, Fr, P, C), 6, dtype, scale=2.0, shift=0.5)
    g = torch.Generator().manual_seed(7)
    gamma, beta, pe = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(32, C, generator=g)
    ref = F.layer_norm(xo, (C,), gamma, beta, 1e-5)
    y = K.layernorm(xd, gamma.cuda(), beta.cuda(), 1e-5)
    assert rel_inf(y.float(), ref) < TOL[dtype]
    ref_pe = ref + pe[:Fr][None, :, None, :]                                  # native [B,F,P,C]: frame = dim 1
    y = K.layernorm(xd, gamma.cuda(), beta.cuda(), 1e-5, pe.cuda(), P, Fr)
    assert rel_inf(y.float(), ref_pe) < TOL[dtype]
    x3 = xd.permute(0, 2, 1, 3).reshape(B * P, Fr, C).contiguous()            # reference (b h w) f c layout
    ref3 = F.layer_norm(x3.float().cpu(), (C,), gamma, beta, 1e-5) + pe[:Fr][None]
    y3 = K.layernorm(x3, gamma.cuda(), beta.cuda(), 1e-5, pe.cuda(), 1, Fr)
    assert rel_inf(y3.float(), ref3) < TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_geglu(K, dtype):
    xo, xd = rnd((3, 50, 2 * 1280), 8, dtype, scale=2.0)
    a, gte = xo.chunk(2, dim=-1)
    ref = a * F.gelu(gte)
    assert rel_inf(K.geglu(xd).float(), ref) < TOL[dtype]


# ---------------------------------------------------------------------------------------------
def oracle_attention(q, k, v, heads):
    """The oracle's un-fused chain (diffusers Attention helpers: head_to_batch_dim, baddbmm+softmax, bmm)."""
    C = q.shape[-1]
    attn = OD.Attention(query_dim=C, heads=heads, dim_head=C // heads)
    qh, kh, vh = attn.head_to_batch_dim(q), attn.head_to_batch_dim(k), attn.head_to_batch_dim(v)
    return attn.batch_to_head_dim(torch.bmm(attn.get_attention_scores(qh, kh), vh))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,Skv,H,D", [(2, 160, 160, 8, 40), (2, 200, 200, 8, 80), (1, 130, 130, 8, 160),
                                         (2, 40, 40, 8, 160), (3, 300, 77, 8, 40), (2, 64, 77, 8, 160),
                                         (2, 257, 257, 4, 8), (1, 2560, 2560, 8, 40), (2, 96, 96, 2, 64),
                                         # the whole-K/V kernel of the inner levels (d = 160, S_kv <= 160): several query blocks, ragged key counts
                                         (2, 200, 77, 8, 160), (1, 330, 100, 8, 160), (3, 160, 160, 8, 160), (2, 33, 1, 8, 160),
                                         # the big-tile kernel of the 20x32 level (d = 80, S_kv % 32 == 0): two tiles, a partial last tile, ragged query blocks
                                         (2, 640, 640, 8, 80), (1, 384, 384, 8, 80), (2, 500, 352, 8, 80), (1, 170, 256, 4, 80), (1, 1280, 960, 2, 80)])
def test_spatial_attention(K, dtype, B, S, Skv, H, D):
    C = H * D
    qo, qd = rnd((B, S, C), 10, dtype)
    ko, kd = rnd((B, Skv, C), 11, dtype)
    vo, vd = rnd((B, Skv, C), 12, dtype)
    ref = oracle_attention(qo, ko, vo, H)
    out, lse = K.spatial_attention(qd, kd, vd, H, return_lse=True)
    assert rel_inf(out.float(), ref) < TOL[dtype]
    # log-sum-exp of the scaled scores
    qh = qo.view(B, S, H, D).permute(0, 2, 1, 3)
    kh = ko.view(B, Skv, H, D).permute(0, 2, 1, 3)
    lse_ref = torch.logsumexp(qh @ kh.transpose(-1, -2) * D ** -0.5, dim=-1)
    assert (lse.cpu() - lse_ref).abs().max() < (1e-4 if dtype == torch.float32 else 2e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_spatial_attention_fused_qkv_views_and_shared_text(K, dtype):
    """q/k/v as strided slices of one fused projection; text K/V shared by the F frames of a clip."""
    B, Fr, S, H, D = 2, 4, 96, 8, 40
    C = H * D
    qkvo, qkvd = rnd((B * Fr, S, 3 * C), 13, dtype)
    ref = oracle_attention(qkvo[..., :C], qkvo[..., C:2 * C], qkvo[..., 2 * C:], H)
    out = K.spatial_attention(qkvd[..., :C], qkvd[..., C:2 * C], qkvd[..., 2 * C:], H)
    assert rel_inf(out.float(), ref) < TOL[dtype]
    kvo, kvd = rnd((B, 77, 2 * C), 14, dtype)
    qo, qd = rnd((B * Fr, S, C), 15, dtype)
    kv_rep = kvo.repeat_interleave(Fr, dim=0)                                 # what `repeat(b n c -> (b f) n c)` does
    ref = oracle_attention(qo, kv_rep[..., :C], kv_rep[..., C:], H)
    out = K.spatial_attention(qd, kvd[..., :C], kvd[..., C:], H)
    assert rel_inf(out.float(), ref) < TOL[dtype]


def test_spatial_attention_softmax_stress(K):
    """online-softmax rescale must survive a key whose score dwarfs everything seen before it."""
    B, S, H, D = 1, 256, 2, 40
    C = H * D
    q = torch.randn(B, S, C, generator=torch.Generator().manual_seed(16))
    k = torch.randn(B, S, C, generator=torch.Generator().manual_seed(17))
    v = torch.randn(B, S, C, generator=torch.Generator().manual_seed(18))
    k[0, 200] = q[0, 7] * 6.0                                                  # spike late in the key sequence
    ref = oracle_attention(q, k, v, H)
    out = K.spatial_attention(q.cuda(), k.cuda(), v.cuda(), H)
    # logits reach |s| ~ 100 here: the split-bf16 products carry 2^-17 RELATIVE error, i.e. ~1e-3 absolute in such a
    # logit, hence a looser bound than for O(1..10) logits (measured 2.1e-5; the fp32 oracle itself is 5e-7 off fp64)
    assert rel_inf(out, ref) < 1e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,D", [(2, 40), (2, 160), (2, 64), (2, 80)])          # d = 80, S = 320: the big-tile kernel
def test_spatial_attention_reference_redo(K, dtype, H, D):
    """A late key whose logit exceeds the first-tile row maximum by more than the kernel's fixed-reference range
    (64 log2 units): the workgroup must redo its K/V sweep with the exact row maxima.  Rows without the spike in the
    same workgroup must be unaffected; the output LSE must be the true one."""
    B, S = 1, 320
    C = H * D
    qo, qd = rnd((B, S, C), 40, dtype)
    ko, kd = rnd((B, S, C), 41, dtype)
    vo, vd = rnd((B, S, C), 42, dtype)
    gain = 90.0 / float((qo[0, 7, :D] ** 2).sum() * D ** -0.5)                 # head-0 logit of (row 7, key 250) ~ 90
    for t in (ko, kd):
        t[0, 250] = (qo[0, 7] * gain).to(t.dtype)
    ko[0, 250] = kd[0, 250].float().cpu()
    spike = (qo[0, 7, :D] * ko[0, 250, :D]).sum() * D ** -0.5
    assert spike * 1.4427 > 100.0, spike                                        # far outside the fixed-reference range
    ref = oracle_attention(qo, ko, vo, H)
    out, lse = K.spatial_attention(qd, kd, vd, H, return_lse=True)
    assert torch.isfinite(out).all()
    # bf16: the kernel rounds q*scale*log2(e) to bf16 once more (2^-9 relative), which on |logit| ~ 100 is a few
    # 1e-2 absolute in the logit -- the same sensitivity the bf16 inputs themselves carry; hence the looser bound here
    # (the O(1..10)-logit cases above hold 1e-2)
    assert rel_inf(out.float(), ref) < (1e-4 if dtype == torch.float32 else 5e-2)
    qh = qo.view(B, S, H, D).permute(0, 2, 1, 3)
    kh = ko.view(B, S, H, D).permute(0, 2, 1, 3)
    lse_ref = torch.logsumexp(qh @ kh.transpose(-1, -2) * D ** -0.5, dim=-1)
    assert (lse.cpu() - lse_ref).abs().max() < (2e-3 if dtype == torch.float32 else 0.5)


@pytest.mark.parametrize("B,S,Skv,H,fused", [(8, 256, 256, 8, True), (3, 512, 128, 8, False), (1, 256, 1536, 2, False),
                                             (16, 768, 768, 8, True), (2, 256, 192, 5, False)])
def test_spatial_attention_pipelined_d40(K, B, S, Skv, H, fused):
    """The software-pipelined d = 40 kernel (bf16, S_q % 256 == 0, S_kv % 64 == 0: `sa40d_kernel`): every block -> XCD map
    (batch % 8 == 0, (batch * heads) % 8 == 0, neither), 2 .. 24 K/V tiles (the 4-buffer DMA ring wraps, and with 2 or 3
    tiles part of the prologue's requests are out of range), q/k/v as slices of one fused projection, LSE."""
    D, dtype = 40, torch.bfloat16
    C = H * D
    if fused:
        qkvo, qkvd = rnd((B, S, 3 * C), 60, dtype)
        qo, ko, vo = qkvo[..., :C], qkvo[..., C:2 * C], qkvo[..., 2 * C:]
        qd, kd, vd = qkvd[..., :C], qkvd[..., C:2 * C], qkvd[..., 2 * C:]
    else:
        qo, qd = rnd((B, S, C), 61, dtype)
        ko, kd = rnd((B, Skv, C), 62, dtype)
        vo, vd = rnd((B, Skv, C), 63, dtype)
    ref = oracle_attention(qo, ko, vo, H)
    out, lse = K.spatial_attention(qd, kd, vd, H, return_lse=True)
    assert rel_inf(out.float(), ref) < TOL[dtype]
    qh = qo.reshape(B, S, H, D).permute(0, 2, 1, 3)
    kh = ko.reshape(B, Skv, H, D).permute(0, 2, 1, 3)
    lse_ref = torch.logsumexp(qh @ kh.transpose(-1, -2) * D ** -0.5, dim=-1)
    assert (lse.cpu() - lse_ref).abs().max() < 2e-2
    # shared text-style K/V (kv batch = batch / frames) through the same kernel
    if not fused and Skv == 128:
        k1o, k1d = rnd((1, Skv, C), 64, dtype)
        v1o, v1d = rnd((1, Skv, C), 65, dtype)
        ref = oracle_attention(qo, k1o.expand(B, -1, -1), v1o.expand(B, -1, -1), H)
        assert rel_inf(K.spatial_attention(qd, k1d, v1d, H).float(), ref) < TOL[dtype]


@pytest.mark.parametrize("B,S,Skv,kvdiv", [(8, 64, 77, 4), (4, 256, 20, 1), (6, 32, 96, 2), (32, 640, 77, 16), (2, 96, 1, 2)])
def test_text_cross_attention_kv_stationary(K, B, S, Skv, kvdiv):
    """`xattn40_kernel` (bf16, d = 40, 8 heads, S_kv <= 96, S_q % 32 == 0): a wave keeps its head's K / V^T fragments in registers and walks
    the query units of its text batch.  1 .. 96 keys (masking inside and across the three key blocks), K / V shared by `kvdiv` batch
    entries, K / V as slices of one fused [.., 2C] projection, LSE."""
    H, D, dtype = 8, 40, torch.bfloat16
    C = H * D
    qo, qd = rnd((B, S, C), 80, dtype)
    kvo, kvd = rnd((B // kvdiv, Skv, 2 * C), 81, dtype)
    kv_rep = kvo.repeat_interleave(kvdiv, dim=0)
    ref = oracle_attention(qo, kv_rep[..., :C], kv_rep[..., C:], H)
    out, lse = K.spatial_attention(qd, kvd[..., :C], kvd[..., C:], H, return_lse=True)
    assert rel_inf(out.float(), ref) < TOL[dtype]
    qh = qo.reshape(B, S, H, D).permute(0, 2, 1, 3)
    kh = kv_rep[..., :C].reshape(B, Skv, H, D).permute(0, 2, 1, 3)
    lse_ref = torch.logsumexp(qh @ kh.transpose(-1, -2) * D ** -0.5, dim=-1)
    assert (lse.cpu() - lse_ref).abs().max() < 2e-2


def test_spatial_attention_pipelined_reference_redo(K):
    """The pipelined kernel keeps no running maximum: a row whose logits leave the range of the first-tile reference shows as
    an overflowing denominator, the workgroup finds the exact maxima in a plain sweep and repeats the pipelined one.  The
    spike sits in tile 5 of 8 (behind the prologue's tiles); the other workgroup of the launch must be unaffected."""
    B, S, H, D, dtype = 1, 512, 2, 40, torch.bfloat16
    C = H * D
    qo, qd = rnd((B, S, C), 70, dtype)
    ko, kd = rnd((B, S, C), 71, dtype)
    vo, vd = rnd((B, S, C), 72, dtype)
    gain = 90.0 / float((qo[0, 7, :D] ** 2).sum() * D ** -0.5)
    for t in (ko, kd):
        t[0, 330] = (qo[0, 7] * gain).to(t.dtype)
    ko[0, 330] = kd[0, 330].float().cpu()
    spike = (qo[0, 7, :D] * ko[0, 330, :D]).sum() * D ** -0.5
    assert spike * 1.4427 > 100.0, spike
    ref = oracle_attention(qo, ko, vo, H)
    out, lse = K.spatial_attention(qd, kd, vd, H, return_lse=True)
    assert torch.isfinite(out).all()
    assert rel_inf(out.float(), ref) < 5e-2                                     # |logit| ~ 100 in bf16, as in the test above
    assert rel_inf(out[:, 256:].float(), ref[:, 256:]) < 5e-2                   # the other workgroup (no redo there; its logits against the spike key reach ~40)
    qh = qo.view(B, S, H, D).permute(0, 2, 1, 3)
    kh = ko.view(B, S, H, D).permute(0, 2, 1, 3)
    lse_ref = torch.logsumexp(qh @ kh.transpose(-1, -2) * D ** -0.5, dim=-1)
    assert (lse.cpu() - lse_ref).abs().max() < 0.5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,Fr,P,H,D", [(2, 16, 20, 8, 40), (1, 16, 9, 8, 80), (2, 16, 5, 8, 160), (1, 32, 6, 8, 40),
                                        (1, 32, 3, 8, 160), (2, 16, 7, 4, 8), (1, 16, 4, 8, 16)])
def test_temporal_attention_native_and_reference_layouts(K, dtype, B, Fr, P, H, D):
    C = H * D
    qkvo, qkvd = rnd((B, Fr, P, 3 * C), 20, dtype)
    # oracle on the reference layout (b h w) f c
    ref_in = qkvo.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
    ref = oracle_attention(ref_in[..., :C], ref_in[..., C:2 * C], ref_in[..., 2 * C:], H)
    out = K.temporal_attention(qkvd[..., :C], qkvd[..., C:2 * C], qkvd[..., 2 * C:], H)       # native [B,F,P,C]
    got = out.permute(0, 2, 1, 3).reshape(B * P, Fr, C)
    assert rel_inf(got.float(), ref) < TOL[dtype]
    r3 = qkvd.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C).contiguous()                       # reference layout in
    out3 = K.temporal_attention(r3[..., :C], r3[..., C:2 * C], r3[..., 2 * C:], H)
    assert rel_inf(out3.float(), ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S,H,D", [(2560, 8, 40), (640, 8, 80), (160, 8, 160)])
def test_spatial_attention_at_bench_size(K, dtype, S, H, D):
    """The launches of the benchmarked U-Net (CFG batch 2 x 16 frames = 32 batch entries, 8 heads: 256 (batch, head)
    pairs; q/k/v slices of ONE fused projection) -- the XCD-aware block map and the two-query-block path only show at
    this grid size.  The oracle runs on a sample of batch entries (first, last, and one per XCD slot of the map)."""
    B, C = 32, H * D
    qkvo, qkvd = rnd((B, S, 3 * C), 50, dtype)
    out = K.spatial_attention(qkvd[..., :C], qkvd[..., C:2 * C], qkvd[..., 2 * C:], H)
    assert torch.isfinite(out).all()
    sample = [0, 1, 7, 8, 13, 22, 30, 31]
    ref = oracle_attention(qkvo[sample][..., :C], qkvo[sample][..., C:2 * C], qkvo[sample][..., 2 * C:], H)
    assert rel_inf(out[sample].float(), ref) < TOL[dtype]
    # every (batch, head) pair was written by its own workgroup: no pair may equal another entry's result
    flat = out.float().view(B, -1)
    assert (flat[1:] - flat[:-1]).abs().amax(dim=1).min() > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Fr,P,H,D", [(16, 2560, 8, 40), (16, 640, 8, 80), (32, 4096, 8, 40)])
def test_temporal_attention_at_bench_size(K, dtype, Fr, P, H, D):
    """Level-0 / level-1 temporal attention of the benchmarked step (2 clips x 2560 pixels x 8 heads = 40 960 units)
    and the level-0 shape of BASELINE configs[4] (32 frames, 64x64 latent), against the oracle on ALL units."""
    B, C = 2, H * D
    qkvo, qkvd = rnd((B, Fr, P, 3 * C), 51, dtype)
    ref_in = qkvo.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
    ref = oracle_attention(ref_in[..., :C], ref_in[..., C:2 * C], ref_in[..., 2 * C:], H)
    out = K.temporal_attention(qkvd[..., :C], qkvd[..., C:2 * C], qkvd[..., 2 * C:], H)
    got = out.permute(0, 2, 1, 3).reshape(B * P, Fr, C)
    assert rel_inf(got.float(), ref) < TOL[dtype]


# ---- fp8 (e4m3) temporal attention: BASELINE.json configs[4] -------------------------------------------------------------
def _quant(x, scale):
    """per-tensor e4m3 quantisation as the projection epilogue does it: sat(x / scale) -> float8_e4m3fn"""
    return (x.float() / scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


@pytest.mark.parametrize("M,C,Kd", [(4100, 320, 320), (2048, 640, 640), (700, 64, 128)])
def test_linear_fp8_qkv_epilogue(K, M, C, Kd):
    """The fused q | k | v projection with the e4m3 epilogue against `quant((x @ W^T) / scale_block)` computed by torch
    from the SAME bf16 operands, and the running |max| per block it records."""
    xo, xd = rnd((M, Kd), 70, torch.bfloat16)
    w = torch.randn(3 * C, Kd, generator=torch.Generator().manual_seed(71)) * Kd ** -0.5
    w[C:2 * C] *= 3.0                                                        # three different ranges -> three different scales
    wo, wd = w.bfloat16().float(), w.bfloat16().cuda()
    ref = F.linear(xo, wo)                                                    # fp32 accumulate of the bf16 values
    sc = K.Fp8QKVScales(xd.device, margin=1.25)
    blocks = [ref[:, i * C:(i + 1) * C] for i in range(3)]
    sc.calibrate(*[b.cuda() for b in blocks])
    sc.roll()
    out = K.linear_fp8_qkv(xd, wd, sc)
    assert out.dtype == torch.float8_e4m3fn and out.shape == (M, 3 * C)
    amax = sc.amax.cpu()
    for i, b in enumerate(blocks):
        assert abs(float(amax[i]) - float(b.abs().max())) < 2e-3 * float(b.abs().max())      # max |acc| of this call
        s = float(sc.scale[i])
        assert abs(s - 1.25 * float(b.abs().max()) / 448.0) < 1e-5 * s
        got = out[:, i * C:(i + 1) * C].float().cpu() * s
        want = _quant(b, s).float() * s
        exact = (got == want).float().mean().item()
        assert exact > 0.98, exact                                            # (ties at a rounding boundary may flip: other summation order)
        # never more than one e4m3 step (2^-3 of the value's binade) apart
        assert ((got - want).abs() <= 0.13 * torch.maximum(got.abs(), want.abs()).clamp_min(s * 2 ** -6)).all()


@pytest.mark.parametrize("B,Fr,P,H,D", [(2, 16, 20, 8, 40), (1, 32, 6, 8, 40), (1, 32, 3, 8, 160), (1, 16, 9, 8, 80),
                                        (2, 16, 7, 8, 8), (2, 32, 4096, 8, 40)])
def test_temporal_attention_fp8_forward(K, B, Fr, P, H, D):
    """fp8 temporal attention against the oracle evaluated on the SAME e4m3-rounded q, k, v (so the bound is the bf16
    kernel's: bf16 rounding of P and O, 1e-2) -- incl. the level-0 shape of BASELINE configs[4] (32 frames, 64x64 latent)."""
    C = H * D
    g = torch.Generator().manual_seed(72)
    qkv = torch.randn(B, Fr, P, 3 * C, generator=g)
    qkv[..., C:2 * C] *= 2.0
    scales = torch.tensor([qkv[..., :C].abs().max(), qkv[..., C:2 * C].abs().max(), qkv[..., 2 * C:].abs().max()]) * 1.25 / 448.0
    q8 = torch.cat([_quant(qkv[..., i * C:(i + 1) * C], float(scales[i])) for i in range(3)], dim=-1)
    deq = torch.cat([q8[..., i * C:(i + 1) * C].float() * float(scales[i]) for i in range(3)], dim=-1)
    ref_in = deq.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
    ref = oracle_attention(ref_in[..., :C], ref_in[..., C:2 * C], ref_in[..., 2 * C:], H)
    out = K._temporal_fp8_raw(q8.cuda(), scales.cuda(), H, D ** -0.5)
    got = out.permute(0, 2, 1, 3).reshape(B * P, Fr, C)
    assert out.dtype == torch.bfloat16 and rel_inf(got.float(), ref) < 1e-2


def test_temporal_attention_fp8_autograd(K):
    """x -> (QKV projection, e4m3 epilogue) -> fp8 attention as one autograd node: output and input / weight gradients
    against torch autograd through `quantise (straight-through) -> softmax attention` on the same operands."""
    B, Fr, P, H, D = 1, 16, 12, 8, 40
    C = H * D
    xo, xd = rnd((B, Fr, P, C), 73, torch.bfloat16)
    wo, wd = rnd((3 * C, C), 74, torch.bfloat16, scale=C ** -0.5)
    do, dd = rnd((B, Fr, P, C), 75, torch.bfloat16)
    sc = K.Fp8QKVScales(xd.device)
    xg, wg = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True)
    out = K.temporal_attention_fp8(xg, wg, sc, H, D ** -0.5)                 # (first call calibrates from a bf16 projection)
    out.backward(dd)
    scales = sc.scale.cpu()
    xr, wr = xo.clone().requires_grad_(True), wo.clone().requires_grad_(True)
    qkv = F.linear(xr, wr)
    deq = torch.cat([_quant(qkv[..., i * C:(i + 1) * C].detach(), float(scales[i])).float() * float(scales[i]) for i in range(3)], -1)
    qkv_ste = qkv + (deq - qkv).detach()                                      # straight-through estimator
    t = qkv_ste.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
    ref = oracle_attention(t[..., :C], t[..., C:2 * C], t[..., 2 * C:], H).reshape(B, P, Fr, C).permute(0, 2, 1, 3)
    ref.backward(do)
    assert rel_inf(out.float(), ref) < 2e-2           # (+ fp8 ties of the projection output flipping against torch's summation order)
    assert rel_inf(xg.grad.float(), xr.grad) < 3e-2
    assert rel_inf(wg.grad.float(), wr.grad) < 3e-2


# ---------------------------------------------------------------------------------------------
def test_plucker_against_golden_and_oracle(K, golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "g1_plucker.npz"))
    Kt, c2w = torch.from_numpy(g["K"]), torch.from_numpy(g["c2w"])
    H, W = int(g["H"]), int(g["W"])
    out = K.plucker(Kt.cuda(), c2w.cuda(), H, W, "bfhwc")
    assert rel_inf(out, torch.from_numpy(g["out"])) < 2e-6                     # the reference's own output
    out1 = K.plucker(Kt.cuda(), c2w[:, :, :3].contiguous().cuda(), H, W, "bcfhw")
    assert rel_inf(out1, out.permute(0, 4, 1, 2, 3)) < 1e-6       # same math, separate template instance (fma contraction)
    out2 = K.plucker(Kt.cuda(), c2w.cuda(), H, W, "unshuffle8")
    ref2 = F.pixel_unshuffle(out.permute(0, 1, 4, 2, 3).reshape(-1, 6, H, W), 8).permute(0, 2, 3, 1)
    assert rel_inf(out2, ref2) < 1e-6
    Kb, cb = torch.from_numpy(g["K_b"]), torch.from_numpy(g["c2w_b"])
    outb = K.plucker(Kb.cuda(), cb.cuda(), int(g["H_b"]), int(g["W_b"]), "bfhwc")
    assert rel_inf(outb[:, :, :: int(g["row_step"])], torch.from_numpy(g["out_b"])) < 2e-6
    outbf = K.plucker(Kb.cuda(), cb.cuda(), int(g["H_b"]), int(g["W_b"]), "bfhwc", torch.bfloat16)
    assert rel_inf(outbf.float(), outb) < 5e-3


def test_rasterize_against_golden(K, golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "g3_traj.npz"))
    B, Fr, n, _, H, W = g["masks"].shape
    masks = torch.from_numpy(g["masks"]).reshape(B * Fr, n, H, W)
    poses = torch.from_numpy(g["infos"]).reshape(B * Fr, n, 12).float()
    feat, m = K.omc_rasterize(poses.cuda(), masks.cuda(), "planar")
    assert torch.equal(m.cpu(), torch.from_numpy(g["raster_mask"]))            # bit exact: selection + copy
    assert rel_inf(feat, torch.from_numpy(g["raster"])) < 1e-7
    feat2, m2 = K.omc_rasterize(poses.cuda(), masks.cuda(), "unshuffle8")
    assert torch.equal(feat2.cpu(), F.pixel_unshuffle(feat, 8).permute(0, 2, 3, 1).cpu())
    assert torch.equal(m2.cpu(), m[:, 0].cpu())
    # ragged / empty: no object at all -> zeros
    f0, m0 = K.omc_rasterize(poses.cuda(), torch.zeros_like(masks).cuda(), "planar")
    assert float(f0.abs().max()) == 0.0 and float(m0.abs().max()) == 0.0


def test_get_traj_features_null_condition_against_reference_golden(K, golden_dir):
    """`get_traj_features_v2(..., cfg_random_null_om=True, ratio)` on the GPU path against the reference's own outputs:
    kept clip = golden G3, dropped clip = golden G3b (zero features, REAL mask -> the Adapter's propagated biases)."""
    import os
    from synfmc_amd.util import get_traj_features_v2
    from tests.test_host_logic import _product_small_adapter
    g, gn = np.load(os.path.join(golden_dir, "g3_traj.npz")), np.load(os.path.join(golden_dir, "g3_traj_null.npz"))
    masks = [[torch.from_numpy(g["masks"][b, f]) for f in range(g["masks"].shape[1])] for b in range(g["masks"].shape[0])]
    infos = [[g["infos"][b, f] for f in range(g["infos"].shape[1])] for b in range(g["infos"].shape[0])]
    ad = _product_small_adapter(golden_dir, "cuda")
    with torch.no_grad():
        kept = get_traj_features_v2(infos, masks, ad, True, 0.0, [False], 0, torch.float32)
        null = get_traj_features_v2(infos, masks, ad, True, 1.0, [False], 0, torch.float32)
    for i in range(4):
        assert rel_inf(kept[i], torch.from_numpy(g[f"feat_{i}"])) < 1e-4
        assert rel_inf(null[i], torch.from_numpy(gn[f"feat_{i}"])) < 1e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mask_modulate_cascade(K, dtype):
    N, H, W = 3, 64, 96
    mask = torch.rand(N, H, W, generator=torch.Generator().manual_seed(30))
    mask = mask * (mask > 0.4)
    m_ref, m_dev = mask[:, None], mask.cuda()
    for (h, w, C) in [(8, 12, 320), (4, 6, 640), (2, 3, 1280), (1, 1, 1280)]:
        xo, xd = rnd((N, h * w, C), 31, dtype)
        m_ref = F.interpolate(m_ref, size=(h, w), mode="nearest")              # cascaded, like adapter.py:175-177
        ref = xo * m_ref.reshape(N, h * w, 1)
        y, m_dev = K.mask_modulate(xd, m_dev, h, w)
        assert torch.equal(m_dev.cpu(), m_ref[:, 0])
        assert rel_inf(y.float(), ref) < TOL[dtype]
    # non-divisible sizes follow PyTorch's floor(dst * in/out) rule
    m7 = F.interpolate(mask[:, None], size=(7, 11), mode="nearest")
    _, got = K.mask_modulate(torch.ones(N, 77, 8).cuda(), mask.cuda(), 7, 11)
    assert torch.equal(got.cpu(), m7[:, 0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_feature_add_cfg_half(K, dtype):
    ho, hd = rnd((4, 16, 20, 320), 40, dtype)
    to, td = rnd((2, 16, 20, 320), 41, dtype)
    ref = ho.clone()
    ref[2:] += to
    out = K.feature_add(hd, td)
    assert rel_inf(out.float(), ref) < TOL[dtype]
    assert torch.equal(out[:2], hd[:2])                                         # unconditional half untouched
    full_o, full_d = rnd((4, 16, 20, 320), 42, dtype)
    assert rel_inf(K.feature_add(hd, full_d).float(), ho + full_o) < TOL[dtype]
    h2 = hd.clone()
    K.feature_add(h2, td, inplace=True)
    assert torch.equal(h2, out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cfg_ddim_step(K, dtype):
    sch = OD.DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear",
                           steps_offset=1, clip_sample=False)
    sch.set_timesteps(25)
    from synfmc_amd.schedulers import DDIMScheduler
    mine = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear",
                         steps_offset=1, clip_sample=False)
    mine.set_timesteps(25)
    assert mine._timesteps_host == sch.timesteps.tolist()
    x = torch.randn(1, 4, 16, 8, 8, generator=torch.Generator().manual_seed(50))
    eo, ed = rnd((2, 4, 16, 8, 8), 51, dtype)
    for t in (961, 481, 1):
        eps = eo[:1] + 8.0 * (eo[1:] - eo[:1])
        ref = sch.step(eps, t, x).prev_sample
        got = mine.step_cfg(ed, t, x.cuda(), 8.0, True)
        assert rel_inf(got, ref) < 1e-5


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,Kd,bias,res,alpha", [(300, 320, 320, True, True, 1.0), (1000, 960, 320, False, False, 1.0),
                                                    (129, 640, 2560, True, True, 0.5), (77 * 2, 640, 768, False, False, 1.0),
                                                    (4096, 1280, 1280, True, False, 1.0), (64, 8, 64, True, True, 1.0)])
def test_linear_bf16_fused_epilogue(K, M, N, Kd, bias, res, alpha):
    dtype = torch.bfloat16
    xo, xd = rnd((M, Kd), 60, dtype)
    wo, wd = rnd((N, Kd), 61, dtype, scale=Kd ** -0.5)
    bo, bd = rnd((N,), 62, dtype)
    ro, rd = rnd((M, N), 63, dtype)
    ref = F.linear(xo.double(), wo.double(), bo.double() if bias else None) * alpha + (ro.double() if res else 0)
    mag = (xo.abs().double() @ wo.abs().double().t() + (bo.abs().double() if bias else 0)) * abs(alpha) + (ro.abs().double() if res else 0)
    out = K.linear_bf16(xd, wd, bd if bias else None, rd if res else None, alpha)
    assert rel_inf(out.float(), ref) < 1e-2
    assert_bf16_close(out, ref, mag, "linear_bf16")
    # strided input rows (a slice of a wider matrix)
    wide = torch.cat([xd, xd], dim=1)
    out2 = K.linear_bf16(wide[:, Kd:], wd, bd if bias else None, rd if res else None, alpha)
    assert torch.equal(out2, out)


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
def test_gemm_tile_geometries_agree(K, tile):
    """every `tile` arm (3 geometries x k-tile depth 64 / 32 x ring depth 2..4) must compute the same function, ragged edges included"""
    dtype = torch.bfloat16
    xo, xd = rnd((777, 320), 67, dtype)
    wo, wd = rnd((328, 320), 68, dtype, scale=320 ** -0.5)
    bo, bd = rnd((328,), 69, dtype)
    ro, rd = rnd((777, 328), 59, dtype)
    ref = F.linear(xo.double(), wo.double(), bo.double()) + ro.double()
    out = K.linear_bf16(xd, wd, bd, rd, 1.0, tile=tile)
    assert_bf16_close(out, ref, xo.abs().double() @ wo.abs().double().t() + bo.abs() + ro.abs(), f"linear tile {tile}")
    assert torch.equal(out, K.linear_bf16(xd, wd, bd, rd, 1.0, tile=1))         # same accumulation order in every arm
    co, cd = rnd((2, 128, 11, 13), 58, dtype)
    fo, fd = rnd((72, 128, 3, 3), 57, dtype, scale=(9 * 128) ** -0.5)
    refc = F.conv2d(co.double(), fo.double(), None, 1, 1)
    outc = K.conv3x3_bf16(cd.permute(0, 2, 3, 1).contiguous(), fd.contiguous(memory_format=torch.channels_last), None,
                          None, None, tile=tile)
    assert_bf16_close(outc.permute(0, 3, 1, 2), refc, F.conv2d(co.abs().double(), fo.abs().double(), None, 1, 1), f"conv tile {tile}")
    from synfmc_amd.models.layers import interleave_geglu
    go, gd = rnd((512, 320), 56, dtype, scale=320 ** -0.5)
    wi, bi = interleave_geglu(gd, None)
    a, g = F.linear(xo, go).chunk(2, dim=-1)
    outg = K.linear_bf16(xd, wi, bi, geglu=True, tile=tile)
    assert rel_inf(outg.float(), a * F.gelu(g)) < 1e-2


@pytest.mark.parametrize("tile", [0, 1, 3, 4, 11, 1 + 16, 128 + 2])
def test_linear_second_residual(K, tile):
    """`alpha * (x W^T + b) + residual + residual2` (plain, split-K and stream-K arms) -- the Camera-Adapter merge with the
    per-clip pose term pre-computed: s*(W(h+pose)+b)+h == s*(W h) + h + s*(W pose + b)."""
    dtype = torch.bfloat16
    M, C, s_ = 2100, 1280, 0.7
    ho, hd = rnd((M, C), 70, dtype)
    po, pd = rnd((M, C), 71, dtype)
    wo, wd = rnd((C, C), 72, dtype, scale=C ** -0.5)
    bo, bd = rnd((C,), 73, dtype)
    ref = F.linear(ho + po, wo, bo) * s_ + ho                                   # attention_processor.py:257
    term = K.linear_bf16(pd, wd, bd, None, s_)
    out = K.linear_bf16(hd, wd, None, hd, s_, tile=tile, residual2=term)
    assert rel_inf(out.float(), ref) < 1e-2
    r2o, r2d = rnd((M, C), 74, dtype)
    want = F.linear(ho, wo, bo) * s_ + po + r2o
    got = K.linear_bf16(hd, wd, bd, pd, s_, tile=tile, residual2=r2d)
    assert rel_inf(got.float(), want) < 1e-2
    with pytest.raises((ValueError, AssertionError)):
        K.linear_bf16(hd, wd, bd, None, s_, residual2=r2d)                      # a second residual needs the first


def test_launch_lds_grows_for_one_instantiation(K):
    """One instantiation of the ring kernel, two dynamic-LDS sizes, in one fresh process: tile 6 (256 x 256 tiles, 32-deep k-tiles) runs
    with 67,584 B when a second residual keeps the epilogue on the fp32 slab, and with 135,168 B when it stages the whole bf16 tile.
    The launch helper must raise the attribute a second time for the larger size -- a "raised" flag fails the second launch (an error
    status, no fault).  Bound: the one of the other linear_bf16 tests (bf16 rounding of the output)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "launch_child.py"), root, "0:6:256:256:64:1", "0:6:256:256:64:0"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    errs = json.loads(out.stdout.splitlines()[-1])
    print("rel-inf, 67,584 B then 135,168 B:", errs)
    assert len(errs) == 2 and all(e < 1e-2 for e in errs), errs


@pytest.mark.parametrize("tile", [0, 1, 3, 5, 7, 11])
def test_conv_epilogue_variants_plain_grid(K, tile):
    """plain-grid epilogues of the conv kernel (one bf16 staging round): bias only, temb only (per-image and per-clip
    rows), residual only, temb + residual; ragged Cout (tile columns beyond N) and ragged pixel count."""
    dtype = torch.bfloat16
    n, ci, co, h, w = 6, 128, 136, 13, 11
    xo, xd = rnd((n, ci, h, w), 150, dtype)
    fo, fd = rnd((co, ci, 3, 3), 151, dtype, scale=(9 * ci) ** -0.5)
    bo, bd = rnd((co,), 152, dtype)
    to, td = rnd((n, co), 153, dtype)
    t2o, t2d = rnd((n // 3, co), 154, dtype)
    ro, rd = rnd((n, co, h, w), 155, dtype)
    x_cl, f_cl, r_cl = xd.permute(0, 2, 3, 1).contiguous(), fd.contiguous(memory_format=torch.channels_last), \
        rd.permute(0, 2, 3, 1).contiguous()
    base = F.conv2d(xo, fo, None, 1, 1)
    cases = [(bd, None, None, 1, base + bo[None, :, None, None]),
             (None, td, None, 1, base + to[:, :, None, None]),
             (None, t2d, None, 3, base + t2o.repeat_interleave(3, 0)[:, :, None, None]),
             (None, None, r_cl, 1, base + ro),
             (bd, td, r_cl, 1, base + bo[None, :, None, None] + to[:, :, None, None] + ro)]
    for bias, temb, res, div, ref in cases:
        out = K.conv3x3_bf16(x_cl, f_cl, bias, temb, res, tile=tile, temb_div=div)
        assert rel_inf(out.permute(0, 3, 1, 2).float(), ref) < 1e-2


@pytest.mark.parametrize("split_k", [2, 4, 8])
@pytest.mark.parametrize("tile", [1, 2, 9])
def test_gemm_split_k(K, tile, split_k):
    """split-K arms: fp32 partial sums in a workspace + a fixed-order reduce; ragged k-tile division included"""
    dtype = torch.bfloat16
    xo, xd = rnd((333, 1280 + 64), 50, dtype)                                   # 21 k-tiles: not divisible by 2/4/8
    wo, wd = rnd((200, 1280 + 64), 51, dtype, scale=1344 ** -0.5)
    bo, bd = rnd((200,), 52, dtype)
    ro, rd = rnd((333, 200), 53, dtype)
    ref = (F.linear(xo, wo, bo)) * 0.5 + ro
    out = K.linear_bf16(xd, wd, bd, rd, 0.5, tile=tile, split_k=split_k)
    assert rel_inf(out.float(), ref) < 1e-2
    assert torch.equal(out, K.linear_bf16(xd, wd, bd, rd, 0.5, tile=tile, split_k=split_k))   # deterministic
    assert torch.equal(out, K.linear_bf16(xd, wd, bd, rd, 0.5, tile=tile + 16 * {2: 1, 4: 2, 8: 3}[split_k]))  # arm id
    co, cd = rnd((2, 256, 5, 8), 54, dtype)
    fo, fd = rnd((136, 256, 3, 3), 55, dtype, scale=(9 * 256) ** -0.5)
    to, td = rnd((2, 136), 49, dtype)
    so, sd = rnd((2, 136, 5, 8), 48, dtype)
    refc = F.conv2d(co, fo, None, 1, 1) + to[:, :, None, None] + so
    outc = K.conv3x3_bf16(cd.permute(0, 2, 3, 1).contiguous(), fd.contiguous(memory_format=torch.channels_last), None,
                          td, sd.permute(0, 2, 3, 1).contiguous(), tile=tile, split_k=split_k)
    assert rel_inf(outc.permute(0, 3, 1, 2).float(), refc) < 1e-2


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5])
def test_gemm_stream_k(K, tile):
    """stream-K arms (persistent workgroups, tiles cut at range boundaries, fp32 partials handed over through flags):
    ragged M / N, conv and GEGLU epilogues, and -- because the partial slots and flags are reused by every launch and
    per-XCD L2s are not coherent -- many back-to-back launches on fresh data"""
    dtype = torch.bfloat16
    M, N, Kd = 4100, 1032, 1280
    wo, wd = rnd((N, Kd), 45, dtype, scale=Kd ** -0.5)
    bo, bd = rnd((N,), 46, dtype)
    for it in range(12):
        xo, xd = rnd((M, Kd), 200 + it, dtype)
        ro, rd = rnd((M, N), 300 + it, dtype)
        want = K.linear_bf16(xd, wd, bd, rd, 1.0, tile=tile)
        got = K.linear_bf16(xd, wd, bd, rd, 1.0, tile=128 + tile)
        assert rel_inf(got.float(), want.float()) < 4e-3, it                     # same products, other summation order
        if it == 0:
            assert rel_inf(got.float(), F.linear(xo, wo, bo) + ro) < 1e-2
            assert torch.equal(got, K.linear_bf16(xd, wd, bd, rd, 1.0, tile=128 + tile))   # deterministic
    co, cd = rnd((4, 320, 36, 30), 47, dtype)
    fo, fd = rnd((328, 320, 3, 3), 44, dtype, scale=(9 * 320) ** -0.5)
    to, td = rnd((4, 328), 43, dtype)
    refc = F.conv2d(co, fo, None, 1, 1) + to[:, :, None, None]
    outc = K.conv3x3_bf16(cd.permute(0, 2, 3, 1).contiguous(), fd.contiguous(memory_format=torch.channels_last), None,
                          td, None, tile=128 + tile)
    assert rel_inf(outc.permute(0, 3, 1, 2).float(), refc) < 1e-2
    from synfmc_amd.models.layers import interleave_geglu
    go, gd = rnd((2048, Kd), 42, dtype, scale=Kd ** -0.5)
    xo, xd = rnd((M, Kd), 41, dtype)
    wi, bi = interleave_geglu(gd, None)
    a, g = F.linear(xo, go).chunk(2, dim=-1)
    outg = K.linear_bf16(xd, wi, bi, geglu=True, tile=128 + tile)
    assert rel_inf(outg.float(), a * F.gelu(g)) < 1e-2
    ws = K._sk_ws[(torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)]
    assert int(ws[:1024].view(torch.int32).abs().sum()) == 0                      # flags handed back as zeros


def test_gemm_k320_weight_stationary_arm(K):
    """Arm 15: the persistent kernel of the K = 320 projections (weights of a 320-column block resident in registers, A tiles by
    LDS-DMA two tiles ahead, residual rows DMA'd into the output staging tile).  One .. many tiles per workgroup (the grid is
    min(tiles, CUs)), 1 / 2 / 3 column blocks, every epilogue it takes (bias, alpha, residual), column slices of wider tensors as x and
    residual, repeated launches on fresh data; shapes it does not take (K != 320, M % 64 != 0, two residuals)
    must fall back to the ring kernel with the same results."""
    dtype = torch.bfloat16
    for (M, N) in [(64, 320), (640, 320), (64 * 300, 640), (64 * 515, 960), (81920, 320)]:
        wo, wd = rnd((N, 320), 145, dtype, scale=320 ** -0.5)
        bo, bd = rnd((N,), 146, dtype)
        for it in range(3):
            xo, xd = rnd((M, 320), 500 + it, dtype)
            ro, rd = rnd((M, N), 600 + it, dtype)
            got = K.linear_bf16(xd, wd, bd, rd, 0.5, tile=15)
            ref = K.linear_bf16(xd, wd, bd, rd, 0.5, tile=5)
            assert rel_inf(got.float(), 0.5 * F.linear(xo, wo, bo) + ro) < 1e-2, (M, N, it)
            assert rel_inf(got.float(), ref.float()) < 4e-3                          # (bias enters the accumulator first: last-bit differences)
            if it == 0:
                assert torch.equal(got, K.linear_bf16(xd, wd, bd, rd, 0.5, tile=15))   # deterministic
                assert rel_inf(K.linear_bf16(xd, wd, None, None, 1.0, tile=15).float(), F.linear(xo, wo)) < 1e-2
                assert rel_inf(K.linear_bf16(xd, wd, bd, None, 1.0, tile=15).float(), F.linear(xo, wo, bo)) < 1e-2
    # x and the residual as column slices of wider tensors (row strides 960 / 640 elements)
    wo, wd = rnd((320, 320), 156, dtype, scale=320 ** -0.5)
    bigx_o, bigx_d = rnd((1280, 960), 157, dtype)
    bigr_o, bigr_d = rnd((1280, 640), 158, dtype)
    got = K.linear_bf16(bigx_d[:, 320:640], wd, None, bigr_d[:, 320:], 1.0, tile=15)
    assert rel_inf(got.float(), F.linear(bigx_o[:, 320:640], wo) + bigr_o[:, 320:]) < 1e-2
    # fall-backs: same entry point, other kernels
    xo, xd = rnd((700, 320), 147, dtype)
    wo, wd = rnd((320, 320), 148, dtype, scale=320 ** -0.5)
    ro, rd = rnd((700, 320), 149, dtype)
    r2o, r2d = rnd((700, 320), 150, dtype)
    assert rel_inf(K.linear_bf16(xd, wd, None, rd, 1.0, tile=15).float(), F.linear(xo, wo) + ro) < 1e-2          # M % 64 != 0
    xo, xd = rnd((640, 320), 151, dtype)
    ro, rd = rnd((640, 320), 152, dtype)
    r2o, r2d = rnd((640, 320), 153, dtype)
    assert rel_inf(K.linear_bf16(xd, wd, None, rd, 1.0, tile=15, residual2=r2d).float(), F.linear(xo, wo) + ro + r2o) < 1e-2
    wo6, wd6 = rnd((320, 640), 154, dtype, scale=640 ** -0.5)
    xo6, xd6 = rnd((640, 640), 155, dtype)
    assert rel_inf(K.linear_bf16(xd6, wd6, None, None, 1.0, tile=15).float(), F.linear(xo6, wo6)) < 1e-2           # K != 320


@pytest.mark.parametrize("arm", [600, 601, 602, 603])
def test_gemm_small_m_tiles(K, arm):
    """The 64 x 128 tiles of the ring kernel (a wave = 32 x 64; C-ABI tiles 19 .. 22, autotune arms 600 .. 603 -- 64 x 128 on 4 waves, 128 x 128 and 64 x 256 on 8: offered for M <= 2560 projections, where
    128 x 128 tiles leave more than half of the 256 CUs idle): ragged M / N, bias / alpha / residual, bit-identical to the 128 x 128 kernel (same
    products in the same order), deterministic; two residuals and split-K fall back to tile 1."""
    dtype = torch.bfloat16
    for (M, N, Kd) in [(1280, 1280, 1280), (640, 3840, 1280), (2560, 1280, 5120), (1000, 328, 320), (70, 136, 64)]:
        wo, wd = rnd((N, Kd), 45, dtype, scale=Kd ** -0.5)
        bo, bd = rnd((N,), 46, dtype)
        xo, xd = rnd((M, Kd), 47, dtype)
        ro, rd = rnd((M, N), 48, dtype)
        r2o, r2d = rnd((M, N), 49, dtype)
        got = K.linear_bf16(xd, wd, bd, rd, 0.5, tile=arm)
        assert rel_inf(got.float(), 0.5 * F.linear(xo, wo, bo) + ro) < 1e-2, (M, N, Kd)
        assert torch.equal(got, K.linear_bf16(xd, wd, bd, rd, 0.5, tile=arm))
        assert torch.equal(got, K.linear_bf16(xd, wd, bd, rd, 0.5, tile=4 if arm == 601 else 1))          # (tile 1: 64-deep k-tiles, tile 4: 32-deep)
        assert rel_inf(K.linear_bf16(xd, wd, bd, None, 1.0, tile=arm).float(), F.linear(xo, wo, bo)) < 1e-2
        assert rel_inf(K.linear_bf16(xd, wd, None, rd, 1.0, tile=arm, residual2=r2d).float(), F.linear(xo, wo) + ro + r2o) < 1e-2


@pytest.mark.parametrize("tile", [13, 14, 128 + 13, 128 + 14, 256 + 13, 384 + 13])
def test_gemm_8phase_arms(K, tile):
    """The 8-phase 256x256 kernel (staggered wave rows, half-tile DMA with counted vmcnt): ragged M / N (partial tiles),
    K from one k-tile up, every epilogue (bias, alpha, one / two residuals, GEGLU, two-source A operand), the conv loader
    (plain, + temb, + residual, upsample, stride 2), determinism, and repeated launches on fresh data (a racy schedule
    shows up as rare wrong tiles)."""
    dtype = torch.bfloat16
    from synfmc_amd.models.layers import interleave_geglu
    # (5120 x 4096: 320 tiles on 256 CUs -- the hybrid arm 256 + 13 runs 256 of them on the plain grid and stream-Ks the other 64)
    for (M, N, Kd) in [(4100, 1032, 1280), (256, 256, 64), (700, 320, 320), (5120, 1280, 128), (1000, 2560, 640), (5120, 4096, 640)]:
        wo, wd = rnd((N, Kd), 45, dtype, scale=Kd ** -0.5)
        bo, bd = rnd((N,), 46, dtype)
        for it in range(4):
            xo, xd = rnd((M, Kd), 200 + it, dtype)
            ro, rd = rnd((M, N), 300 + it, dtype)
            r2o, r2d = rnd((M, N), 400 + it, dtype)
            got = K.linear_bf16(xd, wd, bd, rd, 0.5, tile=tile)
            assert rel_inf(got.float(), 0.5 * F.linear(xo, wo, bo) + ro) < 1e-2, (M, N, Kd, it)
            if it == 0 and M * N <= 6_000_000:
                assert_bf16_close(got, 0.5 * F.linear(xo.double(), wo.double(), bo.double()) + ro.double(),
                                  0.5 * (xo.abs().double() @ wo.abs().double().t() + bo.abs()) + ro.abs(), f"8-phase arm {tile} {(M, N, Kd)}")
            if it == 0:
                assert torch.equal(got, K.linear_bf16(xd, wd, bd, rd, 0.5, tile=tile))                      # deterministic
                if tile < 128:                                                                              # == the plain kernel
                    assert torch.equal(got, K.linear_bf16(xd, wd, bd, rd, 0.5, tile=1))
                got2 = K.linear_bf16(xd, wd, None, rd, 1.0, tile=tile, residual2=r2d)
                assert rel_inf(got2.float(), F.linear(xo, wo) + ro + r2o) < 1e-2
                got0 = K.linear_bf16(xd, wd, bd, None, 1.0, tile=tile)
                assert rel_inf(got0.float(), F.linear(xo, wo, bo)) < 1e-2
    # two-source A operand (concat-free up blocks)
    xo1, xd1 = rnd((900, 640), 50, dtype)
    xo2, xd2 = rnd((900, 320), 51, dtype)
    wo, wd = rnd((640, 960), 52, dtype, scale=960 ** -0.5)
    got = K.linear_bf16(xd1, wd, None, None, 1.0, tile=tile, x2=xd2)
    assert rel_inf(got.float(), F.linear(torch.cat([xo1, xo2], -1), wo)) < 1e-2
    # GEGLU
    M, Kd = 4100, 1280
    go, gd = rnd((2048, Kd), 42, dtype, scale=Kd ** -0.5)
    gbo, gbd = rnd((2048,), 40, dtype)
    xo, xd = rnd((M, Kd), 41, dtype)
    wi, bi = interleave_geglu(gd, gbd)
    a, g = F.linear(xo, go, gbo).chunk(2, dim=-1)
    outg = K.linear_bf16(xd, wi, bi, geglu=True, tile=tile)
    assert rel_inf(outg.float(), a * F.gelu(g)) < 1e-2
    # conv loader
    co, cd = rnd((4, 320, 36, 30), 47, dtype)
    fo, fd = rnd((328, 320, 3, 3), 44, dtype, scale=(9 * 320) ** -0.5)
    to, td = rnd((4, 328), 43, dtype)
    ro, rd = rnd((4, 328, 36, 30), 48, dtype)
    x_nhwc, f_cl = cd.permute(0, 2, 3, 1).contiguous(), fd.contiguous(memory_format=torch.channels_last)
    refc = F.conv2d(co, fo, None, 1, 1)
    outc = K.conv3x3_bf16(x_nhwc, f_cl, None, td, None, tile=tile)
    assert rel_inf(outc.permute(0, 3, 1, 2).float(), refc + to[:, :, None, None]) < 1e-2
    outr = K.conv3x3_bf16(x_nhwc, f_cl, None, None, rd.permute(0, 2, 3, 1).contiguous(), tile=tile)
    assert rel_inf(outr.permute(0, 3, 1, 2).float(), refc + ro) < 1e-2
    outu = K.conv3x3_bf16(x_nhwc, f_cl, None, None, None, tile=tile, upsample=True)
    assert rel_inf(outu.permute(0, 3, 1, 2).float(), F.conv2d(F.interpolate(co, scale_factor=2.0, mode="nearest"), fo, None, 1, 1)) < 1e-2
    outs = K.conv3x3_bf16(x_nhwc, f_cl, None, None, None, tile=tile, stride2=True)
    assert rel_inf(outs.permute(0, 3, 1, 2).float(), F.conv2d(co, fo, None, 2, 1)) < 1e-2
    # bench-size conv, sampled check against the plain kernel (bit-identical: same products, same summation order per element)
    co, cd = rnd((8, 640, 20, 32), 53, dtype)
    fo, fd = rnd((640, 640, 3, 3), 54, dtype, scale=(9 * 640) ** -0.5)
    x_nhwc, f_cl = cd.permute(0, 2, 3, 1).contiguous(), fd.contiguous(memory_format=torch.channels_last)
    want = K.conv3x3_bf16(x_nhwc, f_cl, None, None, None, tile=3)
    for it in range(6):
        got = K.conv3x3_bf16(x_nhwc, f_cl, None, None, None, tile=tile)
        assert torch.equal(got, want) if tile < 128 else rel_inf(got.float(), want.float()) < 4e-3          # (stream-K: other summation order)
    if tile >= 128:                            # stream-K: big enough to be cut (>= 4 k-tiles per CU), many launches on fresh data, flags back to zero
        M, N, Kd = 20480, 1280, 1280
        wo, wd = rnd((N, Kd), 60, dtype, scale=Kd ** -0.5)
        for it in range(8):
            xo, xd = rnd((M, Kd), 500 + it, dtype)
            ro, rd = rnd((M, N), 600 + it, dtype)
            got = K.linear_bf16(xd, wd, None, rd, 1.0, tile=tile)
            want = K.linear_bf16(xd, wd, None, rd, 1.0, tile=3)
            assert rel_inf(got.float(), want.float()) < 8e-3, it                  # (one bf16 ulp of the largest output)
            assert torch.equal(got, K.linear_bf16(xd, wd, None, rd, 1.0, tile=tile))                          # deterministic
        ws = K._sk_ws[(torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)]
        assert int(ws[:1024].view(torch.int32).abs().sum()) == 0


@pytest.mark.parametrize("chunks", [2, 3, 5, 7, 16])
def test_gemm_8phase_k_lockstep_split(K, chunks):
    """`split_k = -(16 + S)` on the 8-phase kernel: every tile's reduction cut into S chunks, unit (chunk, tile) -> workgroup so that the CUs of an
    XCD work on the same k-chunk (the filter leaves the Infinity Cache once per XCD), fp32 partials in accumulator layout, `sk_finish_kernel`
    sums them in chunk order and applies the epilogue.  Ragged M / N, chunk lengths that do not divide K / 64 (the last chunk is shorter), more
    units than CUs (several rounds), bias / alpha / temb / one and two residuals, conv loader (plain, upsample, stride 2), the GEGLU form (finished
    by the 8-phase kernel's own epilogue), determinism, repeated launches on fresh data."""
    dtype = torch.bfloat16
    sk = -(16 + chunks)
    for (M, N, Kd) in [(4100, 1032, 1280), (1280, 1280, 5120), (700, 320, 1088), (5120, 1280, 2304)]:
        wo, wd = rnd((N, Kd), 45, dtype, scale=Kd ** -0.5)
        bo, bd = rnd((N,), 46, dtype)
        for it in range(3):
            xo, xd = rnd((M, Kd), 200 + it, dtype)
            ro, rd = rnd((M, N), 300 + it, dtype)
            r2o, r2d = rnd((M, N), 400 + it, dtype)
            got = K.linear_bf16(xd, wd, bd, rd, 0.5, tile=13, split_k=sk)
            assert rel_inf(got.float(), 0.5 * F.linear(xo, wo, bo) + ro) < 1e-2, (M, N, Kd, it)
            assert rel_inf(got.float(), K.linear_bf16(xd, wd, bd, rd, 0.5, tile=13).float()) < 8e-3
            if it == 0:
                assert torch.equal(got, K.linear_bf16(xd, wd, bd, rd, 0.5, tile=13, split_k=sk))                   # deterministic
                got2 = K.linear_bf16(xd, wd, None, rd, 1.0, tile=13, split_k=sk, residual2=r2d)
                assert rel_inf(got2.float(), F.linear(xo, wo) + ro + r2o) < 1e-2
                assert rel_inf(K.linear_bf16(xd, wd, None, None, 1.0, tile=13, split_k=sk).float(), F.linear(xo, wo)) < 1e-2
    from synfmc_amd.models.layers import interleave_geglu
    go, gd = rnd((2048, 1280), 42, dtype, scale=1280 ** -0.5)
    gbo, gbd = rnd((2048,), 40, dtype)
    xo, xd = rnd((1100, 1280), 41, dtype)
    wi, bi = interleave_geglu(gd, gbd)
    a, g = F.linear(xo, go, gbo).chunk(2, dim=-1)
    assert rel_inf(K.linear_bf16(xd, wi, bi, geglu=True, tile=13, split_k=sk).float(), a * F.gelu(g)) < 1e-2
    # conv loader: the 5x8 / 10x16-level shapes the arm is for (reduced image count), temb + residual, upsample, stride 2
    for (n, h, w, cin, cout) in [(4, 5, 8, 1280, 1280), (2, 10, 16, 640, 1288), (3, 10, 16, 1920, 328)]:
        co, cd = rnd((n, cin, h, w), 47, dtype)
        fo, fd = rnd((cout, cin, 3, 3), 44, dtype, scale=(9 * cin) ** -0.5)
        bo, bd = rnd((cout,), 49, dtype)
        to, td = rnd((n, cout), 43, dtype)
        ro, rd = rnd((n, cout, h, w), 48, dtype)
        x_nhwc, f_cl = cd.permute(0, 2, 3, 1).contiguous(), fd.contiguous(memory_format=torch.channels_last)
        refc = F.conv2d(co, fo, bo, 1, 1)
        outc = K.conv3x3_bf16(x_nhwc, f_cl, bd, td, rd.permute(0, 2, 3, 1).contiguous(), tile=13, split_k=sk)
        assert rel_inf(outc.permute(0, 3, 1, 2).float(), refc + to[:, :, None, None] + ro) < 1e-2, (n, h, w, cin, cout)
        outu = K.conv3x3_bf16(x_nhwc, f_cl, None, None, None, tile=13, split_k=sk, upsample=True)
        assert rel_inf(outu.permute(0, 3, 1, 2).float(), F.conv2d(F.interpolate(co, scale_factor=2.0, mode="nearest"), fo, None, 1, 1)) < 1e-2
        if h % 2 == 0:
            outs = K.conv3x3_bf16(x_nhwc, f_cl, None, None, None, tile=13, split_k=sk, stride2=True)
            assert rel_inf(outs.permute(0, 3, 1, 2).float(), F.conv2d(co, fo, None, 2, 1)) < 1e-2


@pytest.mark.parametrize("n,H,W,cin,cout", [(4, 12, 20, 64, 128), (16, 4, 6, 320, 320), (2, 32, 48, 320, 64), (3, 7, 9, 128, 72)])
def test_conv3x3_weight_grad(K, n, H, W, cin, cout):
    """dW of the 3x3 / stride 1 / pad 1 convolution as pixel-reduction GEMMs over the zero-padded, pixel-minor layouts
    (`fmc_nhwc_to_cmajor_padded` + split-K `fmc_linear_bf16`) against autograd through F.conv2d on the same bf16 operands;
    and the trainable-conv autograd node end to end (forward, dX, dW, db)."""
    dtype = torch.bfloat16
    xo, xd = rnd((n, cin, H, W), 80, dtype)
    go, gd = rnd((n, cout, H, W), 81, dtype)
    wo, wd = rnd((cout, cin, 3, 3), 82, dtype, scale=(9 * cin) ** -0.5)
    wr = wo.clone().requires_grad_(True)
    xr = xo.clone().requires_grad_(True)
    F.conv2d(xr, wr, None, 1, 1).backward(go)
    dw = K.conv3x3_weight_grad(xd.permute(0, 2, 3, 1).contiguous(), gd.permute(0, 2, 3, 1).contiguous())
    assert dw.shape == (cout, cin, 3, 3)
    assert rel_inf(dw.float(), wr.grad) < 1e-2
    if cin % 64 == 0 and cout % 64 == 0:
        bo, bd = rnd((cout,), 83, dtype)
        x_cl = xd.contiguous(memory_format=torch.channels_last).requires_grad_(True)
        w32, b32 = wd.float().requires_grad_(True), bd.float().requires_grad_(True)
        y = K.conv3x3_trainable(x_cl, w32, b32)
        br = bo.clone().requires_grad_(True)
        xr.grad = wr.grad = None
        yr = F.conv2d(xr, wr, br, 1, 1)
        assert rel_inf(y.float(), yr) < 1e-2
        y.backward(gd.contiguous(memory_format=torch.channels_last))
        yr.backward(go)
        assert rel_inf(x_cl.grad.float(), xr.grad) < 1e-2
        assert rel_inf(w32.grad, wr.grad) < 1e-2
        assert rel_inf(b32.grad, br.grad) < 1e-2


def test_linear_bf16_geglu(K):
    dtype = torch.bfloat16
    M, C, Cff = 513, 320, 1280
    xo, xd = rnd((M, C), 64, dtype)
    wo, wd = rnd((2 * Cff, C), 65, dtype, scale=C ** -0.5)
    bo, bd = rnd((2 * Cff,), 66, dtype)
    a, g = F.linear(xo, wo, bo).chunk(2, dim=-1)
    ref = a * F.gelu(g)
    from synfmc_amd.models.layers import interleave_geglu
    wi, bi = interleave_geglu(wd, bd)
    out = K.linear_bf16(xd, wi, bi, geglu=True)
    assert out.shape == (M, Cff)
    assert rel_inf(out.float(), ref) < 1e-2


@pytest.mark.parametrize("n,H,W,cin,cout,temb,res", [(2, 10, 16, 320, 320, True, True), (3, 9, 7, 640, 320, False, False),
                                                     (1, 40, 64, 320, 320, True, False), (2, 5, 8, 1280, 1280, True, True),
                                                     (2, 12, 12, 64, 136, False, True)])
def test_conv3x3_bf16_fused_epilogue(K, n, H, W, cin, cout, temb, res):
    dtype = torch.bfloat16
    xo, xd = rnd((n, cin, H, W), 70, dtype)
    wo, wd = rnd((cout, cin, 3, 3), 71, dtype, scale=(9 * cin) ** -0.5)
    bo, bd = rnd((cout,), 72, dtype)
    to, td = rnd((n, cout), 73, dtype)
    ro, rd = rnd((n, cout, H, W), 74, dtype)
    ref = F.conv2d(xo, wo, bo, 1, 1)
    if temb:
        ref = ref + to[:, :, None, None]
    if res:
        ref = ref + ro
    out = K.conv3x3_bf16(xd.permute(0, 2, 3, 1).contiguous(), wd.contiguous(memory_format=torch.channels_last), bd,
                         td if temb else None, rd.permute(0, 2, 3, 1).contiguous() if res else None)
    assert rel_inf(out.permute(0, 3, 1, 2).float(), ref) < 1e-2


@pytest.mark.parametrize("tile", [0, 1, 3, 11, 128 + 2])
def test_conv3x3_bf16_fused_upsample(K, tile):
    """diffusers Upsample2D: nearest 2x then 3x3 conv; the kernel reads the half-resolution source directly"""
    dtype = torch.bfloat16
    n, cin, cout, h, w = 3, 128, 320, 10, 14
    xo, xd = rnd((n, cin, h, w), 75, dtype)
    wo, wd = rnd((cout, cin, 3, 3), 76, dtype, scale=(9 * cin) ** -0.5)
    bo, bd = rnd((cout,), 77, dtype)
    ref = F.conv2d(F.interpolate(xo, scale_factor=2.0, mode="nearest"), wo, bo, 1, 1)
    out = K.conv3x3_bf16(xd.permute(0, 2, 3, 1).contiguous(), wd.contiguous(memory_format=torch.channels_last), bd,
                         None, None, tile=tile, upsample=True)
    assert out.shape == (n, 2 * h, 2 * w, cout)
    assert rel_inf(out.permute(0, 3, 1, 2).float(), ref) < 1e-2


@pytest.mark.parametrize("tile", [0, 2, 5, 11])
def test_conv3x3_bf16_stride2(K, tile):
    """diffusers Downsample2D: 3x3, stride 2, pad 1"""
    dtype = torch.bfloat16
    n, cin, cout, h, w = 3, 128, 320, 20, 28
    xo, xd = rnd((n, cin, h, w), 78, dtype)
    wo, wd = rnd((cout, cin, 3, 3), 79, dtype, scale=(9 * cin) ** -0.5)
    bo, bd = rnd((cout,), 80, dtype)
    ref = F.conv2d(xo, wo, bo, 2, 1)
    out = K.conv3x3_bf16(xd.permute(0, 2, 3, 1).contiguous(), wd.contiguous(memory_format=torch.channels_last), bd,
                         None, None, tile=tile, stride2=True)
    assert out.shape == (n, h // 2, w // 2, cout)
    assert rel_inf(out.permute(0, 3, 1, 2).float(), ref) < 1e-2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,HW,C1,C2", [(2, 2560, 320, 320), (3, 160, 1280, 640), (2, 40, 1280, 1280), (2, 640, 640, 320)])
def test_groupnorm_two_source_concat(K, dtype, N, HW, C1, C2):
    """up-block ResNet input: GroupNorm(+SiLU) of cat([hidden, skip], channels) with the concat never materialised
    (two-pass kernels at 40x64, single-pass kernel at the smaller levels)"""
    xo, xd = rnd((N, HW, C1), 90, dtype, scale=1.3, shift=0.2)
    so, sd = rnd((N, HW, C2), 91, dtype, scale=0.7, shift=-0.4)
    go, gd = rnd((C1 + C2,), 92, torch.float32)
    bo, bd = rnd((C1 + C2,), 93, torch.float32)
    cat = torch.cat([xo, so], dim=-1)
    ref = F.silu(F.group_norm(cat.permute(0, 2, 1), 32, go, bo, 1e-5)).permute(0, 2, 1)
    out = K.groupnorm_silu(xd, gd, bd, 32, 1e-5, True, x2=sd)
    assert out.shape == (N, HW, C1 + C2) and rel_inf(out.float(), ref) < TOL[dtype] * (5 if dtype == torch.float32 else 1)
    assert torch.equal(out, K.groupnorm_silu(torch.cat([xd, sd], dim=-1), gd, bd, 32, 1e-5, True))


@pytest.mark.parametrize("tile", [0, 1, 3, 5, 11, 128 + 2])
def test_linear_two_source_concat(K, tile):
    """1x1 shortcut conv of an up-block ResNet: x @ W^T with x = cat([hidden, skip]) read from the two tensors"""
    dtype = torch.bfloat16
    M, K1, K2, N = 1000, 640, 320, 328
    xo, xd = rnd((M, K1), 94, dtype)
    so, sd = rnd((M, K2), 95, dtype)
    wo, wd = rnd((N, K1 + K2), 96, dtype, scale=(K1 + K2) ** -0.5)
    bo, bd = rnd((N,), 97, dtype)
    ref = F.linear(torch.cat([xo, so], -1), wo, bo)
    out = K.linear_bf16(xd, wd, bd, None, 1.0, tile=tile, x2=sd)
    assert rel_inf(out.float(), ref) < 1e-2
    if tile < 128:
        assert torch.equal(out, K.linear_bf16(torch.cat([xd, sd], -1), wd, bd, None, 1.0, tile=tile))


# ---------------------------------------------------------------------------------------------
# backward kernels vs autograd through the oracle's forward (fp32 CPU)
# ---------------------------------------------------------------------------------------------
GTOL = {torch.float32: 1e-4, torch.bfloat16: 3e-2}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [64, 320, 1280])
def test_layernorm_backward(K, dtype, C):
    xo, xd = rnd((3, 16, 7, C), 80, dtype, scale=1.5, shift=0.3)
    do, dd = rnd((3, 16, 7, C), 81, dtype)
    g = torch.Generator().manual_seed(82)
    gamma, beta = torch.randn(C, generator=g).requires_grad_(True), torch.randn(C, generator=g).requires_grad_(True)
    xr = xo.clone().requires_grad_(True)
    F.layer_norm(xr, (C,), gamma, beta, 1e-5).backward(do)
    gd, bd_ = gamma.detach().cuda().requires_grad_(True), beta.detach().cuda().requires_grad_(True)
    xg = xd.clone().requires_grad_(True)
    K.layernorm(xg, gd, bd_, 1e-5).backward(dd)
    assert rel_inf(xg.grad.float(), xr.grad) < GTOL[dtype]
    assert rel_inf(gd.grad, gamma.grad) < GTOL[dtype] and rel_inf(bd_.grad, beta.grad) < GTOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_geglu_backward(K, dtype):
    xo, xd = rnd((5, 33, 2 * 640), 83, dtype, scale=1.5)
    do, dd = rnd((5, 33, 640), 84, dtype)
    xr = xo.clone().requires_grad_(True)
    a, g = xr.chunk(2, dim=-1)
    (a * F.gelu(g)).backward(do)
    xg = xd.clone().requires_grad_(True)
    K.geglu(xg).backward(dd)
    assert rel_inf(xg.grad.float(), xr.grad) < GTOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,H,D", [(2, 160, 8, 40), (1, 200, 8, 80), (2, 70, 8, 160), (1, 300, 4, 8)])
def test_spatial_attention_backward_self(K, dtype, B, S, H, D):
    C = H * D
    qkvo, qkvd = rnd((B, S, 3 * C), 85, dtype)
    do, dd = rnd((B, S, C), 86, dtype)
    xr = qkvo.clone().requires_grad_(True)
    oracle_attention(xr[..., :C], xr[..., C:2 * C], xr[..., 2 * C:], H).backward(do)
    xg = qkvd.clone().requires_grad_(True)
    K.spatial_attention(xg[..., :C], xg[..., C:2 * C], xg[..., 2 * C:], H).backward(dd)
    assert rel_inf(xg.grad.float(), xr.grad) < GTOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_spatial_attention_backward_cross_shared_text(K, dtype):
    B, Fr, S, H, D = 2, 3, 100, 8, 40
    C = H * D
    qo, qd = rnd((B * Fr, S, C), 87, dtype)
    kvo, kvd = rnd((B, 77, 2 * C), 88, dtype)
    do, dd = rnd((B * Fr, S, C), 89, dtype)
    qr, kvr = qo.clone().requires_grad_(True), kvo.clone().requires_grad_(True)
    rep = kvr.repeat_interleave(Fr, dim=0)
    oracle_attention(qr, rep[..., :C], rep[..., C:], H).backward(do)
    qg, kvg = qd.clone().requires_grad_(True), kvd.clone().requires_grad_(True)
    K.spatial_attention(qg, kvg[..., :C], kvg[..., C:], H).backward(dd)
    assert rel_inf(qg.grad.float(), qr.grad) < GTOL[dtype]
    assert rel_inf(kvg.grad.float(), kvr.grad) < GTOL[dtype]          # summed over the F frames of each clip


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("clips,kv_grad", [(1, True), (2, True), (1, False)])
def test_cross_attention_fused_kv_backward(K, dtype, clips, kv_grad):
    """Fused K|V projection: one clip = per-frame partial dK|dV summed afterwards, several clips = summed inside the
    kernel, frozen K/V (the FMC training stages) = no dK/dV kernel; dQ identical in all three."""
    Fr, S, H, D = 4, 130, 8, 40
    C = H * D
    qo, qd = rnd((clips * Fr, S, C), 187, dtype)
    kvo, kvd = rnd((clips, 77, 2 * C), 188, dtype)
    do, dd = rnd((clips * Fr, S, C), 189, dtype)
    qr, kvr = qo.clone().requires_grad_(True), kvo.clone().requires_grad_(True)
    rep = kvr.repeat_interleave(Fr, dim=0)
    oracle_attention(qr, rep[..., :C], rep[..., C:], H).backward(do)
    qg, kvg = qd.clone().requires_grad_(True), kvd.clone().requires_grad_(kv_grad)
    K.cross_attention_q_kv(qg, kvg, H, D ** -0.5).backward(dd)
    assert rel_inf(qg.grad.float(), qr.grad) < GTOL[dtype]
    if kv_grad:
        assert rel_inf(kvg.grad.float(), kvr.grad) < GTOL[dtype]
    else:
        assert kvg.grad is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,Fr,P,H,D", [(2, 16, 6, 8, 40), (1, 16, 5, 8, 160), (1, 32, 3, 8, 80), (2, 16, 4, 4, 8)])
def test_temporal_attention_backward(K, dtype, B, Fr, P, H, D):
    C = H * D
    qkvo, qkvd = rnd((B, Fr, P, 3 * C), 90, dtype)
    do, dd = rnd((B, Fr, P, C), 91, dtype)
    xr = qkvo.clone().requires_grad_(True)
    ref_in = xr.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
    out = oracle_attention(ref_in[..., :C], ref_in[..., C:2 * C], ref_in[..., 2 * C:], H)
    out.backward(do.permute(0, 2, 1, 3).reshape(B * P, Fr, C))
    xg = qkvd.clone().requires_grad_(True)
    K.temporal_attention(xg[..., :C], xg[..., C:2 * C], xg[..., 2 * C:], H).backward(dd)
    assert rel_inf(xg.grad.float(), xr.grad) < GTOL[dtype]


def test_gaussian_circle_masks_match_oracle(K):
    """dataset.py:5365-5380 analytic mask: float centres (incl. off-image and x.5 ties), truncated disc radius."""
    from oracle import conditioning as OC
    from synfmc_amd.data.dataset import gaussian_circle_masks
    H, W = 96, 136
    rng = np.random.default_rng(7)
    circ = np.concatenate([rng.uniform([0, 0, 4], [W, H, 50], size=(20, 3)),
                           [[10.5, 20.5, 7.9], [-3.2, 5.0, 12.0], [W + 4.0, H - 1.0, 30.0], [50.0, 40.0, 1.0]]])
    out = gaussian_circle_masks(circ.reshape(4, 6, 3), H, W)
    assert out.shape == (4, 6, H, W) and out.dtype == torch.float32
    ref = np.stack([OC.gaussian_circle_mask(H, W, c[:2], c[2]) for c in circ]).reshape(4, 6, H, W)
    assert np.abs(out.cpu().numpy() - ref).max() < 2e-6
    assert ((out.cpu().numpy() > 0) == (ref > 0)).all()


# ---------------------------------------------------------------------------------------------
# fp32-storage ("parity") mode of the GEMM / conv kernels: split-bf16 x3 operands on the SAME tile maps, loaders and fragment
# layouts (fmc_split_bf16x3, fmc_linear_x3_f32, fmc_conv3x3_x3_f32), checked element by element against an fp64 reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6, 7, 11, 13, 1 + 16, 2 + 32])
def test_linear_f32_split3(K, tile):
    g = torch.Generator().manual_seed(900)
    for (M, N, Kd) in [(777, 328, 320), (4100, 1032, 1280), (130, 64, 64)]:
        x, w = torch.randn(M, Kd, generator=g), torch.randn(N, Kd, generator=g) * Kd ** -0.5
        b, r, r2 = torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
        mag = x.abs().double() @ w.abs().double().t()
        ref = F.linear(x.double(), w.double())
        xd, wd, bd, rd, r2d = x.cuda(), w.cuda(), b.cuda(), r.cuda(), r2.cuda()
        got = K.linear_f32(xd, wd, None, None, 1.0, tile=tile)
        assert got.dtype == torch.float32
        assert_f32_close(got, ref, mag, f"plain {tile} {(M, N, Kd)}")
        got = K.linear_f32(xd, wd, bd, rd, 0.5, tile=tile)
        assert_f32_close(got, 0.5 * (ref + b.double()) + r.double(), 0.5 * (mag + b.abs()) + r.abs(), f"bias+res {tile}")
        got = K.linear_f32(xd, wd, None, rd, 0.7, tile=tile, residual2=r2d)
        assert_f32_close(got, 0.7 * ref + r.double() + r2.double(), 0.7 * mag + r.abs() + r2.abs(), f"two residuals {tile}")
        # strided rows (a column slice of a wider matrix)
        wide = torch.cat([xd, xd], dim=1)
        assert torch.equal(K.linear_f32(wide[:, Kd:], wd, None, None, 1.0, tile=tile), K.linear_f32(xd, wd, None, None, 1.0, tile=tile))
    # two-source operand
    x1, x2 = torch.randn(900, 640, generator=g), torch.randn(900, 320, generator=g)
    w = torch.randn(640, 960, generator=g) * 960 ** -0.5
    xc = torch.cat([x1, x2], -1)
    got = K.linear_f32(x1.cuda(), w.cuda(), None, None, 1.0, tile=tile, x2=x2.cuda())
    assert_f32_close(got, F.linear(xc.double(), w.double()), xc.abs().double() @ w.abs().double().t(), f"two-source {tile}")
    if tile < 16:                                             # GEGLU (no split-K)
        from synfmc_amd.models.layers import interleave_geglu
        x = torch.randn(1000, 320, generator=g)
        w, b = torch.randn(512, 320, generator=g) * 320 ** -0.5, torch.randn(512, generator=g)
        wi, bi = interleave_geglu(w.cuda(), b.cuda())
        a, gt = F.linear(x.double(), w.double(), b.double()).chunk(2, dim=-1)
        ma, mg = (x.abs().double() @ w.abs().double().t() + b.abs()).chunk(2, dim=-1)
        got = K.linear_f32(x.cuda(), wi, bi, geglu=True, tile=tile)
        # d(a gelu(g)) <= |gelu(g)| da + |a| |gelu'| dg, |gelu'| <= 1.13
        bound_mag = F.gelu(gt).abs() * ma + 1.13 * a.abs() * mg + 1e-3
        assert_f32_close(got, a * F.gelu(gt), bound_mag, f"geglu {tile}")


@pytest.mark.parametrize("tile", [0, 1, 3, 5, 11, 13, 2 + 16])
def test_conv3x3_f32_split3(K, tile):
    g = torch.Generator().manual_seed(901)
    x = torch.randn(4, 320, 18, 14, generator=g)
    w = torch.randn(328, 320, 3, 3, generator=g) * (9 * 320) ** -0.5
    b, t, r = torch.randn(328, generator=g), torch.randn(2, 328, generator=g), torch.randn(4, 328, 18, 14, generator=g)
    xd = x.cuda().permute(0, 2, 3, 1).contiguous()
    wd = w.cuda().contiguous(memory_format=torch.channels_last)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    mag = F.conv2d(x.abs().double(), w.abs().double(), None, 1, 1)
    got = K.conv3x3_f32(xd, wd, None, None, None, tile=tile)
    assert_f32_close(got.permute(0, 3, 1, 2), ref, mag, f"conv {tile}")
    got = K.conv3x3_f32(xd, wd, b.cuda(), t.cuda(), r.cuda().permute(0, 2, 3, 1).contiguous(), tile=tile, temb_div=2)
    tt = t.repeat_interleave(2, dim=0)[:, :, None, None].double()
    assert_f32_close(got.permute(0, 3, 1, 2), ref + b.double()[None, :, None, None] + tt + r.double(),
                     mag + b.abs()[None, :, None, None] + tt.abs() + r.abs(), f"conv + bias + temb + residual {tile}")
    got = K.conv3x3_f32(xd, wd, None, None, None, tile=tile, upsample=True)
    xu = F.interpolate(x, scale_factor=2.0, mode="nearest")
    assert_f32_close(got.permute(0, 3, 1, 2), F.conv2d(xu.double(), w.double(), None, 1, 1),
                     F.conv2d(xu.abs().double(), w.abs().double(), None, 1, 1), f"conv upsample {tile}")
    got = K.conv3x3_f32(xd, wd, None, None, None, tile=tile, stride2=True)
    assert_f32_close(got.permute(0, 3, 1, 2), F.conv2d(x.double(), w.double(), None, 2, 1),
                     F.conv2d(x.abs().double(), w.abs().double(), None, 2, 1), f"conv stride 2 {tile}")


def test_f32_front_ends_take_the_split3_path(K):
    """`hip_ops.linear` / `conv3x3` / `geglu_linear` on fp32 tensors run the gfx950 kernels (not F.linear / F.conv2d): results
    equal the explicit split-bf16 x3 calls bit for bit."""
    g = torch.Generator().manual_seed(902)
    x, w, b = torch.randn(2, 300, 320, generator=g).cuda(), (torch.randn(640, 320, generator=g) * 0.05).cuda(), torch.randn(640, generator=g).cuda()
    r = torch.randn(2, 300, 640, generator=g).cuda()
    assert torch.equal(K.linear(x, w, b, r, 0.5), K.linear_f32(x, w, b, r, 0.5))
    xc = torch.randn(2, 64, 9, 7, generator=g).cuda().contiguous(memory_format=torch.channels_last)
    wc = (torch.randn(72, 64, 3, 3, generator=g) * 0.05).cuda().contiguous(memory_format=torch.channels_last)
    got = K.conv3x3(xc, wc, None)
    assert torch.equal(got, K.conv3x3_f32(xc.permute(0, 2, 3, 1), wc).permute(0, 3, 1, 2))
    assert rel_inf(got, F.conv2d(xc.cpu().double(), wc.cpu().double(), None, 1, 1)) < 1e-5


# ---------------------------------------------------------------------------------------------
# arm 16: 160 x 320 tiles on the 8-phase schedule (16x16x32 MFMA)
# ---------------------------------------------------------------------------------------------
def test_gemm_160x320_arm(K):
    """Ragged M (partial last tile), 1 / 2 / 3 / 8 column tiles, K from one k-tile up, every epilogue (bias, alpha, one / two
    residuals, GEGLU with the [8 value | 8 gate] row order), the conv loader (plain, + temb, + residual, upsample, stride 2),
    the fp32-storage mode, determinism, repeated launches on fresh data (a racy schedule shows as rare wrong tiles), and the
    fall-back when N is not a multiple of 320."""
    dtype = torch.bfloat16
    from synfmc_amd.models.layers import interleave_geglu
    for (M, N, Kd) in [(777, 320, 320), (4100, 640, 1280), (160, 320, 64), (8000, 960, 320), (2560, 2560, 640), (20480, 640, 640)]:
        wo, wd = rnd((N, Kd), 45, dtype, scale=Kd ** -0.5)
        bo, bd = rnd((N,), 46, dtype)
        for it in range(3):
            xo, xd = rnd((M, Kd), 700 + it, dtype)
            ro, rd = rnd((M, N), 800 + it, dtype)
            got = K.linear_bf16(xd, wd, bd, rd, 0.5, tile=512)
            ref = 0.5 * F.linear(xo.double(), wo.double(), bo.double()) + ro.double()
            mag = 0.5 * (xo.abs().double() @ wo.abs().double().t() + bo.abs()) + ro.abs()
            assert_bf16_close(got, ref, mag, f"arm 16 {(M, N, Kd)} it {it}")
            if it == 0:
                assert torch.equal(got, K.linear_bf16(xd, wd, bd, rd, 0.5, tile=512))                       # deterministic
                r2o, r2d = rnd((M, N), 900, dtype)
                got2 = K.linear_bf16(xd, wd, None, rd, 1.0, tile=512, residual2=r2d)
                assert_bf16_close(got2, F.linear(xo.double(), wo.double()) + ro.double() + r2o.double(),
                                  xo.abs().double() @ wo.abs().double().t() + ro.abs() + r2o.abs(), "arm 16 two residuals")
                got0 = K.linear_bf16(xd, wd, bd, None, 1.0, tile=512)
                assert_bf16_close(got0, F.linear(xo.double(), wo.double(), bo.double()), xo.abs().double() @ wo.abs().double().t() + bo.abs(),
                                  "arm 16 bias only")
    # N not a multiple of 320: falls back to the 8-phase 256 x 256 kernel (same function)
    xo, xd = rnd((700, 320), 41, dtype)
    wo, wd = rnd((328, 320), 42, dtype, scale=320 ** -0.5)
    assert torch.equal(K.linear_bf16(xd, wd, None, None, 1.0, tile=512), K.linear_bf16(xd, wd, None, None, 1.0, tile=13))
    # GEGLU
    for (M, N, Kd) in [(4100, 2560, 320), (1000, 640, 640)]:
        go, gd = rnd((N, Kd), 42, dtype, scale=Kd ** -0.5)
        gbo, gbd = rnd((N,), 40, dtype)
        xo, xd = rnd((M, Kd), 41, dtype)
        wi, bi = interleave_geglu(gd, gbd, 8)
        a, g = F.linear(xo.double(), go.double(), gbo.double()).chunk(2, dim=-1)
        ma, mg = (xo.abs().double() @ go.abs().double().t() + gbo.abs()).chunk(2, dim=-1)
        outg = K.linear_bf16(xd, wi, bi, geglu=True, tile=512)
        assert_bf16_close(outg, a * F.gelu(g), F.gelu(g).abs() * ma + 1.13 * a.abs() * mg + 1e-3, f"arm 16 geglu {(M, N, Kd)}")
        wi32, bi32 = interleave_geglu(gd, gbd)
        assert rel_inf(outg.float(), K.linear_bf16(xd, wi32, bi32, geglu=True, tile=3).float()) < 8e-3      # (one bf16 ulp of the largest output)
    # conv loader
    co, cd = rnd((4, 320, 36, 30), 47, dtype)
    fo, fd = rnd((320, 320, 3, 3), 44, dtype, scale=(9 * 320) ** -0.5)
    to, td = rnd((4, 320), 43, dtype)
    ro, rd = rnd((4, 320, 36, 30), 48, dtype)
    x_nhwc, f_cl = cd.permute(0, 2, 3, 1).contiguous(), fd.contiguous(memory_format=torch.channels_last)
    refc = F.conv2d(co.double(), fo.double(), None, 1, 1)
    magc = F.conv2d(co.abs().double(), fo.abs().double(), None, 1, 1)
    outc = K.conv3x3_bf16(x_nhwc, f_cl, None, td, None, tile=512)
    assert_bf16_close(outc.permute(0, 3, 1, 2), refc + to.double()[:, :, None, None], magc + to.abs()[:, :, None, None], "arm 16 conv + temb")
    outr = K.conv3x3_bf16(x_nhwc, f_cl, None, None, rd.permute(0, 2, 3, 1).contiguous(), tile=512)
    assert_bf16_close(outr.permute(0, 3, 1, 2), refc + ro.double(), magc + ro.abs(), "arm 16 conv + residual")
    xu = F.interpolate(co, scale_factor=2.0, mode="nearest")
    outu = K.conv3x3_bf16(x_nhwc, f_cl, None, None, None, tile=512, upsample=True)
    assert_bf16_close(outu.permute(0, 3, 1, 2), F.conv2d(xu.double(), fo.double(), None, 1, 1), F.conv2d(xu.abs().double(), fo.abs().double(), None, 1, 1),
                      "arm 16 conv upsample")
    outs = K.conv3x3_bf16(x_nhwc, f_cl, None, None, None, tile=512, stride2=True)
    assert_bf16_close(outs.permute(0, 3, 1, 2), F.conv2d(co.double(), fo.double(), None, 2, 1), F.conv2d(co.abs().double(), fo.abs().double(), None, 2, 1),
                      "arm 16 conv stride 2")
    # bench-size conv against the plain kernel, many launches
    co, cd = rnd((8, 640, 20, 32), 53, dtype)
    fo, fd = rnd((640, 640, 3, 3), 54, dtype, scale=(9 * 640) ** -0.5)
    x_nhwc, f_cl = cd.permute(0, 2, 3, 1).contiguous(), fd.contiguous(memory_format=torch.channels_last)
    want = K.conv3x3_bf16(x_nhwc, f_cl, None, None, None, tile=3)
    first = K.conv3x3_bf16(x_nhwc, f_cl, None, None, None, tile=512)
    assert rel_inf(first.float(), want.float()) < 8e-3
    for it in range(8):
        assert torch.equal(K.conv3x3_bf16(x_nhwc, f_cl, None, None, None, tile=512), first)
    # fp32-storage mode
    g = torch.Generator().manual_seed(903)
    x, w = torch.randn(777, 320, generator=g), torch.randn(640, 320, generator=g) * 320 ** -0.5
    b, r = torch.randn(640, generator=g), torch.randn(777, 640, generator=g)
    got = K.linear_f32(x.cuda(), w.cuda(), b.cuda(), r.cuda(), 0.5, tile=512)
    assert_f32_close(got, 0.5 * (F.linear(x.double(), w.double()) + b.double()) + r.double(),
                     0.5 * (x.abs().double() @ w.abs().double().t() + b.abs()) + r.abs(), "arm 16 fp32")
    gw, gb = torch.randn(640, 320, generator=g) * 320 ** -0.5, torch.randn(640, generator=g)
    wi, bi = interleave_geglu(gw.cuda(), gb.cuda(), 8)
    a, gt = F.linear(x.double(), gw.double(), gb.double()).chunk(2, dim=-1)
    ma, mg = (x.abs().double() @ gw.abs().double().t() + gb.abs()).chunk(2, dim=-1)
    got = K.linear_f32(x.cuda(), wi, bi, geglu=True, tile=512)
    assert_f32_close(got, a * F.gelu(gt), F.gelu(gt).abs() * ma + 1.13 * a.abs() * mg + 1e-3, "arm 16 fp32 geglu")


def test_gemm_160x320_persistent_form(K):
    """More 160 x 320 tiles than CUs on a token projection: arm 512 runs gemm160p_kernel (one workgroup per CU walks the tiles, the next
    tile's operands stream in under the epilogue; exact-count stores around the counted vmcnt).  Every epilogue, several launches on fresh
    data, against an fp64 reference element by element and against the 8-phase arm."""
    dtype = torch.bfloat16
    from synfmc_amd.models.layers import interleave_geglu
    for (M, N, Kd) in [(81920, 320, 320), (41600, 640, 320), (48000, 960, 640), (81920, 320, 1280)]:
        wo, wd = rnd((N, Kd), 45, dtype, scale=Kd ** -0.5)
        bo, bd = rnd((N,), 46, dtype)
        for it in range(3):
            xo, xd = rnd((M, Kd), 710 + it, dtype)
            ro, rd = rnd((M, N), 810 + it, dtype)
            got = K.linear_bf16(xd, wd, bd, rd, 0.5, tile=512)
            ref = 0.5 * F.linear(xo.double(), wo.double(), bo.double()) + ro.double()
            mag = 0.5 * (xo.abs().double() @ wo.abs().double().t() + bo.abs()) + ro.abs()
            assert_bf16_close(got, ref, mag, f"persistent {(M, N, Kd)} it {it}")
            assert torch.equal(got, K.linear_bf16(xd, wd, bd, rd, 0.5, tile=512))
            if it == 0:
                r2o, r2d = rnd((M, N), 910, dtype)
                got2 = K.linear_bf16(xd, wd, None, rd, 1.0, tile=512, residual2=r2d)
                assert_bf16_close(got2, F.linear(xo.double(), wo.double()) + ro.double() + r2o.double(),
                                  xo.abs().double() @ wo.abs().double().t() + ro.abs() + r2o.abs(), "persistent, two residuals")
                got0 = K.linear_bf16(xd, wd, None, None, 1.0, tile=512)
                assert rel_inf(got0.float(), K.linear_bf16(xd, wd, None, None, 1.0, tile=13).float()) < 8e-3
    for (M, N, Kd) in [(48000, 2560, 320), (20480, 5120, 640)]:
        go, gd = rnd((N, Kd), 42, dtype, scale=Kd ** -0.5)
        gbo, gbd = rnd((N,), 40, dtype)
        wi, bi = interleave_geglu(gd, gbd, 8)
        wi32, bi32 = interleave_geglu(gd, gbd)
        for it in range(3):
            xo, xd = rnd((M, Kd), 720 + it, dtype)
            outg = K.linear_bf16(xd, wi, bi, geglu=True, tile=512)
            assert torch.equal(outg, K.linear_bf16(xd, wi, bi, geglu=True, tile=512))
            assert rel_inf(outg.float(), K.linear_bf16(xd, wi32, bi32, geglu=True, tile=3).float()) < 8e-3
            if it == 0:
                a, g = F.linear(xo.double(), go.double(), gbo.double()).chunk(2, dim=-1)
                ma, mg = (xo.abs().double() @ go.abs().double().t() + gbo.abs()).chunk(2, dim=-1)
                assert_bf16_close(outg, a * F.gelu(g), F.gelu(g).abs() * ma + 1.13 * a.abs() * mg + 1e-3, f"persistent geglu {(M, N, Kd)}")


@pytest.mark.parametrize("tile", [513, 514, 515, 545, 546, 547])
def test_gemm_160x320_split_k(K, tile):
    """Arm 512 + log2(split): the 160 x 320 kernel writes fp32 partial sums of 2 / 4 / 8 k ranges, splitk_reduce_kernel finishes (the
    5x8-level shapes: 32 tiles cannot fill 256 CUs)."""
    dtype = torch.bfloat16
    for (M, N, Kd) in [(1280, 1280, 2560), (1300, 640, 1280), (160, 320, 64)]:
        xo, xd = rnd((M, Kd), 730, dtype)
        wo, wd = rnd((N, Kd), 731, dtype, scale=Kd ** -0.5)
        bo, bd = rnd((N,), 732, dtype)
        ro, rd = rnd((M, N), 733, dtype)
        got = K.linear_bf16(xd, wd, bd, rd, 0.5, tile=tile)
        assert_bf16_close(got, 0.5 * F.linear(xo.double(), wo.double(), bo.double()) + ro.double(),
                          0.5 * (xo.abs().double() @ wo.abs().double().t() + bo.abs()) + ro.abs(), f"split-K arm {tile} {(M, N, Kd)}")
        assert torch.equal(got, K.linear_bf16(xd, wd, bd, rd, 0.5, tile=tile))
    co, cd = rnd((32, 1280, 5, 8), 734, dtype)
    fo, fd = rnd((1280, 1280, 3, 3), 735, dtype, scale=(9 * 1280) ** -0.5)
    to, td = rnd((32, 1280), 736, dtype)
    ro, rd = rnd((32, 1280, 5, 8), 737, dtype)
    x_nhwc, f_cl = cd.permute(0, 2, 3, 1).contiguous(), fd.contiguous(memory_format=torch.channels_last)
    got = K.conv3x3_bf16(x_nhwc, f_cl, None, td, rd.permute(0, 2, 3, 1).contiguous(), tile=tile)
    ref = F.conv2d(co.double(), fo.double(), None, 1, 1) + to.double()[:, :, None, None] + ro.double()
    mag = F.conv2d(co.abs().double(), fo.abs().double(), None, 1, 1) + to.abs()[:, :, None, None] + ro.abs()
    assert_bf16_close(got.permute(0, 3, 1, 2), ref, mag, f"split-K arm {tile} conv 5x8")


@torch.no_grad()
def test_groupnorm_statistics_from_the_producing_epilogue(K):
    """f1: the 160 x 320 kernels (plain grid: conv; persistent: token projection with residual) emit per-(image, tile, group) sums of
    their rounded outputs; `fmc_groupnorm_apply_fwd` normalises with them.  Same result as the two-pass GroupNorm on the same tensor
    (to the last bf16 ulp: other fp32 partial-sum order), and vs the fp32 oracle."""
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(950)
    gamma, beta = (torch.randn(320, generator=g) + 1.0).cuda(), torch.randn(320, generator=g).cuda()
    # conv producer: 8 images of 40 x 64, 320 -> 320, + temb, + residual
    co, cd = rnd((8, 320, 40, 64), 951, dtype)
    fo, fd = rnd((320, 320, 3, 3), 952, dtype, scale=(9 * 320) ** -0.5)
    ro, rd = rnd((8, 320, 40, 64), 953, dtype)
    x_cl, f_cl, r_cl = cd.contiguous(memory_format=torch.channels_last), fd.contiguous(memory_format=torch.channels_last), rd.contiguous(memory_format=torch.channels_last)
    before = dict(K.gn_epilogue_calls)
    y = K.conv3x3(x_cl, f_cl, None, None, r_cl, emit_gn=True)
    assert K.gn_epilogue_calls["emitted"] == before["emitted"] + 1 and getattr(y, "_fmc_gn", None) is not None
    plain = K.conv3x3_bf16(x_cl.permute(0, 2, 3, 1), f_cl, None, None, r_cl.permute(0, 2, 3, 1), tile=512)
    assert torch.equal(y.permute(0, 2, 3, 1), plain)                                      # the emission does not change the output
    tok = y.permute(0, 2, 3, 1).reshape(8, 2560, 320)
    part, C = y._fmc_gn
    # (how a producer cuts an image into partial sums is its own business -- 160-pixel runs, 10 x 32 tiles, 10 x 16 row blocks: the consumer adds them up)
    want_s = tok.float().view(8, 2560, 32, 10).sum(dim=(1, 3))
    want_ss = (tok.float() ** 2).view(8, 2560, 32, 10).sum(dim=(1, 3))
    assert part.shape[0] == 8 and part.shape[2:] == (32, 2) and part.shape[1] <= 64
    assert rel_inf(part[..., 0].sum(1), want_s) < 1e-4 and rel_inf(part[..., 1].sum(1), want_ss) < 1e-5
    for act in (True, False):
        got = K.groupnorm_silu(tok, gamma, beta, 32, 1e-5, act, gn_tag=y._fmc_gn)
        two = K.groupnorm_silu(tok, gamma, beta, 32, 1e-5, act)
        ref = F.group_norm(tok.float().cpu().permute(0, 2, 1), 32, gamma.cpu(), beta.cpu(), 1e-5)
        ref = (F.silu(ref) if act else ref).permute(0, 2, 1)
        assert rel_inf(got.float(), ref) < 1e-2 and rel_inf(got.float(), two.float()) < 4e-3
    assert K.gn_epilogue_calls["consumed"] == before["consumed"] + 2
    # token producer (persistent kernel: 512 tiles), residual + bias
    xo, xd = rnd((32, 2560, 320), 954, dtype)
    wo, wd = rnd((320, 320), 955, dtype, scale=320 ** -0.5)
    bo, bd = rnd((320,), 956, dtype)
    ro, rd = rnd((32, 2560, 320), 957, dtype)
    out = K.linear(xd, wd, bd, rd, 1.0, gn_hw=2560)
    assert getattr(out, "_fmc_gn", None) is not None
    assert torch.equal(out, K.linear_bf16(xd, wd, bd, rd, 1.0, tile=512))
    part = out._fmc_gn[0]
    want_s = out.float().view(32, 16, 160, 32, 10).sum(dim=(2, 4))
    assert part.shape == (32, 16, 32, 2) and rel_inf(part[..., 0], want_s) < 1e-4
    got = K.groupnorm_silu(out, gamma, beta, 32, 1e-6, False, gn_tag=out._fmc_gn)
    assert rel_inf(got.float(), K.groupnorm_silu(out, gamma, beta, 32, 1e-6, False).float()) < 4e-3
    # not eligible (20x32 level: the single-pass GroupNorm reads x once anyway): no tag
    x1, w1 = rnd((8, 640, 640), 958, dtype)[1], rnd((640, 640), 959, dtype, scale=640 ** -0.5)[1]
    assert getattr(K.linear(x1, w1, None, None, 1.0, gn_hw=640), "_fmc_gn", None) is None


def test_linear_backward_data_cache_dies_with_its_weight(K):
    """`linear_frozen`'s backward uses a cached W^T.  The cache lives on the tensor that owns the storage: a second weight of the same
    shape that lands on the freed first one's address must get ITS transpose (a storage-pointer-keyed cache returned the first one's --
    found as a 0.39 rel-inf Adapter gradient late in a long test session), and a fresh `view` of a frozen weight must hit the cache."""
    g = torch.Generator().manual_seed(77)
    dy = torch.randn(256, 128, generator=g).to("cuda", torch.bfloat16)
    ptrs = set()
    for rep in range(4):
        w = (torch.randn(128, 192, generator=g) * 0.1).to("cuda", torch.bfloat16)
        ptrs.add(w.data_ptr())
        got = K.linear_backward_data(dy, w)
        ref = dy.float() @ w.float()
        assert_bf16_close(got.float().cpu(), ref.cpu(), (dy.float().abs() @ w.float().abs()).cpu(), f"rep {rep}")
        del w, got
    assert len(ptrs) < 4, "the allocator never re-used an address: the test did not exercise the stale-cache case"
    w4 = (torch.randn(128, 192, 1, 1, generator=g) * 0.1).to("cuda", torch.bfloat16)
    t0 = K._transposed_weight(w4.view(128, 192))
    assert K._transposed_weight(w4.view(128, 192)) is t0
    w4.mul_(2.0)                                           # a new version of the owner: re-made
    assert torch.equal(K._transposed_weight(w4.view(128, 192)), w4.view(128, 192).t().contiguous())


def test_gemm_256x320_persistent_geglu(K):
    """Arm 528 (C-ABI tile 17): gemm160p_kernel<1, 8> -- persistent 256 x 320 tiles, 5 operand requests and 40 MFMAs per wave and sub-tile,
    GEGLU by half-wave swap, two 128-row passes through the staging tile.  Element-wise against an fp64 reference, bit-equal to the
    160 x 320 arm (same products in the same order per output), deterministic over launches on fresh data; shapes it does not take
    (M % 256 != 0, too few tiles, plain epilogue) must fall back to tile 16 and give the same function."""
    dtype = torch.bfloat16
    from synfmc_amd.models.layers import interleave_geglu
    for (M, N, Kd) in [(81920, 2560, 320), (20480, 5120, 640), (66560, 640, 64)]:
        go, gd = rnd((N, Kd), 42, dtype, scale=Kd ** -0.5)
        gbo, gbd = rnd((N,), 40, dtype)
        wi, bi = interleave_geglu(gd, gbd, 8)
        for it in range(3):
            xo, xd = rnd((M, Kd), 730 + it, dtype)
            outg = K.linear_bf16(xd, wi, bi, geglu=True, tile=K.ARM_256)
            assert torch.equal(outg, K.linear_bf16(xd, wi, bi, geglu=True, tile=K.ARM_256))
            assert torch.equal(outg, K.linear_bf16(xd, wi, bi, geglu=True, tile=K.ARM_160))
            if it == 0:
                a, g = F.linear(xo.double(), go.double(), gbo.double()).chunk(2, dim=-1)
                ma, mg = (xo.abs().double() @ go.abs().double().t() + gbo.abs()).chunk(2, dim=-1)
                assert_bf16_close(outg, a * F.gelu(g), F.gelu(g).abs() * ma + 1.13 * a.abs() * mg + 1e-3, f"256x320 geglu {(M, N, Kd)}")
                outn = K.linear_bf16(xd, wi, None, geglu=True, tile=K.ARM_256)                       # no bias
                a0, g0 = F.linear(xo.double(), go.double()).chunk(2, dim=-1)
                assert_bf16_close(outn, a0 * F.gelu(g0), F.gelu(g0).abs() * ma + 1.13 * a0.abs() * mg + 1e-3, "256x320 geglu, no bias")
    # fall-backs: ragged M, few tiles, plain epilogue
    go, gd = rnd((640, 320), 42, dtype, scale=320 ** -0.5)
    wi, bi = interleave_geglu(gd, None, 8)
    for M in (4100, 2560):
        xo, xd = rnd((M, 320), 41, dtype)
        assert torch.equal(K.linear_bf16(xd, wi, None, geglu=True, tile=K.ARM_256), K.linear_bf16(xd, wi, None, geglu=True, tile=K.ARM_160))
    xo, xd = rnd((81920, 320), 43, dtype)
    assert torch.equal(K.linear_bf16(xd, gd, None, None, 1.0, tile=K.ARM_256), K.linear_bf16(xd, gd, None, None, 1.0, tile=K.ARM_160))


@torch.no_grad()
def test_linear_with_the_consumers_layernorm_in_its_epilogue(K):
    """`fmc_linear_bf16_ln` (persistent 160 x 320 kernel, N == 320): `out` is bit-identical to the plain launch; `ln_out` is the LayerNorm
    (+ positional-encoding row of the tile's frame) of the ROUNDED rows -- element-wise against an fp64 LayerNorm of `out`, and within one
    bf16 ulp of what `fmc_layernorm_fwd` makes of the same tensor.  Several launches on fresh data (exact-count stores around the counted
    vmcnt double with the second output), bias / residual / two residuals, K = 320 and 1280; ineligible shapes carry no tag."""
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(5)
    gamma, beta = (1.0 + 0.3 * torch.randn(320, generator=g)).cuda(), (0.2 * torch.randn(320, generator=g)).cuda()
    pe = torch.randn(32, 320, generator=g).cuda()
    for (M, Kd, frames, inner) in [(81920, 320, 16, 2560), (81920, 1280, 16, 2560), (48000, 320, 3, 16000)]:
        wo, wd = rnd((320, Kd), 45, dtype, scale=Kd ** -0.5)
        bo, bd = rnd((320,), 46, dtype)
        for it in range(3):
            xo, xd = rnd((M, Kd), 740 + it, dtype)
            ro, rd = rnd((M, 320), 840 + it, dtype)
            use_pe = it != 1
            spec = K.LnSpec(gamma, beta, 1e-5, pe if use_pe else None, inner if use_pe else 1, frames if use_pe else 1, ("test", it))
            assert K.ln_emit_ok(xd, wd, rd, None, spec)
            got = K.linear(xd, wd, bd, rd, 0.5, ln=spec)
            want = K.linear_bf16(xd, wd, bd, rd, 0.5, tile=512)
            assert torch.equal(got, want), f"out differs from the plain launch {(M, Kd)} it {it}"
            ln_out, key, stats_only = got._fmc_ln
            assert not stats_only
            assert key == ("test", it) and K.take_ln(got, ("other",)) is None and torch.equal(K.take_ln(got, key), ln_out)
            o64 = got.double().cpu()
            mu, var = o64.mean(-1, keepdim=True), o64.var(-1, unbiased=False, keepdim=True)
            ref = (o64 - mu) / torch.sqrt(var + 1e-5) * gamma.double().cpu() + beta.double().cpu()
            mag = ((o64 - mu).abs() / torch.sqrt(var + 1e-5) * gamma.double().cpu().abs() + beta.double().cpu().abs())
            if use_pe:
                rows = (torch.arange(M) // inner) % frames
                ref = ref + pe.double().cpu()[rows]
                mag = mag + pe.double().cpu()[rows].abs()
            assert_bf16_close(ln_out, ref, 8.0 * mag + 1.0, f"ln_out {(M, Kd)} it {it}")
            sep = K.layernorm(got, gamma, beta, 1e-5, pe if use_pe else None, inner if use_pe else 1, frames if use_pe else 1)
            d = (ln_out.float() - sep.float()).abs()
            assert float((d / sep.float().abs().clamp_min(1e-2)).max()) < 2.0 ** -6, "more than a bf16 ulp or two from the LayerNorm kernel"
            assert float((d > 0).float().mean()) < 0.02
            if it == 0:
                assert torch.equal(K.linear(xd, wd, bd, rd, 0.5, ln=spec)._fmc_ln[0], ln_out)                     # deterministic
                r2o, r2d = rnd((M, 320), 940, dtype)
                got2 = K.linear(xd, wd, None, rd, 1.0, residual2=r2d, ln=spec)
                assert torch.equal(got2, K.linear_bf16(xd, wd, None, rd, 1.0, tile=512, residual2=r2d))
                assert rel_inf(got2._fmc_ln[0].float(), K.layernorm(got2, gamma, beta, 1e-5, pe, inner, frames).float()) < 8e-3
    # ineligible: too few tiles, N != 320, frames that are not whole tiles -> plain result, no tag
    xo, xd = rnd((20480, 320), 41, dtype)
    wo, wd = rnd((320, 320), 42, dtype, scale=320 ** -0.5)
    spec = K.LnSpec(gamma, beta, 1e-5, None, 1, 1, ("t",))
    assert getattr(K.linear(xd, wd, None, None, 1.0, ln=spec), "_fmc_ln", None) is None
    xo, xd = rnd((81920, 320), 43, dtype)
    assert getattr(K.linear(xd, wd, None, None, 1.0, ln=K.LnSpec(gamma, beta, 1e-5, pe, 2000, 16, ("t",))), "_fmc_ln", None) is None
    w6o, w6d = rnd((640, 320), 44, dtype, scale=320 ** -0.5)
    g6 = torch.ones(640, device="cuda")
    assert getattr(K.linear(xd, w6d, None, None, 1.0, ln=K.LnSpec(g6, g6, 1e-5, None, 1, 1, ("t",))), "_fmc_ln", None) is None


@torch.no_grad()
def test_layernorm_applied_in_the_consuming_gemm(K):
    """`fmc_linear_bf16_ln(ln_stats=...)` + `fmc_linear_bf16_lnc`: the producer's epilogue leaves (mean, rstd) of its rounded output rows,
    the consumer GEMM runs on gamma-scaled weights and applies `rstd (acc - mean c) + (W beta + b)` -- LayerNorm(x) is never written.
    Against an fp64 LayerNorm + projection of the SAME bf16 producer output (so the bound is the usual one for a bf16 GEMM: the
    gamma-scaled weights are rounded where the unfused path rounds the normalised activations), plain and GEGLU epilogues, a non-zero
    row mean (cancellation in `acc - mean c`), several launches; and the front-end's fall-back when the consumer is not eligible."""
    dtype = torch.bfloat16
    from synfmc_amd.models.layers import interleave_geglu
    g = torch.Generator().manual_seed(6)
    gamma, beta = (1.0 + 0.3 * torch.randn(320, generator=g)).cuda(), (0.2 * torch.randn(320, generator=g)).cuda()
    M = 81920
    wo, wd = rnd((320, 320), 45, dtype, scale=320 ** -0.5)
    for it in range(3):
        xo, xd = rnd((M, 320), 750 + it, dtype)
        ro, rd = rnd((M, 320), 850 + it, dtype)
        rd = (rd.float() + (3.0 if it == 2 else 0.0)).to(dtype)                                     # it 2: rows with mean ~ 3 sigma
        spec = K.LnSpec(gamma, beta, 1e-5, None, 1, 1, ("t", it), stats_only=True)
        h = K.linear(xd, wd, None, rd, 1.0, ln=spec)
        assert torch.equal(h, K.linear_bf16(xd, wd, None, rd, 1.0, tile=512))
        stats = K.take_ln_stats(h, ("t", it))
        assert stats is not None and K.take_ln(h, ("t", it)) is None
        h64 = h.double().cpu()
        mu, var = h64.mean(-1), h64.var(-1, unbiased=False)
        assert float((stats[:, 0].double().cpu() - mu).abs().max()) < 1e-5 * (1.0 + float(mu.abs().max()))
        assert float((stats[:, 1].double().cpu() * torch.sqrt(var + 1e-5) - 1.0).abs().max()) < 1e-4
        ln64 = (h64 - mu[:, None]) / torch.sqrt(var + 1e-5)[:, None] * gamma.double().cpu() + beta.double().cpu()
        pend = K.pending_ln(h, stats, gamma, beta, 1e-5)
        for (N, bias_on) in [(960, False), (320, True)]:
            qo, qd = rnd((N, 320), 47 + N, dtype, scale=320 ** -0.5)
            bo, bd = rnd((N,), 48, dtype)
            got = K.linear(pend, qd, bd if bias_on else None)
            ref = F.linear(ln64, qo.double(), bo.double() if bias_on else None)
            mag = ln64.abs() @ qo.abs().double().t() + (bo.abs().double() if bias_on else 0.0)
            assert got.shape == (M, N)
            assert float(((got.double().cpu() - ref).abs() / (2.0 ** -7 * mag + 2.0 ** -8 * ref.abs() + 1e-3)).max()) < 1.0, f"lnc plain N={N} it={it}"
            unfused = K.linear(K.layernorm(h, gamma, beta, 1e-5), qd, bd if bias_on else None)
            assert rel_inf(got.float(), unfused.float()) < 2e-2
        go, gd = rnd((2560, 320), 42, dtype, scale=320 ** -0.5)
        gbo, gbd = rnd((2560,), 40, dtype)
        wi32, bi32 = interleave_geglu(gd, gbd)
        wi8, bi8 = interleave_geglu(gd, gbd, 8)
        before = dict(K.ln_epilogue_calls)
        outg = K.geglu_linear(pend, gd, gbd, wi32, bi32, wi8, bi8)
        assert K.ln_epilogue_calls["consumed"] == before["consumed"] + 1 and K.ln_epilogue_calls.get("materialised", 0) == before.get("materialised", 0)
        a, gt = F.linear(ln64, go.double(), gbo.double()).chunk(2, dim=-1)
        ma, mg = (ln64.abs() @ go.abs().double().t() + gbo.abs().double()).chunk(2, dim=-1)
        refg = a * F.gelu(gt)
        magg = F.gelu(gt).abs() * ma + 1.13 * a.abs() * mg
        assert float(((outg.double().cpu() - refg).abs() / (2.0 ** -7 * magg + 2.0 ** -8 * refg.abs() + 2e-3)).max()) < 1.0, f"lnc geglu it={it}"
        assert torch.equal(outg, K.geglu_linear(pend, gd, gbd, wi32, bi32, wi8, bi8))
    # not eligible (N % 320 != 0): the front-end materialises the norm and gives the unfused result
    qo, qd = rnd((328, 320), 49, dtype, scale=320 ** -0.5)
    before = K.ln_epilogue_calls.get("materialised", 0)
    got = K.linear(pend, qd, None)
    assert K.ln_epilogue_calls.get("materialised", 0) == before + 1
    assert torch.equal(got, K.linear(K.layernorm(h, gamma, beta, 1e-5), qd, None))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_norm_with_skip_is_one_autograd_node(K, dtype):
    """`layernorm_skip` / `groupnorm_silu_skip`: `(h, norm(h))` as one node whose backward adds the skip gradient inside the norm's backward
    kernel (`fmc_layernorm_bwd_add` / `fmc_groupnorm_silu_bwd_add`).  Gradients of `sum(w1 * h_skip) + sum(w2 * norm(h))` against plain
    PyTorch autograd in fp64, and the cases where only one of the two outputs is used."""
    g = torch.Generator().manual_seed(21)
    tol = 2e-5 if dtype == torch.float32 else 1.5e-2
    # LayerNorm (+ positional encoding)
    x0 = torch.randn(2, 16, 40, 320, generator=g)
    gamma, beta = 1.0 + 0.2 * torch.randn(320, generator=g), 0.1 * torch.randn(320, generator=g)
    pe = torch.randn(16, 320, generator=g)
    w1, w2 = torch.randn(x0.shape, generator=g), torch.randn(x0.shape, generator=g)
    xr = x0.to(dtype).double().requires_grad_(True)
    ref_y = F.layer_norm(xr, (320,), gamma.double(), beta.double(), 1e-5) + pe.double()[None, :, None, :]
    (w1.double() * xr).sum().add((w2.double() * ref_y).sum()).backward()
    for use in ("both", "norm", "skip"):
        x = x0.to("cuda", dtype).requires_grad_(True)
        xs, y = K.layernorm_skip(x, gamma.cuda(), beta.cuda(), 1e-5, pe.cuda(), 40, 16)
        assert rel_inf(y, ref_y) < (1e-5 if dtype == torch.float32 else 1e-2) and torch.equal(xs, x)
        loss = 0.0
        if use in ("both", "skip"):
            loss = loss + (w1.cuda().to(dtype) * xs).float().sum()
        if use in ("both", "norm"):
            loss = loss + (w2.cuda().to(dtype) * y).float().sum()
        loss.backward()
        if use == "both":
            assert rel_inf(x.grad, xr.grad) < tol
        elif use == "skip":
            assert rel_inf(x.grad, w1.to(dtype).double()) < tol
    # GroupNorm + SiLU
    x0 = torch.randn(3, 640, 320, generator=g)
    w1, w2 = torch.randn(x0.shape, generator=g), torch.randn(x0.shape, generator=g)
    xr = x0.to(dtype).double().requires_grad_(True)
    ref_y = F.silu(F.group_norm(xr.transpose(1, 2), 32, gamma.double(), beta.double(), 1e-6)).transpose(1, 2)
    (w1.double() * xr).sum().add((w2.double() * ref_y).sum()).backward()
    x = x0.to("cuda", dtype).requires_grad_(True)
    xs, y = K.groupnorm_silu_skip(x, gamma.cuda(), beta.cuda(), 32, 1e-6, True)
    assert rel_inf(y, ref_y) < (1e-5 if dtype == torch.float32 else 1e-2)
    ((w1.cuda().to(dtype) * xs).float().sum() + (w2.cuda().to(dtype) * y).float().sum()).backward()
    assert rel_inf(x.grad, xr.grad) < tol


@torch.no_grad()
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [320, 640, 1280])
def test_layernorm_with_the_residual_add_in_front(K, dtype, C):
    """`fmc_layernorm_add_fwd`: `h = x + addend` rounded to the storage type, `y = LayerNorm(h) (+ pe)` -- bit-identical to the separate
    `torch.add` + `fmc_layernorm_fwd` pair it replaces; and the front-end's lazy residual (`linear(..., lazy_residual=True)` on the vendor
    arm + `resolve_pending_add`)."""
    g = torch.Generator().manual_seed(31)
    M = 2 * 16 * 40
    x = torch.randn(2, 16, 40, C, generator=g).to("cuda", dtype)
    r = torch.randn(2, 16, 40, C, generator=g).to("cuda", dtype)
    gamma, beta = (1.0 + 0.2 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
    pe = torch.randn(16, C, generator=g).cuda()
    for use_pe in (False, True):
        args = (pe, 40, 16) if use_pe else (None, 1, 1)
        h, y = K.layernorm_add(x, r, gamma, beta, 1e-5, *args)
        h_ref = torch.add(r, x)
        assert torch.equal(h, h_ref)
        assert torch.equal(y, K.layernorm(h_ref, gamma, beta, 1e-5, *args))
    t = x.view(x.shape)
    t._fmc_pending_add = r
    assert torch.equal(K.resolve_pending_add(t), torch.add(r, x)) and K.resolve_pending_add(x) is x


@torch.no_grad()
def test_feed_forward_with_a_tile_major_intermediate(K):
    """`fmc_linear_bf16_ffblk`: the GEGLU projection writes its gated output as `[M / 160][Cff / 32][160][32]`, the second GEMM requests each
    32-deep A sub-tile as one contiguous block.  The intermediate is the row-major one permuted, the pair's result is BIT-IDENTICAL to the
    row-major path on tile 16 (same products, same order) -- persistent and plain-grid form of the second GEMM, with and without residual,
    with the GEGLU projection also applying its input's LayerNorm; several launches on fresh data."""
    dtype = torch.bfloat16
    from synfmc_amd.models.layers import interleave_geglu
    for (M, C) in [(81920, 320), (20480, 640)]:
        Cff = 4 * C
        w1o, w1d = rnd((2 * Cff, C), 42, dtype, scale=C ** -0.5)
        b1o, b1d = rnd((2 * Cff,), 40, dtype)
        w2o, w2d = rnd((C, Cff), 43, dtype, scale=Cff ** -0.5)
        b2o, b2d = rnd((C,), 44, dtype)
        wi8, bi8 = interleave_geglu(w1d, b1d, 8)
        for it in range(2):
            xo, xd = rnd((M, C), 760 + it, dtype)
            ro, rd = rnd((M, C), 860 + it, dtype)
            assert K.ff_blocked_ok(xd, wi8, w2d, rd)
            mid_rm = K.linear_bf16(xd, wi8, bi8, geglu=True, tile=512)
            mid_tm = K.geglu_linear_blocked(xd, wi8, bi8)
            assert torch.equal(mid_tm.view(M // 160, Cff // 32, 160, 32).permute(0, 2, 1, 3).reshape(M, Cff), mid_rm)
            for res in (rd, None):
                got = K.linear_from_blocked(mid_tm, w2d, b2d, res)
                assert torch.equal(got, K.linear_bf16(mid_rm, w2d, b2d, res, 1.0, tile=512)), f"ff blocked {(M, C)} it {it} res {res is not None}"
    # with the input's LayerNorm applied by the GEGLU projection (deferred norm3 / ff_norm)
    g = torch.Generator().manual_seed(8)
    gamma, beta = (1.0 + 0.3 * torch.randn(320, generator=g)).cuda(), (0.2 * torch.randn(320, generator=g)).cuda()
    M, C, Cff = 81920, 320, 1280
    w1o, w1d = rnd((2 * Cff, C), 52, dtype, scale=C ** -0.5)
    b1o, b1d = rnd((2 * Cff,), 50, dtype)
    wi8, bi8 = interleave_geglu(w1d, b1d, 8)
    wi32, bi32 = interleave_geglu(w1d, b1d)
    xo, xd = rnd((M, C), 770, dtype)
    wo, wd = rnd((320, 320), 45, dtype, scale=320 ** -0.5)
    h = K.linear(xd, wd, None, None, 1.0, ln=K.LnSpec(gamma, beta, 1e-5, None, 1, 1, ("ff",), stats_only=True))
    pend = K.pending_ln(h, K.take_ln_stats(h, ("ff",)), gamma, beta, 1e-5)
    mid_rm = K.geglu_linear(pend, w1d, b1d, wi32, bi32, wi8, bi8)
    mid_tm = K.geglu_linear_blocked(pend, wi8, bi8)
    assert torch.equal(mid_tm.view(M // 160, Cff // 32, 160, 32).permute(0, 2, 1, 3).reshape(M, Cff), mid_rm)


@torch.no_grad()
def test_tile_major_weights_are_bit_identical(K):
    """Tile 18 (arm 544) = tile 16 on a weight pre-packed `[N / 320][K / 32][320][32]` (filters: `[Cout / 320][Cin / 64][9][2][320][32]`, the conv
    kernel's own sub-tile order): same products in the same order, so every output is bit-identical to tile 16 -- plain and persistent form,
    bias / residual / GEGLU, conv with temb / residual / upsample / stride 2, the GroupNorm- and LayerNorm-emitting entry points; shapes tile 16
    does not take on a packed weight fall back to the row-major path."""
    dtype = torch.bfloat16
    from synfmc_amd.models.layers import interleave_geglu
    for (M, N, Kd) in [(81920, 320, 320), (20480, 640, 640), (4100, 960, 1280), (5120, 1280, 5120)]:
        xo, xd = rnd((M, Kd), 780, dtype)
        wo, wd = rnd((N, Kd), 45, dtype, scale=Kd ** -0.5)
        bo, bd = rnd((N,), 46, dtype)
        ro, rd = rnd((M, N), 880, dtype)
        assert torch.equal(K.linear_bf16(xd, wd, bd, rd, 0.5, tile=K.ARM_160B), K.linear_bf16(xd, wd, bd, rd, 0.5, tile=K.ARM_160)), (M, N, Kd)
        assert torch.equal(K.linear_bf16(xd, wd, None, None, 1.0, tile=K.ARM_160B), K.linear_bf16(xd, wd, None, None, 1.0, tile=K.ARM_160))
    go, gd = rnd((2560, 320), 42, dtype, scale=320 ** -0.5)
    gbo, gbd = rnd((2560,), 40, dtype)
    w8, b8 = interleave_geglu(gd, gbd, 8)
    for M in (48000, 4100):
        xo, xd = rnd((M, 320), 781, dtype)
        assert torch.equal(K.linear_bf16(xd, w8, b8, geglu=True, tile=K.ARM_160B), K.linear_bf16(xd, w8, b8, geglu=True, tile=K.ARM_160))
    co, cd = rnd((4, 36, 30, 320), 47, dtype)
    fo, fd = rnd((640, 320, 3, 3), 44, dtype, scale=(9 * 320) ** -0.5)
    f_cl = fd.contiguous(memory_format=torch.channels_last)
    to, td = rnd((4, 640), 43, dtype)
    ro, rd = rnd((4, 36, 30, 640), 48, dtype)
    for kw in ({}, {"upsample": True}, {"stride2": True}):
        assert torch.equal(K.conv3x3_bf16(cd, f_cl, None, None, None, tile=K.ARM_160B, **kw), K.conv3x3_bf16(cd, f_cl, None, None, None, tile=K.ARM_160, **kw)), kw
    assert torch.equal(K.conv3x3_bf16(cd, f_cl, None, td, rd, tile=K.ARM_160B), K.conv3x3_bf16(cd, f_cl, None, td, rd, tile=K.ARM_160))
    # not taken on a packed weight: N % 320 != 0, two-source operand -> the row-major path, same function as before
    xo, xd = rnd((700, 320), 41, dtype)
    wo, wd = rnd((328, 320), 42, dtype, scale=320 ** -0.5)
    assert torch.equal(K.linear_bf16(xd, wd, None, None, 1.0, tile=K.ARM_160B), K.linear_bf16(xd, wd, None, None, 1.0, tile=13))
    x1o, x1d = rnd((700, 128), 51, dtype)
    x2o, x2d = rnd((700, 192), 52, dtype)
    w3o, w3d = rnd((320, 320), 53, dtype, scale=320 ** -0.5)
    assert torch.equal(K.linear_bf16(x1d, w3d, None, None, 1.0, tile=K.ARM_160B, x2=x2d), K.linear_bf16(x1d, w3d, None, None, 1.0, tile=13, x2=x2d))
    # the flag of the tile-16-only entry points (GroupNorm partials here; the LayerNorm ones are covered by their own tests, which run with it on)
    assert K.W_TILEMAJOR
    xo, xd = rnd((2, 2560, 320), 54, dtype)
    y = K.linear(xd, w3d, None, None, 1.0, gn_hw=2560)
    assert getattr(y, "_fmc_gn", None) is not None and torch.equal(y, K.linear_bf16(xd, w3d, None, None, 1.0, tile=K.ARM_160))


def _temporal_block_reference(h, gamma, beta, pe, eps, wqkv, wout, bout, heads, wm=None, bm=None, pose=None, s=1.0, round_bf16=True):
    """fp32 restatement of one attention block of the temporal transformer (fmc/models/motion_module.py:287-300, 349-389;
    fmc/models/attention_processor.py:202-293): h `[B, F, hw, C]`.  With `round_bf16` the tensors the fused kernel keeps in bf16 (x, the pose
    term, m, q / k / v, the probabilities, o) are rounded where the kernel rounds them, so that the comparison isolates the arithmetic."""
    r = (lambda t: t.bfloat16().float()) if round_bf16 else (lambda t: t)
    B, Fr, hw, C = h.shape
    d = C // heads
    x = r(F.layer_norm(h, (C,), gamma, beta, eps) + pe[None, :Fr, None, :])
    m = x
    if wm is not None:
        pt = r(s * F.linear(pose, wm, bm))
        m = r(s * F.linear(x, wm) + pt + x)
    qkv = r(F.linear(m, wqkv))
    q, k, v = (t.reshape(B, Fr, hw, heads, d).permute(0, 2, 3, 1, 4) for t in qkv.chunk(3, dim=-1))      # [B, hw, H, F, d]
    p = r(torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1))
    o = r(p @ v).permute(0, 3, 1, 2, 4).reshape(B, Fr, hw, C)
    return F.linear(o, wout, bout) + h


@pytest.mark.parametrize("M,cff,C", [(80, 320, 640), (20480, 2560, 640), (240, 640, 640), (80, 160, 320), (81920, 1280, 320), (400, 480, 320), (320, 640, 320)])
def test_geglu_ln_direct(K, M, cff, C):
    """`fmc_geglu640_ln_bf16` / `fmc_geglu320_ln_bf16`: LayerNorm + GEGLU projection with the A operand resident in LDS and the (value / gate row-permuted) weight streamed in
    fragment order; against fp32 (max norm), the same with the kernel's rounding points (element-wise bf16 bound), and deterministic."""
    dtype = torch.bfloat16
    ho, hd = rnd((M, C), 1, dtype, scale=1.5, shift=0.2)
    go, _ = rnd((C,), 2, torch.float32, scale=0.3, shift=1.0)
    bo, _ = rnd((C,), 3, torch.float32, scale=0.2)
    wo, wd = rnd((2 * cff, C), 4, dtype, scale=C ** -0.5)
    bio, bid = rnd((2 * cff,), 5, dtype, scale=0.3)
    out = K.geglu_ln_direct(hd, go.cuda(), bo.cuda(), 1e-5, K.pack_geglu_frag80(wd), bid, cff)

    def reference(round_bf16):
        r = (lambda t: t.bfloat16().float()) if round_bf16 else (lambda t: t)
        n = r(F.layer_norm(ho, (C,), go, bo, 1e-5))
        y = F.linear(n, wo, bio)
        return y[:, :cff] * F.gelu(y[:, cff:])
    ref_r, ref_f = reference(True), reference(False)
    assert rel_inf(out.float(), ref_f) < 2e-2
    err = (out.float().cpu() - ref_r).abs()                # (a bf16 flip of a normalised element moves a product by 2^-8 |n w|: absolute slack next to the relative bound)
    bound = 2.0 ** -8 * ref_r.abs() + 0.02
    assert not bool((err > bound).any()), f"{int((err > bound).sum())} / {err.numel()} beyond the bound, worst {float((err - bound).max()):.3e}"
    assert torch.equal(out, K.geglu_ln_direct(hd, go.cuda(), bo.cuda(), 1e-5, K.pack_geglu_frag80(wd), bid, cff))
    out_nb = K.geglu_ln_direct(hd, go.cuda(), bo.cuda(), 1e-5, K.pack_geglu_frag80(wd), None, cff)
    y = F.linear(F.layer_norm(ho, (C,), go, bo, 1e-5), wo)
    assert rel_inf(out_nb.float(), y[:, :cff] * F.gelu(y[:, cff:])) < 2e-2
    if M % 160 == 0:
        # tile-major output [M / 160][cff / 32][160][32] (the feed-forward's private intermediate): the same values, bit for bit, and the second GEMM
        # reads them back as the row-major result (`linear_from_blocked` against the tuned front-end on the row-major tensor)
        blk = K.geglu_ln_direct(hd, go.cuda(), bo.cuda(), 1e-5, K.pack_geglu_frag80(wd), bid, cff, blocked=True)
        assert torch.equal(blk.view(M // 160, cff // 32, 160, 32).permute(0, 2, 1, 3).reshape(M, cff), out)
        if C == 320 and M >= 81920:
            w2o, w2d = rnd((C, cff), 6, dtype, scale=cff ** -0.5)
            b2o, b2d = rnd((C,), 7, dtype, scale=0.3)
            assert K.geglu_direct_blocked_ok(hd, w2d, hd)
            got = K.linear_from_blocked(blk, w2d, b2d, hd)
            ref2 = F.linear(out.float().cpu(), w2o, b2o) + ho
            assert rel_inf(got.float(), ref2) < 1e-2


@pytest.mark.parametrize("B,Fr,hw,S", [(1, 1, 160, 77), (2, 16, 2560, 77), (3, 2, 320, 80), (2, 3, 160, 5)])
def test_xattn_block_fused_320(K, B, Fr, hw, S):
    """`fmc_xattn_block320_bf16` + `fmc_xattn_pack_kv40`: the text cross-attention block at the 40x64 level (C = 320, 8 heads x 40) on the 160-row
    persistent skeleton of the temporal block, with the row statistics for the next LayerNorm; same checks as at C = 640."""
    dtype = torch.bfloat16
    C, H, d = 320, 8, 40
    N = B * Fr
    ho, hd = rnd((N, hw, C), 1, dtype, scale=1.5, shift=0.2)
    go, _ = rnd((C,), 2, torch.float32, scale=0.3, shift=1.0)
    bo, _ = rnd((C,), 3, torch.float32, scale=0.2)
    wqo, wqd = rnd((C, C), 5, dtype, scale=C ** -0.5 * 1.5)
    woo, wod = rnd((C, C), 6, dtype, scale=C ** -0.5)
    boo, bod = rnd((C,), 7, dtype, scale=0.3)
    kvo, kvd = rnd((B, S, 2 * C), 8, dtype, scale=1.2)
    btab = bo[None].expand(16, C).contiguous().cuda()
    run = lambda **k: K.xattn_block(hd, go.cuda(), btab, 1e-5, K.pack_xattn_q40(wqd), kvd, K._w_tilemajor(wod), bod, d ** -0.5, Fr, **k)
    out, stats = run(stats_eps=1e-5)

    def reference(round_bf16):
        r = (lambda t: t.bfloat16().float()) if round_bf16 else (lambda t: t)
        x = r(F.layer_norm(ho, (C,), go, bo, 1e-5))
        q = r(F.linear(x, wqo)).reshape(B, Fr * hw, H, d).permute(0, 2, 1, 3)
        k = kvo[..., :C].reshape(B, S, H, d).permute(0, 2, 1, 3)
        v = kvo[..., C:].reshape(B, S, H, d).permute(0, 2, 1, 3)
        p = r(torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1))
        o = r(p @ v).permute(0, 2, 1, 3).reshape(N, hw, C)
        return F.linear(o, woo, boo) + ho
    ref_r, ref_f = reference(True), reference(False)
    assert rel_inf(out.float(), ref_f) < 2e-2, (B, Fr, hw, S)
    err = (out.float().cpu() - ref_r).abs()
    print(f"fused block: worst |err| - 2^-8 |ref| = {float((err - 2.0 ** -8 * ref_r.abs()).max()):.4f} (|ref| max {float(ref_r.abs().max()):.2f})")
    # element-wise bound: one bf16 ulp of the element + 1.5 ulp of the LARGEST output (a flipped rounding of an intermediate -- LayerNorm output, merged
    # token, q / k / v, probability -- moves an output by a fraction of an ulp of the row's largest terms; measured on MI355X, round 5: worst excess over
    # 2^-8 |ref| = 0.95 x 2^-8 max|ref| across the four fused-block tests, gpurun_out/r05e/slack.log -- the former flat 0.08 was 1.3 - 3.7 x the measurement)
    bound = 2.0 ** -8 * ref_r.abs() + 1.5 * 2.0 ** -8 * float(ref_r.abs().max())
    assert not bool((err > bound).any()), f"{int((err > bound).sum())} / {err.numel()} beyond the bound, worst {float((err - bound).max()):.3e}"
    mu = out.float().mean(-1).view(-1)
    rstd = (out.float().var(-1, unbiased=False) + 1e-5).rsqrt().view(-1)
    assert rel_inf(stats[:, 0], mu) < 1e-4 and rel_inf(stats[:, 1], rstd) < 1e-4
    assert torch.equal(run(), out)
    with pytest.raises(ValueError):
        K.xattn_block(hd[:, :hw - 16].contiguous(), go.cuda(), btab, 1e-5, K.pack_xattn_q40(wqd), kvd, K._w_tilemajor(wod), bod, d ** -0.5, Fr)


@pytest.mark.parametrize("B,Fr,hw,S", [(1, 1, 80, 77), (2, 16, 640, 77), (3, 2, 160, 80), (2, 3, 80, 5)])
def test_xattn_block_fused_640(K, B, Fr, hw, S):
    """`fmc_xattn_block640_bf16` + `fmc_xattn_pack_kv`: LayerNorm -> to_q -> attention over the text tokens (k | v of a `[B, S, 1280]` projection shared by
    the Fr images of a batch entry; S = 77 masks the three padded keys) -> to_out + bias + residual in one launch, against the fp32 restatement with the
    kernel's bf16 rounding points (element-wise) and the plain fp32 chain (max norm); the bench size is 2 x 16 images x 640 tokens = 256 tiles."""
    dtype = torch.bfloat16
    C, H, d = 640, 8, 80
    N = B * Fr
    ho, hd = rnd((N, hw, C), 1, dtype, scale=1.5, shift=0.2)
    go, _ = rnd((C,), 2, torch.float32, scale=0.3, shift=1.0)
    bo, _ = rnd((C,), 3, torch.float32, scale=0.2)
    wqo, wqd = rnd((C, C), 5, dtype, scale=C ** -0.5 * 1.5)
    woo, wod = rnd((C, C), 6, dtype, scale=C ** -0.5)
    boo, bod = rnd((C,), 7, dtype, scale=0.3)
    kvo, kvd = rnd((B, S, 2 * C), 8, dtype, scale=1.2)
    btab = bo[None].expand(16, C).contiguous().cuda()
    run = lambda: K.xattn_block640(hd, go.cuda(), btab, 1e-5, K.pack_w_frag80(wqd), kvd, K.pack_w_frag80(wod), bod, d ** -0.5, Fr)
    out = run()

    def reference(round_bf16):
        r = (lambda t: t.bfloat16().float()) if round_bf16 else (lambda t: t)
        x = r(F.layer_norm(ho, (C,), go, bo, 1e-5))
        q = r(F.linear(x, wqo)).reshape(B, Fr * hw, H, d).permute(0, 2, 1, 3)                     # [B, H, Fr hw, d]
        k = kvo[..., :C].reshape(B, S, H, d).permute(0, 2, 1, 3)
        v = kvo[..., C:].reshape(B, S, H, d).permute(0, 2, 1, 3)
        p = r(torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1))
        o = r(p @ v).permute(0, 2, 1, 3).reshape(N, hw, C)
        return F.linear(o, woo, boo) + ho
    ref_r, ref_f = reference(True), reference(False)
    assert rel_inf(out.float(), ref_f) < 2e-2, (B, Fr, hw, S)
    err = (out.float().cpu() - ref_r).abs()
    print(f"fused block: worst |err| - 2^-8 |ref| = {float((err - 2.0 ** -8 * ref_r.abs()).max()):.4f} (|ref| max {float(ref_r.abs().max()):.2f})")
    # element-wise bound: one bf16 ulp of the element + 1.5 ulp of the LARGEST output (a flipped rounding of an intermediate -- LayerNorm output, merged
    # token, q / k / v, probability -- moves an output by a fraction of an ulp of the row's largest terms; measured on MI355X, round 5: worst excess over
    # 2^-8 |ref| = 0.95 x 2^-8 max|ref| across the four fused-block tests, gpurun_out/r05e/slack.log -- the former flat 0.08 was 1.3 - 3.7 x the measurement)
    bound = 2.0 ** -8 * ref_r.abs() + 1.5 * 2.0 ** -8 * float(ref_r.abs().max())
    assert not bool((err > bound).any()), f"{int((err > bound).sum())} / {err.numel()} beyond the bound, worst {float((err - bound).max()):.3e}"
    assert torch.equal(run(), out)
    with pytest.raises(ValueError):
        K.xattn_block640(hd[:, :hw - 8].contiguous(), go.cuda(), btab, 1e-5, K.pack_w_frag80(wqd), kvd, K.pack_w_frag80(wod), bod, d ** -0.5, Fr)


@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("B,hw", [(1, 5), (2, 640), (3, 35)])
def test_temporal_block_fused_640(K, merge, B, hw):
    """The same block at the 20x32 level (C = 640, 8 heads x 80; `temporal_block640.hip`: 80-row tiles, weights streamed in fragment order straight into
    registers): one tile, the bench size (2 x 640 pixels = 256 tiles), an odd tile count; element-wise bf16 bound against the restatement with the
    kernel's rounding points, max norm against the plain fp32 chain; deterministic."""
    dtype = torch.bfloat16
    C, H, Fr, d = 640, 8, 16, 80
    ho, hd = rnd((B, Fr, hw, C), 1, dtype, scale=1.5, shift=0.2)
    go, _ = rnd((C,), 2, torch.float32, scale=0.3, shift=1.0)
    bo, _ = rnd((C,), 3, torch.float32, scale=0.2)
    peo, _ = rnd((32, C), 4, torch.float32, scale=0.7)
    wqo, wqd = rnd((3 * C, C), 5, dtype, scale=C ** -0.5 * 1.5)
    woo, wod = rnd((C, C), 6, dtype, scale=C ** -0.5)
    boo, bod = rnd((C,), 7, dtype, scale=0.3)
    wmo, wmd = rnd((C, C), 8, dtype, scale=C ** -0.5)
    bmo, bmd = rnd((C,), 9, dtype, scale=0.3)
    poo, pod = rnd((B, Fr, hw, C), 10, dtype)
    s = 0.7
    bpe = (bo[None] + peo[:Fr]).cuda().contiguous()
    pt = K.linear_bf16(pod.view(-1, C), wmd, bmd, None, s).view(B, Fr, hw, C) if merge else None
    # the pose term `s (W pose + b)` on the CPU as well: the reference chain below must not inherit the device GEMM's output (a wrong
    # `linear_bf16(alpha=s)` would cancel); the device term is held to the bf16 rounding of the CPU one
    pt_ref = (s * (F.linear(poo, wmo) + bmo)).bfloat16().float() if merge else None
    if merge:
        assert rel_inf(pt.float(), pt_ref) < 6e-3
    kw = dict(w_merge_tm=K.pack_w_frag80(wmd), pose_term=pt, merge_scale=s) if merge else {}
    run = lambda: K.temporal_block(hd, go.cuda(), bpe, 1e-5, K.pack_temporal_qkv80(wqd), K.pack_w_frag80(wod), bod, d ** -0.5, **kw)
    out = run()

    def reference(round_bf16):
        r = (lambda t: t.bfloat16().float()) if round_bf16 else (lambda t: t)
        x = r(F.layer_norm(ho, (C,), go, bo, 1e-5) + peo[None, :Fr, None, :])
        m = r(s * F.linear(x, wmo) + pt_ref + x) if merge else x
        qkv = r(F.linear(m, wqo))
        q, k, v = (t.reshape(B, Fr, hw, H, d).permute(0, 2, 3, 1, 4) for t in qkv.chunk(3, dim=-1))
        p = r(torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1))
        o = r(p @ v).permute(0, 3, 1, 2, 4).reshape(B, Fr, hw, C)
        return F.linear(o, woo, boo) + ho
    ref_r, ref_f = reference(True), reference(False)
    assert rel_inf(out.float(), ref_f) < 2e-2, (merge, B, hw)
    err = (out.float().cpu() - ref_r).abs()
    print(f"fused block: worst |err| - 2^-8 |ref| = {float((err - 2.0 ** -8 * ref_r.abs()).max()):.4f} (|ref| max {float(ref_r.abs().max()):.2f})")
    # element-wise bound: one bf16 ulp of the element + 1.5 ulp of the LARGEST output (a flipped rounding of an intermediate -- LayerNorm output, merged
    # token, q / k / v, probability -- moves an output by a fraction of an ulp of the row's largest terms; measured on MI355X, round 5: worst excess over
    # 2^-8 |ref| = 0.95 x 2^-8 max|ref| across the four fused-block tests, gpurun_out/r05e/slack.log -- the former flat 0.08 was 1.3 - 3.7 x the measurement)
    bound = 2.0 ** -8 * ref_r.abs() + 1.5 * 2.0 ** -8 * float(ref_r.abs().max())
    assert not bool((err > bound).any()), f"{int((err > bound).sum())} / {err.numel()} beyond the bound, worst {float((err - bound).max()):.3e} at {int((err - bound).flatten().argmax())}"
    for it in range(3):
        assert torch.equal(run(), out)
    with pytest.raises(ValueError):
        K.temporal_block(hd[:, :, :hw - 1].contiguous(), go.cuda(), bpe, 1e-5, K.pack_temporal_qkv80(wqd), K.pack_w_frag80(wod), bod, d ** -0.5)


@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("B,hw", [(1, 10), (2, 2560), (3, 70)])
def test_temporal_block_fused(K, merge, B, hw):
    """`fmc_temporal_block_bf16`: LayerNorm + pe -> [Camera-Adapter merge + pose term] -> q | k | v -> attention over the 16 frames ->
    out-projection + bias + residual, one launch, a 160-row tile resident in LDS.  Against the fp32 restatement with the kernel's bf16
    rounding points (element-wise bf16 bound on the output) and against the plain fp32 chain (max norm); one tile, the bench size (2 clips x
    2560 pixels = 512 tiles on 256 CUs: two per workgroup), an odd tile count; the row statistics for the next LayerNorm; repeated launches."""
    dtype = torch.bfloat16
    C, H, Fr = 320, 8, 16
    ho, hd = rnd((B, Fr, hw, C), 1, dtype, scale=1.5, shift=0.2)
    go, _ = rnd((C,), 2, torch.float32, scale=0.3, shift=1.0)
    bo, _ = rnd((C,), 3, torch.float32, scale=0.2)
    peo, _ = rnd((32, C), 4, torch.float32, scale=0.7)
    wqo, wqd = rnd((3 * C, C), 5, dtype, scale=C ** -0.5 * 1.5)
    woo, wod = rnd((C, C), 6, dtype, scale=C ** -0.5)
    boo, bod = rnd((C,), 7, dtype, scale=0.3)
    wmo, wmd = rnd((C, C), 8, dtype, scale=C ** -0.5)
    bmo, bmd = rnd((C,), 9, dtype, scale=0.3)
    poo, pod = rnd((B, Fr, hw, C), 10, dtype)
    s = 0.7
    bpe = (bo[None] + peo[:Fr]).cuda().contiguous()
    pt = K.linear_bf16(pod.view(-1, C), wmd, bmd, None, s).view(B, Fr, hw, C) if merge else None
    pt_ref = (s * (F.linear(poo, wmo) + bmo)).bfloat16().float() if merge else None      # (CPU pose term: see test_temporal_block_fused_640)
    if merge:
        assert rel_inf(pt.float(), pt_ref) < 6e-3
    kw = dict(w_merge_tm=K._w_tilemajor(wmd), pose_term=pt, merge_scale=s) if merge else {}
    out, stats = K.temporal_block(hd, go.cuda(), bpe, 1e-5, K.pack_temporal_qkv(wqd), K._w_tilemajor(wod), bod, 40 ** -0.5, stats_eps=1e-5, **kw)
    rk = dict(wm=wmo, bm=bmo, pose=poo, s=s) if merge else {}
    if merge:                                            # the pose term the kernel reads is the GEMM's own rounding of s (W pose + b)
        rk["pose"] = None
    ref_args = (ho, go, bo, peo, 1e-5, wqo, woo, boo, H)

    def reference(round_bf16):
        if not merge:
            return _temporal_block_reference(*ref_args, round_bf16=round_bf16)
        r = (lambda t: t.bfloat16().float()) if round_bf16 else (lambda t: t)
        # (restated here with the device's own pose term so that its rounding is not compared)
        x = r(F.layer_norm(ho, (C,), go, bo, 1e-5) + peo[None, :Fr, None, :])
        m = r(s * F.linear(x, wmo) + pt_ref + x)
        qkv = r(F.linear(m, wqo))
        q, k, v = (t.reshape(B, Fr, hw, H, 40).permute(0, 2, 3, 1, 4) for t in qkv.chunk(3, dim=-1))
        p = r(torch.softmax(q @ k.transpose(-1, -2) * 40 ** -0.5, dim=-1))
        o = r(p @ v).permute(0, 3, 1, 2, 4).reshape(B, Fr, hw, C)
        return F.linear(o, woo, boo) + ho
    ref_r, ref_f = reference(True), reference(False)
    assert rel_inf(out.float(), ref_f) < 2e-2, (merge, B, hw)
    # element-wise: the kernel's bf16 intermediates can round the other way on ties / accumulation order: bound = bf16 output rounding + the
    # out-projection's amplification of a 2^-8 error in o (|W_out| row sums ~ 14 x C^-1/2 x |o|)
    err = (out.float().cpu() - ref_r).abs()
    print(f"fused block: worst |err| - 2^-8 |ref| = {float((err - 2.0 ** -8 * ref_r.abs()).max()):.4f} (|ref| max {float(ref_r.abs().max()):.2f})")
    # element-wise bound: one bf16 ulp of the element + 1.5 ulp of the LARGEST output (a flipped rounding of an intermediate -- LayerNorm output, merged
    # token, q / k / v, probability -- moves an output by a fraction of an ulp of the row's largest terms; measured on MI355X, round 5: worst excess over
    # 2^-8 |ref| = 0.95 x 2^-8 max|ref| across the four fused-block tests, gpurun_out/r05e/slack.log -- the former flat 0.08 was 1.3 - 3.7 x the measurement)
    bound = 2.0 ** -8 * ref_r.abs() + 1.5 * 2.0 ** -8 * float(ref_r.abs().max())
    assert not bool((err > bound).any()), f"{int((err > bound).sum())} / {err.numel()} beyond the bound, worst {float((err - bound).max()):.3e} at {int((err - bound).flatten().argmax())}"
    # row statistics of the rounded output
    mu = out.float().mean(-1).view(-1)
    rstd = (out.float().var(-1, unbiased=False) + 1e-5).rsqrt().view(-1)
    assert rel_inf(stats[:, 0], mu) < 1e-4 and rel_inf(stats[:, 1], rstd) < 1e-4
    for it in range(3):                                  # deterministic, no state between launches
        again = K.temporal_block(hd, go.cuda(), bpe, 1e-5, K.pack_temporal_qkv(wqd), K._w_tilemajor(wod), bod, 40 ** -0.5, **kw)
        assert torch.equal(again, out)
    with pytest.raises(ValueError):                      # shapes outside the fused block's domain are refused (callers keep the un-fused chain)
        K.temporal_block(hd[:, :, :hw - 1].contiguous(), go.cuda(), bpe, 1e-5, K.pack_temporal_qkv(wqd), K._w_tilemajor(wod), bod, 40 ** -0.5)


@torch.no_grad()
@pytest.mark.parametrize("M,N,Kd,extras", [(5120, 1280, 1280, 2), (1280, 1280, 5120, 2), (5120, 3840, 1280, 0), (5120, 1280, 1280, 1), (304, 200, 128, 2)])
def test_vendor_linear_direct(K, M, N, Kd, extras):
    """`fmc_vendor_linear_bf16` (csrc/vendor_gemm.hip): the library arm of the token projections as ONE hipBLASLt launch, `x W^T + b + r` with bias and
    residual in the GEMM's epilogue (torch: F.linear + add).  Element-wise bf16 bound against the exact result; every heuristic candidate; strided rows; and
    the front-end's vendor arm goes through it (no torch add behind the GEMM)."""
    dtype = torch.bfloat16
    xo, xd = rnd((M, Kd), 981, dtype)
    wo, wd = rnd((N, Kd), 982, dtype, scale=Kd ** -0.5)
    bo, bd = rnd((N,), 983, dtype) if extras >= 1 else (None, None)
    ro, rd = rnd((M, N), 984, dtype) if extras >= 2 else (None, None)
    ref = xo.double() @ wo.double().t()
    mag = xo.abs().double() @ wo.abs().double().t()
    if bo is not None:
        ref, mag = ref + bo.double(), mag + bo.abs().double()
    if ro is not None:
        ref, mag = ref + ro.double(), mag + ro.abs().double()
    got = K.vendor_linear(xd, wd, bd, rd)
    assert_bf16_close(got, ref, mag, f"vendor_linear {(M, N, Kd)}")
    n = K._lib.load().fmc_vendor_linear_candidates(M, N, Kd, Kd, N if rd is not None else 0, N, int(bd is not None), int(rd is not None))
    assert n >= 1
    lib = K._lib.load()
    ws = K._vendor_workspace(xd.device)                                       # the scratch is the caller's (one per stream), never the library's
    assert ws.numel() == lib.fmc_vendor_workspace_bytes() and K.vendor_version() > 0
    need_ws = 0
    for algo in range(n):
        out = torch.empty_like(got)
        K._lib.check(lib.fmc_vendor_linear_bf16(xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if bd is not None else None, rd.data_ptr() if rd is not None else None,
                                                out.data_ptr(), M, N, Kd, Kd, N if rd is not None else 0, N, algo, ws.data_ptr(), ws.numel(),
                                                torch.cuda.current_stream().cuda_stream), "vendor")
        assert_bf16_close(out, ref, mag, f"vendor_linear candidate {algo}")
        # without a workspace a candidate either needs none (runs, same result) or is refused loudly -- it never allocates behind the caller's back
        rc = lib.fmc_vendor_linear_bf16(xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if bd is not None else None, rd.data_ptr() if rd is not None else None,
                                        out.data_ptr(), M, N, Kd, Kd, N if rd is not None else 0, N, algo, None, 0, torch.cuda.current_stream().cuda_stream)
        need_ws += rc != 0
        if rc == 0:
            assert_bf16_close(out, ref, mag, f"vendor_linear candidate {algo} without workspace")
    assert need_ws < n or n == 1
    assert lib.fmc_vendor_linear_bf16(xd.data_ptr(), wd.data_ptr(), None, None, got.data_ptr(), M, N, Kd, Kd, 0, N, n, ws.data_ptr(), ws.numel(), 0) != 0   # past the list: refused
    wide = torch.cat([xd, xd.flip(0)], dim=1)                                # rows of a wider matrix (ldx > K)
    assert_bf16_close(K.vendor_linear(wide[:, :Kd], wd, bd, rd), ref, mag, "vendor_linear strided")
    if rd is not None:
        K._choice[("lin", M, N, Kd, bd is not None, 1, 0)] = 0               # the front-end's vendor arm
        before = dict(K.vendor_direct_calls)
        y = K.linear(xd, wd, bd, residual=rd)
        assert K.vendor_direct_calls["with_residual"] == before["with_residual"] + 1
        assert_bf16_close(y, ref, mag, "linear -> vendor arm")
        # a broadcastable residual is not the library's full [M, N] C matrix: the arm must take the torch path (which broadcasts), not read out of bounds
        assert not K.vendor_linear_ok(xd, wd, bd, rd[:1])
        assert not K.vendor_linear_ok(xd[:, 4:], wd[:, 4:].contiguous(), None, None)       # rows 8 bytes off a 16-byte boundary: F.linear's business


@torch.no_grad()
@pytest.mark.parametrize("M,N,Kd,extras", [(5120, 1280, 1280, 3), (1280, 1280, 1280, 2), (5120, 3840, 1280, 0), (5120, 1280, 5120, 1),
                                           (300, 200, 128, 3), (160, 160, 64, 0), (20480, 640, 640, 2)])
def test_linear4_small_m_projection(K, M, N, Kd, extras):
    """`fmc_linear4_bf16` (csrc/gemm4.hip): `alpha (x W^T + b) + r + r2` on 160 x 160 software-pipelined tiles -- the M <= 5120 projections of the inner
    levels (attention_processor.py:50-69,255-283; motion_module.py:219,228,284).  Element-wise bf16 bound against the exact result on the same rounded
    operands; edge tiles (M, N not multiples of 160), the shortest reduction (two sub-tiles), K = 5120; bit-identical repeats; strided rows."""
    dtype = torch.bfloat16
    xo, xd = rnd((M, Kd), 971, dtype)
    wo, wd = rnd((N, Kd), 972, dtype, scale=Kd ** -0.5)
    bo, bd = rnd((N,), 973, dtype) if extras >= 1 else (None, None)
    ro, rd = rnd((M, N), 974, dtype) if extras >= 2 else (None, None)
    r2o, r2d = rnd((M, N), 975, dtype) if extras >= 3 else (None, None)
    alpha = 0.7 if extras >= 2 else 1.0
    got = K.linear4_bf16(xd, wd, bd, rd, alpha, r2d)
    ref = xo.double() @ wo.double().t()
    mag = xo.abs().double() @ wo.abs().double().t()
    if bo is not None:
        ref, mag = ref + bo.double(), mag + bo.abs().double()
    ref, mag = alpha * ref, alpha * mag
    for r in (ro, r2o):
        if r is not None:
            ref, mag = ref + r.double(), mag + r.abs().double()
    assert_bf16_close(got, ref, mag, f"linear4 {(M, N, Kd)}")
    assert torch.equal(got, K.linear4_bf16(xd, wd, bd, rd, alpha, r2d))
    if M % 2 == 0:                                                       # rows of a wider matrix (a column slice: ldx > K)
        wide = torch.cat([xd, xd.flip(0)], dim=1)
        assert torch.equal(K.linear4_bf16(wide[:, :Kd], wd, bd, rd, alpha, r2d), got)


# ---- f4: attention either side of the loop (csrc/attn_generic.hip) -----------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 1.5e-2)])
@pytest.mark.parametrize("B,H,Sq,Skv,D,causal,keep", [
    (2, 1, 300, 300, 512, False, False),       # the VAE mid block: one head of width 512, a ragged last query / key block
    (1, 1, 2560, 2560, 512, False, False),     # ... at the 40x64 latent of the benchmarked clip
    (3, 1, 384, 384, 128, False, False),       # the reduced VAE of the model tests
    (2, 12, 77, 77, 64, True, False),          # CLIP-L text self-attention: causal
    (4, 12, 77, 77, 64, True, True),           # ... with a key-padding mask (`use_attention_mask` configurations)
    (2, 2, 70, 130, 32, False, True),          # cross shapes, narrow heads, keys masked
    (1, 3, 200, 200, 256, True, False),
])
def test_attention_generic_against_exact_softmax(K, dtype, tol, B, H, Sq, Skv, D, causal, keep):
    """`fmc_attention_fwd`: softmax(q k^T scale + mask) v for head widths up to 512 with causal / key-padding masks, against the same arithmetic in fp64 on
    the same (rounded) inputs; q | k | v are slices of ONE fused projection (strided rows), as the text encoder issues them."""
    C = H * D
    g = torch.Generator().manual_seed(4100 + Sq + D)
    qkv = (torch.randn(B, max(Sq, Skv), 3 * C, generator=g) * 1.5).to(dtype)
    qd = qkv.cuda()
    q, k, v = qd[:, :Sq, :C], qd[:, :Skv, C:2 * C], qd[:, :Skv, 2 * C:]
    kk = None
    if keep:
        kk = torch.rand(B, Skv, generator=g) > 0.3
        kk[:, 0] = True                                                  # (every causal row keeps at least key 0)
    got = K.attention(q, k, v, H, causal=causal, key_keep=None if kk is None else kk.cuda())
    q64, k64, v64 = (t.double().cpu().view(B, -1, H, D).transpose(1, 2) for t in (q, k, v))
    s = q64 @ k64.transpose(-1, -2) * D ** -0.5
    mask = torch.ones(Sq, Skv, dtype=torch.bool)
    if causal:
        mask = mask.tril()
    mask = mask[None, None].expand(B, 1, Sq, Skv)
    if kk is not None:
        mask = mask & kk[:, None, None, :]
    p = s.masked_fill(~mask, float("-inf")).softmax(-1)
    want = (p @ v64).transpose(1, 2).reshape(B, Sq, C)
    assert got.shape == (B, Sq, C) and got.dtype == dtype
    err = rel_inf(got, want)
    assert err < tol, f"attention {(B, H, Sq, Skv, D, causal, keep)} {dtype}: rel-inf {err:.3e}"
    # element-wise too: a wrong tile cannot hide under the maximum (outputs are convex combinations of v rows)
    bound = (2.0 ** -7 if dtype == torch.bfloat16 else 1e-5) * v64.abs().amax(dim=(1, 2, 3)).view(B, 1, 1) * 1.5
    assert bool(((got.double().cpu() - want).abs() <= bound).all())


def test_attention_generic_refuses_what_it_does_not_take(K):
    q = torch.randn(1, 16, 80, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        K.attention(q, q, q, 2)                                          # head width 40: the hot-path kernels' shape, not this one's
    with pytest.raises(NotImplementedError):
        with torch.enable_grad():
            qg = torch.randn(1, 16, 64, device="cuda", dtype=torch.bfloat16, requires_grad=True)
            K.attention(qg, qg, qg, 1)


@pytest.mark.parametrize("M,cff,C,variant", [(80, 128, 320, 0), (81920, 1280, 320, 0), (81920, 1280, 320, 1), (320, 384, 320, 1), (400, 256, 320, 0),
                                             (20480, 2560, 640, 0), (240, 640, 640, 0), (160, 128, 320, 1)])
def test_geglu_ln_pipe(K, M, cff, C, variant):
    """`fmc_geglu_pipe_ln_bf16` (csrc/geglu_pipe.hip): LayerNorm + GEGLU projection with the gate of chunk c - 1 software-pipelined under the MFMAs of chunk c
    (two accumulator sets, no staging tile, stores straight from registers), both tilings, odd and even chunk counts, row-major and tile-major output:
    against fp32 (max norm), against the same arithmetic with the kernel's rounding points (element-wise bf16 bound), deterministic, and within bf16
    rounding of `geglu_ln_direct` (same function, other summation / gate order)."""
    dtype = torch.bfloat16
    ho, hd = rnd((M, C), 1, dtype, scale=1.5, shift=0.2)
    go, _ = rnd((C,), 2, torch.float32, scale=0.3, shift=1.0)
    bo, _ = rnd((C,), 3, torch.float32, scale=0.2)
    wo, wd = rnd((2 * cff, C), 4, dtype, scale=C ** -0.5)
    bio, bid = rnd((2 * cff,), 5, dtype, scale=0.3)
    wp = K.pack_geglu_frag(wd, 16 if variant == 1 else 32)
    out = K.geglu_ln_pipe(hd, go.cuda(), bo.cuda(), 1e-5, wp, bid, cff, variant=variant)

    def reference(round_bf16):
        r = (lambda t: t.bfloat16().float()) if round_bf16 else (lambda t: t)
        n = r(F.layer_norm(ho, (C,), go, bo, 1e-5))
        y = F.linear(n, wo, bio)
        return y[:, :cff] * F.gelu(y[:, cff:])
    ref_r, ref_f = reference(True), reference(False)
    assert rel_inf(out.float(), ref_f) < 2e-2
    err = (out.float().cpu() - ref_r).abs()
    bound = 2.0 ** -8 * ref_r.abs() + 0.02
    assert not bool((err > bound).any()), f"{int((err > bound).sum())} / {err.numel()} beyond the bound, worst {float((err - bound).max()):.3e}"
    assert torch.equal(out, K.geglu_ln_pipe(hd, go.cuda(), bo.cuda(), 1e-5, wp, bid, cff, variant=variant))
    out_nb = K.geglu_ln_pipe(hd, go.cuda(), bo.cuda(), 1e-5, wp, None, cff, variant=variant)
    y = F.linear(F.layer_norm(ho, (C,), go, bo, 1e-5), wo)
    assert rel_inf(out_nb.float(), y[:, :cff] * F.gelu(y[:, cff:])) < 2e-2
    if M % 160 == 0:
        blk = K.geglu_ln_pipe(hd, go.cuda(), bo.cuda(), 1e-5, wp, bid, cff, blocked=True, variant=variant)
        assert torch.equal(blk.view(M // 160, cff // 32, 160, 32).permute(0, 2, 1, 3).reshape(M, cff), out)
    if cff % (160 if C == 320 else 320) == 0 and M % 80 == 0:
        direct = K.geglu_ln_direct(hd, go.cuda(), bo.cuda(), 1e-5, K.pack_geglu_frag80(wd), bid, cff)
        d = (out.float() - direct.float()).abs().cpu()
        assert bool((d <= 2.0 ** -7 * ref_r.abs() + 1e-3).all())
    with pytest.raises(ValueError):
        K.geglu_ln_pipe(hd[:M - 8].contiguous(), go.cuda(), bo.cuda(), 1e-5, wp, bid, cff, variant=variant)


@pytest.mark.parametrize("M,cff,C,hw", [(81920, 1280, 320, 2560), (40960, 1280, 320, 0), (46080, 640, 320, 2560)])
def test_ff_tail_folded_output_projection_and_proj_out(K, M, cff, C, hw):
    """`fmc_linear_bf16_fftail` (gemm160p_kernel's two-segment reduction): `proj_out(ff2(g) + b2 + h) + bp + x` as ONE product `[g | h] [Wp W2 | Wp]^T + b' + x`
    on the tile-major g -- against the un-folded fp32 chain on the same rounded inputs (the fold re-rounds the weight once: bf16 noise, not bit equality),
    element-wise against the folded product in fp64 (one rounding of an fp32 accumulator), the GroupNorm partial sums against the rounded output, and
    deterministic.  The tile-major operand is built in torch: independent of the GEGLU kernels."""
    dtype = torch.bfloat16
    go, gd = rnd((M, cff), 1, dtype, scale=0.7)
    ho, hd = rnd((M, C), 2, dtype, scale=1.2, shift=0.1)
    xo, xd = rnd((M, C), 3, dtype, scale=1.0, shift=-0.2)
    w2o, w2d = rnd((C, cff), 4, dtype, scale=cff ** -0.5)
    b2o, b2d = rnd((C,), 5, dtype, scale=0.2)
    wpo, wpd = rnd((C, C), 6, dtype, scale=C ** -0.5)
    bpo, bpd = rnd((C,), 7, dtype, scale=0.2)
    blk = gd.view(M // 160, 160, cff // 32, 32).permute(0, 2, 1, 3).contiguous()
    wc, bc = K.fold_ff_tail(w2d, b2d, wpd, bpd)
    assert wc.shape == (C, cff + C) and wc.dtype == dtype and torch.equal(wc[:, cff:], wpd)
    blk = blk.view(M, cff)                                   # (same shape as the row-major tensor, private layout: as the GEGLU kernels return it)
    xres = xd.view(M // hw, hw, C) if hw else xd
    with torch.no_grad():                                    # (the GroupNorm partials are an inference-path epilogue)
        got = K.ff_tail(blk, hd, wc, bc, xres, gn_hw=hw)
    assert got.shape == xres.shape and got.dtype == dtype
    chain = F.linear(F.linear(go, w2o, b2o) + ho, wpo, bpo) + xo
    assert rel_inf(got.view(M, C), chain) < 1e-2
    a64 = torch.cat([go, ho], dim=1).double()
    folded = a64 @ wc.double().cpu().t() + bc.double().cpu() + xo.double()
    mag = a64.abs() @ wc.double().cpu().abs().t() + bc.double().cpu().abs() + xo.double().abs()
    assert_bf16_close(got.view(M, C), folded, mag, "ff_tail")
    with torch.no_grad():
        assert torch.equal(got, K.ff_tail(blk, hd, wc, bc, xres, gn_hw=hw))
    if hw:
        part, n = got._fmc_gn
        assert n == C and part.shape == (M // hw, hw // 160, 32, 2)
        v = got.float().view(M // hw, hw // 160, 160, 32, C // 32)
        assert rel_inf(part[..., 0], v.sum(dim=(2, 4))) < 1e-4 and rel_inf(part[..., 1], (v * v).sum(dim=(2, 4))) < 1e-4
    else:
        assert getattr(got, "_fmc_gn", None) is None
    # no bias anywhere
    wc0, bc0 = K.fold_ff_tail(w2d, None, wpd, None)
    assert bc0 is None
    with torch.no_grad():
        got0 = K.ff_tail(blk, hd, wc0, None, xres)
    assert rel_inf(got0.view(M, C), F.linear(F.linear(go, w2o) + ho, wpo) + xo) < 1e-2
    # the model-level switch: the pair of launches it replaces gives the same values to bf16 rounding of the intermediate
    with torch.no_grad():
        pair = K.linear(K.linear_from_blocked(blk, w2d, b2d, hd), wpd, bpd, xd)
    d = (got.view(M, C).float() - pair.float()).abs().cpu()
    assert bool((d <= 2.0 ** -6 * chain.abs() + 0.05).all())


@pytest.mark.parametrize("n_img,hw,C,N,splits,with_ln", [(32, 2560, 320, 320, 16, True), (32, 2560, 320, 320, 8, False), (18, 2560, 320, 640, 16, False),
                                                            (16, 2560, 320, 320, 16, True)])      # (the last: exactly one round of tiles, the CFG-shared half batch)
def test_linear_gnfold_groupnorm_folded_into_per_image_weights(K, n_img, hw, C, N, splits, with_ln):
    """`fmc_groupnorm_fold_linear` + `fmc_linear_bf16_imgw`: `proj(GroupNorm(x))` from the producer's partial sums without the normalised tensor -- groups
    with |mean| up to 6 sigma (the mean must cancel against the fp32 bias row built from the ROUNDED per-image weights), against fp32 GroupNorm -> linear
    (max norm), element-wise against the folded product in fp64 on the weights the kernel wrote, the LayerNorm statistics of the rounded rows, deterministic."""
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(11)
    base = torch.randn(n_img, hw, C, generator=g) * (0.5 + torch.rand(n_img, 1, C, generator=g))
    shift = (torch.rand(n_img, 1, 32, generator=g) * 12.0 - 6.0).repeat_interleave(C // 32, dim=2)       # per (image, group) offsets of up to 6 sigma
    xo = (base + shift).to(dtype).float()
    xd = xo.to(dtype).cuda()
    gam, _ = rnd((C,), 2, torch.float32, scale=0.3, shift=1.0)
    bet, _ = rnd((C,), 3, torch.float32, scale=0.3)
    wo, wd = rnd((N, C), 4, dtype, scale=C ** -0.5)
    bo, bd = rnd((N,), 5, dtype, scale=0.2)
    v = xo.view(n_img, splits, hw // splits, 32, C // 32)
    part = torch.stack([v.sum(dim=(2, 4)), (v * v).sum(dim=(2, 4))], dim=-1).contiguous()                # [n_img, splits, 32, 2]
    ln = None
    if with_ln:
        lg, lb = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
        ln = K.LnSpec(gamma=lg, beta=lb, eps=1e-5, pe=None, pe_inner=1, pe_frames=1, key=("t",), stats_only=True)
    with torch.no_grad():
        assert K.gn_fold_ok(xd, (part.cuda(), C), 32, wd, ln)
        got = K.linear_gnfold(xd, (part.cuda(), C), gam.cuda(), bet.cuda(), 32, 1e-6, wd, bd, ln)
        again = K.linear_gnfold(xd, (part.cuda(), C), gam.cuda(), bet.cuda(), 32, 1e-6, wd, bd, ln)
    assert got.shape == (n_img, hw, N) and torch.equal(got, again)
    want = F.linear(F.group_norm(xo.transpose(1, 2), 32, gam, bet, 1e-6).transpose(1, 2), wo, bo)
    assert rel_inf(got, want) < 1.2e-2
    # element-wise: the folded product in fp64 with W' rounded as the kernel rounds it (statistics in fp64 from the same partial sums)
    s = part.double().sum(dim=1)
    cnt = hw * (C // 32)
    mean = s[..., 0] / cnt
    rstd = 1.0 / torch.sqrt((s[..., 1] / cnt - mean * mean).clamp_min(0) + 1e-6)
    a = (rstd.float().repeat_interleave(C // 32, dim=1) * gam[None, :])                                  # [n_img, C] as the kernel forms it (fp32)
    wq = (wo[None] * a[:, None, :]).to(dtype).double()                                                   # [n_img, N, C]
    xc = xo.double() - mean.repeat_interleave(C // 32, dim=1)[:, None, :]
    folded = torch.einsum("imc,inc->imn", xc, wq) + (wo.double() @ bet.double() + bo.double())[None, None, :]
    mag = torch.einsum("imc,inc->imn", xc.abs(), wq.abs()) + (wo.double().abs() @ bet.double().abs() + bo.double().abs())[None, None, :]
    assert_bf16_close(got, folded, mag * 4, "linear_gnfold")            # (x4: a weight whose fp32 scale differs by an ulp may round the other way)
    if with_ln:
        stats, key, only = got._fmc_ln
        assert only and key == ("t",)
        r = got.float().cpu().view(-1, N)
        assert rel_inf(stats[:, 0], r.mean(dim=1)) < 1e-3 and rel_inf(stats[:, 1], (r.var(dim=1, unbiased=False) + 1e-5).rsqrt()) < 1e-3

"""Fixed inputs and the four temporal-attention entry points on them, shared by tests/test_gpu_clip_lengths.py and
tests/golden/make_golden_clip_lengths.py (which records the whole-tile results, F = 16 and F = 32, that the partial-tile work
must leave bit-identical)."""
import torch

GOLD_B, GOLD_P, GOLD_H, GOLD_D = 1, 2, 4, 40          # small P: a few KB per array; GH = 4 heads = the 4-wave units of the product shapes


def hashed(shape, salt, scale=1.0):
    """Deterministic pseudo-random fp32 values in (-scale, scale) from integer arithmetic only (no generator whose stream
    could differ between library versions): Knuth's multiplicative hash of the element index."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64) + 1 + 7919 * salt
    h = (i * 2654435761) % (1 << 32)
    h = (h ^ (h >> 15)) * 2246822519 % (1 << 32)
    h = h ^ (h >> 13)
    return ((h.double() / float(1 << 32) - 0.5) * 2.0 * scale).float().reshape(shape)


def quant_e4m3(x, scale):
    """per-tensor e4m3 quantisation as the projection epilogue does it: sat(x / scale) -> float8_e4m3fn"""
    return (x.float() / scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def bits(t):
    """Tensor -> numpy array of its raw bits (bf16 as int16, fp32 as int32)."""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def full_tile_outputs(K, Fr):
    """The four entry points (fmc_temporal_attn_fwd / _bwd in both storage types, fmc_temporal_attn_fp8_fwd / _bwd) on fixed
    inputs of `Fr` frames in the native fused `[B, F, P, 3C]` layout -> {name: raw bits}."""
    import ctypes  # noqa: F401
    from synfmc_amd import _lib
    B, P, H, D = GOLD_B, GOLD_P, GOLD_H, GOLD_D
    C = H * D
    out = {}
    qkv32 = hashed((B, Fr, P, 3 * C), 1, 1.5)
    do32 = hashed((B, Fr, P, C), 2, 1.0)
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        qkv, do = qkv32.to(dtype).cuda(), do32.to(dtype).cuda()
        out[f"fwd_{tag}"] = bits(K.temporal_attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], H))
        xg = qkv.clone().requires_grad_(True)
        K.temporal_attention(xg[..., :C], xg[..., C:2 * C], xg[..., 2 * C:], H).backward(do)
        out[f"bwd_{tag}"] = bits(xg.grad)
    # fp8: fixed per-tensor scales, e4m3 bytes made on the CPU
    scales = torch.tensor([1.5, 1.5, 1.5]) * 1.25 / 448.0
    q8 = torch.cat([quant_e4m3(qkv32[..., i * C:(i + 1) * C], float(scales[i])) for i in range(3)], dim=-1).cuda()
    sc = scales.cuda()
    out["fp8_fwd"] = bits(K._temporal_fp8_raw(q8, sc, H, D ** -0.5))
    q, k, v = q8[..., :C], q8[..., C:2 * C], q8[..., 2 * C:]
    do = do32.bfloat16().cuda()
    dqkv = torch.empty(q8.shape, dtype=torch.bfloat16, device="cuda")
    dq, dk, dv = dqkv[..., :C], dqkv[..., C:2 * C], dqkv[..., 2 * C:]
    Bq, Pq, Fq, cs, fs, ps = K._tstrides(q)
    _, _, _, ocs, ofs, ops = K._tstrides(do)
    _, _, _, dcs, dfs, dps = K._tstrides(dq)
    _lib.check(_lib.load().fmc_temporal_attn_fp8_bwd(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), sc.data_ptr(), do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
        Bq, Pq, Fq, H, D, cs, fs, ps, ocs, ofs, ops, dcs, dfs, dps, float(D ** -0.5), K._stream()), "fmc_temporal_attn_fp8_bwd")
    torch.cuda.synchronize()
    out["fp8_bwd"] = bits(dqkv)
    return out

"""OCP MXFP8 in plain torch (float64; imports no GPU code): the reference quantiser and dequantiser of csrc/gemm_mxfp8.hip, the row order of its packed GEGLU
weight, float64 references and plain-torch emulations of the kernels' rounding chains, and the assertions that test_gpu_mxfp8.py applies (test_mxfp8_host.py
shows on the CPU that the emulations meet them and that wrong stand-ins do not).

Format: elements e4m3fn, one E8M0 byte per 32 consecutive elements of the last axis.  A block with amax > 0 has the shared exponent e = floor(log2 amax) - 8
and the byte clamp(e + 127, 0, 254); elements are x * 2^-e, clamped to +-448 (the scaled amax lies in [256, 512): saturation happens), rounded to nearest even.
An all-zero block: byte 0, zero elements.  Inputs are finite.

Bounds (profiles/mxfp8_ff.md has the derivations):
  * bf16 output of the GEMM: `assert_bf16_close`, 2^-8 |ref| + 1e-5 sum |terms|, the reference float64 on the dequantised operands;
  * MXFP8 output of the GEGLU GEMM: |dq(got) - clamp(ref)| <= half an e4m3 step at the emitted scale + F, F = 1e-5 sum |terms| of the value and the gate
    (through |gelu| <= |gate| and |gelu'| <= 1.13) + 2^-21 |ref| for the hardware reciprocal and exp2 of `fmc_gelu_fast`; the emitted scale byte lies
    between the bytes of the block's amax of |ref| - F and |ref| + F;
  * LayerNorm + quantise: the kernel's normalised value differs from float64 by at most LN_EPS_REL (|y| + |beta| + |gamma| sqrt C) (counted fp32
    roundings); an element may therefore land one e4m3 step away where it is within that of a rounding tie, and a whole block may move by one scale byte
    where its amax is within that of a power of two.  Elements: the MXFP8 bound above with that error as F (half a step at the EMITTED scale); the SHARE
    of elements whose bytes differ from the float64 chain's is capped at LN_DIFF_SHARE.
"""
import math

import torch

TILE_M, TILE_N = 128, 128            # fmc_mxfp8_tile_rows / _cols: token rows and weight rows of a workgroup (GEGLU: 64 output columns)
E4M3_MAX = 448.0
LN_EPS_REL = 2.0 ** -20              # 16 fp32 roundings of half an ulp (2^-24) each on the path of one normalised value: statistics (mean, centred square sum over C
                                     # terms in pairwise-like lane order: log2-depth), rsqrt (1 ulp), 3 multiplies / adds of the affine map
LN_DIFF_SHARE = 0.02                 # share of elements allowed to differ from the float64 chain (ties / amax at a power of two); the fp32 emulation stays below it


def _floor_log2(a):
    """floor(log2 a) of positive float64 values, exact (frexp)."""
    _, ex = torch.frexp(a)
    return ex - 1


def scale_bytes(amax):
    """E8M0 byte of blocks with these amax (float64, >= 0)."""
    byte = (_floor_log2(amax.clamp_min(1e-300)) - 8 + 127).clamp(0, 254)
    return torch.where(amax > 0, byte, torch.zeros_like(byte)).to(torch.uint8)


def round_e4m3(v, mode="rne", saturate=True):
    """float64 values -> the nearest e4m3fn values (float64).  `mode` / `saturate`: the wrong stand-ins of the host test."""
    a = v.abs()
    if saturate:
        a = a.clamp_max(E4M3_MAX)
    e = _floor_log2(a.clamp_min(1e-300)).clamp_min(-6)                      # binade; below 2^-6 the subnormal step 2^-9
    step = torch.ldexp(torch.ones_like(a), e - 3)
    q = (a / step)
    q = torch.round(q) if mode == "rne" else torch.floor(q)
    return torch.copysign(q * step, v)


def encode_e4m3(v):
    """Exact e4m3fn values (float64, |v| <= 448) -> bytes."""
    a = v.abs()
    e = _floor_log2(a.clamp_min(1e-300)).clamp_min(-6)
    normal = a >= 2.0 ** -6
    mant = torch.where(normal, a / torch.ldexp(torch.ones_like(a), e) * 8 - 8, a * 512).round().to(torch.int64)
    expo = torch.where(normal, e + 7, torch.zeros_like(e)).to(torch.int64)
    sign = (torch.signbit(v)).to(torch.int64) << 7
    return (sign | (expo << 3) | mant).to(torch.uint8)


def decode_e4m3(b):
    b = b.to(torch.int64)
    mant, expo = (b & 7).double(), (b >> 3) & 15
    mag = torch.where(expo > 0, torch.ldexp(1 + mant / 8, (expo - 7).to(torch.int32)), mant / 512)
    return torch.where((b >> 7) > 0, -mag, mag)


def quantize(x, block=32, mode="rne", saturate=True):
    """x `[..., K]` -> (bytes `[..., K]` uint8, scales `[..., K / 32]` uint8).  `block`, `mode`, `saturate`: the wrong stand-ins."""
    x = x.double()
    K = x.shape[-1]
    assert K % 32 == 0 and K % block == 0
    b = x.reshape(*x.shape[:-1], K // block, block)
    byte = scale_bytes(b.abs().amax(-1))
    scaled = torch.ldexp(b, (127 - byte.to(torch.int32)).unsqueeze(-1))
    q = round_e4m3(scaled, mode, saturate)
    qb = encode_e4m3(q.clamp(-E4M3_MAX, E4M3_MAX))
    if not saturate:                                                       # (an unsaturated cast: the NaN pattern, as torch's own cast gives)
        qb = torch.where(q.abs() > E4M3_MAX, qb | 0x7F, qb)
    if block != 32:
        byte = byte.reshape(*x.shape[:-1], K // 32, 32 // block)[..., 0]   # (a stand-in's scale array keeps the format's shape)
    return qb.reshape(x.shape), byte


def dequantize(q, s):
    """(bytes `[..., K]`, scales `[..., K / 32]`) -> float64 `[..., K]`."""
    K = q.shape[-1]
    v = decode_e4m3(q).reshape(*q.shape[:-1], K // 32, 32)
    return torch.ldexp(v, (s.to(torch.int32) - 127).unsqueeze(-1)).reshape(q.shape)


def geglu_pack_rows(inner):
    """Source row of every packed row of `fmc_mxfp8_pack_weight(geglu_inner = inner)`: packed 64 t + 32 g + c <- g * inner + 32 t + c."""
    p = torch.arange(2 * inner)
    return ((p >> 5) & 1) * inner + (p >> 6) * 32 + (p & 31)


# ---- GELU as the kernels compute it (csrc/common.h: fmc_gelu_fast), float64 or float32 ---------------------------------------------------------------------
def gelu_fast(g):
    g2 = (g * g).clamp_max(81.0)
    s = (1.0142630198970437e-3 * g2 - 0.10677571594715118) * g2 - 2.301121234893799
    return g / (1 + torch.exp2(g * s))


# ---- references ---------------------------------------------------------------------------------------------------------------------------------------------
def linear_reference(xq, xs, wq, ws, bias=None, residual=None):
    """float64 product on the dequantised operands: (ref, sum |terms|)."""
    x, w = dequantize(xq, xs), dequantize(wq, ws)
    ref, mag = x @ w.T, x.abs() @ w.abs().T
    for t in (bias, residual):
        if t is not None:
            ref, mag = ref + t.double(), mag + t.double().abs()
    return ref, mag


def geglu_reference(xq, xs, wq, ws, bias, inner):
    """float64 GEGLU value on the dequantised operands (weights in the MODULE's row order: value rows, then gate rows): (ref, F) with F the fp32 term of
    the bound (module docstring)."""
    x, w = dequantize(xq, xs), dequantize(wq, ws)
    y, mag = x @ w.T, x.abs() @ w.abs().T
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    v, g = y[:, :inner], y[:, inner:]
    ref = v * gelu_fast(g)
    F = 1e-5 * (mag[:, :inner] * g.abs() + 1.13 * v.abs() * mag[:, inner:]) + 2.0 ** -21 * ref.abs()
    return ref, F


def layernorm_reference(h, gamma, beta, eps):
    """float64 LayerNorm and the per-element bound of the kernel's fp32 value."""
    x = h.double()
    C = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    err = LN_EPS_REL * (y.abs() + beta.double().abs() + gamma.double().abs() * math.sqrt(C))
    return y, err


# ---- plain-torch emulations of the kernels' rounding chains (fp32 where the kernels are) ----------------------------------------------------------------------
def emulate_linear(xq, xs, wq, ws, bias=None, residual=None):
    acc = (dequantize(xq, xs).float() @ dequantize(wq, ws).float().T)
    if bias is not None:
        acc = acc + bias.float()
    if residual is not None:
        acc = acc + residual.float()
    return acc.bfloat16()


def emulate_geglu(xq, xs, wq, ws, bias, inner, block=32, swap=False):
    acc = (dequantize(xq, xs).float() @ dequantize(wq, ws).float().T)
    if bias is not None:
        acc = acc + bias.float()
    v, g = (acc[:, inner:], acc[:, :inner]) if swap else (acc[:, :inner], acc[:, inner:])
    return quantize(v * gelu_fast(g), block=block)


def emulate_layernorm_mxfp8(h, gamma, beta, eps):
    x = h.float()
    C = x.shape[-1]
    mean = x.sum(-1, keepdim=True) * (1.0 / C)
    d = x - mean
    rs = torch.rsqrt((d * d).sum(-1, keepdim=True) * (1.0 / C) + eps)
    return quantize(d * rs * gamma.float() + beta.float())


# ---- assertions -------------------------------------------------------------------------------------------------------------------------------------------------
def e4m3_step(v):
    """The e4m3 step at magnitude v (float64, in units of the block scale)."""
    e = _floor_log2(v.clamp_min(1e-300)).clamp(-6, 8)
    return torch.ldexp(torch.ones_like(v), e - 3)


def _block_amax(t):
    return t.reshape(*t.shape[:-1], t.shape[-1] // 32, 32).amax(-1)


def assert_mx_close(got_q, got_s, ref, F, what=""):
    """The MXFP8 output bound of the module docstring.  Returns the largest err / bound."""
    got_q, got_s, ref, F = got_q.cpu(), got_s.cpu(), ref.double().cpu(), F.double().cpu()
    assert got_q.shape == ref.shape and got_s.shape == (*ref.shape[:-1], ref.shape[-1] // 32), f"{what}: shapes {tuple(got_q.shape)} {tuple(got_s.shape)}"
    lo, hi = scale_bytes(_block_amax((ref.abs() - F).clamp_min(0))), scale_bytes(_block_amax(ref.abs() + F))
    bad_s = (got_s < lo) | (got_s > hi)
    assert not bool(bad_s.any()), f"{what}: {int(bad_s.sum())} / {bad_s.numel()} scale bytes outside [byte(amax - F), byte(amax + F)], first at {tuple(bad_s.nonzero()[0].tolist())}"
    scale = torch.ldexp(torch.ones(got_s.shape, dtype=torch.float64), got_s.to(torch.int32) - 127).repeat_interleave(32, -1)
    target = torch.minimum(torch.maximum(ref, -E4M3_MAX * scale), E4M3_MAX * scale)
    bound = 0.5 * e4m3_step((target.abs() + F) / scale) * scale + F
    err = (dequantize(got_q, got_s) - target).abs()
    bad = err > bound
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} / {bad.numel()} elements beyond half an e4m3 step + the fp32 term, worst err / bound "
                                 f"{float((err / bound.clamp_min(1e-300)).max()):.3f} at {tuple(bad.nonzero()[0].tolist())}")
    return float((err / bound.clamp_min(1e-300)).max())


def assert_ln_mx_close(got_q, got_s, h, gamma, beta, eps, what=""):
    """LayerNorm + quantise against the float64 chain (module docstring).  Returns (worst err / bound, share of differing bytes)."""
    y, err = layernorm_reference(h.cpu(), gamma.cpu(), beta.cpu(), eps)
    worst = assert_mx_close(got_q, got_s, y, err, what)
    rq, rs = quantize(y)
    share = float((rq != got_q.cpu()).double().mean())
    share_s = float((rs != got_s.cpu()).double().mean())
    assert share <= LN_DIFF_SHARE and share_s <= LN_DIFF_SHARE, f"{what}: {share:.4f} of the bytes and {share_s:.4f} of the scales differ from the float64 chain (cap {LN_DIFF_SHARE})"
    return worst, share

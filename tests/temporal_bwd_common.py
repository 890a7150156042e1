"""Reference, bound, inputs and CPU emulations of the temporal-attention backward tests (pure torch, runs on the CPU).

The kernel (`temporal_attn_bwd_kernel`, synfmc_amd/csrc/temporal_attn.hip) works on the native `[B, F, P, C]` tensors: attention over
the frame axis per (clip, pixel, head).  The reference is `attn_bwd_common.reference_backward` -- the float64 closed form with the sum
of |terms| behind every element -- on the `(b p) f c` rearrangement of the rounded inputs, mapped back to the native layout.

Bound in bf16 storage: `assert_grad_close` with c = 2^-7 = 2 roundings x 2^-8.  Counted in the source: the kernel saves no O, it
recomputes P and `rowsum(P * dP)` in fp32 from the staged inputs, and rounds

    dV   2   P (`make_f4(p4, pf[qt])`, layout L2), the output (`st4` into the dV tile; the copy to global memory is exact)
    dQ   2   scale * dS (`make_f4(d4, dsf[kt])`, layout L1), the output (`st4` into the dQ tile)
    dK   2   scale * dS (`make_f4(d4, dsf[qt])`, layout L2), the output (`st4` into the dK tile)

The fp8 entry stages `bf16(float(byte) * scale)` and runs the same arithmetic: the same two roundings against the closed form on those
staged values.  fp32 storage: the project's `C_F32 = 1e-4` (split-bf16 x3 products).

Used by test_temporal_bwd_reference_host.py (CPU) and test_gpu_temporal_backward.py.
"""
import torch

from tests import attn_bwd_common as AB

BF = torch.bfloat16

# (B, F, P, H, D) -> what it exercises; GH = heads per workgroup as the launch code picks it (the largest divisor of H with GH * D <= 320
# whose seven LDS tiles of ceil16(F) rows fit in 150 KiB), written down here by hand: bf16 / fp32 storage.
CASES = {
    (3, 16, 5, 8, 40): "GH 8 / 8: two heads per wave; bf16 stages with every load first at 40 chunks per row",
    (3, 16, 5, 8, 160): "GH 2 / 2: clips, pixels and four head groups together, two waves",
    (2, 32, 3, 8, 80): "GH 4 / 2: bf16 two groups, fp32 four groups",
    (2, 32, 3, 8, 160): "GH 2 / 1: fp32 one wave, eight groups",
    (2, 32, 3, 8, 40): "GH 8 / 4: fp32 one head per wave",
    (2, 7, 5, 8, 40): "GH 8 / 8: partial single tile on the staged path",
    (2, 17, 3, 8, 80): "GH 4 / 2: one valid row in the second tile",
    (2, 31, 3, 8, 160): "GH 2 / 1: second tile one frame short",
    (2, 15, 3, 4, 8): "GH 4 / 4: D = 8, the `d0 < D` and `dO_ < D` masks; 64 chunks for 256 threads",
    (2, 16, 3, 6, 40): "GH 6 / 6: uneven over four waves",
    (2, 16, 3, 3, 80): "GH 3 / 3: uneven over two waves",
    (2, 16, 3, 8, 16): "GH 8 / 8: D = 16",
    (2, 24, 3, 8, 32): "GH 8 / 4: D = 32",
    (2, 25, 3, 4, 64): "GH 4 / 2: D = 64",
    (1, 1, 4, 8, 40): "GH 8 / 8: one frame -- P = 1, dQ = dK = 0, dV = dO",
}
SHARP_CASES = [(3, 16, 5, 8, 40), (2, 17, 3, 8, 80)]                   # run again with logits four times as large
SHARP = 4.0
FP8_CASES = [(3, 16, 5, 8, 40), (3, 16, 5, 8, 160), (2, 17, 3, 8, 80), (2, 32, 3, 8, 40)]
FP8_POW2_SCALES = (0.5, 0.25, 1.0)                                     # q, k, v: `byte * scale` is exact in bf16
KEYS = ("dq", "dk", "dv")


def case_id(case):
    return "b%d_f%d_p%d_h%d_d%d" % case


def _seed(case):
    return 6000 + 10 * list(CASES).index(case)


def make_inputs(case, dtype, logit_scale=1.0):
    """`(qkv [B, F, P, 3C], dO [B, F, P, C])` as fp32 CPU tensors holding values of `dtype`; `logit_scale` multiplies q."""
    B, Fr, P, H, D = case
    C = H * D
    qkv = AB.rnd_cpu((B, Fr, P, 3 * C), _seed(case), dtype)
    if logit_scale != 1.0:
        qkv[..., :C] = (qkv[..., :C] * logit_scale).to(dtype).float()
    return qkv, AB.rnd_cpu((B, Fr, P, C), _seed(case) + 1, dtype)


def to_ref(t):
    """native `[B, F, P, C]` -> `[(B P), F, C]`"""
    B, Fr, P, C = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * P, Fr, C)


def to_native(t, B):
    N, Fr, C = t.shape
    return t.reshape(B, N // B, Fr, C).permute(0, 2, 1, 3)


def split_qkv(qkv):
    C = qkv.shape[-1] // 3
    return qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]


def reference_native(q, k, v, g, heads, scale):
    """Float64 closed form on native `[B, F, P, C]` operands: dict of dq, dk, dv, mag_dq, mag_dk, mag_dv in the native layout."""
    B = q.shape[0]
    ref = AB.reference_backward(to_ref(q), to_ref(k), to_ref(v), to_ref(g), heads, scale)
    return {key: to_native(t, B) for key, t in ref.items()}


def reference(case, dtype, logit_scale=1.0):
    qkv, g = make_inputs(case, dtype, logit_scale)
    return reference_native(*split_qkv(qkv), g, case[3], case[4] ** -0.5)


def _bf(t):
    return t.to(BF).double()


def emulate_bf16_backward(q, k, v, g, heads, scale, pad_key_unmasked=False, v_behind=None, dk_unscaled=False):
    """The bf16 kernel's rounding chain on `[N, F, C]` operands, everything else float64: round P (dV), round scale * dS (dQ, dK), round
    the outputs.  The frames fill ceil(F / 16) tiles of 16 rows; the K and V rows behind frame F are zero, so a pad key has score 0.

    Faults (each must fail the bound):
      pad_key_unmasked   the pad keys' scores are not replaced by -inf: they take part in the softmax
      v_behind           `[N, pad, C]`: what a kernel does that neither zeroes V's pad rows nor keeps the pad keys out of
                         `rowsum(P * dP)`: the V rows that follow the clip in memory enter the row sum with the weight of score 0
      dk_unscaled        dK without the softmax scale
    Returns dq, dk, dv `[N, F, C]`."""
    N, Fr, C = q.shape
    pad = -Fr % 16
    qh, kh, vh, gh = (AB._heads(t, heads) for t in (q, k, v, g))
    S = qh @ kh.transpose(-1, -2) * scale
    if pad_key_unmasked and pad:
        P = torch.softmax(torch.cat([S, S.new_zeros(*S.shape[:-1], pad)], -1), dim=-1)[..., :Fr]
    else:
        P = torch.softmax(S, dim=-1)
    dP = gh @ vh.transpose(-1, -2)
    rowsum = (P * dP).sum(-1, keepdim=True)
    if v_behind is not None and pad:
        w = torch.exp(-torch.logsumexp(S, dim=-1, keepdim=True))                    # exp(0) over the sum of the valid keys' exp(S)
        rowsum = rowsum + (w * (gh @ AB._heads(v_behind, heads).transpose(-1, -2))).sum(-1, keepdim=True)
    dS, Pb = _bf(scale * P * (dP - rowsum)), _bf(P)
    dk = AB._merge(dS.transpose(-1, -2) @ qh)
    return dict(dq=_bf(AB._merge(dS @ kh)), dk=_bf(dk / scale if dk_unscaled else dk), dv=_bf(AB._merge(Pb.transpose(-1, -2) @ gh)))


def decode_extents_swapped(t, groups):
    """A native `[B, F, P, C]` gradient as a kernel leaves it whose unit decode takes the pixel and head-group extents for each other
    (`hg = u % n_pix; pix = (u / n_pix) % groups`): the units with `hg >= groups` do not exist, so head group hg of pixel pix is written
    only where `hg < n_pix` and `pix < groups`; everything else keeps the zeros of this buffer.  (Merely exchanging the ORDER of the two
    indices is a bijection of the units and changes nothing.)"""
    B, Fr, P, C = t.shape
    cw = C // groups
    out = torch.zeros_like(t)
    for pix in range(min(P, groups)):
        for hg in range(min(groups, P)):
            out[:, :, pix, hg * cw:(hg + 1) * cw] = t[:, :, pix, hg * cw:(hg + 1) * cw]
    return out


def _split(t):
    hi = t.to(BF).double()
    return hi, (t - hi).to(BF).double()


def _mm3(a, b):
    """`a @ b` as the fp32-storage kernels form it: both operands split into bf16 hi + lo, the lo * lo product dropped."""
    (ah, al), (bh, bl) = _split(a), _split(b)
    return ah @ bh + ah @ bl + al @ bh


def emulate_f32_backward(q, k, v, g, heads, scale):
    """fp32 storage: every matrix product as three split-bf16 products (see the header of temporal_attn.hip), everything else float64."""
    qh, kh, vh, gh = (AB._heads(t, heads) for t in (q, k, v, g))
    P = torch.softmax(_mm3(qh, kh.transpose(-1, -2)) * scale, dim=-1)
    dP = _mm3(gh, vh.transpose(-1, -2))
    dS = scale * P * (dP - (P * dP).sum(-1, keepdim=True))
    return dict(dq=AB._merge(_mm3(dS, kh)), dk=AB._merge(_mm3(dS.transpose(-1, -2), qh)), dv=AB._merge(_mm3(P.transpose(-1, -2), gh)))


def fp8_inputs(case, scales):
    """Seeded e4m3 bytes `[B, F, P, 3C]` (uint8) and what the backward stages from them: `bf16(float(byte) * scale)` per block -- an
    fp32 multiply, then round-to-nearest-even -- as fp32; `scales` a float32 tensor of three."""
    B, Fr, P, H, D = case
    C = H * D
    x = torch.randn(B, Fr, P, 3 * C, generator=torch.Generator().manual_seed(_seed(case) + 5)) * 2.0
    q8 = x.to(torch.float8_e4m3fn)
    s = scales.float().reshape(3, 1).expand(3, C).reshape(3 * C)
    return q8.view(torch.uint8), (q8.float() * s).to(BF).float()

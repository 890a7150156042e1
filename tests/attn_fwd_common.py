"""Shared by tests/test_gpu_attn_forward_elementwise.py (GPU) and tests/test_attn_fwd_reference_host.py (CPU): the case table of every attention
forward kernel and instantiation the default dispatch reaches, a Python restatement of that dispatch, the two input generators, the float64 references
of output and LSE, the element-wise bounds composed from a table of each kernel's rounding points, a plain-torch emulation of each rounding chain and
the wrong stand-ins the bounds have to catch.  profiles/attn_forward_bounds.md is the record (source lines, derivations, measured shares).

Two instruments, every case gets both:

* EXACT runs.  Every ABI forms `scale_log2 = scale * LOG2E` in fp32; with `scale = float32(0.6931472) * 2^-k` that product is exactly 2^-k
  (`exact_scale`, asserted with numpy float32).  Integer q (three nonzero entries per row, multiples of 2^k) and k in {-1, 0, 1} make every logit an
  integer n_ij in log2 units, so p_ij = 2^(n_ij - m) is a power of two whatever reference m the kernel picks and whether or not it rounds p to bf16.
  With integer v in [-2, 2], a logit range <= 8 per row and Skv * max|v| <= 2^13 (asserted on the reference, `assert_exact_conditions`) every partial
  sum of numerator and denominator fits in 21 bits: exact in fp32 in ANY order, tiling or wave split.  The kernel's output is the float64 result after
  one division and one output rounding: |got - ref| <= 2^-8 |ref| + c sum_j p_ij |v_jc| (bf16 storage), c sum_j p_ij |v_jc| (fp32 storage),
  plus 2^-9 sum_j p_ij |v_jc| for a kernel that rounds the NORMALISED p (none does: the temporal kernels did, and missed this bound for it).  A dropped key, a mis-paired value, a pad key, a
  truncated output move most elements beyond that.
* ROUNDED runs.  Gaussian data as tests/test_gpu_kernels.py makes it; the bound of `reference` (`rounded_out`, `rounded_lse`), composed from the
  family's rounding points.

The reference takes the logits as `scale_log2 * q.k` in log2 units with the fp32 product `scale_log2 = scale * LOG2E` every entry point forms
(`fmc_spatial_attn_fwd`, `ta_fill` of temporal_attn.hip, `fmc_attention_fwd`; within 2^-23 of scale * log2(e)), evaluated in float64 on the operands as stored."""
import functools
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

F64 = torch.float64
LOG2E32 = np.float32(1.4426950408889634)            # `constexpr float LOG2E` of spatial_attn.hip:36, temporal_attn.hip:30, the literal in `fmc_attention_fwd`
LN2 = math.log(2.0)
SA_BQ, SA_BK, REF_LIMIT = 128, 64, 64.0             # spatial_attn.hip:33, :35, :62

Case = namedtuple("Case", "abi dtype B H Sq Skv D kvdiv layout kernel k2 spike causal keep pix")


# =====================================================================================================================================================
# dispatch restatement (csrc/spatial_attn.hip, csrc/temporal_attn.hip, csrc/attn_generic.hip)
# =====================================================================================================================================================
def xcd_remap(B, H):
    """`P.xcd_remap` in `fmc_spatial_attn_fwd`."""
    return 2 if B % 8 == 0 else (1 if (B * H) % 8 == 0 else 0)


def expected_kernel(dtype, B, H, Sq, Skv, D, kv_div):
    """The kernel `fmc_spatial_attn_fwd` launches with every A/B switch at its default."""
    bf = dtype == "bf16"
    if bf and D == 40 and H == 8 and 1 <= Skv <= 96 and Sq % 32 == 0 and B % kv_div == 0:                       # xattn40_ok (asked first by fmc_spatial_attn_fwd)
        return "xattn40_kernel"
    if bf and D == 80 and Skv % 32 == 0 and Skv >= 256 and Sq >= 160:                                          # sa_big80_ok (second)
        return "sa_big80_kernel_w10"                                                                           # launch_sa_big80: SASwitches::big80_waves, default 10
    if bf and D == 160 and Skv <= 160:                                                                         # sa_small_ok (third)
        return "sa_small160_kernel<3>" if Skv <= 96 else "sa_small160_kernel<5>"                               # launch_sa_small
    if bf and D == 40 and Skv % SA_BK == 0 and Skv >= 2 * SA_BK and Sq % 256 == 0:                             # sa40_ok (fourth); krs * 2 * Skv < 2^31
        return "sa40d_kernel"                                                                                  # holds at every size here
    nks = (D + 15) // 16                                                                                       # fmc_pick_nks (attn_common.h)
    assert nks in (1, 2, 3, 4, 5, 6, 8, 10), D
    short = Skv <= 2 * SA_BK                                                                                   # launch_sa
    pf, nq, mk, vr = False, 1, False, False
    if bf and nks <= 6 and (Skv > SA_BK if short else True):                                                   # launch_sa_forms: `prefetch` (SA_PREFETCH_DEFAULT)
        pf = True
        if nks <= 3 and Sq >= 2 * SA_BQ:                                                                       # launch_sa_forms: SASwitches::nq, default 2
            nq, vr = 2, True                                                                                   # SASwitches::vr, default 1
            mk = D % 16 == 8                                                                                   # SASwitches::mk, default 1
    return tiled_name(dtype, nks, short, pf, nq, mk, vr)


def tiled_name(dtype, nks, short, pf, nq, mk, vr):
    return f"spatial_attn_kernel<{dtype},{nks},{int(short)},{int(pf)},{nq},{int(mk)},{int(vr)}>"


def default_tiled_instantiations():
    """Every `spatial_attn_kernel` instantiation that `launch_sa` (through `launch_sa_forms`, once per SHORT_KV) can reach with the switches at their defaults, listed from the template
    arguments of its `launch_sa_v` calls -- NOT from `expected_kernel`."""
    names = set()
    for nks in (1, 2, 3, 4, 5, 6, 8, 10):
        for short in (True, False):
            names.add(tiled_name("fp32", nks, short, False, 1, False, False))           # sizeof(T) == 4: the last line of launch_sa_forms only
            if short or nks > 6:                                                         # the last line: short, Skv <= SA_BK; long only for NKS > 6
                names.add(tiled_name("bf16", nks, short, False, 1, False, False))
            if nks <= 6:
                names.add(tiled_name("bf16", nks, short, True, 1, False, False))        # `launch_sa_v<T, NKS, SHORT_KV, true>`
            if nks <= 3:
                names.add(tiled_name("bf16", nks, short, True, 2, True, True))          # `<.., true, 2, true, true>`  (D % 16 == 8)
                names.add(tiled_name("bf16", nks, short, True, 2, False, True))         # `<.., true, 2, false, true>`
    return names


SPECIAL_KERNELS = {"xattn40_kernel", "sa_big80_kernel_w10", "sa_small160_kernel<3>", "sa_small160_kernel<5>", "sa40d_kernel"}


def temporal_kernel(dtype, F, H, D, fp8=False):
    """temporal_attn.hip, `launch_ta` (and `launch_ta8` for fp8) through `ta_dispatch`: tiles, k-steps, waves, partial flag."""
    gh = 1
    for g in range(1, H + 1):                                                                                  # ta_head_group, with the fp8 forward's `extra`
        if H % g == 0 and g * D <= 320 and (not fp8 or (g * D) % 16 == 0):
            gh = g
    nw = 4 if gh >= 4 else (2 if gh >= 2 else 1)                                                               # ta_waves
    ft, part = (1 if F <= 16 else 2), F not in (16, 32)                                                        # ta_tiles
    return f"temporal_attn_{'fp8_' if fp8 else ''}kernel<{dtype},{ft},{(D + 31) // 32},{nw},{int(part)}>", gh, nw


# =====================================================================================================================================================
# rounding points, per kernel family (profiles/attn_forward_bounds.md has the table with the derivations)
# =====================================================================================================================================================
# q_round   the pre-scaled q is rounded (bf16: p_frag of q * scale_log2; fp32 storage: split into hi + lo, 16 bits)
# p_norm    p is rounded AFTER the normalisation (p * 1/l), otherwise before it
# l_rounded the denominator is summed from the rounded p (ones row / column of V in the PV MFMAs), otherwise from the fp32 p
# ref       "tile": fixed reference = row maximum over the first `ref_keys` keys with a redo pass per workgroup of `wg_rows` rows; "exact": row maximum
# mk        the reference is rounded to bf16 (it rides in the QK^T reduction)
# lse       m * ln2 + logf(l) in fp32
Family = namedtuple("Family", "q_round p_norm l_rounded ref ref_keys wg_rows mk lse src")
FAMILIES = {
    # spatial_attn.hip: q :350-353 / :364-365, p :169 / :239 (p_frag), l :158-163 + :529-530, out :531-541, lse :545, reference :456-459, redo :516-522
    "tiled_odd": Family(True, False, True, "tile", 64, 128, False, True, "spatial_attn.hip:350,169,529,540,545"),
    "tiled_even": Family(True, False, False, "tile", 64, 128, False, True, "spatial_attn.hip:350,169,530,540,545"),
    "tiled_nq2": Family(True, False, True, "tile", 64, 256, False, True, "spatial_attn.hip:350,239,529,540,545"),
    "tiled_nq2_even": Family(True, False, False, "tile", 64, 256, False, True, "spatial_attn.hip:350,239,530,540,545"),
    "tiled_nq2_mk": Family(True, False, True, "tile", 64, 256, True, True, "spatial_attn.hip:350,440,239,529,540,545"),
    "sa40d": Family(True, False, True, "tile", 64, 256, True, True, "spatial_attn.hip:857,886-899"),
    "xattn40": Family(True, False, True, "exact", 0, 0, False, True, "spatial_attn.hip:990-991,1032-1039,1044-1056"),
    "small160": Family(True, False, False, "exact", 0, 0, False, True, "spatial_attn.hip:1088-1089,1222-1232"),
    "big80": Family(True, False, True, "tile", 32, 320, False, True, "spatial_attn.hip:1309-1312,1328,1369-1388"),
    # temporal_attn.hip: scale after the MFMA :237, exact maximum :239-242, l from the fp32 p :247-249, p rounded as it leaves the exp :257-258,
    # 1 / l on the PV accumulator and the output rounding :288-289; fp8: :418, :428-430, scale_v / l :431, p :435-436, output :454-455
    "temporal": Family(False, False, False, "exact", 0, 0, False, False, "temporal_attn.hip:237,247,253-258,288-289"),
    "temporal_fp8": Family(False, False, False, "exact", 0, 0, False, False, "temporal_attn.hip:418,428,431-436,454-455"),
    # attn_generic.hip: scale after the MFMA :163, running maximum :168-181, l from fp32 p :176-178, p rounded :189-197, out :218-226
    "generic": Family(False, False, False, "exact", 0, 0, False, False, "attn_generic.hip:163,175-178,189,218-226"),
}

# c: what is left of the fp32 arithmetic once every sum is exact, in units of sum_j p_ij |v_jc| (>= |ref|).  Counted in half-ulps 2^-24:
#   1  `1.f / l_tot` (IEEE division, correctly rounded)      1  the multiply `oacc * inv`
#   2  v_exp_f32, 1 ulp, entering an UNROUNDED l (a rounded p drops it: 2^n is a bf16 value)
# = 4 half-ulps = 2^-22; the additions of an unrounded l whose terms carry that last bit add at most one half-ulp each over the <= 16 in-lane
# terms of a block and the Skv / 32 blocks; 2^-20 leaves room for them.  The same figure for every kernel; far below the 2^-16 the issue allows.
C_EXACT = 2.0 ** -20
# c_lse: fp32 `m * 0.6931...f` (1 half-ulp of |m ln2|), logf (<= 2 ulp = 4 half-ulps of |log l|), the add (1 half-ulp of |lse|); |m ln2| and |log l|
# are each at most |lse| + ln(Skv 2^8) < |lse| + 14:  (1 + 4 + 1) half-ulps * (|lse| + 14) = 3.6e-7 |lse| + 5e-6  <=  2^-17 (1 + |lse|).
C_LSE = 2.0 ** -17
U_BF16 = 2.0 ** -9                                  # per bf16 rounding (the issue's figure)
U_F32 = 2e-5                                        # the split-bf16 figure of `assert_f32_close` (tests/conv_fwd_common.py)


def family(case):
    k = case.kernel
    if case.abi == "temporal":
        return "temporal"
    if case.abi == "fp8":
        return "temporal_fp8"
    if case.abi == "generic":
        return "generic"
    if k in ("xattn40_kernel", "sa40d_kernel"):
        return k.split("_")[0]
    if k.startswith("sa_small160"):
        return "small160"
    if k.startswith("sa_big80"):
        return "big80"
    _, nks, _, _, nq, mk, _ = k[k.index("<") + 1:-1].split(",")
    odd = int(nks) % 2 == 1
    if int(nq) == 2:
        return "tiled_nq2_mk" if int(mk) else ("tiled_nq2" if odd else "tiled_nq2_even")
    return "tiled_odd" if odd else "tiled_even"


# =====================================================================================================================================================
# case table
# =====================================================================================================================================================
def sp(dtype, B, H, Sq, Skv, D, kvdiv=1, layout="separate", k2=0, spike=0):
    return Case("spatial", dtype, B, H, Sq, Skv, D, kvdiv, layout, expected_kernel(dtype, B, H, Sq, Skv, D, kvdiv), k2, spike, False, False, 1)


def ta(dtype, B, P, F, H, D, layout, fp8=False):
    if layout == "nfc":
        assert B == 1
    return Case("fp8" if fp8 else "temporal", dtype, B, H, F, F, D, 1, layout, temporal_kernel(dtype, F, H, D, fp8)[0], 0, 0, False, False, P)


def ag(dtype, B, H, Sq, Skv, D, causal=False, keep=False, layout="separate"):
    return Case("generic", dtype, B, H, Sq, Skv, D, 1, layout, f"attn_generic_kernel<{dtype},{D // 32}>", 0, 0, causal, keep, 1)


TILED_SHAPES = [(33, 1), (130, 64), (130, 77), (257, 128), (33, 130), (257, 257), (257, 192)]       # (Sq, Skv): one tile, a whole tile, SA_BK < Skv <= 2 SA_BK
                                                                                                  # ragged and whole, > 2 tiles ragged (tail 1 / 2) and whole;
                                                                                                  # Sq < 2 SA_BQ and >= 2 SA_BQ, all ragged
TILED_D = [8, 16, 24, 32, 40, 48, 64, 80, 96, 128, 152, 160]                                       # NKS 1, 1, 2, 2, 3, 3, 4, 5, 6, 8, 10, 10; D % 16 == 8 and == 0 for NKS <= 3


def _tiled_cases():
    out = []
    for dtype in ("bf16", "fp32"):
        for D in TILED_D:
            for Sq, Skv in TILED_SHAPES:
                out.append(sp(dtype, 1, 2, Sq, Skv, D, k2=1 if (D, Skv) == (64, 77) else 0))
        # K/V arrangements and block orders: q | k | v slices of one fused projection; text K/V shared by 4 frames (fused k | v); xcd_remap 2, 1, 0
        out += [sp(dtype, 8, 2, 257, 257, 40, layout="fused"), sp(dtype, 4, 2, 130, 130, 24, layout="fused"), sp(dtype, 1, 3, 257, 130, 16),
                sp(dtype, 4, 2, 257, 77, 40, kvdiv=4, layout="fused_kv"), sp(dtype, 8, 2, 33, 77, 64, kvdiv=4, layout="fused_kv"),
                sp(dtype, 3, 2, 130, 257, 96, kvdiv=1, layout="fused_kv")]
    return out


TILED = _tiled_cases()
SA40D = [sp("bf16", 1, 2, 256, 128, 40), sp("bf16", 1, 2, 256, 192, 40), sp("bf16", 1, 2, 256, 320, 40), sp("bf16", 1, 2, 256, 1536, 40),
         sp("bf16", 8, 2, 256, 256, 40, layout="fused"), sp("bf16", 4, 2, 256, 128, 40), sp("bf16", 2, 5, 512, 192, 40, kvdiv=2, layout="fused_kv")]
XATTN40 = [sp("bf16", 2, 8, 32, 1, 40), sp("bf16", 4, 8, 96, 20, 40, kvdiv=2, layout="fused_kv"), sp("bf16", 1, 8, 640, 32, 40),
           sp("bf16", 16, 8, 32, 33, 40, kvdiv=16, layout="fused_kv"), sp("bf16", 2, 8, 96, 64, 40, kvdiv=2), sp("bf16", 16, 8, 96, 77, 40, kvdiv=16, layout="fused_kv"),
           sp("bf16", 2, 8, 640, 77, 40, kvdiv=2, layout="fused_kv"), sp("bf16", 3, 8, 32, 96, 40)]
SMALL160 = [sp("bf16", 3, 2, Sq, Skv, 160) for Sq, Skv in ((33, 1), (200, 77), (160, 96), (330, 100))] + [sp("bf16", 2, 2, 160, 160, 160, layout="fused")]
BIG80 = [sp("bf16", 1, 2, Sq, Skv, 80) for Sq, Skv in ((170, 256), (500, 352))] + [sp("bf16", 1, 2, 384, 384, 80, layout="fused"),
                                                                                   sp("bf16", 8, 2, 640, 640, 80, layout="fused")]
# one spike per kernel with a redo path: one row's late key lies 70 log2 units above everything else (REF_LIMIT = 64); that row is waived
SPIKES = [sp("bf16", 1, 2, 257, 257, 40, spike=1), sp("bf16", 1, 2, 130, 192, 64, spike=1), sp("fp32", 1, 2, 130, 192, 64, spike=1),
          sp("bf16", 1, 2, 256, 192, 40, spike=1), sp("bf16", 1, 2, 384, 384, 80, spike=1)]
SPATIAL = TILED + SA40D + XATTN40 + SMALL160 + BIG80 + SPIKES

# (D, H): head groups GH = 6, 5, 3, 1 -> 4, 4, 2, 1 waves: 6 heads over 4 waves, 5 over 4, 3 over 2 (uneven), 3 groups of one head
TEMPORAL_DH = [(8, 6), (40, 5), (80, 3), (160, 3)]
TEMPORAL = [ta(dtype, 2 if (i + j) % 2 == 0 else 1, 3 if (i + j) % 2 == 0 else 5, F, H, D, "native" if (i + j) % 2 == 0 else "nfc")
            for dtype in ("bf16", "fp32") for i, F in enumerate((1, 7, 16, 17, 24, 32)) for j, (D, H) in enumerate(TEMPORAL_DH)]
FP8 = [ta("bf16", 2, 3, F, H, D, "native", fp8=True) for F, (D, H) in zip((1, 7, 16, 17, 24, 32), ((8, 6), (40, 4), (80, 3), (160, 2), (40, 4), (8, 6)))]
# fmc_attention_fwd takes D in {32, 64, 128, 256, 512} only (`fmc_attention_supported`): 128 stands where the issue names 160
GENERIC = [c for dtype in ("bf16", "fp32") for c in (
    ag(dtype, 2, 2, 70, 77, 64), ag(dtype, 2, 2, 77, 77, 64, causal=True, layout="fused"), ag(dtype, 2, 2, 50, 65, 64, keep=True),
    ag(dtype, 1, 2, 33, 130, 128, causal=True, keep=True), ag(dtype, 1, 2, 130, 33, 128), ag(dtype, 1, 1, 65, 40, 512), ag(dtype, 1, 1, 40, 65, 512, causal=True))]


def all_cases():
    return SPATIAL + TEMPORAL + FP8 + GENERIC


def case_id(c):
    tag = f"{c.abi}-{c.dtype}-B{c.B}H{c.H}-{c.Sq}x{c.Skv}x{c.D}"
    if c.pix > 1 or c.abi in ("temporal", "fp8"):
        tag += f"-P{c.pix}"
    for flag, text in ((c.kvdiv > 1, f"div{c.kvdiv}"), (c.layout != "separate", c.layout), (c.k2, f"k{c.k2}"), (c.spike, "spike"), (c.causal, "causal"),
                       (c.keep, "keep")):
        if flag:
            tag += "-" + text
    return tag


# =====================================================================================================================================================
# inputs
# =====================================================================================================================================================
def exact_scale(k2):
    """`scale` with float32(scale) * float32(LOG2E) == 2^-k2 exactly."""
    scale = np.float32(0.6931472) * np.float32(2.0 ** -k2)
    assert np.float32(scale) * LOG2E32 == np.float32(2.0 ** -k2), (k2, scale)
    return float(scale)


def scale_log2(scale):
    """The fp32 product every ABI forms, as a float64."""
    return float(np.float32(scale) * LOG2E32)


def bf16r(t):
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def f32r(t):
    return t.to(torch.float32).to(F64)


def split16(t):
    hi = bf16r(t)
    return hi + bf16r(t - hi)


def truncate_bf16(t):
    return (t.to(torch.float32).view(torch.int32) & -65536).view(torch.float32).to(F64)


FP8_SCALES = (0.5, 2.0, 0.25)                       # q, k, v: powers of two (value = byte * scale)


def _groups(c):
    """(query batch, kv batch) of the canonical [G, H, S, D] tensors."""
    g = c.B * c.pix
    return g, g // c.kvdiv


def keep_mask(c):
    """`key_keep [B, Skv]`: kept keys on both sides of the 32-key stage seam, the last key masked, key 0 kept (a causal row 0 needs it)."""
    g = torch.Generator().manual_seed(977)
    keep = torch.rand(c.B, c.Skv, generator=g) < 0.6
    keep[:, 0] = keep[:, 31] = keep[:, 32] = True
    keep[:, 30] = keep[:, 33] = False
    keep[:, -1] = False
    return keep


@functools.lru_cache(maxsize=None)
def inputs(c, instrument):
    """Canonical float64 q [G, H, Sq, D], k / v [Gkv, H, Skv, D] holding exactly the values the storage type holds, and `scale`."""
    G, Gkv = _groups(c)
    g = torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()))
    if instrument == "exact":
        scale = exact_scale(c.k2)
        pos = torch.rand(G, c.H, c.Sq, c.D, generator=g).argsort(-1)[..., :3]
        q = torch.zeros(G, c.H, c.Sq, c.D, dtype=F64).scatter_(-1, pos, torch.randint(-1, 2, pos.shape, generator=g).to(F64)) * 2.0 ** c.k2
        k = torch.randint(-1, 2, (Gkv, c.H, c.Skv, c.D), generator=g).to(F64)
        v = torch.randint(-2, 3, (Gkv, c.H, c.Skv, c.D), generator=g).to(F64)
        if c.spike:
            # (group 0, head 0): channel 0 of K is zero except at the last key; query row 7 is 70 * e_0: logit 70 there, 0 at every other key
            k[0, 0, :, 0] = 0.0
            k[0, 0, -1, 0] = 1.0
            q[0, 0, 7] = 0.0
            q[0, 0, 7, 0] = 70.0 * 2.0 ** c.k2
        if c.abi == "fp8":
            sq, sk, sv = FP8_SCALES
            q, k, v = q * sq, k * sk, v * sv
    else:
        scale = float(c.D) ** -0.5
        q = torch.randn(G, c.H, c.Sq, c.D, generator=g)
        k = torch.randn(Gkv, c.H, c.Skv, c.D, generator=g)
        v = torch.randn(Gkv, c.H, c.Skv, c.D, generator=g)
        if c.abi == "fp8":
            q, k, v = ((t / s).to(torch.float8_e4m3fn).to(F64) * s for t, s in zip((q, k, v), FP8_SCALES))
        elif c.dtype == "bf16":
            q, k, v = bf16r(q), bf16r(k), bf16r(v)
        else:
            q, k, v = f32r(q), f32r(k), f32r(v)
    return {"q": q, "k": k, "v": v, "scale": scale, "keep": keep_mask(c) if c.keep else None}


def torch_dtype(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def _rows(c, t, S):
    """canonical [G, H, S, D] -> the ABI's row tensor: spatial / generic [B, S, H D]; temporal native [B, F, P, H D], reference layout [N, F, H D]."""
    G, H, _, D = t.shape
    if c.abi in ("spatial", "generic"):
        return t.permute(0, 2, 1, 3).reshape(G, S, H * D)
    if c.layout == "native":
        return t.reshape(c.B, c.pix, H, S, D).permute(0, 3, 1, 2, 4).reshape(c.B, S, c.pix, H * D)
    return t.permute(0, 2, 1, 3).reshape(G, S, H * D)


def pack(c, d):
    """The storage tensors of a case (CPU): {"qkv"} (one fused projection), {"q", "kv"} or {"q", "k", "v"}."""
    dt = torch_dtype(c)
    q, k, v = _rows(c, d["q"], c.Sq), _rows(c, d["k"], c.Skv), _rows(c, d["v"], c.Skv)
    if c.abi == "fp8":
        sq, sk, sv = FP8_SCALES
        return {"qkv": torch.cat([q / sq, k / sk, v / sv], -1).to(torch.float32).to(torch.float8_e4m3fn)}
    if c.abi in ("temporal",) or c.layout == "fused":
        return {"qkv": torch.cat([q, k, v], -1).to(dt)}
    if c.layout == "fused_kv":
        return {"q": q.to(dt).contiguous(), "kv": torch.cat([k, v], -1).to(dt)}
    return {"q": q.to(dt).contiguous(), "k": k.to(dt).contiguous(), "v": v.to(dt).contiguous()}


def views(c, bufs):
    """(q, k, v) as the (strided) views the wrappers take."""
    C = c.H * c.D
    if "qkv" in bufs:
        t = bufs["qkv"]
        return t[..., :C], t[..., C:2 * C], t[..., 2 * C:]
    if "kv" in bufs:
        return bufs["q"], bufs["kv"][..., :C], bufs["kv"][..., C:]
    return bufs["q"], bufs["k"], bufs["v"]


def canonical(c, out):
    """A kernel output (ABI layout, any device) -> float64 [G, H, Sq, D] on the CPU."""
    o = out.detach().to("cpu", F64)
    if c.abi in ("spatial", "generic") or c.layout == "nfc":
        G = o.shape[0]
        return o.reshape(G, c.Sq, c.H, c.D).permute(0, 2, 1, 3)
    return o.reshape(c.B, c.Sq, c.pix, c.H, c.D).permute(0, 2, 3, 1, 4).reshape(c.B * c.pix, c.H, c.Sq, c.D)


# =====================================================================================================================================================
# references and bounds
# =====================================================================================================================================================
def _mask(c, d, kv_index=None):
    """Additive mask [G or 1, 1, Sq, Skv] (0 / -inf) or None."""
    m = None
    if c.causal:
        m = torch.where(torch.arange(c.Skv)[None, :] <= torch.arange(c.Sq)[:, None], 0.0, -math.inf).to(F64)[None, None]
    if d["keep"] is not None:
        km = torch.where(d["keep"], 0.0, -math.inf).to(F64)[:, None, None, :]
        m = km if m is None else m + km
    return m


def logits(c, d):
    """Logits in log2 units, float64 [G, H, Sq, Skv], masked."""
    k = d["k"].repeat_interleave(c.kvdiv, 0)
    s = torch.einsum("ghid,ghjd->ghij", d["q"], k) * scale_log2(d["scale"])
    m = _mask(c, d)
    return s if m is None else s + m


def spike_rows(c):
    """Boolean [G, H, Sq]: the rows waived from the exactness conditions."""
    G, _ = _groups(c)
    w = torch.zeros(G, c.H, c.Sq, dtype=torch.bool)
    if c.spike:
        w[0, 0, 7] = True
    assert int(w.sum()) == c.spike
    return w


def _weighted_dev(w, v, ref, chunk=32):
    """sum_j w_ij |v_jc - ref_ic| without the [Sq, Skv, D] intermediate in one piece."""
    out = torch.empty_like(ref)
    for g in range(ref.shape[0]):
        for h in range(ref.shape[1]):
            for i in range(0, ref.shape[2], chunk):
                dev = (v[g, h][None, :, :] - ref[g, h, i:i + chunk][:, None, :]).abs()
                out[g, h, i:i + chunk] = torch.einsum("ij,ijc->ic", w[g, h, i:i + chunk], dev)
    return out


@functools.lru_cache(maxsize=None)
def reference(c, instrument):
    """Float64 `out` [G, H, Sq, D], `lse` [G, H, Sq] (natural log) and both instruments' bounds for the case's inputs."""
    d = inputs(c, instrument)
    fam = FAMILIES[family(c)]
    s2 = logits(c, d)
    mx = s2.amax(-1, keepdim=True)
    e = torch.exp2(s2 - mx)
    l = e.sum(-1, keepdim=True)
    p = e / l
    v = d["v"].repeat_interleave(c.kvdiv, 0)
    out = p @ v
    lse = (mx + torch.log2(l)).squeeze(-1) * LN2
    pav = p @ v.abs()
    r = {"out": out, "lse": lse, "pav": pav, "p": p, "s2": s2, "waived": spike_rows(c)}
    f32 = c.dtype == "fp32"
    # ---- rounded-run bound (also what the waived spike rows of an exact run are held to) ----
    u_q = (U_F32 if f32 else U_BF16) if fam.q_round else (U_F32 if f32 else 0.0)       # fp32 storage: the split products of Q K^T carry it either way
    u_p = U_F32 if f32 else U_BF16
    k = d["k"].repeat_interleave(c.kvdiv, 0)
    e_ij = u_q * d["scale"] * torch.einsum("ghid,ghjd->ghij", d["q"].abs(), k.abs())
    ebar = (p * e_ij).sum(-1)
    r["rounded_out"] = ((0.0 if f32 else 2.0 ** -8) * out.abs() + u_p * (pav + out.abs()) + _weighted_dev(p * (e_ij + ebar[..., None]), v, out) + 1e-5 * pav)
    r["rounded_lse"] = ebar + u_p + C_LSE * (1 + lse.abs())
    # ---- exact-run bound ----
    assert C_EXACT <= 2.0 ** -16
    ex = C_EXACT * pav + (0.0 if f32 else 2.0 ** -8) * out.abs()
    if fam.p_norm and not f32:
        ex = ex + 2.0 ** -9 * pav
    w = r["waived"]
    r["exact_out"] = torch.where(w[..., None], r["rounded_out"], ex)
    r["exact_lse"] = torch.where(w, r["rounded_lse"], C_LSE * (1 + lse.abs()))
    return r


def assert_exact_conditions(c):
    """Power-of-two scale, integer logits, logit range <= 8 and Skv * max|v| <= 2^13 outside the waived rows."""
    d, r = inputs(c, "exact"), reference(c, "exact")
    sl2 = scale_log2(d["scale"])
    assert sl2 == 2.0 ** -c.k2
    s2 = r["s2"]
    fin = torch.isfinite(s2)
    assert bool((s2[fin] == s2[fin].round()).all()), "logits must be integers in log2 units"
    hi = torch.where(fin, s2, torch.full_like(s2, -math.inf)).amax(-1)
    lo = torch.where(fin, s2, torch.full_like(s2, math.inf)).amin(-1)
    rng = torch.where(r["waived"], torch.zeros_like(hi), hi - lo)
    assert float(rng.max()) <= 8, float(rng.max())
    v_int = d["v"] / (FP8_SCALES[2] if c.abi == "fp8" else 1.0)                # fp8: the bytes are the integers, the scale leaves the sums alone
    assert torch.equal(v_int, v_int.round())
    assert c.Skv * float(v_int.abs().max()) <= 2 ** 13
    if c.spike:
        assert float((hi - lo)[r["waived"]].min()) > REF_LIMIT
    dt = torch.float8_e4m3fn if c.abi == "fp8" else torch_dtype(c)
    for name in "qkv":
        t = d[name] / (FP8_SCALES["qkv".index(name)] if c.abi == "fp8" else 1.0)
        assert torch.equal(t.to(torch.float32).to(dt).to(F64), t), f"{name} must be exact in the storage type"


def check(c, instrument, out, lse=None, what=""):
    """Every output (and LSE) element against the case's bound.  Returns the largest err / bound of output and LSE (None without LSE)."""
    r = reference(c, instrument)
    key = "exact" if instrument == "exact" else "rounded"
    got = canonical(c, out)
    assert got.shape == r["out"].shape, (what, got.shape, r["out"].shape)
    shares = []
    for name, g, ref, bound in (("out", got, r["out"], r[key + "_out"]), ("lse", lse, r["lse"], r[key + "_lse"])):
        if g is None:
            shares.append(None)
            continue
        g = g.detach().to("cpu", F64).reshape(ref.shape)
        err = (g - ref).abs()
        bad = ~(err <= bound)                                              # (a NaN is beyond every bound)
        assert not bool(bad.any()), (f"{what} {instrument} {name}: {int(bad.sum())} / {bad.numel()} elements beyond the bound, worst err / bound "
                                     f"{float((err / bound.clamp_min(1e-300))[bad].max()):.3e} at {tuple(int(i) for i in bad.nonzero()[0])}")
        shares.append(float((err / bound.clamp_min(1e-300)).max()))
    return tuple(shares)


def rel_inf(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# =====================================================================================================================================================
# emulation of each rounding chain, and the wrong stand-ins
# =====================================================================================================================================================
FAULTS = ["drop_last_key", "pad_key_counted", "mispaired_tile", "next_head_v", "kvdiv_ignored", "truncated_output", "l_first_tile", "nq2_second_block_ref",
          "causal_off_by_one", "keep_ignored_last", "lse_log2", "lse_no_redo_shift"]


def emulate(c, instrument, fault=None):
    """(out [G, H, Sq, D], lse [G, H, Sq] or None) as the case's kernel computes them, rounding where its table entry says it rounds, in plain torch:
    fp32 values held in float64 tensors.  `fault`: one of FAULTS, the same chain with that mistake."""
    d = inputs(c, instrument)
    fam = FAMILIES[family(c)]
    f32 = c.dtype == "fp32"
    rnd = split16 if f32 else bf16r
    sl2 = scale_log2(d["scale"])
    G, Gkv = _groups(c)
    idx = torch.arange(G) // c.kvdiv
    if fault == "kvdiv_ignored":
        idx = torch.arange(G) % Gkv
    q, k, v = d["q"], d["k"][idx], d["v"][idx]
    if c.abi == "fp8":
        q, k, v = q / FP8_SCALES[0], k / FP8_SCALES[1], v / FP8_SCALES[2]
        sl2 = sl2 * FP8_SCALES[0] * FP8_SCALES[1]
    if fault == "next_head_v":
        v = v.roll(-1, 1)
    if fault == "pad_key_counted":
        k = torch.cat([k, torch.zeros_like(k[:, :, :1])], 2)
        v = torch.cat([v, torch.zeros_like(v[:, :, :1])], 2)
    Skv = k.shape[2]
    if fam.q_round:
        s = f32r(torch.einsum("ghid,ghjd->ghij", rnd(f32r(q * sl2)), rnd(k) if f32 else k))
    else:
        s = f32r(f32r(torch.einsum("ghid,ghjd->ghij", rnd(q) if f32 else q, rnd(k) if f32 else k)) * sl2)
    dd = dict(d)
    if fault == "keep_ignored_last":
        dd["keep"] = d["keep"].clone()
        dd["keep"][:, -1] = True
    m = _mask(c, dd)
    if fault == "causal_off_by_one":
        m = torch.where(torch.arange(c.Skv)[None, :] <= torch.arange(c.Sq)[:, None] + 1, 0.0, -math.inf).to(F64)[None, None]
        if dd["keep"] is not None:
            m = m + torch.where(dd["keep"], 0.0, -math.inf).to(F64)[:, None, None, :]
    if m is not None:
        s = s + (m if fault != "pad_key_counted" else torch.cat([m, torch.zeros_like(m[..., :1])], -1))
    if fault == "drop_last_key":
        s[..., -1] = -math.inf
    exact_max = s.amax(-1)
    m_first = None
    if fam.ref == "tile":
        m_ref = s[..., :fam.ref_keys].amax(-1)
        if fam.mk:
            m_ref = bf16r(m_ref)
        m_first = m_ref.clone()
        worst = f32r(exact_max - m_ref)
        for i in range(0, c.Sq, fam.wg_rows):                              # the redo decision is per workgroup
            blk = slice(i, i + fam.wg_rows)
            redo = (worst[..., blk] > REF_LIMIT).any(-1, keepdim=True)
            upd = f32r(m_ref[..., blk] + worst[..., blk])
            m_ref[..., blk] = torch.where(redo, bf16r(upd) if fam.mk else upd, m_ref[..., blk])
    else:
        m_ref = exact_max
    m_used = m_ref
    if fault == "nq2_second_block_ref":
        m_used = m_ref.clone()
        rows = torch.arange(c.Sq)
        second = (rows % 64 >= 32)
        m_used[..., second] = m_ref[..., rows[second] - 32]
    p = f32r(torch.exp2(f32r(s - m_used[..., None])))
    l_src = p
    if fam.p_norm:
        l = f32r(p.sum(-1))
        pn = rnd(f32r(p * f32r(1.0 / l)[..., None]))
        out = f32r(pn @ (rnd(v) if f32 else v))
        if c.abi == "fp8":
            out = f32r(out * FP8_SCALES[2])
    else:
        pr = rnd(p)
        if fam.l_rounded:
            l_src = pr
        if fault == "l_first_tile":
            l_src = l_src[..., :SA_BK]
        l = f32r(l_src.sum(-1))
        vv = rnd(v) if f32 else v
        if fault == "mispaired_tile":
            vv = vv.clone()
            hi = min(2 * SA_BK, Skv)
            vv[:, :, SA_BK:hi] = vv[:, :, SA_BK:hi].roll(-1, 2)
        num = f32r(pr @ vv)
        inv = torch.where(l > 0, f32r((FP8_SCALES[2] if c.abi == "fp8" else 1.0) / l), torch.zeros_like(l))     # fp8: scale_v / l in one division
        out = f32r(num * inv[..., None])
    if not f32:
        out = truncate_bf16(out) if fault == "truncated_output" else bf16r(out)
    lse = None
    if fam.lse:
        m_l = m_ref
        if fault == "lse_no_redo_shift":
            m_l = m_first
        if fault == "lse_log2":
            lse = f32r(m_l + f32r(torch.log2(l)))
        else:
            lse = f32r(f32r(m_l * np.float32(0.6931471805599453).item()) + f32r(torch.log(l)))
    return out, lse


# the case at which each stand-in is run (CPU test: it must fail the exact instrument there)
def _find(cases, **kw):
    for c in cases:
        if all(getattr(c, k) == v for k, v in kw.items()):
            return c
    raise KeyError(kw)


def fault_case(fault):
    nq2 = _find(TILED, dtype="bf16", D=40, Sq=257, Skv=257, layout="separate")
    return {
        "drop_last_key": nq2, "pad_key_counted": nq2, "mispaired_tile": nq2, "next_head_v": nq2, "truncated_output": nq2, "l_first_tile": nq2,
        "nq2_second_block_ref": nq2, "lse_log2": nq2,
        "kvdiv_ignored": _find(TILED, dtype="bf16", D=64, kvdiv=4),            # B = 8 over Bkv = 2
        "causal_off_by_one": _find(GENERIC, dtype="bf16", causal=True, keep=False, D=64),
        "keep_ignored_last": _find(GENERIC, dtype="bf16", causal=False, keep=True),
        "lse_no_redo_shift": SPIKES[0],
    }[fault]


def violations(c, instrument, out, lse):
    """Share of the output (and LSE) elements beyond the case's bound."""
    r = reference(c, instrument)
    key = "exact" if instrument == "exact" else "rounded"
    bad_o = ~((out - r["out"]).abs() <= r[key + "_out"])
    bad_l = ~((lse - r["lse"]).abs() <= r[key + "_lse"]) if lse is not None else torch.zeros(1, dtype=torch.bool)
    return float(bad_o.double().mean()), float(bad_l.double().mean())


# =====================================================================================================================================================
# the A/B switch arms (GPU: one fresh child process per setting, tests/attn_fwd_child.py)
# =====================================================================================================================================================
# (environment, cases whose launch the switch changes)
SWITCH_ARMS = [
    ({"FMC_SA_BIG80_WAVES": "8"}, BIG80 + SPIKES[4:5]),
    ({"FMC_SA_BIG80_WAVES": "5"}, BIG80 + SPIKES[4:5]),
    ({"FMC_SA_BIG80": "0"}, BIG80 + SPIKES[4:5]),
    ({"FMC_SA_SMALL": "0"}, SMALL160),
    ({"FMC_SA_PIPE": "0"}, SA40D + SPIKES[3:4]),
    ({"FMC_SA_PIPE": "4"}, SA40D + SPIKES[3:4]),
    ({"FMC_SA_VR": "0"}, [c for c in TILED + SPIKES[:1] if ",2," in c.kernel and c.kernel.endswith(",1>")]),
    ({"FMC_SA_MK": "0"}, [c for c in TILED + SPIKES[:1] if c.kernel.endswith(",1,1>")]),
    ({"FMC_SA_NQ": "1"}, [c for c in TILED + SPIKES[:1] if ",2," in c.kernel and c.kernel.endswith(",1>")]),
]


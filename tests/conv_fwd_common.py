"""Shared by tests/test_gpu_conv_forward_elementwise.py (GPU) and tests/test_conv_fwd_reference_host.py (CPU): the float64 references of every
3x3 convolution forward launch, the two input generators, the element-wise bounds and the wrong stand-ins the bounds have to catch.
profiles/conv_forward_bounds.md is the record (derivations, measured shares of the bounds).

Two instruments, every launch form gets both:

* EXACT runs.  Integer activations in [-2, 2], integer filter entries in [-2, 2] that are nonzero with probability ~ 48 / K, small integer bias /
  temb / residual / shortcut.  While `sum|terms| + |bias| + |temb| + |residual| < 256` for every output (asserted on the reference), every product
  and every partial sum in ANY order is an integer that fp32 and bf16 hold exactly: the kernel's output equals the float64 reference bit for bit,
  whatever its accumulation order, split, wave count or tile order, and a dropped, doubled or mis-addressed term changes an output by >= 1.
* ROUNDING runs.  Gaussian data as the kernels' own tests make it; `|got - ref| <= 2^-8 |ref| + 1e-5 sum|terms|` for every element
  (`assert_bf16_close`), plus -- GroupNorm + SiLU operand path only -- the operand elements whose pre-rounding value lies within the kernel's
  evaluation error of a bf16 rounding tie (`GN_DELTA`, counted from csrc/conv_halo.hip) at one bf16 ulp each.

Statistics (`gn_partials`) are compared per (image, tile, group); the tile's pixel set follows from the geometry include/fmc_hip.h documents
(`slot_map`)."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

F64 = torch.float64


# ---- the project's element-wise bounds (moved here from tests/test_gpu_kernels.py, which imports them back) ---------------------------------------
def assert_bf16_close(got, ref, mag, what="", extra=None):
    """Element-wise bound for a kernel that rounds ONCE to bf16 from an fp32 accumulator: |got - ref| <= 2^-8 |ref| + 1e-5 mag,
    `ref` the exact result on the same (rounded) inputs, `mag` the sum of |terms| behind every element (fp32 accumulation error of
    kernel and reference).  A mis-indexed tile / row / column fails this where a max-norm `rel_inf` can hide it.
    `extra` (default none): a per-element addend to the bound that the caller has derived (`conv_fwd_common.reference`: the rounding ties of the GroupNorm + SiLU operand).  Returns the largest
    err / bound."""
    got, ref, mag = got.detach().double().cpu(), ref.detach().double().cpu(), mag.detach().double().cpu()
    err = (got - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-5 * mag
    if extra is not None:
        bound = bound + extra.detach().double().cpu()
    bad = err > bound
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} / {bad.numel()} elements beyond the bf16 bound, worst "
                                 f"err {float((err - bound).max()):.3e} at {tuple(int(i) for i in (err - bound).flatten().argmax().unsqueeze(0))}")
    return float((err / bound.clamp_min(1e-300)).max())


def assert_f32_close(got, ref, mag, what=""):
    """fp32-storage (split-bf16 x3) kernels: every product carries <= ~3 * 2^-18 relative error (dropped lo*lo + the two split
    remainders), so |got - ref| <= 2e-5 * sum |terms| element by element.  Returns the largest err / bound."""
    got, ref, mag = got.detach().double().cpu(), ref.detach().double().cpu(), mag.detach().double().cpu()
    err = (got - ref).abs()
    bad = err > 2e-5 * mag
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} / {bad.numel()} elements beyond 2e-5 * |terms|, worst {float((err / mag.clamp_min(1e-30)).max()):.3e}"
    return float((err / (2e-5 * mag).clamp_min(1e-300)).max())


def rel_inf(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ---- constants counted from the source (profiles/conv_forward_bounds.md has the derivations) --------------------------------------------------------
# GroupNorm + SiLU operand, conv_halo.hip `halo_transform` / `silu_fast`: z = fma(x, a, b); t = -log2(e) * z; e = exp2(t); d = 1 + e; r = rcp(d);
# v = z * r.  Absolute error of v in units of 2^-24 |z| (half an fp32 ulp of z; |z| <= |x a| + |b|), s = sigmoid(z):
#   1.1   the fma's one rounding of z, through |silu'| <= 1.1
#   0.34  t: the product's rounding and the rounded constant (1.5 half-ulps of t) become a relative error 1.5 |z| of e, weight |v| (1 - s) = |z| s (1 - s) <= 0.224
#   0.5   v_exp_f32, 1 ulp = 2 half-ulps of e, weight |v| (1 - s) <= 0.25 |z|
#   1     the add 1 + e        2   v_rcp_f32, 1 ulp        1   the multiply z * r        (weight |v| <= |z| each)
# = 5.94, taken as 8 half-ulps: delta = 8 * 2^-24 = 2^-21.
GN_DELTA = 2.0 ** -21
GN_DELTA_AFFINE = 2.0 ** -24        # gn_act = False: the fma alone
AMBIGUOUS_CAP = 0.01                # at most 1 % of the operand elements may be ambiguous in any case
# Statistics epilogues (conv_halo.hip:493-527, conv_halo4.hip:374-407, gemm_conv.hip gn_tile_accumulate / gn_tile_finish): thread t adds the values
# of group t % GT over its rows one after the other -- 320 rows x 160 channels over 512 threads = 100 values in conv_halo_kernel and, 160 rows x 320
# channels, in the ring kernel; 50 per row block in conv_halo4_kernel -- and one thread then adds the RP = 512 / GT <= 64 partials of a group (Cout =
# 640: 20 channels per group, GT = 8).  The longest chain of dependent fp32 additions behind a partial is 100 + 64 = 164, each rounding at most 2^-24
# of the running sum of |addends| (the squares of bf16 values are exact in fp32).
STATS_CHAIN = 164
STATS_REL = STATS_CHAIN * 2.0 ** -24          # 9.8e-6

Spec = namedtuple("Spec", "kind n h w cin cout c2 ups s2 extras tdiv gn cs1 cs2")


def spec(kind, n, h, w, cin, cout, c2=0, ups=False, s2=False, extras="", tdiv=1, gn=0, cs1=0, cs2=0):
    """`h x w` is the OUTPUT size of a stride-1 launch (the source is h / 2 x w / 2 with `ups`) and the INPUT size with `s2`; `extras` names the
    epilogue addends ("b" bias, "t" temb with `n / tdiv` rows, "r" residual); gn: 0 plain, 1 GroupNorm + SiLU operand, 2 GroupNorm operand without
    the activation; cs1 / cs2: channels of the 1x1 shortcut's sources.  kind: "bf16" or "f32" (storage)."""
    assert n % tdiv == 0
    return Spec(kind, n, h, w, cin, cout, c2, ups, s2, extras, tdiv, gn, cs1, cs2)


def out_hw(s):
    return (s.h // 2, s.w // 2) if s.s2 else (s.h, s.w)


def src_hw(s):
    return (s.h // 2, s.w // 2) if s.ups else (s.h, s.w)


def reduction_length(s):
    return 9 * s.cin + s.cs1 + s.cs2


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------
def _cl(w):
    return w.contiguous(memory_format=torch.channels_last)


def gauss_inputs(s, seed):
    """Gaussian data as tests/test_gpu_conv_halo.py, test_gpu_conv_shortcut_fold.py and test_gpu_kernels.py make it, rounded to the storage type."""
    g = torch.Generator().manual_seed(seed)
    dt = torch.bfloat16 if s.kind == "bf16" else torch.float32
    hs, ws = src_hw(s)
    ho, wo = out_hw(s)
    d = {"tdiv": s.tdiv}
    d["x"] = torch.randn(s.n, hs, ws, s.cin - s.c2, generator=g).to(dt)
    d["x2"] = torch.randn(s.n, hs, ws, s.c2, generator=g).to(dt) if s.c2 else None
    d["w"] = _cl((torch.randn(s.cout, s.cin, 3, 3, generator=g) * (9 * s.cin) ** -0.5).to(dt))
    d["bias"] = torch.randn(s.cout, generator=g).to(dt) if "b" in s.extras else None
    d["temb"] = torch.randn(s.n // s.tdiv, s.cout, generator=g).to(dt) if "t" in s.extras else None
    d["res"] = torch.randn(s.n, ho, wo, s.cout, generator=g).to(dt) if "r" in s.extras else None
    d["coef"] = None
    if s.gn:                              # GroupNorm(32) coefficients of the input itself, as fmc_groupnorm_coef leaves them: (rstd gamma, beta - mean rstd gamma) in fp32
        d["x"] = (d["x"].float() * 1.7 + 0.3).to(dt)
        gamma, beta = torch.randn(s.cin, generator=g) * 0.3 + 1.0, torch.randn(s.cin, generator=g) * 0.2
        xin = d["x"].double() if d["x2"] is None else torch.cat([d["x"].double(), d["x2"].double()], -1)
        xg = xin.reshape(s.n, hs * ws, 32, s.cin // 32)
        mean, var = xg.mean((1, 3)), xg.var((1, 3), unbiased=False)
        rstd = (var + 1e-5).rsqrt()
        a = rstd.repeat_interleave(s.cin // 32, 1) * gamma.double()
        b = beta.double() - mean.repeat_interleave(s.cin // 32, 1) * a
        d["coef"] = torch.stack([a, b], -1).float().contiguous()
    if s.cs1:
        csc = s.cs1 + s.cs2
        d["xs"] = torch.randn(s.n, ho, wo, s.cs1, generator=g).to(dt)
        d["xs2"] = torch.randn(s.n, ho, wo, s.cs2, generator=g).to(dt) if s.cs2 else None
        d["wsc"] = (torch.randn(s.cout, csc, generator=g) * csc ** -0.5).to(dt)
        d["bsc"] = torch.randn(s.cout, generator=g).to(dt)
    return d


def int_inputs(s, seed, density=48.0):
    """Integer data for the exact runs: activations in [-2, 2], filter entries in [-2, 2] nonzero with probability `density / K` (the shortcut filter
    as sparse), bias / temb / residual in [-2, 2].  GroupNorm operand: per (image, channel) a scale from {0.5, 1, 2} and a shift in [-1, 1]; where the
    scale is 0.5 the activations are even, so the operand x * scale + shift is an integer of magnitude <= 5."""
    g = torch.Generator().manual_seed(seed)
    dt = torch.bfloat16 if s.kind == "bf16" else torch.float32
    hs, ws = src_hw(s)
    ho, wo = out_hw(s)
    ints = lambda *shape, lo=-2, hi=2: torch.randint(lo, hi + 1, shape, generator=g).float()
    p = min(1.0, density / reduction_length(s))

    def sparse(*shape):
        v = torch.randint(1, 3, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
        return v * (torch.rand(shape, generator=g) < p)

    d = {"tdiv": s.tdiv}
    x = ints(s.n, hs, ws, s.cin)
    d["coef"] = None
    if s.gn:
        a = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (s.n, s.cin), generator=g)]
        b = ints(s.n, s.cin, lo=-1, hi=1)
        half = (a == 0.5)[:, None, None, :]
        x = torch.where(half, 2.0 * ints(s.n, hs, ws, s.cin, lo=-1, hi=1), x)
        d["coef"] = torch.stack([a, b], -1).float().contiguous()
    d["x"] = x[..., :s.cin - s.c2].contiguous().to(dt)
    d["x2"] = x[..., s.cin - s.c2:].contiguous().to(dt) if s.c2 else None
    d["w"] = _cl(sparse(s.cout, s.cin, 3, 3).to(dt))
    d["bias"] = ints(s.cout).to(dt) if "b" in s.extras else None
    d["temb"] = ints(s.n // s.tdiv, s.cout).to(dt) if "t" in s.extras else None
    d["res"] = ints(s.n, ho, wo, s.cout).to(dt) if "r" in s.extras else None
    if s.cs1:
        d["xs"] = ints(s.n, ho, wo, s.cs1).to(dt)
        d["xs2"] = ints(s.n, ho, wo, s.cs2).to(dt) if s.cs2 else None
        d["wsc"] = sparse(s.cout, s.cs1 + s.cs2).to(dt)
        d["bsc"] = ints(s.cout).to(dt)
    return d


# ---- the float64 reference ----------------------------------------------------------------------------------------------------------------------------
def bf16_ulp(v):
    """Spacing of the bf16 values around `v` (float64 tensor; 8 significand bits)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def operand(s, d, act=None):
    """The convolution's operand `[n, hs, ws, cin]` in float64 -> (operand, ambiguous mask or None).  With `coef`: act(x * a + b) evaluated in float64 and
    rounded to bf16 ONCE; an element is ambiguous when the pre-rounding value lies within `delta (|x a| + |b|)` of a rounding tie (the kernel evaluates the
    same expression in fp32 with the hardware exp2 / rcp and may land on the other neighbour)."""
    xin = d["x"].double() if d["x2"] is None else torch.cat([d["x"].double(), d["x2"].double()], -1)
    if d["coef"] is None:
        return xin, None
    act = (s.gn == 1) if act is None else act
    a, b = d["coef"].double()[:, None, None, :, 0], d["coef"].double()[:, None, None, :, 1]
    z = xin * a + b
    v = z * torch.sigmoid(z) if act else z
    ulp = bf16_ulp(v)
    frac = v / ulp - torch.floor(v / ulp)
    dist = (frac - 0.5).abs() * ulp
    amb = dist < (GN_DELTA if act else GN_DELTA_AFFINE) * ((xin * a).abs() + b.abs())
    return v.bfloat16().double(), amb


def _resample(s, t):
    """[n, hs, ws, c] -> NCHW at the resolution the 3x3 window walks."""
    t = t.permute(0, 3, 1, 2)
    return F.interpolate(t, scale_factor=2.0, mode="nearest") if s.ups else t


def reference(s, d, act=None):
    """float64 on the operands as stored -> dict(ref, mag [n, ho, wo, cout]; extra: the ambiguity addend to the bound or None; amb_share).
    `mag` = sum|terms| including every epilogue addend."""
    op, amb = operand(s, d, act)
    w = d["w"].double()
    stride = 2 if s.s2 else 1
    ref = F.conv2d(_resample(s, op), w, None, stride, 1)
    mag = F.conv2d(_resample(s, op.abs()), w.abs(), None, stride, 1)
    extra, share = None, 0.0
    if amb is not None:
        extra = F.conv2d(_resample(s, amb.double() * bf16_ulp(op)), w.abs(), None, stride, 1).permute(0, 2, 3, 1)
        share = float(amb.double().mean())
    if d["bias"] is not None:
        ref, mag = ref + d["bias"].double()[None, :, None, None], mag + d["bias"].double().abs()[None, :, None, None]
    if d["temb"] is not None:
        t = d["temb"].double().repeat_interleave(d["tdiv"], 0)[:, :, None, None]
        ref, mag = ref + t, mag + t.abs()
    if d["res"] is not None:
        r = d["res"].double().permute(0, 3, 1, 2)
        ref, mag = ref + r, mag + r.abs()
    ref, mag = ref.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)
    if s.cs1:
        cat = d["xs"].double() if d["xs2"] is None else torch.cat([d["xs"].double(), d["xs2"].double()], -1)
        ref = ref + cat @ d["wsc"].double().t() + d["bsc"].double()
        mag = mag + cat.abs() @ d["wsc"].double().abs().t() + d["bsc"].double().abs()
    return {"ref": ref.contiguous(), "mag": mag.contiguous(), "extra": extra, "amb_share": share}


def folded_reference(s, d):
    """The folded upsample launches' reference: the filter folded in float64 (`hip_ops.upsample_fold_weights`), rounded to bf16 ONCE, four 2x2-tap phase
    convolutions of the source (`hip_ops.conv3x3_upfold_reference`) in float64; `mag` likewise on the absolute values."""
    from synfmc_amd import hip_ops as K
    assert s.ups and not s.c2 and not s.gn
    wf = K.upsample_fold_weights(d["w"].double().contiguous()).bfloat16().double()
    x = d["x"].double().permute(0, 3, 1, 2)
    b = None if d["bias"] is None else d["bias"].double()
    ref = K.conv3x3_upfold_reference(x, wf, b)
    mag = K.conv3x3_upfold_reference(x.abs(), wf.abs(), None if b is None else b.abs())
    return {"ref": ref.permute(0, 2, 3, 1).contiguous(), "mag": mag.permute(0, 2, 3, 1).contiguous(), "extra": None, "amb_share": 0.0}


@functools.lru_cache(maxsize=6)
def case(s, instrument, folded=False):
    """(inputs, reference) of a case, computed once and shared by the tests that run it: `instrument` "exact" | "rounding".  The exact runs take the
    GroupNorm operand path without the activation; their folded reference is the 9-tap one (the fold of integers is exact)."""
    seed = 1000 * s.h + 10 * s.cin + s.n + s.cs1 + (7 if s.gn else 0)
    if instrument == "exact":
        d = int_inputs(s, seed, density=32.0 if s.gn else 48.0)        # (|operand| <= 5 instead of 2: the sparser filter keeps sum|terms| < 256)
        r = reference(s, d, act=False)
        assert_exact_conditions(r, s)
    else:
        d = gauss_inputs(s, seed)
        r = folded_reference(s, d) if folded else reference(s, d)
        assert r["amb_share"] <= AMBIGUOUS_CAP, f"{r['amb_share']:.4f} of the operand elements are ambiguous (cap {AMBIGUOUS_CAP})"
    return d, r


# ---- statistics: which pixels a `gn_partials` slot sums ------------------------------------------------------------------------------------------------
def slot_map(layout, h, w):
    """-> (slot of every output pixel `[h, w]`, slots per image).  Layouts, from include/fmc_hip.h and the launch code:
    "halo": 10 x 32-pixel tiles, row-major over the image (fmc_conv3x3_halo_bf16 / _sc_bf16);
    "halo4": row blocks of 10 x 16 pixels where W % 16 == 0, else 5 x 8, row-major (fmc_conv3x3_halo4_bf16, both wave counts);
    "ring": 160 consecutive pixels of the image (fmc_conv3x3_bf16_gn);
    "halo_fold" / "halo4_fold": the SOURCE image's tiles / row blocks, four slots each: slot 4 t + 2 py + px sums the outputs (2 i + py, 2 j + px)."""
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    if layout.endswith("_fold"):
        base, per = slot_map(layout[:-5], h // 2, w // 2)
        return base[y // 2, x // 2] * 4 + (y % 2) * 2 + (x % 2), 4 * per
    if layout == "halo":
        return (y // 10) * (w // 32) + x // 32, (h + 9) // 10 * (w // 32)
    if layout == "halo4":
        tw = 16 if w % 16 == 0 else 8
        th = 10 if tw == 16 else 5
        return (y // th) * (w // tw) + x // tw, (h + th - 1) // th * (w // tw)
    assert layout == "ring" and (h * w) % 160 == 0
    return (y * w + x) // 160, h * w // 160


def tile_stats(out, layout):
    """out `[n, h, w, cout]` -> (partials `[n, slots, 32, 2]` = (sum, sum of squares) per image, slot and group of cout / 32 channels in float64,
    the same sums over the absolute values)."""
    n, h, w, cout = out.shape
    slot, per = slot_map(layout, h, w)
    o = out.double().reshape(n, h * w, 32, cout // 32)
    both = torch.stack([o.sum(-1), (o * o).sum(-1), o.abs().sum(-1)], -1)                     # [n, hw, 32, 3]
    acc = torch.zeros(n, per, 32, 3, dtype=F64).index_add_(1, slot.reshape(-1), both)
    return acc[..., :2].contiguous(), acc[..., [2, 1]].contiguous()


def assert_exact_conditions(r, s):
    """What the exact instrument needs of its inputs, asserted on the reference: sum|terms| (epilogue addends included) < 256 for every output, and every
    tile's sum of squares < 2^24 (the coarsest slots any launch uses: whole 10-row x 32-pixel tiles)."""
    assert float(r["mag"].max()) < 256.0, f"sum|terms| reaches {float(r['mag'].max())}"
    assert bool((r["ref"] == r["ref"].round()).all())
    if s.cout % 32 == 0:
        n, h, w, c = r["ref"].shape
        sq = (r["ref"] ** 2).reshape(n, h * w, 32, c // 32).sum((1, 3))
        assert float(sq.max()) < 2.0 ** 24, f"an image's sum of squares reaches {float(sq.max())}"


def check_exact(got, ref, what=""):
    """Zero tolerance: every element equal.  The message names the first differing coordinates (image, row, column, channel)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = got != ref
    if bool(bad.any()):
        idx = bad.nonzero()
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} elements differ from the exact result; first at {tuple(idx[0].tolist())} "
                             f"(got {float(got[tuple(idx[0])])}, want {float(ref[tuple(idx[0])])}), last at {tuple(idx[-1].tolist())}")


def check_stats_exact(parts, out_ref, layout, what=""):
    want, _ = tile_stats(out_ref, layout)
    assert float(want[..., 1].max()) < 2.0 ** 24
    check_exact(parts.reshape(want.shape), want, what + " gn_partials")


def check_stats_rounding(parts, got_out, layout, what=""):
    """Partials against the float64 sums of the kernel's OWN rounded output over the slot's pixels: |err| <= STATS_REL * sum|addends|.  Returns the largest
    err / bound."""
    want, mag = tile_stats(got_out, layout)
    err = (parts.detach().double().cpu().reshape(want.shape) - want).abs()
    bound = STATS_REL * mag
    bad = err > bound
    assert not bool(bad.any()), (f"{what} gn_partials: {int(bad.sum())} / {bad.numel()} entries beyond {STATS_REL:.2e} * sum|addends|, first at "
                                 f"(image, slot, group, which) {tuple(bad.nonzero()[0].tolist())}")
    return float((err / bound.clamp_min(1e-300)).max())


# ---- plain-torch emulation of the documented rounding chain (CPU) ------------------------------------------------------------------------------------------
def emulate(s, d, folded=False, act=None):
    """What the kernels document, in plain torch: the operand act(fma(x, a, b)) evaluated in fp32 and rounded to bf16 once; products of bf16 values and
    their sum in fp32; bias + temb summed in fp32, then the residual; ONE rounding to bf16.  fp32 storage: the three split-bf16 products in fp32.
    Folded launches: the filter folded in fp32 and rounded to bf16 once."""
    from synfmc_amd import hip_ops as K
    xin = d["x"].float() if d["x2"] is None else torch.cat([d["x"].float(), d["x2"].float()], -1)
    if d["coef"] is not None:
        act = (s.gn == 1) if act is None else act
        z = torch.addcmul(d["coef"][:, None, None, :, 1], xin, d["coef"][:, None, None, :, 0])
        xin = (z * torch.sigmoid(z) if act else z).bfloat16().float()
    w = d["w"].float()
    stride = 2 if s.s2 else 1
    if s.kind == "f32":
        xh, wh = xin.bfloat16().float(), w.bfloat16().float()
        xl, wl = (xin - xh).bfloat16().float(), (w - wh).bfloat16().float()
        y = sum(F.conv2d(_resample(s, a), b, None, stride, 1) for a, b in ((xh, wh), (xh, wl), (xl, wh)))
    elif folded:
        y = K.conv3x3_upfold_reference(xin.permute(0, 3, 1, 2), K.upsample_fold_weights(w.contiguous()).bfloat16().float())
    else:
        y = F.conv2d(_resample(s, xin), w, None, stride, 1)
    if s.cs1:
        cat = d["xs"].float() if d["xs2"] is None else torch.cat([d["xs"].float(), d["xs2"].float()], -1)
        y = y + (cat @ d["wsc"].float().t()).permute(0, 3, 1, 2)
    side = None
    for t in (d["bias"], d["bsc"] if s.cs1 else None):
        if t is not None:
            side = t.float()[None, :, None, None] if side is None else side + t.float()[None, :, None, None]
    if d["temb"] is not None:
        t = d["temb"].float().repeat_interleave(d["tdiv"], 0)[:, :, None, None]
        side = t if side is None else side + t
    if side is not None:
        y = y + side
    if d["res"] is not None:
        y = y + d["res"].float().permute(0, 3, 1, 2)
    y = y.permute(0, 2, 3, 1).contiguous()
    return y if s.kind == "f32" else y.bfloat16()


def emulate_stats(out, layout):
    """The statistics epilogue in plain torch: fp32 sums of the rounded outputs per slot."""
    n, h, w, cout = out.shape
    slot, per = slot_map(layout, h, w)
    o = out.float().reshape(n, h * w, 32, cout // 32)
    both = torch.stack([o.sum(-1), (o * o).sum(-1)], -1)
    return torch.zeros(n, per, 32, 2).index_add_(1, slot.reshape(-1), both)


def truncate_bf16(t):
    """fp32 -> bf16 by dropping the low 16 bits (a wrong stand-in: the kernels round to nearest even)."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


# ---- the cases both files run --------------------------------------------------------------------------------------------------------------------------------
# conv_halo_kernel, (n, H, W, Cin, Cout) with H x W the output: the shapes of tests/test_gpu_conv_halo.py plus three full row tiles, the GroupNorm
# operand across two sources, and -- new -- a tile over the last image row at a Cout that emits statistics.
HALO = [
    spec("bf16", 1, 7, 32, 64, 160),
    spec("bf16", 2, 24, 32, 192, 160, extras="btr", tdiv=2),
    spec("bf16", 3, 10, 64, 128, 320, extras="btr", tdiv=3),
    spec("bf16", 2, 20, 32, 320, 320, c2=128, extras="btr", tdiv=2),
    spec("bf16", 2, 20, 64, 128, 160, ups=True, extras="btr", tdiv=2),
    spec("bf16", 2, 30, 32, 64, 160, extras="b"),
    spec("bf16", 2, 10, 32, 640, 640, c2=320, gn=1),
    spec("bf16", 2, 20, 32, 320, 320, gn=1),
    spec("bf16", 2, 20, 32, 128, 320, gn=2),
    spec("bf16", 2, 24, 32, 64, 320, extras="btr", tdiv=1),
    spec("bf16", 3, 13, 64, 128, 320, c2=64, gn=1, extras="t", tdiv=3),
]
# shortcut mode: (n, H, W, Cin, Cout, Cs1, Cs2)
HALO_SC = [
    spec("bf16", 1, 10, 32, 64, 160, extras="b", cs1=64),
    spec("bf16", 2, 13, 64, 128, 320, extras="b", cs1=64, cs2=128),
    spec("bf16", 1, 20, 32, 320, 320, extras="b", cs1=640, cs2=320),
    spec("bf16", 2, 24, 32, 64, 320, extras="b", cs1=64, cs2=128),
]
# conv_halo4_kernel: the ten cases of tests/test_gpu_conv_halo.py, and -- new -- four at Cout = 320, the smallest Cout whose statistics the kernel emits
HALO4 = [
    spec("bf16", 4, 10, 16, 64, 80),
    spec("bf16", 5, 10, 16, 192, 160, extras="btr"),
    spec("bf16", 6, 10, 16, 256, 160, c2=128, extras="btr", tdiv=2),
    spec("bf16", 4, 10, 16, 128, 80, ups=True, extras="btr", tdiv=2),
    spec("bf16", 16, 5, 8, 128, 160, extras="btr", tdiv=2),
    spec("bf16", 11, 5, 8, 64, 80),
    spec("bf16", 3, 16, 16, 64, 80, extras="btr"),
    spec("bf16", 2, 20, 32, 128, 160, extras="btr", tdiv=2),
    spec("bf16", 2, 32, 48, 64, 80, extras="btr", tdiv=2),
    spec("bf16", 3, 16, 24, 128, 160, c2=64, extras="btr"),
    spec("bf16", 5, 10, 16, 64, 320, extras="b"),
    spec("bf16", 3, 16, 16, 64, 320, extras="btr", tdiv=3),
    spec("bf16", 11, 5, 8, 64, 320),
    spec("bf16", 3, 16, 24, 64, 320, extras="r"),
]
# folded upsample launches: EDGE_SHAPES of tests/test_conv_upsample_fold.py as (n, source H, source W, Cin, Cout, arm), and -- new -- Cout = 320 on the
# halo4 arms (statistics)
FOLD = [
    (3, 13, 32, 128, 160, "halo"), (2, 7, 64, 64, 320, "halo"), (3, 10, 16, 128, 160, "halo4"), (2, 13, 32, 64, 80, "halo4"), (11, 5, 8, 64, 80, "halo4"),
    (3, 7, 24, 128, 160, "halo4"), (2, 10, 32, 128, 160, "halo4w"),
    (3, 13, 16, 64, 320, "halo4"), (3, 7, 24, 64, 320, "halo4"), (2, 13, 32, 64, 320, "halo4w"),
]


def fold_spec(n, hs, ws, cin, cout, with_bias):
    return spec("bf16", n, 2 * hs, 2 * ws, cin, cout, ups=True, extras="b" if with_bias else "")


# the ring kernel fmc_conv3x3_bf16: the five epilogues of test_conv_epilogue_variants_plain_grid (ragged Cout and pixel count), stride 2, upsample, split-K
RING_EPILOGUE = [spec("bf16", 6, 13, 11, 128, 136, extras=e, tdiv=t) for e, t in (("b", 1), ("t", 1), ("t", 3), ("r", 1), ("btr", 1))]
RING_EPILOGUE_TILES = [0, 1, 3, 5, 7, 11]
RING_STRIDE2 = spec("bf16", 3, 20, 28, 128, 320, s2=True, extras="b")
RING_STRIDE2_TILES = [0, 2, 5, 11]
RING_UPSAMPLE = spec("bf16", 3, 20, 28, 128, 320, ups=True, extras="b")
RING_UPSAMPLE_TILES = [0, 1, 3, 11, 128 + 2]
RING_SPLIT = spec("bf16", 2, 5, 8, 256, 136, extras="tr")
RING_SPLIT_TILES, RING_SPLITS = [1, 2, 9], [2, 4, 8]
RING_GN = spec("bf16", 2, 20, 16, 64, 320, extras="btr", tdiv=2)          # H W % 160 == 0, Cout % 320 == 0; two statistics tiles per image
F32 = [spec("f32", 2, 18, 14, 128, 136), spec("f32", 2, 18, 14, 128, 136, extras="btr", tdiv=2), spec("f32", 2, 18, 14, 128, 136, ups=True),
       spec("f32", 2, 18, 14, 128, 136, s2=True)]
F32_TILES = [0, 1, 3, 5, 11, 13, 2 + 16]


def all_cases():
    """(spec, folded) of every GPU case, for the CPU tests that run the emulation and the input conditions at every GPU shape."""
    out = [(s, False) for s in HALO + HALO_SC + HALO4 + RING_EPILOGUE + [RING_STRIDE2, RING_UPSAMPLE, RING_SPLIT, RING_GN] + F32]
    seen = set()
    for n, hs, ws, cin, cout, _ in FOLD:
        for wb in (False, True):
            s = fold_spec(n, hs, ws, cin, cout, wb)
            if s not in seen:
                seen.add(s)
                out.append((s, True))
    return out

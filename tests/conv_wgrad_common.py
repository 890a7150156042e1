"""Shared pieces of the tests of the direct 3x3 weight gradient, `fmc_conv3x3_wgrad_bf16` (csrc/conv_wgrad.hip).  Pure torch: imports no GPU code.

    dW[co][ky][kx][ci] = alpha * sum over (n, yo, xo) of dY[n, yo, xo, co] * X[n, s yo + ky - 1, s xo + kx - 1, ci]   (+ dW)

* `reference`: a float64 loop over the nine taps that also returns `sum |terms|` per element (the scale of both error bounds);
* `plan`: the launcher's split plan restated (tiles, slabs, splits, slabs per split, longest fp32 addition chain);
* `emulate`: the kernel's order of accumulation in plain torch -- per split, per wave, per MFMA step of 16 pixels, the waves in order,
  the splits in order, then alpha / accumulate / layout -- with one `defect` switch per wrong stand-in;
* `CASES`: the shapes of tests/test_gpu_conv_wgrad.py with the placement each one claims, asserted from `plan` on the CPU;
* the two instruments, `check_integer` (bit equality with float64) and `check_gaussian` (1e-5 * sum |terms|).
"""
import torch

BT, BN, BK = 128, 64, 64                 # pixels per staged slab, output channels / input channels per workgroup (wgrad_common.h)
MIN_SLABS, TARGET = 4, 1024              # a split reduces at least 4 slabs; workgroups a problem is split towards
FP32_BOUND = 1e-5                        # the project's fp32 bound: |error| <= 1e-5 * sum |terms|
CHAIN_LIMIT = int(FP32_BOUND / 2.0 ** -24)      # 167: sequential fp32 additions of half an ulp each that the bound pays for

OIHW, OHWI = 0, 1                        # FMC_DW_OIHW / FMC_DW_OHWI


def out_size(h, stride):
    return (h - 1) // stride + 1


# ---- float64 reference ------------------------------------------------------------------------------------------------------------
def reference(x, dy, stride):
    """x `[n, H, W, Cin]`, dy `[n, Ho, Wo, Cout]` -> (dW, sum |terms|), float64 `[Cout, Cin, 3, 3]` each."""
    n, H, W, cin = x.shape
    _, ho, wo, cout = dy.shape
    assert (ho, wo) == (out_size(H, stride), out_size(W, stride))
    xp = torch.zeros(n, H + 2, W + 2, cin, dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = x.double()
    d = dy.double().reshape(-1, cout)
    dw = torch.zeros(cout, cin, 3, 3, dtype=torch.float64)
    mag = torch.zeros_like(dw)
    for ky in range(3):
        for kx in range(3):
            src = xp[:, ky: ky + stride * (ho - 1) + 1: stride, kx: kx + stride * (wo - 1) + 1: stride].reshape(-1, cin)
            dw[:, :, ky, kx] = d.t() @ src
            mag[:, :, ky, kx] = d.abs().t() @ src.abs()
    return dw, mag


def finish(dw, mag, alpha, old):
    """(alpha dW (+ old), its sum |terms|): what the launch leaves in `dw`."""
    if old is None:
        return alpha * dw, abs(alpha) * mag
    return alpha * dw + old.double(), abs(alpha) * mag + old.double().abs()


# ---- the split plan, restated -----------------------------------------------------------------------------------------------------
def plan(n, H, W, cin, cout, stride):
    P = n * out_size(H, stride) * out_size(W, stride)
    tiles_co, tiles_ci = -(-cout // BN), -(-cin // BK)
    wgs = tiles_co * tiles_ci * 9                     # one workgroup per (tap, 64 ci, 64 co) and split
    slabs = -(-P // BT)
    s = max(1, min((TARGET + wgs // 2) // wgs, slabs // MIN_SLABS))      # towards TARGET workgroups, to the nearest multiple
    chunk = -(-slabs // s)
    splits = -(-slabs // chunk)
    # a wave runs 2 MFMA steps per slab into one accumulator; then 3 cross-wave additions, then splits - 1 in the combine
    chain = 2 * chunk + 3 + (splits - 1)
    return dict(P=P, tiles_co=tiles_co, tiles_ci=tiles_ci, slabs=slabs, splits=splits, chunk_slabs=chunk, chain=chain,
                ws_floats=splits * cout * 9 * cin if splits > 1 else 0)


# ---- the kernel's accumulation order, and its wrong stand-ins ---------------------------------------------------------------------------
DEFECTS = ("swap_ky_kx", "wrap_columns", "previous_image", "stride2_offset", "drop_last_slab", "split_twice", "alpha_on_old", "layout_confused")


def gather(x, stride, ky, kx, defect=None):
    """B of one tap: `[P, Cin]` float64, row (n, yo, xo) = X[n, s yo + ky - 1, s xo + kx - 1] or zero outside the image."""
    n, H, W, cin = x.shape
    ho, wo = out_size(H, stride), out_size(W, stride)
    if defect == "swap_ky_kx":
        ky, kx = kx, ky
    img, yo, xo = torch.meshgrid(torch.arange(n), torch.arange(ho), torch.arange(wo), indexing="ij")
    off = stride if defect == "stride2_offset" else 1            # (the pad scaled by the stride: right at stride 1 only)
    yi, xi = stride * yo + ky - off, stride * xo + kx - off
    ok_y, ok_x = (yi >= 0) & (yi < H), (xi >= 0) & (xi < W)
    if defect == "wrap_columns":                                 # no column test: the flat address lands in the neighbouring row
        ok_x = torch.ones_like(ok_x)
    if defect == "previous_image":                               # no row test: the flat address lands in the neighbouring image
        ok_y = torch.ones_like(ok_y)
    flat = (img * H + yi) * W + xi
    ok = ok_y & ok_x & (flat >= 0) & (flat < n * H * W)
    rows = x.double().reshape(-1, cin)[flat.clamp(0, n * H * W - 1).reshape(-1)]
    return rows * ok.reshape(-1, 1)


def emulate(x, dy, stride, alpha=1.0, old=None, layout=OIHW, defect=None):
    """The launch in plain torch, fp32 where the kernel is fp32.  Returns the flat fp32 buffer the kernel leaves (`9 Cin Cout` words in
    `layout` order).  One MFMA step = the 16 pixel products of an element summed exactly (float64) and added to the fp32 accumulator."""
    n, H, W, cin = x.shape
    cout = dy.shape[-1]
    pl = plan(n, H, W, cin, cout, stride)
    P = pl["P"]
    a = dy.double().reshape(P, cout)
    n_pix = (P // BT) * BT if defect == "drop_last_slab" else P
    parts = []
    for split in range(pl["splits"]):
        m0 = split * pl["chunk_slabs"] * BT
        m1 = min(m0 + pl["chunk_slabs"] * BT, n_pix)
        part = torch.zeros(cout, 9, cin, dtype=torch.float32)
        for tap in range(9):
            b = gather(x, stride, tap // 3, tap % 3, defect)
            waves = torch.zeros(4, cout, cin, dtype=torch.float32)
            for slab in range(m0, m1, BT):
                for wave in range(4):
                    for ks in range(2):
                        lo = slab + 32 * wave + 16 * ks
                        hi = min(lo + 16, m1)
                        if lo < hi:
                            waves[wave] += (a[lo:hi].t() @ b[lo:hi]).float()
            part[:, tap] = ((waves[0] + waves[1]) + waves[2]) + waves[3]
        parts.append(part)
    total = parts[0].clone()
    for part in parts[1:]:
        total += part
    if defect == "split_twice" and len(parts) > 1:
        total += parts[-1]
    order = 1 - layout if defect == "layout_confused" else layout
    res = (total if order == OHWI else total.permute(0, 2, 1)).reshape(-1).double()          # total is [Cout][9][Cin]; OIHW is [Cout][Cin][9]
    if old is None:
        out = alpha * res
    elif defect == "alpha_on_old":
        out = alpha * (res + old.reshape(-1).double())
    else:
        out = alpha * res + old.reshape(-1).double()                 # (one rounding: the kernel's fma)
    return out.float()


def to_oihw(flat, cout, cin, layout):
    """The flat buffer of a launch as logical `[Cout, Cin, 3, 3]`."""
    if layout == OIHW:
        return flat.reshape(cout, cin, 3, 3)
    return flat.reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)


# ---- the two instruments ------------------------------------------------------------------------------------------------------------
class Rejected(AssertionError):
    pass


def check_integer(got, ref, mag, what=""):
    """Integer operands with sum |terms| < 2^24: every partial sum is an integer below 2^24, exact in fp32 in any order."""
    assert float(mag.max()) < 2 ** 24, f"{what}: the integer case is not exact in fp32 (sum |terms| up to {float(mag.max()):.0f})"
    if not torch.equal(got.double(), ref):
        bad = got.double() != ref
        raise Rejected(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from float64, the largest by "
                       f"{float((got.double() - ref).abs().max()):.3e}")


def check_gaussian(got, ref, mag, what=""):
    excess = (got.double() - ref).abs() - FP32_BOUND * mag
    share = float(((got.double() - ref).abs() / (FP32_BOUND * mag).clamp_min(1e-300)).max())
    if not bool(torch.isfinite(got).all()) or float(excess.max()) > 0:
        raise Rejected(f"{what}: {int((excess > 0).sum())} of {excess.numel()} elements beyond 1e-5 * sum |terms| (worst: {share:.3g} of the bound)")
    return share


def operands(case, kind, seed=0):
    """(x, dy, old) of a case, bf16 / bf16 / fp32-or-None.  `kind`: "integer" (values in -3 .. 3) or "gaussian"."""
    n, H, W, cin, cout, stride = case["shape"]
    ho, wo = out_size(H, stride), out_size(W, stride)
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + cin)
    if kind == "integer":
        x = torch.randint(-3, 4, (n, H, W, cin), generator=g).to(torch.bfloat16)
        dy = torch.randint(-3, 4, (n, ho, wo, cout), generator=g).to(torch.bfloat16)
        old = torch.randint(-40, 41, (cout * 9 * cin,), generator=g).float()              # (alpha = 3 / 8 or -2: every value is an integer / 8, exact)
    else:
        x = torch.randn(n, H, W, cin, generator=g).to(torch.bfloat16)
        dy = torch.randn(n, ho, wo, cout, generator=g).to(torch.bfloat16)
        old = torch.randn(cout * 9 * cin, generator=g) * 5.0
    return x, dy, (old if case["accumulate"] else None)


def expected(case, x, dy, old):
    """(reference, sum |terms|) of what the launch leaves, logical `[Cout, Cin, 3, 3]` float64."""
    n, H, W, cin, cout, stride = case["shape"]
    dw, mag = reference(x, dy, stride)
    return finish(dw, mag, case["alpha"], None if old is None else to_oihw(old, cout, cin, case["layout"]))


# ---- the cases: (n, H, W, Cin, Cout, stride) and the placement each claims ------------------------------------------------------------------
def _case(name, shape, claim, alpha=1.0, accumulate=False, layout=OIHW):
    return dict(name=name, shape=shape, claim=claim, alpha=alpha, accumulate=accumulate, layout=layout)


CASES = [
    _case("one_pixel", (1, 1, 1, 16, 16, 1), dict(P=1, slabs=1, splits=1)),                            # only the centre tap is non-zero
    _case("slab_spans_rows", (1, 3, 5, 64, 128, 1), dict(P=15, slabs=1, splits=1, tiles_co=2)),
    _case("slab_spans_images", (3, 9, 13, 64, 128, 1), dict(P=351, slabs=3, splits=1), layout=OHWI),    # image 1 starts at pixel 117, inside slab 0
    _case("tile_tails", (1, 5, 6, 80, 48, 1), dict(P=30, tiles_ci=2, tiles_co=1, splits=1)),            # 80 = 64 + 16, 48 < 64
    _case("tile_tails_acc", (1, 5, 6, 80, 48, 1), dict(P=30, tiles_ci=2, splits=1), alpha=0.375, accumulate=True, layout=OHWI),
    _case("two_splits", (2, 24, 24, 16, 16, 1), dict(P=1152, slabs=9, splits=2, chunk_slabs=5)),        # split 1 starts at pixel 640: image 1, row 2, column 16
    _case("two_splits_acc", (2, 24, 24, 16, 16, 1), dict(P=1152, splits=2), alpha=0.375, accumulate=True),
    _case("two_splits_ohwi", (2, 24, 24, 32, 16, 1), dict(P=1152, splits=2), alpha=-2.0, layout=OHWI),
    _case("one_slab_exactly", (2, 8, 8, 16, 32, 1), dict(P=128, slabs=1, splits=1)),
    _case("one_slab_plus_one", (1, 3, 43, 16, 16, 1), dict(P=129, slabs=2, splits=1), alpha=0.375, accumulate=True),
    _case("stride2_4x6", (1, 4, 6, 64, 64, 2), dict(P=6, splits=1)),
    _case("stride2_8x12", (2, 8, 12, 64, 64, 2), dict(P=48, splits=1), layout=OHWI),
    _case("stride2_odd_5x7", (1, 5, 7, 32, 16, 2), dict(P=12, splits=1), alpha=0.375, accumulate=True),  # Ho x Wo = 3 x 4: the last tap row / column is outside
    _case("stride2_two_splits", (4, 31, 32, 16, 16, 2), dict(P=1024, slabs=8, splits=2, chunk_slabs=4)),
]


# ---- marked modules for the tests through autograd (GPU; the package is imported when they are called) -----------------------------------
def as_masters(module):
    """cuda, bf16 storage -> fp32 masters that require grad, marked (what `camera_trainable_parameters` does to its modules)."""
    from synfmc_amd.training import _masters, mark_trainable_own
    module = module.to("cuda", torch.bfloat16).eval().requires_grad_(False)
    _masters(list(module.parameters()))
    mark_trainable_own(module)
    return module


def seed_params(module, seed):
    """Fan-in scaled, bf16-representable parameters (the shadows then hold the masters' values)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            fan = p[0].numel() if p.ndim > 1 else 1
            p.copy_((torch.randn(p.shape, generator=g) * (0.7 / fan ** 0.5 if p.ndim > 1 else 0.1)).to(torch.bfloat16).float())
    return module


def marked_conv(cin, cout, stride, nhw, seed=5):
    """(marked `layers.Conv2d` with fp32 masters on the GPU, x `[n, cin, H, W]`, dy) -- x and dy bf16 on the CPU."""
    from synfmc_amd.models.layers import Conv2d
    conv = as_masters(seed_params(Conv2d(cin, cout, 3, stride, 1), seed))
    n, H, W = nhw
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(n, cin, H, W, generator=g).to(torch.bfloat16)
    dy = torch.randn(n, cout, out_size(H, stride), out_size(W, stride), generator=g).to(torch.bfloat16)
    return conv, x, dy

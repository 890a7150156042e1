"""The nearest-2x upsample convolutions in phase mode (`Upsample2D.conv`, up_blocks.0/1/2.upsamplers.0.conv): a 3x3 convolution of a
nearest-2x-upsampled image is four 2x2-tap convolutions of the source image, one per output parity, on a filter folded once per weight version
(`hip_ops.upsample_fold_weights` / `fmc_conv3x3_upfold_pack_weight`; kernels: the PH instantiations of csrc/conv_halo.hip and csrc/conv_halo4.hip).

* CPU: the fold is exact -- fp64, unrounded folded weights, against `conv2d(interpolate(x, 2, "nearest"), w, padding=1)`: rel-inf < 1e-8.
* GPU: the folded launches against the fp32 convolution of the same bf16 operands with the RAW filter (the reference of tests/test_gpu_conv_halo.py,
  restated here), rel-inf < 6e-3 -- that file's bound for this kernel family.  The one re-rounding of the folded filter to bf16 costs 1.2 - 1.4e-3 of
  it, the bf16 rounding of the output up to 2.8e-3 (both measured on the CPU in fp64 at 640 / 1280 channels)."""
import pytest
import torch
import torch.nn.functional as F


def rel_inf(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hs,ws,cin,cout", [
    (2, 1, 5, 64, 64),         # a 1-pixel-high source: both output rows of every pixel touch the top AND the bottom padding
    (1, 3, 1, 8, 16),          # ... and a 1-pixel-wide one
    (2, 5, 7, 64, 96),         # odd sizes
    (1, 10, 16, 640, 64),      # the step's channel counts on the reduction side
    (1, 4, 6, 1280, 32),
    (1, 1, 1, 16, 8),          # a single pixel: all four paddings at once
])
def test_fold_is_exact_in_fp64(n, hs, ws, cin, cout):
    from synfmc_amd import hip_ops as K
    g = torch.Generator().manual_seed(hs * 100 + ws + cin)
    x = torch.randn(n, cin, hs, ws, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * (9 * cin) ** -0.5
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    want = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    wf = K.upsample_fold_weights(w)
    assert wf.shape == (2, 2, 2, 2, cout, cin) and wf.dtype == torch.float64
    got = K.conv3x3_upfold_reference(x, wf, b)
    assert got.shape == want.shape == (n, cout, 2 * hs, 2 * ws)
    err = rel_inf(got, want)
    print(f"fold fp64 n={n} {hs}x{ws} {cin}->{cout}: rel-inf {err:.2e}")
    assert err < 1e-8


def test_fold_sums_the_rows_and_columns_that_share_a_source_pixel():
    from synfmc_amd import hip_ops as K
    w = torch.arange(9, dtype=torch.float64).reshape(1, 1, 3, 3) + 1.0       # w[ky][kx] = 3 ky + kx + 1
    wf = K.upsample_fold_weights(w)[..., 0, 0]
    assert wf[0, 0].tolist() == [[1.0, 2.0 + 3.0], [4.0 + 7.0, 5.0 + 6.0 + 8.0 + 9.0]]
    assert wf[1, 1].tolist() == [[1.0 + 2.0 + 4.0 + 5.0, 3.0 + 6.0], [7.0 + 8.0, 9.0]]
    assert wf[0, 1].tolist() == [[1.0 + 2.0, 3.0], [4.0 + 5.0 + 7.0 + 8.0, 6.0 + 9.0]]
    assert float(wf.sum()) == 4 * 45.0                                         # every phase sees the whole filter once


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def _mk(n, hs, ws, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, hs, ws, cin, generator=g).bfloat16()
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).bfloat16().contiguous(memory_format=torch.channels_last)
    return x, w, g


def _ref(x, w, bias=None):
    """tests/test_gpu_conv_halo.py `_ref(..., upsample=True)`: fp32 convolution of the upsampled bf16 input with the raw bf16 filter."""
    xin = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    return F.conv2d(xin, w.float(), None if bias is None else bias.float(), padding=1).permute(0, 2, 3, 1)


STEP_SHAPES = [                    # (images, source H, source W, Cin, Cout, arm): the three sites of the step, image count reduced
    (4, 20, 32, 640, 640, "halo"),            # up_blocks.2: 20x32 -> 40x64, conv_halo_kernel<0, PH>, 10 x 32 source tiles
    (4, 10, 16, 1280, 1280, "halo4"),         # up_blocks.1: 10x16 -> 20x32, conv_halo4_kernel<16, 4, PH>, two source images per tile
    (4, 10, 16, 1280, 1280, "halo4w"),        # ... and its 8-wave form
    (4, 5, 8, 1280, 1280, "halo4"),           # up_blocks.0: 5x8 -> 10x16, conv_halo4_kernel<8, 4, PH>, (up to) eight source images per tile
]
EDGE_SHAPES = [
    (3, 13, 32, 128, 160, "halo"),            # a source tile hanging over the last image row, an odd image count
    (2, 7, 64, 64, 320, "halo"),              # an image lower than one tile, two tiles side by side, one chunk
    (3, 10, 16, 128, 160, "halo4"),           # an odd image count: the last tile holds one image
    (2, 13, 32, 64, 80, "halo4"),             # row blocks of 10 + 3 rows, two side by side
    (11, 5, 8, 64, 80, "halo4"),              # 5 x 8 sources with a last tile of three images
    (3, 7, 24, 128, 160, "halo4"),            # 5 x 8 row blocks (2 x 3 per image, the lower ones two rows high)
    (2, 10, 32, 128, 160, "halo4w"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("n,hs,ws,cin,cout,arm", STEP_SHAPES + EDGE_SHAPES)
def test_folded_launch_matches_fp32_conv_of_the_upsampled_image(n, hs, ws, cin, cout, arm, with_bias):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops as K
    x, wt, g = _mk(n, hs, ws, cin, cout, seed=hs + cin + n)
    bias = torch.randn(cout, generator=g).bfloat16() if with_bias else None
    want = _ref(x, wt, bias)
    cu = lambda t: None if t is None else t.cuda()
    bn = 80 if arm == "halo4" else 160
    emit = cout % 64 == 0 and bn % (cout // 32) == 0
    xd, wd = x.cuda(), wt.cuda()
    got = K.conv3x3_upfold(xd, wd, cu(bias), emit_gn=emit, arm=arm)
    torch.cuda.synchronize()
    if emit:
        got, parts = got
    assert got.shape == want.shape == (n, 2 * hs, 2 * ws, cout)
    err = rel_inf(got, want)
    print(f"upfold {arm} n={n} {hs}x{ws} {cin}->{cout} bias={with_bias}: rel-inf {err:.3e}")
    assert err < 6e-3
    if emit:
        # statistics epilogue: sums of the ROUNDED outputs per (image, group), summed over (source tile / row block, phase)
        o = got.float().cpu().reshape(n, 4 * hs * ws, 32, cout // 32)
        s_ref = torch.stack([o.sum((1, 3)), (o * o).sum((1, 3))], -1)
        assert parts.shape[0] == n and parts.shape[1] % 4 == 0 and parts.shape[2:] == (32, 2)
        perr = rel_inf(parts.sum(1), s_ref)
        print(f"   partials rel-inf {perr:.3e}")
        assert perr < 1e-4
        # ... in the layout fmc_groupnorm_coef consumes: the mean of the next GroupNorm comes out of them
        gamma, beta = torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")
        _, stats = K.groupnorm_coef(parts, gamma, beta, 4 * hs * ws, cout, 32, 1e-5, want_stats=True)
        assert rel_inf(stats[..., 0], o.mean((1, 3))) < 1e-4
    again = K.conv3x3_upfold(xd, wd, cu(bias), arm=arm)
    assert torch.equal(again, got)                                            # two launches on the same data: bit-equal
    # a second launch on fresh data of the same shape: nothing stale in the halo buffers / the W ring / the cached pack of ANOTHER weight
    x2, wt2, _ = _mk(n, hs, ws, cin, cout, seed=1000 + hs + cin + n)
    got2 = K.conv3x3_upfold(x2.cuda(), wt2.cuda(), cu(bias), arm=arm)
    err2 = rel_inf(got2, _ref(x2, wt2, bias))
    print(f"   fresh data rel-inf {err2:.3e}")
    assert err2 < 6e-3


@pytest.mark.gpu
def test_device_fold_equals_the_reference_fold_rounded_once():
    """`fmc_conv3x3_upfold_pack_weight` against `upsample_fold_weights` in fp32 rounded to bf16 once: the packed buffer, un-permuted, bit for bit."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops as K
    cout, cin = 320, 128
    _, wt, _ = _mk(1, 1, 8, cin, cout, seed=5)
    wf = K.upsample_fold_weights(wt.float().contiguous()).bfloat16()            # [py, px, a, b, Cout, Cin]
    for bn in (80, 160):
        packed = K._w_upfold_packed(wt.cuda(), bn).cpu()
        # [phase][Cout / bn][Cin / 64][tap][half][bn rows][4 chunks of 8], physical chunk p of row r = logical chunk p ^ (3 * ((r >> 3) & 1))
        p = packed.view(4, cout // bn, cin // 64, 4, 2, bn, 4, 8)
        rows = torch.arange(bn)
        logical = torch.empty_like(p)
        for c in range(4):
            phys = c ^ (3 * ((rows >> 3) & 1))
            logical[..., rows, c, :] = p[..., rows, phys, :]
        got = logical.permute(0, 3, 1, 5, 2, 4, 6, 7).reshape(2, 2, 2, 2, cout, cin)      # [phase][tap][Cout][Cin]
        assert torch.equal(got, wf)


def _upsampler(cin, dtype, requires_grad=False):
    from synfmc_amd.models import layers as L
    torch.manual_seed(3)
    conv = L.Conv2d(cin, cin, 3, padding=1)
    with torch.no_grad():
        conv.weight.mul_(0.5)
    return conv.to("cuda", dtype).requires_grad_(requires_grad)


@pytest.mark.gpu
def test_conv2d_front_end_takes_the_folded_path_only_at_inference_in_bf16():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops as K
    n, hs, ws, c = 4, 20, 32, 640
    min_tiles, K.CONV_HALO_MIN_TILES = K.CONV_HALO_MIN_TILES, 1
    log0 = K.call_log
    try:
        conv = _upsampler(c, torch.bfloat16)
        x = torch.randn(n, c, hs, ws, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
        want = _ref(x.permute(0, 2, 3, 1).cpu(), conv.weight.detach().cpu(), conv.bias.detach().cpu()).permute(0, 3, 1, 2)
        shape = (n, 2 * hs, 2 * ws, c, c, True)
        flops9 = 2.0 * n * 4 * hs * ws * c * 9 * c
        # inference, bf16 storage: folded, logged with the 9-tap (algorithmic) flops
        K.call_log = []
        before = K.conv_halo_calls.get("upfold", 0)
        with torch.no_grad():
            y = conv(x, upsample=True)
        assert K.conv_halo_calls.get("upfold", 0) == before + 1
        assert K.call_log == [("conv_halo", shape, flops9)]
        assert rel_inf(y, want) < 6e-3
        # the switch: FMC_UPS_FOLD=0 is the old launch
        K.call_log = []
        fold, K.UPS_FOLD = K.UPS_FOLD, False
        try:
            with torch.no_grad():
                y_old = conv(x, upsample=True)
        finally:
            K.UPS_FOLD = fold
        assert K.conv_halo_calls.get("upfold", 0) == before + 1 and K.call_log == [("conv_halo", shape, flops9)]
        assert rel_inf(y_old, want) < 6e-3
        print(f"front-end: folded {rel_inf(y, want):.3e}  9-tap {rel_inf(y_old, want):.3e}  folded vs 9-tap {rel_inf(y, y_old):.3e}")
        # grad mode on (frozen filter, input without a gradient): the old launch
        K.call_log = []
        with torch.enable_grad():
            y_g = conv(x, upsample=True)
        assert K.conv_halo_calls.get("upfold", 0) == before + 1 and K.call_log == [("conv_halo", shape, flops9)]
        assert torch.equal(y_g, y_old)
        # a trainable filter / an input that needs its gradient: never the fold (autograd's own convolution)
        K.call_log = []
        conv_t = _upsampler(c, torch.bfloat16, requires_grad=True)
        with torch.enable_grad():
            y_t = conv_t(x.clone().requires_grad_(True), upsample=True)
        assert K.conv_halo_calls.get("upfold", 0) == before + 1 and y_t.requires_grad
        assert not any(fe in ("conv_halo", "conv_halo4") for fe, _, _ in K.call_log)
        # fp32 (parity) storage: the split-bf16 x3 convolution, not the fold
        K.call_log = []
        conv32 = _upsampler(c, torch.float32)
        with torch.no_grad():
            y32 = conv32(x.float(), upsample=True)
        assert K.conv_halo_calls.get("upfold", 0) == before + 1 and y32.dtype == torch.float32
        assert not any(fe in ("conv_halo", "conv_halo4") for fe, _, _ in K.call_log)
    finally:
        K.CONV_HALO_MIN_TILES = min_tiles
        K.call_log = log0

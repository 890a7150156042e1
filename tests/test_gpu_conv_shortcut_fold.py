"""`fmc_conv3x3_halo_sc_bf16` (csrc/conv_halo.hip, shortcut mode): conv2 of diffusers' ResnetBlock2D with the block's 1x1 `conv_shortcut` as a
centre-tap segment of the same reduction -- `conv3x3(x) + w_sc . [xs | xs2] + bias + b_sc`.

Reference: the fp32 `F.conv2d` of the bf16-rounded operands plus the fp32 1x1 convolution of `cat(xs, xs2)` plus both biases.  Products are exact
in fp32, so what is left is the bf16 rounding of the output, 2^-8 of the largest one: 6e-3 asserted, the bound of tests/test_gpu_conv_halo.py for
this kernel.  Every operand and every output sits in an arena of tests/edge_guard_common.py (zeros, NaN and +Inf around the inputs, a sentinel
around the outputs)."""
import pytest
import torch
import torch.nn.functional as F

from tests import edge_guard_common as EG

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
BAND = 448              # pixels around the images (more than one 10 x 32 tile)
E_SHAPE, E_ALIGN = -1, -3


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def rel_inf(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _p(t):
    return None if t is None else t.data_ptr()


def _data(n, h, w, cin, cout, cs1, cs2, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, cin, generator=g).bfloat16()
    xs = torch.randn(n, h, w, cs1, generator=g).bfloat16()
    xs2 = torch.randn(n, h, w, cs2, generator=g).bfloat16() if cs2 else None
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).bfloat16().contiguous(memory_format=torch.channels_last)
    wsc = (torch.randn(cout, cs1 + cs2, generator=g) * (cs1 + cs2) ** -0.5).bfloat16()
    bias, bsc = torch.randn(cout, generator=g).bfloat16(), torch.randn(cout, generator=g).bfloat16()
    return x, xs, xs2, wt, wsc, bias, bsc


def _ref(x, xs, xs2, wt, wsc, bias, bsc):
    """fp32: conv3x3 + 1x1 of the concatenated shortcut input + both biases -> (sum, shortcut alone) as [n, h, w, cout]."""
    cat = xs.float() if xs2 is None else torch.cat([xs.float(), xs2.float()], -1)
    sc = cat @ wsc.float().t() + bsc.float()
    y = F.conv2d(x.float().permute(0, 3, 1, 2), wt.float(), bias.float(), padding=1).permute(0, 2, 3, 1)
    return y + sc, sc


def _run_case(K, n, h, w, cin, cout, cs1, cs2, emit, seed):
    L = K._lib.load()
    cin_sc = cs1 + cs2
    assert L.fmc_conv3x3_halo_sc_supported(n, h, w, cin, cout, cin_sc, cs1)
    x, xs, xs2, wt, wsc, bias, bsc = _data(n, h, w, cin, cout, cs1, cs2, seed)
    want, sc = _ref(x, xs, xs2, wt, wsc, bias, bsc)
    tiles = L.fmc_conv3x3_halo_tiles_per_image(h, w)
    assert L.fmc_conv3x3_halo_sc_packed_bytes(cin, cout, cin_sc) == cout * (9 * cin + cin_sc) * 2
    px = lambda t: t.reshape(-1, t.shape[-1])

    def fn(g):
        xd, xsd = g.inp(px(x), BAND, 0, "x"), g.inp(px(xs), BAND, 0, "xs")
        xs2d = g.inp(px(xs2), BAND, 0, "xs2") if xs2 is not None else None
        wd = g.inp(wt.permute(0, 2, 3, 1).reshape(cout * 9, cin), 320, 0, "w")
        wscd = g.inp(wsc, 320, 0, "w_sc")
        bd, bscd = g.inp(bias, 4, 0, "bias"), g.inp(bsc, 4, 0, "b_sc")
        packed = g.out((cout * (9 * cin + cin_sc) // 64, 64), BF16, 2048, 0, "packed filter")
        K._lib.check(L.fmc_conv3x3_halo_sc_pack_weight(wd.data_ptr(), wscd.data_ptr(), packed.data_ptr(), cin, cout, cin_sc, 160, K._stream()), "pack")
        wp = g.inp(packed.clone(), 2048, 0, "packed filter (as an operand)")
        out = g.out((n * h * w, cout), BF16, BAND, 0, "out")
        part = g.out((n * tiles, 64), F32, max(tiles, 4), 0, "gn_partials") if emit else None
        K._lib.check(L.fmc_conv3x3_halo_sc_bf16(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), bscd.data_ptr(), out.data_ptr(), xsd.data_ptr(), _p(xs2d),
                                                cs1, cin_sc, n, h, w, cin, cout, cout, n, _p(part), K._stream()), "fmc_conv3x3_halo_sc_bf16")
        return {"out": out, "gn_partials": part} if emit else {"out": out}

    got = EG.run_surroundings(fn, "cuda", f"conv3x3_halo_sc {(n, h, w, cin, cout, cs1, cs2)}", torch.cuda.synchronize)
    out = got["out"].view(n, h, w, cout)
    # the pair it replaces: the shortcut rounded to bf16 (an exact GEMM's output), added in the convolution's epilogue
    pair = K.conv3x3_halo(x.cuda(), wt.cuda(), bias.cuda(), residual_nhwc=sc.bfloat16().cuda())
    torch.cuda.synchronize()
    e, e_pair = rel_inf(out, want), rel_inf(pair, want)
    print(f"   conv3x3_halo_sc {(n, h, w, cin, cout, cs1, cs2)}: rel-inf {e:.3e} (gate 6e-3); unfused pair {e_pair:.3e}")
    assert e < 6e-3
    if emit:
        o = out.float().cpu().reshape(n, h * w, 32, cout // 32)
        s_ref = torch.stack([o.sum((1, 3)), (o * o).sum((1, 3))], -1)
        assert rel_inf(got["gn_partials"].view(n, tiles, 32, 2).sum(1), s_ref) < 1e-4
    return out


@pytest.mark.parametrize("n,h,w,cin,cout,cs1,cs2,emit", [
    (1, 10, 32, 64, 160, 64, 0, False),          # one 3x3 chunk, one shortcut chunk: both transitions, no second source
    (2, 13, 64, 128, 320, 64, 128, False),       # a ragged last tile row; three shortcut chunks across the source seam, cs1 != cs2
    (1, 20, 32, 320, 320, 640, 320, True),       # 15 shortcut chunks (the first level's up blocks), statistics epilogue
])
def test_conv3x3_halo_shortcut_segment_matches_fp32(K, n, h, w, cin, cout, cs1, cs2, emit):
    _run_case(K, n, h, w, cin, cout, cs1, cs2, emit, seed=h + cin + cs1)


def test_shortcut_argument_checks_launch_nothing(K):
    """A shortcut source of 32 channels is a shape error, a misaligned one an alignment error; neither launch writes a word of `out`."""
    L = K._lib.load()
    n, h, w, cin, cout = 1, 10, 32, 64, 160
    x, xs, _, wt, wsc, bias, bsc = _data(n, h, w, cin, cout, 64, 0, 3)
    xd, xsd, bd, bscd = x.cuda(), xs.cuda(), bias.cuda(), bsc.cuda()
    wp = torch.zeros(cout * (9 * cin + 64), dtype=BF16, device="cuda")
    arena, out = EG.guarded_output((n * h * w, cout), BF16, 8, 8, 0, "cuda")
    call = lambda xs_ptr, xs2_ptr, c1, csc: L.fmc_conv3x3_halo_sc_bf16(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), bscd.data_ptr(), out.data_ptr(),
                                                                       xs_ptr, xs2_ptr, c1, csc, n, h, w, cin, cout, cout, n, None, K._stream())
    assert not L.fmc_conv3x3_halo_sc_supported(n, h, w, cin, cout, 32, 32)
    assert not L.fmc_conv3x3_halo_sc_supported(n, h, w, cin, cout, 96, 32)
    assert call(xsd.data_ptr(), None, 32, 32) == E_SHAPE
    assert call(xsd.data_ptr(), xsd.data_ptr(), 32, 96) == E_SHAPE                 # (the first of two sources)
    assert call(xsd.data_ptr(), xsd.data_ptr(), 64, 96) == E_SHAPE                 # (the second)
    assert call(xsd.data_ptr() + 8, None, 64, 64) == E_ALIGN
    assert call(xsd.data_ptr(), xsd.data_ptr() + 2, 64, 128) == E_ALIGN
    torch.cuda.synchronize()
    assert bool((arena.view(torch.int16) == 0x5A5A).all())


@pytest.mark.parametrize("cout,folds", [(160, 0), (320, 1)])
def test_resnet_block_with_folded_shortcut_matches_the_oracle_block(K, cout, folds):
    """`ResnetBlock2D(128 + 64 -> cout)` reading `cat([x, skip])` in place, the shortcut inside conv2 (default) and as its own GEMM
    (`SHORTCUT_FOLD` off), against the oracle's restatement of diffusers' block.  cout = 320: conv2 takes the shortcut.  cout = 160: conv2 is
    160 -> 160, which no halo kernel takes (Cin % 64) -- an unsupported shape keeps the separate shortcut under either setting."""
    from oracle import diffusers_restated as OD
    from synfmc_amd.models import layers as L
    torch.manual_seed(7)
    c1, c2, n, h, w = 128, 64, 2, 10, 32
    ref = OD.ResnetBlock2D(in_channels=c1 + c2, out_channels=cout, temb_channels=1280, groups=32, eps=1e-5)
    with torch.no_grad():
        for p in ref.parameters():
            p.normal_(0, p[0].numel() ** -0.5) if p.ndim >= 2 else p.normal_(0, 0.2)
        ref.norm1.weight.add_(1.0); ref.norm2.weight.add_(1.0)
    blk = L.ResnetBlock2D(in_channels=c1 + c2, out_channels=cout, temb_channels=1280, groups=32, eps=1e-5)
    blk.load_state_dict(ref.state_dict(), strict=True)
    blk = blk.to("cuda", BF16).eval().requires_grad_(False)
    ref = ref.bfloat16().float()
    x, skip, temb = torch.randn(n, c1, h, w).bfloat16(), torch.randn(n, c2, h, w).bfloat16(), torch.randn(n, 1280).bfloat16()
    cl = lambda t: t.cuda().contiguous(memory_format=torch.channels_last)
    min_tiles, K.CONV_HALO_MIN_TILES = K.CONV_HALO_MIN_TILES, 1                 # (a 2-image test input: 2 workgroups)
    fold0 = K.SHORTCUT_FOLD
    try:
        with torch.no_grad():
            want = ref(torch.cat([x, skip], 1).float(), temb.float())
            K.SHORTCUT_FOLD = True
            f0, c0 = K.shortcut_fold_calls["folded"], K.conv_halo_calls["conv"]
            got = blk(cl(x), temb.cuda(), skip=cl(skip))
            assert K.shortcut_fold_calls["folded"] - f0 == folds and K.conv_halo_calls["conv"] - c0 == 1 + folds
            K.SHORTCUT_FOLD = False
            plain = blk(cl(x), temb.cuda(), skip=cl(skip))
            assert K.shortcut_fold_calls["folded"] - f0 == folds
            torch.cuda.synchronize()
    finally:
        K.CONV_HALO_MIN_TILES, K.SHORTCUT_FOLD = min_tiles, fold0
    e_f, e_p = rel_inf(got, want), rel_inf(plain, want)
    print(f"   block -> {cout} with the shortcut in conv2 {e_f:.3e}, as its own GEMM {e_p:.3e}")
    assert e_f < 2e-2 and e_f < 2.0 * e_p + 2e-3, (e_f, e_p)

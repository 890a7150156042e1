"""Backward-data of the resampling convolutions and of conv_out on the gfx950 kernels (csrc/conv_resample_bwd.hip, hip_ops.conv3x3_down_frozen /
conv3x3_up_frozen / conv3x3_edge_frozen, layers.Conv2d.forward): every element against the float64 closed forms of tests/resample_bwd_common.py.

Bounds (derived, not tuned): `2^-8 |ref|` for the output's rounding to bf16, `+ 1e-5 sum|terms|` for the fp32 accumulation, and for the upsample
`+ 2^-9 sum|terms|` for the one rounding of the folded filter; `sum|terms|` over |W| |dY| of the unfolded filter.  No element is left out."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import edge_guard_common as EG
from tests import resample_bwd_common as RC

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# (n, H, W, Cin, Cout) of the forward's input.  One pixel; odd image counts and sizes that are no multiple of a 16- / 32-pixel tile; Cin != Cout;
# the three feature-map sizes of a 256 x 384 clip at the three channel counts.  With two or three images the launcher's own choice (tile 0) is the
# smallest stride-2 tile and the split upsample launch for every shape here, so the kernel-level tests below run every shape on EVERY tile through the
# ABI's `tile` argument, whatever the device's CU count; DOWN16 are two layers of a 16-frame clip, which take the two larger stride-2 tiles by themselves
# on a 256-CU device (`test_launcher_choice_follows_its_rule`)
DOWN = [(1, 2, 2, 64, 64), (3, 6, 10, 64, 128), (2, 12, 8, 128, 64), (2, 32, 48, 320, 320), (2, 16, 24, 640, 640), (2, 8, 12, 1280, 1280)]
UP = [(1, 1, 1, 64, 64), (3, 3, 5, 128, 64), (2, 4, 6, 1280, 1280), (2, 8, 12, 1280, 1280), (2, 16, 24, 640, 640),
      (8, 32, 40, 640, 64)]          # (the last: 320 pixel tiles x 10 channel tiles, past the threshold below which the upsample launch splits over G's rows)
DOWN16 = [(16, 32, 48, 320, 320), (16, 16, 24, 640, 640)]
EDGE = [(2, 32, 48, 320, 4), (1, 3, 5, 64, 4)]
TILES = {"down": (0, 1, 2, 3), "up": (0, 1, 2)}          # 0: the launcher's choice; down: 32 x 64, 16 x 64, 16 x 32 per wave; up: unsplit, split over G's rows
BAND = 64                            # guard rows (pixels) around dY and dX: two of the largest tile (32 pixels)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _rnd(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF16).cuda()


def _dy_shape(mode, shape):
    n, h, w, cin, cout = shape
    return {"down": (n, h // 2, w // 2, cout), "up": (n, 2 * h, 2 * w, cout), "edge": (n, h, w, cout)}[mode]


@functools.lru_cache(maxsize=None)
def _case(mode, shape):
    """x, W (channels-last), bias, dY (all bf16 on the GPU), and the float64 reference with its sum of |terms| -- computed once per case."""
    n, h, w, cin, cout = shape
    x = _rnd((n, h, w, cin), 11).permute(0, 3, 1, 2)
    wt = _rnd((cout, 3, 3, cin), 12, 0.05).permute(0, 3, 1, 2)
    bias = _rnd((cout,), 13)
    dy = _rnd(_dy_shape(mode, shape), 14).permute(0, 3, 1, 2)
    d, wd = dy.double(), wt.double()
    if mode == "edge":                      # stride 1: the adjoint of F.conv2d in float64 (the closed forms are the resampling convolutions')
        ref, mag = F.conv_transpose2d(d, wd, padding=1), F.conv_transpose2d(d.abs(), wd.abs(), padding=1)
    else:
        ref = RC.up_bwd(d, wd) if mode == "up" else RC.down_bwd(d, wd)
        mag = RC.magnitude(d, wd, mode == "up")
    return x, wt, bias, dy, ref, mag


def _check(got, ref, mag, up, what):
    assert got.shape == ref.shape and got.dtype == BF16
    assert bool(torch.isfinite(got.float()).all())
    bad, share = RC.misses(got, ref, mag, up)
    print(f"{what}: {bad} of {ref.numel()} elements outside the bound, largest share of the bound used {share:.3f}")
    assert bad == 0, f"{what}: {bad} elements outside the bound (largest error / bound {share:.3f})"


def _frozen(K, mode, x, wt, bias):
    x = x.detach().requires_grad_(True)
    if mode == "down":
        return x, K.conv3x3_down_frozen(x, wt, bias)
    if mode == "up":
        return x, K.conv3x3_up_frozen(x, wt, bias)
    from synfmc_amd.models.layers import Conv2d
    conv = Conv2d(wt.shape[1], wt.shape[0], 3, padding=1).to("cuda", BF16).requires_grad_(False)
    conv.weight.copy_(wt)
    conv.bias.copy_(bias)
    return x, K.conv3x3_edge_frozen(x, conv.weight, conv.padded_conv3x3)


@pytest.mark.parametrize("mode,shape", [("down", s) for s in DOWN + DOWN16] + [("up", s) for s in UP] + [("edge", s) for s in EDGE])
def test_backward_data_every_element(K, mode, shape):
    x, wt, bias, dy, ref, mag = _case(mode, shape)
    before = dict(K.resample_bwd_calls)
    xg, y = _frozen(K, mode, x, wt, bias)
    assert type(y.grad_fn).__name__ == {"down": "_Conv3x3DownFrozenBackward", "up": "_Conv3x3UpFrozenBackward", "edge": "_Conv3x3EdgeFrozenBackward"}[mode]
    (dx,) = torch.autograd.grad(y, xg, dy)
    assert K.resample_bwd_calls[mode] == before[mode] + 1
    _check(dx, ref, mag, mode == "up", f"{mode} {shape}")


def _raw(K, mode, shape, dy_nhwc, wp, out, tile=0):
    n, h, w, cin, cout = shape
    fn = "fmc_conv3x3_up_bwd_bf16" if mode == "up" else "fmc_conv3x3_down_bwd_bf16"
    K._lib.check(getattr(K._lib.load(), fn)(dy_nhwc.data_ptr(), wp.data_ptr(), out.data_ptr(), n, h, w, cin, cout, tile,
                                            torch.cuda.current_stream().cuda_stream), fn)


def _rule(mode, shape, cus):
    """The launcher's choice, restated: the largest tile whose waves give every SIMD two (8 per CU); the upsample keeps 32 x 64 and splits instead."""
    n, h, w, cin, _ = shape
    m = n * h * w if mode == "up" else n * (h // 2) * (w // 2)
    waves = lambda pb, cb: -(-m // (16 * pb)) * (cin // (16 * cb)) * (1 if mode == "up" else 4)
    if mode == "up":
        return 1 if waves(2, 4) >= 8 * cus else 2
    return 1 if waves(2, 4) >= 8 * cus else (2 if waves(1, 4) >= 8 * cus else 3)


def test_launcher_choice_follows_its_rule(K):
    """`*_bwd_tile` is the rule above on this device for every case of this file; on a 256-CU device the cases that go through `hip_ops` with the
    launcher's own choice reach all three stride-2 tiles and both upsample launches."""
    L = K._lib.load()
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    seen = {"down": set(), "up": set()}
    for mode, shapes in (("down", DOWN + DOWN16), ("up", UP)):
        for shape in shapes:
            got = (L.fmc_conv3x3_up_bwd_tile if mode == "up" else L.fmc_conv3x3_down_bwd_tile)(*shape)
            assert got == _rule(mode, shape, cus), (mode, shape, got, cus)
            seen[mode].add(got)
    print(f"{cus} CUs: launcher's choices down {sorted(seen['down'])}, up {sorted(seen['up'])}")
    if cus == 256:
        assert seen == {"down": {1, 2, 3}, "up": {1, 2}}
    assert L.fmc_conv3x3_down_bwd_tile(1, 3, 4, 64, 64) == 0 and L.fmc_conv3x3_up_bwd_tile(1, 4, 4, 96, 64) == 0


def _packed(K, mode, wt):
    cout, cin = wt.shape[:2]
    L = K._lib.load()
    nbytes = (L.fmc_conv3x3_up_bwd_packed_bytes if mode == "up" else L.fmc_conv3x3_down_bwd_packed_bytes)(cin, cout)
    assert nbytes == (16 if mode == "up" else 9) * cin * cout * 2
    wp = torch.empty(nbytes // 2, dtype=BF16, device="cuda")
    fn = "fmc_conv3x3_up_bwd_pack_weight" if mode == "up" else "fmc_conv3x3_down_bwd_pack_weight"
    assert wt.is_contiguous(memory_format=torch.channels_last)
    K._lib.check(getattr(L, fn)(wt.data_ptr(), wp.data_ptr(), cin, cout, torch.cuda.current_stream().cuda_stream), fn)
    return wp


@pytest.mark.parametrize("mode,shape,tile", [(m, s, t) for m, shapes in (("down", DOWN), ("up", UP)) for s in shapes for t in TILES[m]])
def test_repeated_launches_are_bit_identical(K, mode, shape, tile):
    """Every kernel instantiation at every shape through the raw ABI: three launches give the same bits, and those meet the bound element by element."""
    x, wt, bias, dy, ref, mag = _case(mode, shape)
    wp = _packed(K, mode, wt)
    d = dy.permute(0, 2, 3, 1).contiguous()
    outs = []
    for _ in range(3):
        out = torch.empty(shape[0], shape[1], shape[2], shape[3], dtype=BF16, device="cuda")
        _raw(K, mode, shape, d, wp, out, tile)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(_packed(K, mode, wt), wp)
    _check(outs[0].permute(0, 3, 1, 2), ref, mag, mode == "up", f"{mode} {shape} tile {tile}")


SMALLEST = {"down": DOWN[:3], "up": sorted(UP, key=lambda s: s[0] * s[1] * s[2] * s[3] * s[4])[:3]}


@pytest.mark.parametrize("mode,shape,tile", [(m, s, t) for m in ("down", "up") for s in SMALLEST[m] for t in TILES[m][1:]])
def test_poisoned_surroundings_and_sentinels(K, mode, shape, tile):
    """dY and the packed filter in arenas whose every other element is zero, quiet NaN and +Inf in turn; dX in a sentinel arena.  Every tile (the
    launcher's own choice is one of them)."""
    x, wt, bias, dy, ref, mag = _case(mode, shape)
    n, h, w, cin, cout = shape
    wp = _packed(K, mode, wt)
    d = dy.permute(0, 2, 3, 1).contiguous()

    def run(g):
        dv = g.inp(d.view(-1, cout), BAND, name="dy")
        wv = g.inp(wp.view(-1, 512), 8, name="w_packed")
        ov = g.out((n * h * w, cin), BF16, BAND, name="dx")
        assert dv.is_contiguous() and wv.is_contiguous() and ov.is_contiguous()
        _raw(K, mode, shape, dv, wv, ov, tile)
        return {"dx": ov}
    out = EG.run_surroundings(run, "cuda", f"{mode}_bwd {shape} tile {tile}", torch.cuda.synchronize)
    _check(out["dx"].view(n, h, w, cin).permute(0, 3, 1, 2), ref, mag, mode == "up", f"{mode} {shape} tile {tile} in the arena")


def test_outside_the_domain_is_a_shape_error(K):
    L = K._lib.load()
    assert L.fmc_conv3x3_down_bwd_supported(1, 2, 2, 64, 64) and L.fmc_conv3x3_up_bwd_supported(1, 1, 1, 64, 64)
    for args in ((1, 3, 4, 64, 64), (1, 4, 5, 64, 64), (1, 4, 4, 32, 64), (1, 4, 4, 64, 96), (0, 4, 4, 64, 64), (1, 0, 4, 64, 64)):
        assert not L.fmc_conv3x3_down_bwd_supported(*args)
    for args in ((1, 4, 4, 96, 64), (1, 4, 4, 64, 8), (0, 4, 4, 64, 64), (1, 0, 4, 64, 64), (4096, 64, 64, 64, 64)):
        assert not L.fmc_conv3x3_up_bwd_supported(*args)
    t = torch.zeros(64 * 64 * 16, dtype=BF16, device="cuda")
    with pytest.raises(ValueError):
        _raw(K, "down", (1, 3, 4, 64, 64), t, t, t)
    with pytest.raises(ValueError):
        _raw(K, "up", (1, 4, 4, 96, 64), t, t, t)
    for mode, tile in (("down", 4), ("down", -1), ("up", 3)):
        with pytest.raises(ValueError):
            _raw(K, mode, (1, 4, 4, 64, 64), t, t, t, tile)


# ---- module level ---------------------------------------------------------------------------------------------------------------------
def _module(kind, cin, cout):
    from synfmc_amd.models import layers as L
    if kind == "down":
        m = L.Downsample2D(cin, use_conv=True, out_channels=cout)
    elif kind == "up":
        m = L.Upsample2D(cin, use_conv=True, out_channels=cout)
    else:
        m = L.Conv2d(cin, cout, 3, padding=1)
    torch.manual_seed(5)
    for p in m.parameters():
        p.data.normal_(0.0, 0.05)
    return m.to("cuda", BF16).requires_grad_(False)


def _module_ref(kind, m, dy):
    conv = m if kind == "edge" else m.conv
    d, wd = dy.double(), conv.weight.detach().double()
    if kind == "edge":
        return F.conv_transpose2d(d, wd, padding=1), F.conv_transpose2d(d.abs(), wd.abs(), padding=1)
    return (RC.up_bwd(d, wd) if kind == "up" else RC.down_bwd(d, wd)), RC.magnitude(d, wd, kind == "up")


# (the last: a thin convolution whose no-grad forward is the front-end, not the padded route -- Cout a multiple of 8 and no multiple of 64)
MODULES = [("down", (3, 6, 10, 64, 128)), ("up", (3, 3, 5, 128, 64)), ("edge", (2, 32, 48, 320, 4)), ("edge", (2, 6, 10, 64, 32))]
NAMES = {"down": "_Conv3x3DownFrozenBackward", "up": "_Conv3x3UpFrozenBackward", "edge": "_Conv3x3EdgeFrozenBackward"}


@pytest.mark.parametrize("kind,shape", MODULES)
def test_module_under_a_gradient_takes_the_own_backward(K, kind, shape):
    n, h, w, cin, cout = shape
    m = _module(kind, cin, cout)
    x = _rnd((n, h, w, cin), 21).permute(0, 3, 1, 2)
    with torch.no_grad():
        y0 = m(x)
    xg = x.detach().requires_grad_(True)
    y = m(xg)
    assert type(y.grad_fn).__name__ == NAMES[kind]
    assert torch.equal(y, y0)
    dy = _rnd(_dy_shape(kind, shape), 22).permute(0, 3, 1, 2)
    y.backward(dy)
    ref, mag = _module_ref(kind, m, dy)
    _check(xg.grad, ref, mag, kind == "up", f"module {kind} {shape}")


# (an odd size is a case of the stride-2 convolution only)
@pytest.mark.parametrize("kind,shape,why", [(k, s, why) for k, s in MODULES for why in ("trainable", "fp32", "switch_off", "odd") if why != "odd" or k == "down"])
def test_module_keeps_the_previous_path_otherwise(K, monkeypatch, kind, shape, why):
    n, h, w, cin, cout = shape
    if why == "odd":
        h, w = 5, 7
    m = _module(kind, cin, cout)
    dtype = torch.float32 if why == "fp32" else BF16
    if why == "fp32":
        m = m.float()
    if why == "trainable":
        (m if kind == "edge" else m.conv).weight.requires_grad_(True)
    if why == "switch_off":
        monkeypatch.setattr(K, "RESAMPLE_BWD", False)
    xg = _rnd((n, h, w, cin), 23).permute(0, 3, 1, 2).to(dtype).detach().requires_grad_(True)
    before = dict(K.resample_bwd_calls)
    y = m(xg)
    assert type(y.grad_fn).__name__ not in NAMES.values()
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(24)).to(dtype).cuda()
    y.backward(dy)
    assert K.resample_bwd_calls == before
    conv = m if kind == "edge" else m.conv
    x64 = xg.detach().double().requires_grad_(True)
    xin = F.interpolate(x64, scale_factor=2, mode="nearest") if kind == "up" else x64
    (want,) = torch.autograd.grad(F.conv2d(xin, conv.weight.detach().double(), None, conv.stride, conv.padding), x64, dy.double())
    assert bool(torch.isfinite(xg.grad.float()).all())
    assert float((xg.grad.double() - want).abs().max()) <= 2e-2 * float(want.abs().max())        # (the previous path: sanity, not this file's bound)


def test_captured_forward_and_backward_replay_the_eager_bits(K):
    """Downsample2D -> Upsample2D under a gradient inside torch.cuda.graph: nothing packs, allocates outside the pool or synchronises."""
    down, up = _module("down", 64, 128), _module("up", 128, 64)
    n, h, w = 3, 6, 10
    x = torch.zeros(n, h, w, 64, dtype=BF16, device="cuda").permute(0, 3, 1, 2).requires_grad_(True)
    dy = torch.zeros(n, h, w, 64, dtype=BF16, device="cuda").permute(0, 3, 1, 2)

    def step():
        y = up(down(x))
        (gx,) = torch.autograd.grad(y, x, dy)
        return y, gx

    def fill(seed):
        with torch.no_grad():
            x.copy_(_rnd((n, h, w, 64), seed).permute(0, 3, 1, 2))
            dy.copy_(_rnd((n, h, w, 64), seed + 1).permute(0, 3, 1, 2))
    fill(30)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                               # the warm-up: packs the two filters, settles the forward's arm
    torch.cuda.current_stream().wait_stream(side)
    packs = dict(K.resample_bwd_calls)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g, gx_g = step()
    assert K.resample_bwd_calls["down"] == packs["down"] + 1 and K.resample_bwd_calls["up"] == packs["up"] + 1
    for seed in (40, 50):
        fill(seed)
        graph.replay()
        torch.cuda.synchronize()
        y_r, gx_r = y_g.clone(), gx_g.clone()
        y_e, gx_e = step()
        assert type(y_e.grad_fn).__name__ == NAMES["up"]
        assert torch.equal(y_r, y_e) and torch.equal(gx_r, gx_e)
    assert float(gx_r.float().abs().max()) > 0


# ---- the small-width stage-3 model --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stage3():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from einops import rearrange
    from oracle import conditioning as OC
    from tests import common_models as CM
    from tests import training_common as TC
    W4 = (64, 128, 256, 256)
    ou, oe, oa = CM.build_oracle(W4, seed=20, fan_in_gain=0.7)
    clip = CM.synthetic_clip(B=1, Fr=16, H=128, W=128)
    with torch.no_grad():
        pose_emb = rearrange(OC.to_plucker_embedding(clip["c2w"], clip["K"], (128, 128)), "b f c h w -> b c f h w")
    noise = torch.randn(clip["latents"].shape, generator=torch.Generator().manual_seed(9))
    t = torch.tensor([801])
    l_ref, g_ref = TC.oracle_grads(ou, oe, oa, clip, pose_emb, t, noise)
    return dict(ou=ou, oe=oe, oa=oa, W4=W4, clip=clip, pose_emb=pose_emb, noise=noise, t=t, l_ref=l_ref, g_ref=g_ref)


@pytest.mark.parametrize("switch", [True, False])
def test_small_width_stage3_gradients_with_and_without(K, monkeypatch, stage3, switch):
    """The gate of test_gpu_model.test_stage3_training_gradients (bf16: loss 2e-2, gradients 6e-2 rel-inf against the oracle's autograd), with
    the resampling convolutions and conv_out on the own backward and with FMC_RESAMPLE_BWD=0."""
    from tests import common_models as CM
    from tests import training_common as TC
    s = stage3
    monkeypatch.setattr(K, "RESAMPLE_BWD", switch)
    pu, pe, pa = CM.build_product(s["ou"], s["oe"], s["oa"], s["W4"], dtype=BF16)
    pa = pa.float()
    before = dict(K.resample_bwd_calls)
    with torch.autocast("cuda", dtype=BF16):
        l_got, g_got = TC.product_grads(pu, pe, pa, s["clip"], s["pose_emb"], s["t"], s["noise"], "cuda", BF16)
    took = {k: K.resample_bwd_calls[k] - before[k] for k in before}
    print(f"backward launches: {took}")
    assert (took["down"] > 0 and took["up"] > 0 and took["edge"] == 1) if switch else not any(took.values()), took
    lerr = abs(float(s["l_ref"]) - float(l_got)) / abs(float(s["l_ref"]))
    err, scale = TC.compare(s["g_ref"], g_got)
    print(f"stage 3, FMC_RESAMPLE_BWD={int(switch)}: loss rel {lerr:.2e}, gradient rel-inf vs the oracle's autograd {err:.3e} (tolerance 6e-2)")
    assert lerr < 2e-2 and scale > 0 and err < 6e-2

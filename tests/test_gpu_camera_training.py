"""The Camera Encoder, the Camera-Adapter merges and the OMC Adapter trained on the own kernels (`training.camera_trainable_parameters`,
`omc_trainable_parameters`) on the MI355X: the kernels of csrc/train_elementwise.hip through the raw ABI inside sentinel arenas, the
marked layers against float64 autograd of the same module on the CPU, stage 2 / stage 3 on the reduced stack against the oracle, the
path proof, the fp32 masters, and one full-width step of either stage."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import camera_train_common as CC
from tests import common_models as CM
from tests import edge_guard_common as EG
from tests.conv_fwd_common import assert_bf16_close

pytestmark = pytest.mark.gpu
W4 = (64, 128, 256, 256)
BF = torch.bfloat16
GEMM_TOL, GEMM_DW_TOL = 1e-2, 1e-5       # test_linear_trainable_matches_fp64: bf16 activations / outputs; dW straight into the fp32 master
MODULE_TOL = 1.6e-2                      # test_motion_module_gradients_match_oracle, bf16


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def rel_inf(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _lib():
    from synfmc_amd import _lib
    return _lib, _lib.load()


# ---- kernels through the raw ABI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 6, 10, 320), (1, 5, 7, 8), (3, 2, 2, 1280), (1, 1, 1, 8), (1, 3, 9, 24)])
def test_avgpool_kernels_in_arenas(K, shape):
    """(1, 1, 1, 8): an empty forward, an all-zero backward; (1, 3, 9, 24): 12 output groups, no multiple of the workgroup."""
    L, lib = _lib()
    n, H, W, C = shape
    ho, wo = H // 2, W // 2
    g = torch.Generator().manual_seed(H * W + C)
    x = torch.randn(shape, generator=g).to(BF)
    dy = torch.randn(n, ho, wo, C, generator=g).to(BF)

    def fwd(guard):
        xv = guard.inp(x.cuda(), 2 * W, name="x")
        yv = guard.out((n, ho, wo, C), BF, 2 * W, name="y")
        L.check(lib.fmc_avgpool2x2_fwd(xv.data_ptr(), yv.data_ptr(), n, H, W, C, K._stream()), "fmc_avgpool2x2_fwd")
        return {"y": yv}

    def bwd(guard):
        dv = guard.inp(dy.cuda(), 2 * W, name="dy")
        xv = guard.out(shape, BF, 2 * W, name="dx")
        L.check(lib.fmc_avgpool2x2_bwd(dv.data_ptr(), xv.data_ptr(), n, H, W, C, K._stream()), "fmc_avgpool2x2_bwd")
        return {"dx": xv}

    y = EG.run_surroundings(fwd, "cuda", f"avgpool fwd {shape}", torch.cuda.synchronize)["y"]
    assert y.shape == (n, ho, wo, C)
    if y.numel():
        xd = x.double()
        assert_bf16_close(y, CC.avgpool_forward(xd), CC.avgpool_forward(xd.abs()), f"avgpool fwd {shape}")
    dx = EG.run_surroundings(bwd, "cuda", f"avgpool bwd {shape}", torch.cuda.synchronize)["dx"]
    want = CC.avgpool_backward(dy.float(), H, W).to(BF)                 # 0.25 dy is exact: rounded once, bit for bit
    assert torch.equal(dx.cpu().view(torch.int16), want.view(torch.int16))
    if H % 2:
        assert not bool(dx[:, H - 1].any())
    if W % 2:
        assert not bool(dx[:, :, W - 1].any())


def _special(n, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g)
    pool = torch.tensor([0.0, -0.0, -1.5, float("inf"), float("-inf"), 3.3895313892515355e38, -3.3895313892515355e38, -2.0 ** -126])
    idx = torch.randperm(n, generator=g)[: max(1, n // 3)]
    v[idx] = pool[torch.randint(0, len(pool), (idx.numel(),), generator=g)]
    if n >= 8:
        v[:8] = pool
    return v.to(BF)


def _flat_case(fn, inputs, n, offs, what):
    """`fn(*input views, out view)` under zeros / NaN / +Inf around the operands; stream k (the inputs, then the output) starts
    `offs[k]` elements behind a 16-byte boundary, so that with unequal offsets some streams move as 16-byte vectors and others element by
    element in the same launch.  The output bit-identical across the three surroundings, nothing outside it written, the inputs'
    surroundings untouched.  Returns the output."""
    assert len(offs) == len(inputs) + 1
    outs = []
    for poison in EG.POISONS:
        ins = []
        for v, off in zip(inputs, offs):
            padded = torch.cat([torch.full((off,), EG.poison_value(poison, BF), dtype=BF), v])
            arena, view = EG.guarded_input(padded.cuda(), poison, 1, 1)
            assert view[off:].data_ptr() % 16 == (2 * off) % 16
            ins.append((arena, view[off:]))
        oa, ov = EG.guarded_output((n + offs[-1],), BF, 1, 1, device="cuda")
        out = ov[offs[-1]:]
        fn(*[v for _, v in ins], out)
        torch.cuda.synchronize()
        EG.assert_contained(oa, out, f"{what} [{poison}]")
        for arena, view in ins:
            EG.assert_poison_intact(arena, view, poison, f"{what} [{poison}]")
        outs.append(out.clone().cpu())
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), f"{what}: the surroundings moved the output"
    return outs[0]


# (first input, second input, output) elements behind a 16-byte boundary: all aligned; all shifted alike (a scalar head, then vectors);
# ONE stream shifted (that stream moves element by element, the others as vectors); three different alignments
FLAT_OFFSETS = [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 5, 2)]


@pytest.mark.parametrize("offs", FLAT_OFFSETS, ids=lambda o: "off%d%d%d" % o)
@pytest.mark.parametrize("n", [1, 7, 8, 8 * 256 + 3, 8 * 256 * 3 + 5])
def test_relu_and_add_kernels_in_arenas(K, n, offs):
    """+-0, negatives, +-Inf, the largest finite bf16; every combination of aligned and unaligned streams (`vec` bits of `flat_launch`);
    8 * 256 * 3 + 5 elements: three workgroups and a tail."""
    L, lib = _lib()
    a, b, dy = _special(n, 3 * n + sum(offs)), _special(n, 5 * n + sum(offs)), _special(n, 7 * n + sum(offs))
    st = K._stream()
    bits = lambda t: t.view(torch.int16)
    s = _flat_case(lambda av, bv, o: L.check(lib.fmc_add_bf16(av.data_ptr(), bv.data_ptr(), o.data_ptr(), n, st), "add"), [a, b], n, offs, "add")
    want = (a.float() + b.float()).bfloat16()
    nan = torch.isnan(want)                                              # (+Inf + -Inf: a NaN is a NaN, its payload is not compared)
    assert torch.equal(torch.isnan(s), nan) and torch.equal(bits(s)[~nan], bits(want)[~nan])
    y = _flat_case(lambda xv, o: L.check(lib.fmc_relu_fwd(xv.data_ptr(), o.data_ptr(), n, st), "relu"), [a], n, (offs[0], offs[2]), "relu fwd")
    assert torch.equal(bits(y), bits(torch.relu(a)))
    dx = _flat_case(lambda dv, yv, o: L.check(lib.fmc_relu_bwd(dv.data_ptr(), yv.data_ptr(), o.data_ptr(), n, st), "relu_bwd"), [dy, y], n, offs,
                    "relu bwd")
    xa = a.clone().requires_grad_(True)
    torch.relu(xa).backward(dy)                                          # torch.relu with its mask: dy where y > 0, +0 elsewhere
    assert torch.equal(bits(dx), bits(xa.grad))
    assert torch.equal(bits(dx), bits(CC.relu_backward(dy, y)))


@pytest.mark.parametrize("src_off,dst_off", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("shape", [(1, 5, 7, 8), (2, 4, 6, 24)])
def test_avgpool_kernels_unaligned_bases(K, shape, src_off, dst_off):
    """A source or destination whose base lies 2 bytes behind a 16-byte boundary moves element by element (`src_vec` / `dst_vec` of
    `pool_args`), the other tensor as vectors: the same bits as the aligned launch, nothing outside the output written."""
    L, lib = _lib()
    n, H, W, C = shape
    ho, wo = H // 2, W // 2
    g = torch.Generator().manual_seed(H * W + C + src_off)
    x = torch.randn(shape, generator=g).to(BF)
    dy = torch.randn(n, ho, wo, C, generator=g).to(BF)
    st = K._stream()
    y = _flat_case(lambda xv, o: L.check(lib.fmc_avgpool2x2_fwd(xv.data_ptr(), o.data_ptr(), n, H, W, C, st), "avgpool fwd"), [x.reshape(-1)],
                   dy.numel(), (src_off, dst_off), f"avgpool fwd {shape}").view(n, ho, wo, C)
    xd = x.double()
    assert_bf16_close(y, CC.avgpool_forward(xd), CC.avgpool_forward(xd.abs()), f"avgpool fwd {shape}")
    assert torch.equal(y, CC.avgpool_forward(x.float()).to(BF))                       # (the kernel's own order of the four adds, in fp32)
    dx = _flat_case(lambda dv, o: L.check(lib.fmc_avgpool2x2_bwd(dv.data_ptr(), o.data_ptr(), n, H, W, C, st), "avgpool bwd"), [dy.reshape(-1)],
                    x.numel(), (src_off, dst_off), f"avgpool bwd {shape}").view(shape)
    assert torch.equal(dx.view(torch.int16), CC.avgpool_backward(dy.float(), H, W).to(BF).view(torch.int16))


def test_elementwise_autograd_functions(K):
    """`hip_ops.avg_pool2x2`, `relu`, `add` as autograd functions (channels-last and odd sizes) against torch on the same bf16 values."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 16, 5, 7, generator=g).to(BF).cuda().contiguous(memory_format=torch.channels_last)
    b = torch.randn(3, 16, 5, 7, generator=g).to(BF).cuda().contiguous(memory_format=torch.channels_last)
    w = torch.randn(3, 16, 2, 3, generator=g).to(BF).cuda()
    xs, xr = x.clone().requires_grad_(True), x.float().requires_grad_(True)
    y = K.avg_pool2x2(xs)
    y.backward(w)
    F.avg_pool2d(xr, 2, 2).backward(w.float())
    assert y.shape == (3, 16, 2, 3) and rel_inf(y, F.avg_pool2d(x.float(), 2, 2)) < 2.0 ** -8
    assert torch.equal(xs.grad.float(), xr.grad.to(BF).float())
    xs, bs = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = K.add(K.relu(xs), bs)
    dy = torch.randn(out.shape, generator=g).to(BF).cuda()
    out.backward(dy)
    assert torch.equal(out, (torch.relu(x).float() + b.float()).to(BF)) and out.stride() == x.stride()
    assert torch.equal(bs.grad, dy) and torch.equal(xs.grad, torch.where(x > 0, dy, torch.zeros_like(dy)))


# ---- marked layers against float64 autograd of the same module on the CPU --------------------------------------------------------
def _round_params(module):
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(p.to(BF).float())
    return module


def _as_masters(module):
    """cuda, bf16 storage -> fp32 masters that require grad, marked (what `camera_trainable_parameters` does to its modules)."""
    from synfmc_amd.training import _masters, mark_trainable_own
    module = module.to("cuda", BF).eval().requires_grad_(False)
    _masters(list(module.parameters()))
    mark_trainable_own(module)
    return module


def _module_case(product, oracle, run_product, run_oracle, inputs, seed, tol=MODULE_TOL, what="", prepare=None, link=None):
    """Seed `product` (fan-in scaled, bf16-representable; `prepare(product)` may then set some), copy into `oracle` (float64, CPU); run both
    on the same bf16-rounded inputs with the loss `(out * w).sum()`, w bf16-representable (the upstream gradient is then the same numbers on
    both sides); compare the output, every parameter gradient and every input gradient (rel-inf per tensor < tol).  Every gradient is
    non-zero where the reference's is, and in the master's dtype.  `link(product, oracle)` runs between the two runs."""
    CM.reseed(product, seed, fan_in_gain=0.7)
    if prepare is not None:
        with torch.no_grad():
            prepare(product)
    _round_params(product)
    oracle.load_state_dict(product.state_dict(), strict=True)
    oracle = oracle.double().requires_grad_(True)
    product = _as_masters(product)
    ins = [x.to(BF) for x in inputs]
    xo = [x.double().requires_grad_(True) for x in ins]
    xp = [x.cuda().requires_grad_(True) for x in ins]
    got = run_product(product, *xp)
    w = torch.randn(got.shape, generator=torch.Generator().manual_seed(seed + 1)).to(BF).float()
    (got.float() * w.cuda()).sum().backward()
    if link is not None:                                 # (something of the product's run that the reference is to share)
        link(product, oracle)
    ref = run_oracle(oracle, *xo)
    (ref * w.double()).sum().backward()
    errs = {"out": rel_inf(got, ref)}
    po = dict(oracle.named_parameters())
    for name, p in product.named_parameters():
        assert p.dtype == torch.float32 and p.grad is not None and p.grad.dtype == torch.float32, name
        if float(po[name].grad.abs().max()) > 0:
            assert float(p.grad.abs().max()) > 0, f"{name}: zero gradient"
        errs[name] = rel_inf(p.grad, po[name].grad)
    for i, (a, b) in enumerate(zip(xp, xo)):
        errs[f"dx{i}"] = rel_inf(a.grad, b.grad)
    print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < tol, {k: v for k, v in errs.items() if v >= tol}
    return errs, product, oracle


def test_merge_layer_matches_fp64(K):
    """m = s ((h + pose) W^T + b) + h with s != 1, h and pose both requiring grad: one GEMM, the bounds of test_linear_trainable_matches_fp64."""
    from synfmc_amd.models.attention_processor import PoseAdaptorAttnProcessor
    C, s = 128, CC.S
    proc = PoseAdaptorAttnProcessor(hidden_size=C, pose_feature_dim=C, query_condition=True, key_value_condition=True)
    CM.reseed(proc, 5, fan_in_gain=0.7)
    _round_params(proc)
    w, b = proc.qkv_merge.weight.detach().double(), proc.qkv_merge.bias.detach().double()
    proc = _as_masters(proc)
    g = torch.Generator().manual_seed(6)
    h, pose, dm = (torch.randn(2, 16, 24, C, generator=g).to(BF) for _ in range(3))
    hs, ps = h.cuda().requires_grad_(True), pose.cuda().requires_grad_(True)
    m, none = proc._merge(hs, None, ps, s)
    assert none is None and m.dtype == BF
    m.backward(dm.cuda())
    hp = (h.float() + pose.float()).to(BF).double()                      # (the kernel chain rounds h + pose once: the GEMM's operand)
    ref = s * (hp @ w.t() + b) + h.double()
    dmd = dm.double()
    dw = s * dmd.reshape(-1, C).t() @ hp.reshape(-1, C)
    db = s * dmd.reshape(-1, C).sum(0)
    dhp = s * (dmd @ w)
    mrg = proc.qkv_merge
    assert mrg.weight.grad.dtype == torch.float32 and mrg.bias.grad.dtype == torch.float32
    errs = dict(y=rel_inf(m, ref), dw=rel_inf(mrg.weight.grad, dw), db=rel_inf(mrg.bias.grad, db), dh=rel_inf(hs.grad, dhp + dmd),
                dpose=rel_inf(ps.grad, dhp))
    print("merge layer: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < GEMM_TOL and errs["dw"] < GEMM_DW_TOL
    assert not torch.equal(hs.grad, ps.grad)                             # h also receives dm through the residual


@pytest.mark.parametrize("ksize", [1, 3])
def test_trainable_conv_matches_fp64(K, ksize):
    """A marked 1x1 (a token GEMM: the single-GEMM bounds) and 3x3 (`conv3x3_trainable`: its dW passes through bf16 like the bf16_params mode
    of test_linear_trainable_matches_fp64, 1e-2) `Conv2d` at an odd size, 64 -> 128 channels."""
    from synfmc_amd.models.layers import Conv2d
    conv = Conv2d(64, 128, ksize, 1, ksize // 2)
    ref = torch.nn.Conv2d(64, 128, ksize, 1, ksize // 2)
    x = torch.randn(3, 64, 9, 13, generator=torch.Generator().manual_seed(ksize))
    errs, *_ = _module_case(conv, ref, lambda m, a: m(a), lambda m, a: m(a), [x], 10 + ksize, GEMM_TOL, f"conv {ksize}x{ksize}")
    if ksize == 1:
        assert errs["weight"] < GEMM_DW_TOL and errs["bias"] < GEMM_DW_TOL


def test_temporal_attention_block_matches_fp64(K):
    """One temporal block of the encoder at (B, F, P, C) = (1, 16, 6, 64), 8 heads: to_q / to_k / to_v each receive their own slice of
    the fused weight gradient."""
    from oracle import fmc_modules as OM
    from synfmc_amd.models.motion_module import TemporalTransformerBlock
    kw = dict(dim=64, num_attention_heads=8, attention_head_dim=8, attention_block_types=("Temporal_Self",), dropout=0.0,
              cross_attention_dim=None, temporal_position_encoding=True, temporal_position_encoding_max_len=16)
    x = torch.randn(1, 16, 6, 64, generator=torch.Generator().manual_seed(20))
    run_o = lambda m, a: m(a[0].permute(1, 0, 2)).permute(1, 0, 2)[None]           # the reference's `(b h w) f c` tokens
    errs, prod, _ = _module_case(TemporalTransformerBlock(**kw), OM.TemporalTransformerBlock(**kw), lambda m, a: m(a), run_o, [x], 21,
                                 what="temporal block")
    qkv = [getattr(prod.attention_blocks[0], n).weight.grad for n in ("to_q", "to_k", "to_v")]
    assert not torch.equal(qkv[0], qkv[1]) and not torch.equal(qkv[1], qkv[2]) and not torch.equal(qkv[0], qkv[2])
    assert all(errs[f"attention_blocks.0.{n}.weight"] < MODULE_TOL for n in ("to_q", "to_k", "to_v"))


def test_geglu_feed_forward_matches_fp64(K):
    from oracle import diffusers_restated as OD
    from synfmc_amd.models.layers import FeedForward
    x = torch.randn(2, 16, 6, 64, generator=torch.Generator().manual_seed(30))
    _module_case(FeedForward(64, activation_fn="geglu"), OD.FeedForward(64, activation_fn="geglu"), lambda m, a: m(a, residual=a),
                 lambda m, a: m(a) + a, [x], 31, what="GEGLU feed-forward")


@pytest.mark.parametrize("which", ["encoder", "omc"])
def test_resnet_blocks_match_fp64(K, which):
    """The shipped Camera-Encoder block (ksize 1, sk=True, down=True with the average pool, 64 -> 128, an odd height: the pool floors)
    and the shipped OMC block (ksize 3, sk=True).
    The bias in front of the ReLU alternates +-0.75 (encoder) / +-2.5 (OMC) over the channels: 3 sigma of the pre-activation at these seeded weights.  With a
    zero-centred pre-activation the comparison measures the number format, not the kernels: the bf16 rounding of the block's intermediate
    flips the ReLU mask of ~0.2 % of the elements against float64, each flip moves a weight gradient by one whole term of a random-sign sum
    of N, and that ratio does not shrink with N -- a float64 emulation of the block with every layer output rounded to bf16 and nothing
    else gives 1.06e-1 (block1.weight) and 3.5e-2 (block1.bias) at the 1.6e-2 gate, the same figures the kernels gave on the MI355X
    (1.06e-1 / 3.6e-2); with the biases it gives 2.9e-3 / 1.6e-3.  The mask still switches channels off and single elements on."""
    from oracle import fmc_modules as OM
    if which == "encoder":
        from synfmc_amd.models.pose_adaptor import ResnetBlock
        prod = ResnetBlock(64, 128, down=True, ksize=1, sk=True, use_conv=False)
        ref = OM._EncResnetBlock(64, 128, down=True, ksize=1, sk=True, use_conv=False, skep_on_input=True)
    else:
        from synfmc_amd.adapter import ResnetBlock
        prod = ResnetBlock(64, 64, down=False, ksize=3, sk=True, use_conv=False)
        ref = OM._EncResnetBlock(64, 64, down=False, ksize=3, sk=True, use_conv=False, skep_on_input=False)
    x = torch.randn(4, 64, 11, 14, generator=torch.Generator().manual_seed(40))
    mag = 0.75 if which == "encoder" else 2.5              # (the OMC block's pre-activation has sigma 0.7, the encoder's 0.25)
    bias = lambda m: m.block1.bias.copy_(torch.where(torch.arange(m.block1.bias.numel()) % 2 == 0, mag, -mag))
    _module_case(prod, ref, lambda m, a: m(a), lambda m, a: m(a), [x], 41, what=f"{which} ResnetBlock", prepare=bias)


class _MaskAct(torch.nn.Module):
    """ReLU with a GIVEN mask: `h * mask` (gradient `dy * mask`)."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, h):
        return h * self.mask


@pytest.mark.parametrize("which", ["encoder", "omc"])
def test_resnet_blocks_zero_centred_with_the_products_mask(K, which):
    """The same two blocks with their seeded, zero-centred pre-activation: half of every channel's elements on either side of the ReLU.
    The float64 reference takes the ReLU mask of the PRODUCT's run (`y > 0` of what `hip_ops.relu` wrote), so that the comparison is
    not about which elements the bf16 rounding pushed across zero: the element-wise mask, the average pool and the add backward inside
    the module, at the module gate."""
    from oracle import fmc_modules as OM
    if which == "encoder":
        from synfmc_amd.models.pose_adaptor import ResnetBlock
        prod = ResnetBlock(64, 128, down=True, ksize=1, sk=True, use_conv=False)
        ref = OM._EncResnetBlock(64, 128, down=True, ksize=1, sk=True, use_conv=False, skep_on_input=True)
    else:
        from synfmc_amd.adapter import ResnetBlock
        prod = ResnetBlock(64, 64, down=False, ksize=3, sk=True, use_conv=False)
        ref = OM._EncResnetBlock(64, 64, down=False, ksize=3, sk=True, use_conv=False, skep_on_input=False)
    seen = {}
    prod.block2.register_forward_pre_hook(lambda mod, inp: seen.__setitem__("a", inp[0].detach()))

    def link(product, oracle):
        a = seen["a"]
        on = float((a > 0).float().mean())
        assert 0.3 < on < 0.7, on                        # zero-centred: the mask is mixed inside every channel
        oracle.act = _MaskAct((a > 0).double().cpu())
    x = torch.randn(4, 64, 11, 14, generator=torch.Generator().manual_seed(40))
    _module_case(prod, ref, lambda m, a: m(a), lambda m, a: m(a), [x], 41, what=f"{which} ResnetBlock, zero-centred, product's mask", link=link)


# ---- stage 2 / stage 3 on the reduced stack ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stack(K):
    from einops import rearrange
    from oracle import conditioning as OC
    ou, oe, oa = CM.build_oracle(W4, seed=21, fan_in_gain=0.7)
    clip = CM.synthetic_clip(B=1, Fr=16, H=128, W=128)
    with torch.no_grad():
        pose_emb = rearrange(OC.to_plucker_embedding(clip["c2w"], clip["K"], (128, 128)), "b f c h w -> b c f h w")
    return dict(ou=ou, oe=oe, oa=oa, clip=clip, pose_emb=pose_emb)


def _stage2_grads(stack, route):
    from synfmc_amd.training import camera_trainable_parameters
    from tests import training_common as TC
    pu, pe, _ = CM.build_product(stack["ou"], stack["oe"], stack["oa"], W4, dtype=BF)
    noise = torch.randn(stack["clip"]["latents"].shape, generator=torch.Generator().manual_seed(11))
    t = torch.tensor([423])
    if route == "new":
        camera_trainable_parameters(pu, pe)
    else:
        pe = pe.float()
    with torch.autocast("cuda", dtype=BF, enabled=route != "new"):
        return TC.product_grads_stage2(pu, pe, stack["clip"], stack["pose_emb"], t, noise, "cuda", BF), (t, noise)


def test_stage2_gradients_on_the_own_route(stack):
    """`camera_trainable_parameters`, no autocast: the loss and the encoder / merge gradient gates of test_stage2_training_gradients (2e-2);
    the parent route (fp32 encoder under autocast) on the same clip is printed next to it."""
    from tests import training_common as TC
    (l_new, g_new), (t, noise) = _stage2_grads(stack, "new")
    (l_par, g_par), _ = _stage2_grads(stack, "parent")
    l_ref, g_ref = TC.oracle_grads_stage2(stack["ou"], stack["oe"], stack["clip"], stack["pose_emb"], t, noise)
    enc = {k: v for k, v in g_ref.items() if k.startswith("enc.")}
    mrg = {k: v for k, v in g_ref.items() if k.startswith("unet.")}
    assert enc and mrg
    for name, part in (("encoder", enc), ("merges", mrg)):
        e_new, scale = TC.compare(part, g_new)
        e_par, _ = TC.compare(part, g_par)
        print(f"stage-2 {name} gradient rel-inf vs the oracle: new route {e_new:.3e}, parent route {e_par:.3e} (gate 2e-2)")
        assert scale > 0 and e_new < 2e-2
    print(f"stage-2 loss: oracle {float(l_ref):.6f} new {float(l_new):.6f} parent {float(l_par):.6f}")
    assert abs(float(l_ref) - float(l_new)) < 2e-2 * abs(float(l_ref))


def test_stage3_gradients_on_the_own_route(stack):
    """`omc_trainable_parameters`, no autocast, against `oracle_grads` at the gate of test_stage3_training_gradients (bf16: 6e-2)."""
    from synfmc_amd.training import omc_trainable_parameters
    from tests import training_common as TC
    noise = torch.randn(stack["clip"]["latents"].shape, generator=torch.Generator().manual_seed(9))
    t = torch.tensor([801])
    out = {}
    for route in ("new", "parent"):
        pu, pe, pa = CM.build_product(stack["ou"], stack["oe"], stack["oa"], W4, dtype=BF)
        if route == "new":
            omc_trainable_parameters(pa)
        else:
            pa = pa.float()
        with torch.autocast("cuda", dtype=BF, enabled=route != "new"):
            out[route] = TC.product_grads(pu, pe, pa, stack["clip"], stack["pose_emb"], t, noise, "cuda", BF)
    l_ref, g_ref = TC.oracle_grads(stack["ou"], stack["oe"], stack["oa"], stack["clip"], stack["pose_emb"], t, noise)
    e_new, scale = TC.compare(g_ref, out["new"][1])
    e_par, _ = TC.compare(g_ref, out["parent"][1])
    print(f"stage-3 Adapter gradient rel-inf vs the oracle: new route {e_new:.3e}, parent route {e_par:.3e} (gate 6e-2); "
          f"loss oracle {float(l_ref):.6f} new {float(out['new'][0]):.6f} parent {float(out['parent'][0]):.6f}")
    assert abs(float(l_ref) - float(out["new"][0])) < 2e-2 * abs(float(l_ref))
    assert scale > 0 and e_new < 6e-2


@pytest.mark.parametrize("stage", [2, 3])
def test_path_proof_no_torch_op_in_the_trained_layers(stack, stage, K, monkeypatch):
    """`F.linear`, `conv2d`, `avg_pool2d`, `relu` and `torch.matmul` raise inside the trained modules' forward and during the whole
    backward: the step runs to the end.  The log holds exactly the expected entries: one `fmc_linear_wgrad_bf16` launch per fused
    q | k | v, per other projection, per 1x1 convolution and per merge that a gradient reaches, and one `conv3x3_trainable` per trained
    3x3 convolution (torch's C++ backward nodes never pass the patched Python functions: the counts are the proof for the backward)."""
    from synfmc_amd.models.layers import Attention, Conv2d, Linear
    from synfmc_amd.training import camera_trainable_parameters, omc_trainable_parameters
    pu, pe, pa = CM.build_product(stack["ou"], stack["oe"], stack["oa"], W4, dtype=BF)
    if stage == 2:
        camera_trainable_parameters(pu, pe)
        trained = pe
        attn = [m for m in pe.modules() if isinstance(m, Attention)]
        inside = {id(l) for a in attn for l in (a.to_q, a.to_k, a.to_v, a.to_out[0])}
        merges = sum(1 for m in pu.modules() if hasattr(m, "qkv_merge"))
        n_wgrad = 2 * len(attn) + sum(1 for m in pe.modules() if isinstance(m, Linear) and id(m) not in inside) + merges
        assert len(attn) == 8 and merges == 20
    else:
        omc_trainable_parameters(pa)
        trained = pa
        n_wgrad = -1                                   # (`zero_conv_out_list.3` feeds nothing the U-Net reads: no gradient reaches it)
    convs = [m for m in trained.modules() if isinstance(m, Conv2d)]
    n_wgrad += sum(1 for m in convs if m.kernel_size == (1, 1))
    n_conv3 = sum(1 for m in convs if m.kernel_size == (3, 3))
    calls = []
    real = K.conv3x3_trainable
    monkeypatch.setattr(K, "conv3x3_trainable", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    noise = torch.randn(stack["clip"]["latents"].shape, generator=torch.Generator().manual_seed(3))
    families, delta = CC.path_proof(stage, pu, pe, pa, stack["clip"], stack["pose_emb"], torch.tensor([500]), noise)
    print(f"stage {stage}: lora_wgrad launches {families.count('lora_wgrad')} (expected {n_wgrad}), conv3x3_trainable {len(calls)} "
          f"(expected {n_conv3}), dispatch {delta}")
    assert delta["conv3x3"]["own"] >= 2 * n_conv3 and delta["conv3x3"]["vendor"] == 0 and delta["conv3x3"]["ineligible"] == 0
    assert delta["linear"]["vendor"] == 0 and delta["linear"]["ineligible"] == 0
    assert families.count("lora_wgrad") == n_wgrad and len(calls) == n_conv3 > 0
    assert "vendor" not in families


def test_path_proof_switch_off_raises_in_a_child():
    """FMC_TRAINABLE_OWN=0 in a fresh process: the marked modules are back on torch ops, the same patch raises."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FMC_TRAINABLE_OWN="0")
    run = subprocess.run([sys.executable, os.path.join(root, "tests", "camera_train_child.py"), root], env=env, capture_output=True, text=True,
                         timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    assert res["own"] is False and res["raised"] in ("linear", "conv2d", "avg_pool2d", "relu", "matmul"), res


# ---- masters ---------------------------------------------------------------------------------------------------------------------
def _encoder_and_adapter_outputs(stack, pu, pe, pa):
    from synfmc_amd.models.pose_adaptor import features_to_video
    from synfmc_amd.util import get_traj_features_v2
    clip = stack["clip"]
    with torch.no_grad():
        feats = pe(stack["pose_emb"].to("cuda", BF))
        traj = get_traj_features_v2(clip["infos"], clip["masks"], pa, False, 0.0, [False], "cuda", BF)
        pred = pu(clip["latents"].to("cuda", BF), torch.tensor([500], device="cuda"), clip["text"].to("cuda", BF),
                  pose_embedding_features=features_to_video(feats, 1), traj_features=traj).sample
    return [f.clone() for f in feats] + [f.clone() for f in traj] + [pred]


@pytest.mark.parametrize("fused", [False, True], ids=["torch_adamw", "fused_adamw"])
def test_masters_inference_is_bit_identical_and_follows_the_optimizer(stack, fused, K, monkeypatch):
    """No-grad encoder / Adapter outputs (and the U-Net output through the merges) with fp32 masters == the bf16-stored model, bit for
    bit, twice; after one AdamW step they equal a fresh bf16 model loaded from `camera_state_dict` / `omc_state_dict`.
    The vendor arms are off, as under FMC_DETERMINISTIC=1 / FMC_NO_VENDOR=1: MIOpen's small-image 3x3 kernels accumulate with atomics
    (hip_ops.DETERMINISTIC: measured on the 4x4 level of this encoder), and two bf16 builds then differ from each other -- asserted first."""
    from synfmc_amd.training import FusedAdamW, camera_state_dict, camera_trainable_parameters, omc_state_dict, omc_trainable_parameters
    monkeypatch.setattr(K, "DETERMINISTIC", True)
    monkeypatch.setattr(K, "NO_VENDOR", True)
    build = lambda: CM.build_product(stack["ou"], stack["oe"], stack["oa"], W4, dtype=BF)
    _encoder_and_adapter_outputs(stack, *build())       # (settles the autotuner's choice for every shape of the no-grad forward: a shape's first call times its arms)
    base = _encoder_and_adapter_outputs(stack, *build())
    pu, pe, pa = build()
    masters = camera_trainable_parameters(pu, pe) + omc_trainable_parameters(pa)
    names = [f"encoder[{i}]" for i in range(4)] + [f"adapter[{i}]" for i in range(4)] + ["unet"]
    differ = lambda xs, ys: {n: float((a.float() - b.float()).abs().max()) for n, a, b in zip(names, xs, ys) if not torch.equal(a, b)}
    assert differ(_encoder_and_adapter_outputs(stack, *build()), base) == {}, "two bf16 builds disagree"
    for _ in range(2):                                                   # (second call: cached shadows and twins)
        assert differ(_encoder_and_adapter_outputs(stack, pu, pe, pa), base) == {}
    opt = FusedAdamW(masters, lr=1e-3).attach(pu, pe, pa) if fused else torch.optim.AdamW(masters, lr=1e-3)
    g = torch.Generator(device="cuda").manual_seed(5)
    for p in masters:
        p.grad = torch.randn(p.shape, device="cuda", generator=g)
    opt.step()
    moved = _encoder_and_adapter_outputs(stack, pu, pe, pa)
    fu, fe, fa = build()
    sd2, sd3 = camera_state_dict(pu, pe), omc_state_dict(pa)
    for model, sd in ((fe, sd2["pose_encoder_state_dict"]), (fu, sd2["attention_processor_state_dict"]), (fa, sd3["omcm_state_dict"])):
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert unexpected == [] and all(p.dtype == BF for p in model.parameters())
    want = _encoder_and_adapter_outputs(stack, fu, fe, fa)
    assert not torch.equal(moved[0], base[0]) and not torch.equal(moved[-1], base[-1])
    assert differ(moved, want) == {}


def test_quarter_ulp_updates_accumulate_in_the_master(K):
    """Two consecutive updates of a quarter bf16 ulp each move the shadow after the second; a bf16-stored parameter never moves.  (The
    start value has an odd last mantissa bit: half an ulp is a tie that rounds to even, away from it.)"""
    from synfmc_amd.models.layers import Linear, bf16_param
    from synfmc_amd.training import _masters, mark_trainable_own
    start, quarter = 1.0 + 2.0 ** -7, 2.0 ** -9
    lin = Linear(64, 64).to("cuda", BF).requires_grad_(False)
    stored = Linear(64, 64).to("cuda", BF).requires_grad_(False)
    with torch.no_grad():
        lin.weight.fill_(start)
        stored.weight.fill_(start)
    _masters(list(lin.parameters()))
    mark_trainable_own(lin)
    x = torch.ones(4, 64, device="cuda", dtype=BF)
    with torch.no_grad():
        y0 = lin(x).clone()
        lin.weight.add_(quarter)
        stored.weight.add_(quarter)
        assert torch.equal(bf16_param(lin, "weight"), torch.full_like(stored.weight, start)) and torch.equal(lin(x), y0)
        lin.weight.add_(quarter)
        stored.weight.add_(quarter)
        assert bool((bf16_param(lin, "weight").float() > start).all()) and not torch.equal(lin(x), y0)
        assert bool((stored.weight.float() == start).all())


# ---- one full-width step of either stage --------------------------------------------------------------------------------------
def _full_width_step(step, trainable, what):
    before = [p.detach().clone() for p in trainable]
    grads = {}
    hooks = [p.register_post_accumulate_grad_hook(lambda q, i=i: grads.__setitem__(i, (q.grad.abs().max().item(), bool(torch.isfinite(q.grad).all()))))
             for i, p in enumerate(trainable)]
    loss = step()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    moved = sum(1 for p, b in zip(trainable, before) if not torch.equal(p.detach(), b))
    print(f"full-width {what} step on the own route: loss {float(loss):.4f}, tensors with gradients {len(grads)} / {len(trainable)}, masters moved {moved}")
    assert torch.isfinite(loss)
    return grads, moved


def test_full_width_stage2_step(K):
    from tools.camera_train_step import build_stage2, stage2_step_fn
    step, trainable = stage2_step_fn(*build_stage2(), "new")
    grads, moved = _full_width_step(step, trainable, "stage-2")
    assert len(grads) == len(trainable) and all(v[0] > 0 and v[1] for v in grads.values())
    assert moved == len(trainable) and all(p.dtype == torch.float32 for p in trainable)


def test_full_width_stage3_step(K):
    """The U-Net hands no OMC feature to its last down block (`DownBlock3D`, as in the reference), so the Adapter's level 3 -- `body.6`,
    `body.7`, `zero_conv_out_list.3`: 10 of its 48 tensors -- feeds nothing and gets no gradient (the reference trains the Adapter with
    `find_unused_parameters`).  Exactly those tensors stay without a gradient and do not move; every other tensor gets a finite, non-zero
    gradient and moves."""
    from tools.camera_train_step import build_stage3, stage3_step_fn
    pu, pe, pa = build_stage3()
    names = [n for n, _ in pa.named_parameters()]
    step, trainable = stage3_step_fn(pu, pe, pa, "new")
    assert len(trainable) == len(names) == 48 and all(a is b for a, (_, b) in zip(trainable, pa.named_parameters()))
    before = [p.detach().clone() for p in trainable]
    grads, moved = _full_width_step(step, trainable, "stage-3")
    unused = {n for n in names if n.startswith(("body.6.", "body.7.", "zero_conv_out_list.3."))}
    assert len(unused) == 10
    assert {names[i] for i in grads} == set(names) - unused
    assert all(v[0] > 0 and v[1] for v in grads.values())
    for n, p, b in zip(names, trainable, before):
        assert p.dtype == torch.float32
        assert torch.equal(p.detach(), b) == (n in unused), n
    assert moved == 38

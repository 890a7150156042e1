"""The direct fp32 weight gradient of the trainable 3x3 convolutions, `fmc_conv3x3_wgrad_bf16` (csrc/conv_wgrad.hip), on the GPU.

Raw ABI: every case of tests/conv_wgrad_common.py runs on integer data (bit equality with float64: any order of exact sums is exact) and on
Gaussian data (every element within 1e-5 * sum |terms| of float64), with the operands in arenas of zeros, quiet NaN and +Inf and `dw` and the
workspace among sentinels (tests/edge_guard_common.py): the three runs are finite and bit-identical, every word of `dw` and of the partials is
written and none outside, and a second launch gives the same bits.  The wrapper `hip_ops.conv3x3_wgrad` gives the ABI's bits in both layouts.

Through autograd: `conv3x3_trainable` with an fp32 master at stride 1 and 2 against float64 autograd, marked `Downsample` / `ResnetBlock`
modules with torch's convolution patched to raise, and the `FMC_CONV_WGRAD=0` switch in a fresh process."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import camera_train_common as CC
from tests import conv_wgrad_common as CW
from tests import edge_guard_common as EG

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
GEMM_TOL, GEMM_DW_TOL = 1e-2, 1e-5       # tests/test_gpu_camera_training.py: bf16 activations / outputs; dW straight into the fp32 master
MODULE_TOL = 1.6e-2                      # the same file: several bf16 layers in a row

# Bands in rows (pixels) of the guarded tensor.  The loader keeps one 128-pixel slab in flight and requests the next; a tap of a pixel reads at
# most W + 1 pixels before / after it at stride 1 and the source of a pixel past the end of a stride-2 problem lies at most 4 x as far out.
X_BAND = 4 * 256 + 64
DY_BAND = 256
DW_BAND = 64                             # rows of 9 Cin floats: one 64-channel tile of output channels


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def rel_inf(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


@functools.lru_cache(maxsize=None)
def _data(name, kind):
    case = next(c for c in CW.CASES if c["name"] == name)
    x, dy, old = CW.operands(case, kind)
    ref, mag = CW.expected(case, x, dy, old)
    return case, x, dy, old, ref, mag


def _launch(K, g, case, x, dy, old):
    n, H, W, cin, cout, stride = case["shape"]
    lib = K._lib.load()
    xd = g.inp(x.reshape(-1, cin), X_BAND, 0, "x")
    dyd = g.inp(dy.reshape(-1, cout), DY_BAND, 0, "dy")
    dw = g.out((cout, 9 * cin), F32, DW_BAND, 0, "dw", init=None if old is None else old.reshape(cout, 9 * cin))
    need = lib.fmc_conv3x3_wgrad_workspace_bytes(n, H, W, cin, cout, stride)
    assert need == 4 * CW.plan(*case["shape"])["ws_floats"], "the restated plan and the launcher disagree on the split"
    ws = g.out((need // (36 * cin), 9 * cin), F32, DW_BAND, 0, "partials") if need else None
    K._lib.check(lib.fmc_conv3x3_wgrad_bf16(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), n, H, W, cin, cout, stride, case["layout"],
                                            float(case["alpha"]), int(old is not None), None if ws is None else ws.data_ptr(), need,
                                            K._stream()), "fmc_conv3x3_wgrad_bf16")
    first = dw.clone()
    if old is None:                                  # the same problem again: the same bits (an accumulating launch would add twice)
        K._lib.check(lib.fmc_conv3x3_wgrad_bf16(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), n, H, W, cin, cout, stride, case["layout"],
                                                float(case["alpha"]), 0, None if ws is None else ws.data_ptr(), need, K._stream()),
                     "fmc_conv3x3_wgrad_bf16")
        assert torch.equal(first, dw), f"{case['name']}: two launches of one problem differ"
    res = {"dw": dw}
    if ws is not None:
        res["partials"] = ws
    return res


@pytest.mark.parametrize("kind", ["integer", "gaussian"])
@pytest.mark.parametrize("name", [c["name"] for c in CW.CASES])
def test_raw_abi(K, name, kind):
    case, x, dy, old, ref, mag = _data(name, kind)
    n, H, W, cin, cout, stride = case["shape"]
    assert K._lib.load().fmc_conv3x3_wgrad_supported(n, H, W, cin, cout, stride) == 1 and K.conv3x3_wgrad_ok(n, H, W, cin, cout, stride)
    pl = CW.plan(*case["shape"])
    assert pl["chain"] < 168
    what = f"conv3x3_wgrad {name} [{kind}]"
    got = EG.run_surroundings(lambda g: _launch(K, g, case, x, dy, old), "cuda", what, torch.cuda.synchronize)
    assert ("partials" in got) == (pl["splits"] > 1)
    dw = CW.to_oihw(got["dw"].cpu().reshape(-1), cout, cin, case["layout"])
    if kind == "integer":
        CW.check_integer(dw, ref, mag, what)
        print(f"{what}: equal to float64 bit for bit (sum |terms| up to {float(mag.max()):.0f}, {pl['splits']} split(s))")
    else:
        share = CW.check_gaussian(dw, ref, mag, what)
        print(f"{what}: worst element at {share:.3f} of 1e-5 * sum |terms| (chain {pl['chain']}, {pl['splits']} split(s))")


@pytest.mark.parametrize("channels_last", [False, True], ids=["contiguous", "channels_last"])
@pytest.mark.parametrize("name", ["slab_spans_images", "two_splits_acc", "stride2_odd_5x7"])
def test_wrapper_gives_the_abi_bits(K, name, channels_last):
    """`hip_ops.conv3x3_wgrad`: `[Cout, Cin, 3, 3]` fp32 in either memory format, one `conv_wgrad` log entry, no entry of another family."""
    case, x, dy, old, _, _ = _data(name, "gaussian")
    n, H, W, cin, cout, stride = case["shape"]
    case = dict(case, layout=CW.OHWI if channels_last else CW.OIHW)
    ref, mag = CW.expected(case, x, dy, old)
    out = None
    if old is not None or channels_last:
        start = torch.zeros(cout * 9 * cin) if old is None else old
        out = CW.to_oihw(start.clone().cuda(), cout, cin, case["layout"])
        assert out.is_contiguous(memory_format=torch.channels_last) if channels_last else out.is_contiguous()
    K.call_log = []
    try:
        got = K.conv3x3_wgrad(x.cuda(), dy.cuda(), stride, case["alpha"], out, old is not None)
        log = list(K.call_log)
    finally:
        K.call_log = None
    assert got.dtype == F32 and tuple(got.shape) == (cout, cin, 3, 3) and (out is None or got is out)
    assert [e[0] for e in log] == ["conv_wgrad"] and log[0][1] == (n, H, W, cin, cout, stride)
    CW.check_gaussian(got.cpu(), ref, mag, f"wrapper {name}")
    raw = EG.Guard("zeros", "cuda")
    bits = _launch(K, raw, case, x, dy, old)["dw"]
    assert torch.equal(CW.to_oihw(bits.reshape(-1), cout, cin, case["layout"]), got)


def test_outside_the_domain_is_refused(K):
    lib = K._lib.load()
    for args in [(1, 4, 4, 24, 16, 1), (1, 4, 4, 16, 8, 1), (1, 4, 4, 16, 16, 3), (0, 4, 4, 16, 16, 1), (1, 0, 4, 16, 16, 2)]:
        assert lib.fmc_conv3x3_wgrad_supported(*args) == 0 and not K.conv3x3_wgrad_ok(*args)
        assert lib.fmc_conv3x3_wgrad_workspace_bytes(*args) == -1
    x, dy = torch.zeros(1, 4, 4, 24, dtype=BF, device="cuda"), torch.zeros(1, 4, 4, 16, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError):
        K.conv3x3_wgrad(x, dy)
    assert lib.fmc_conv3x3_wgrad_supported(1, 1, 1, 16, 16, 1) == 1 and lib.fmc_conv3x3_wgrad_supported(7, 5, 3, 80, 48, 2) == 1


# ---- through autograd -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,nhw", [(1, (3, 9, 13)), (2, (2, 8, 12))], ids=["stride1", "stride2"])
def test_trainable_conv_fp32_master_matches_fp64(K, stride, nhw, monkeypatch):
    """`conv3x3_trainable` behind a marked 64 -> 128 `Conv2d`: `weight.grad` to the bound the 1x1 meets (1e-5 rel-inf), dX and db to the bf16
    bound, against float64 autograd of the shadow values; the step logs one `conv_wgrad` entry."""
    monkeypatch.setattr(K, "NO_VENDOR", True)
    conv, x, dy = CW.marked_conv(64, 128, stride, nhw)
    w64 = conv.weight.detach().double().cpu().requires_grad_(True)
    b64 = conv.bias.detach().double().cpu().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    F.conv2d(x64, w64, b64, stride, 1).backward(dy.double())
    xs = x.cuda().requires_grad_(True)
    K.call_log = []
    try:
        y = conv(xs)
        y.backward(dy.cuda())
        families = [e[0] for e in K.call_log]
    finally:
        K.call_log = None
    assert conv.weight.grad.dtype == F32 and conv.bias.grad.dtype == F32 and conv.weight.grad.is_contiguous()
    errs = dict(y=rel_inf(y, F.conv2d(x64, w64, b64, stride, 1).detach()), dw=rel_inf(conv.weight.grad, w64.grad),
                db=rel_inf(conv.bias.grad, b64.grad), dx=rel_inf(xs.grad, x64.grad))
    print(f"trainable 3x3 stride {stride}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"; families {families}")
    assert families.count("conv_wgrad") == 1
    assert errs["dw"] < GEMM_DW_TOL and max(errs["y"], errs["dx"], errs["db"]) < GEMM_TOL


def test_bf16_parameter_keeps_the_old_route(K, monkeypatch):
    """The autocast route (a bf16 parameter, no shadows): dW through `conv3x3_weight_grad` as before, bit for bit, and no `conv_wgrad` entry."""
    monkeypatch.setattr(K, "NO_VENDOR", True)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 6, 10, generator=g).to(BF).cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn(64, 64, 3, 3, generator=g) * 0.05).to(BF).cuda().requires_grad_(True)
    dy = torch.randn(2, 64, 6, 10, generator=g).to(BF).cuda().contiguous(memory_format=torch.channels_last)
    K.call_log = []
    try:
        K.conv3x3_trainable(x, w, None).backward(dy)
        families = [e[0] for e in K.call_log]
    finally:
        K.call_log = None
    assert "conv_wgrad" not in families and w.grad.dtype == BF
    assert torch.equal(w.grad, K.conv3x3_weight_grad(x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)))


@pytest.mark.parametrize("which", ["downsample", "resnet_block_down"])
def test_marked_downsample_runs_without_torch_convolution(K, which, monkeypatch):
    """A marked `Downsample(64, use_conv=True)` and `ResnetBlock(64, 128, down=True, ksize=3, sk=False, use_conv=True)`: forward and backward with
    `F.conv2d` (and linear / avg_pool2d / relu / matmul) patched to raise; one `conv_wgrad` entry per 3x3 convolution, every gradient fp32."""
    from synfmc_amd.models.layers import Conv2d
    from synfmc_amd.adapter import ResnetBlock
    from synfmc_amd.models.pose_adaptor import Downsample
    monkeypatch.setattr(K, "NO_VENDOR", True)
    mod = Downsample(64, use_conv=True) if which == "downsample" else ResnetBlock(64, 128, down=True, ksize=3, sk=False, use_conv=True)
    ref = CW.seed_params(mod, 11)
    if which != "downsample":
        # block1's pre-activation has sigma 0.35 here; a bias of +-2 keeps it off zero, so that the bf16 run and float64 gate the same elements
        # through the ReLU (test_resnet_blocks_match_fp64 of tests/test_gpu_camera_training.py does the same)
        with torch.no_grad():
            ref.block1.bias.copy_(torch.where(torch.arange(128) % 2 == 0, 2.0, -2.0))
    import copy
    oracle = copy.deepcopy(ref).double()
    mod = CW.as_masters(ref)
    n_conv3 = sum(1 for m in mod.modules() if isinstance(m, Conv2d) and m.kernel_size == (3, 3))
    assert n_conv3 == (1 if which == "downsample" else 5)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 64, 8, 12, generator=g).to(BF)
    xs = x.cuda().requires_grad_(True)
    K.call_log = []
    try:
        with CC.torch_ops_raise() as state:
            state["armed"] = True
            try:
                y = mod(xs)
                dy = torch.randn(y.shape, generator=g).to(BF)
                y.backward(dy.cuda())
            finally:
                state["armed"] = False
        families = [e[0] for e in K.call_log]
    finally:
        K.call_log = None
    assert families.count("conv_wgrad") == n_conv3, families
    x64 = x.double().requires_grad_(True)
    oracle(x64).backward(dy.double())
    errs = {"dx": rel_inf(xs.grad, x64.grad)}
    po = dict(oracle.named_parameters())
    for name, p in mod.named_parameters():
        assert p.grad is not None and p.grad.dtype == F32, name
        errs[name] = rel_inf(p.grad, po[name].grad)
    print(f"{which}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < MODULE_TOL


def test_stage2_step_on_the_reduced_stack_uses_the_direct_kernel(K, monkeypatch):
    """One stage-2 forward + backward of the reduced stack (the child's stack of tests/camera_train_child.py: widths 64 / 128 / 256 / 256, 16
    frames at 64 x 64) with torch's ops patched to raise: one `conv_wgrad` entry per trained 3x3 convolution and no call of the old chain,
    whose first two launches are `fmc_nhwc_to_cmajor_padded`."""
    from synfmc_amd.models.layers import Conv2d
    from synfmc_amd.training import camera_trainable_parameters
    from tests import common_models as CM
    widths = (64, 128, 256, 256)
    ou, oe, oa = CM.build_oracle(widths, seed=21, fan_in_gain=0.7)
    pu, pe, pa = CM.build_product(ou, oe, oa, widths, dtype=BF)
    clip = CM.synthetic_clip(B=1, Fr=16, H=64, W=64)
    camera_trainable_parameters(pu, pe)
    n_conv3 = sum(1 for m in pe.modules() if isinstance(m, Conv2d) and m.kernel_size == (3, 3))
    old_chain = []
    real = K.conv3x3_weight_grad
    monkeypatch.setattr(K, "conv3x3_weight_grad", lambda *a, **k: (old_chain.append(1), real(*a, **k))[1])
    g = torch.Generator().manual_seed(3)
    pose_emb = torch.randn(1, 6, 16, 64, 64, generator=g)
    noise = torch.randn(clip["latents"].shape, generator=g)
    families, _ = CC.path_proof(2, pu, pe, pa, clip, pose_emb, torch.tensor([500]), noise)
    print(f"stage 2, reduced stack: {families.count('conv_wgrad')} conv_wgrad entries for {n_conv3} trained 3x3 convolutions, "
          f"{len(old_chain)} calls of the old chain")
    assert n_conv3 == 9 and families.count("conv_wgrad") == n_conv3 and not old_chain


def test_switch_off_restores_the_old_route_in_a_child(K):
    """In this process (switch on): `weight.grad` of a marked 3x3 comes from `fmc_conv3x3_wgrad_bf16` and meets the fp32 bound.  With
    FMC_CONV_WGRAD=0 in a fresh process: no `conv_wgrad` entry, and the bits of `conv3x3_weight_grad(...).to(float32)`."""
    assert K.CONV_WGRAD, "run the suite without FMC_CONV_WGRAD=0"
    conv, x, dy = CW.marked_conv(64, 128, 1, (3, 9, 13))
    K.call_log = []
    try:
        conv(x.cuda().requires_grad_(True)).backward(dy.cuda())
        families = [e[0] for e in K.call_log]
    finally:
        K.call_log = None
    ref, _ = CW.reference(x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1), 1)
    err_on = rel_inf(conv.weight.grad, ref)
    assert families.count("conv_wgrad") == 1 and err_on < GEMM_DW_TOL, (families, err_on)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, os.path.join(root, "tests", "conv_wgrad_child.py"), root], env=dict(os.environ, FMC_CONV_WGRAD="0"),
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    print(f"3x3 weight.grad rel-inf vs float64: switch on {err_on:.2e}, switch off {res['dw_err']:.2e}")
    assert res["switch"] is False and "conv_wgrad" not in res["families"] and res["old_route_bits"] and res["dtype"] == "torch.float32", res
    assert res["dw_err"] < GEMM_TOL

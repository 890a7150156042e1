"""The spatial-attention backward (csrc/spatial_attn_bwd.hip) and the frozen layers' backward-data on the paths training takes.

Attention: the fused entry points (`self_attention_qkv`, `cross_attention_q_kv`: gradients written through the stride arguments
into ONE buffer), batch counts that switch both kernels to the remapped workgroup order (`B % 8 == 0`), every output compared
element by element with the float64 closed form on the same rounded inputs (tests/attn_bwd_common.py: `assert_grad_close`,
c = 2^-7 in bf16 and 1e-4 in fp32 storage, relative to the sum of |terms| behind the element).  Shapes: the smallest that cross
each tile boundary of the two kernels.  Every test prints its worst error in units of the bound; one run of this file is recorded
in profiles/attn_backward_bounds.md."""
import contextlib
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attn_bwd_common as AB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float32]
TAG = {torch.bfloat16: "bf16", torch.float32: "fp32"}
KEYS = ("dq", "dk", "dv")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


@functools.lru_cache(maxsize=None)
def _reference(name, dtype):
    """Float64 closed form of a case, computed once and shared (read only)."""
    B, Bkv, H, Sq, Skv, D = AB.CASES[name]
    q, k, v, g = AB.make_inputs(name, dtype)
    return AB.reference_backward(q, k, v, g, H, D ** -0.5)


def _check(what, dtype, got, ref, keys=KEYS):
    """Print the worst err / |terms| of every output in units of the bound, then assert each."""
    c = AB.BOUND[dtype]
    ratios = {k: AB.grad_ratio(got[k], ref[k], ref["mag_" + k]) / c for k in keys}
    print(f"attn-bwd {what} {TAG[dtype]}: worst err / |terms| in units of c = {c:.3e}: " + " ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for k in keys:
        assert got[k].dtype == dtype
        AB.assert_grad_close(got[k], ref[k], ref["mag_" + k], c, f"{what} {TAG[dtype]} {k}")


# ---- a. fused self attention ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("name", list(AB.SELF_CASES))
def test_self_attention_qkv_backward(K, name, dtype):
    _check(name, dtype, AB.run_fused(K, name, dtype), _reference(name, dtype))


# ---- b. fused cross attention --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("name", list(AB.CROSS_CASES))
def test_cross_attention_q_kv_backward(K, name, dtype):
    got, ref = AB.run_fused(K, name, dtype), _reference(name, dtype)
    _check(name, dtype, got, ref)
    if AB.CASES[name][4] == 1:                              # one key: P = 1 and dS = 0 exactly, whatever dO is
        assert float(ref["dq"].abs().max()) < 1e-14 and float(ref["dk"].abs().max()) < 1e-14


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
def test_cross_attention_frozen_kv_same_dq(K, dtype):
    """Frozen K / V (every FMC training stage): no dK / dV kernel, no gradient, and the dQ of the trainable case bit for bit."""
    name = "cross_c1_f8"
    frozen, trained = AB.run_fused(K, name, dtype, kv_grad=False), AB.run_fused(K, name, dtype)
    assert frozen["dk"] is None and frozen["dv"] is None
    assert torch.equal(frozen["dq"], trained["dq"])
    _check(name + " frozen kv", dtype, frozen, _reference(name, dtype), keys=("dq",))


# ---- c. unfused: dense q and outputs, k / v strided slices of one tensor, two frames per K / V entry ------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
def test_spatial_attention_backward_sliced_kv(K, dtype):
    name = "cross_c8_f2"
    B, Bkv, H, Sq, Skv, D = AB.CASES[name]
    C = H * D
    q, k, v, g = (t.to(dtype).cuda() for t in AB.make_inputs(name, dtype))
    q.requires_grad_(True)
    kv = torch.cat([k, v], -1).requires_grad_(True)
    K.spatial_attention(q, kv[..., :C], kv[..., C:], H).backward(g)
    _check(name + " unfused", dtype, dict(dq=q.grad, dk=kv.grad[..., :C], dv=kv.grad[..., C:]), _reference(name, dtype))


# ---- d. the block order changes no bit -------------------------------------------------------------------------------------
def test_block_order_changes_no_bit(K, tmp_path):
    """No atomics, every workgroup owns its outputs: the remapped workgroup order and the plain one (`FMC_SAB_XCD0`, read once per
    process -- hence the worker) must give the same bits."""
    if "FMC_SAB_XCD0" in os.environ:
        pytest.skip("FMC_SAB_XCD0 is set in this process: both runs would take the plain order")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_bwd_child.py"), ROOT, str(tmp_path)],
                         env=dict(os.environ, FMC_SAB_XCD0="1"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    compared = 0
    for name in AB.CHILD_CASES:
        for dtype in DTYPES:
            for key, t in AB.run_fused(K, name, dtype).items():
                plain = np.load(os.path.join(str(tmp_path), f"{name}_{TAG[dtype]}_{key}.npy"))
                assert np.array_equal(plain, t.float().cpu().numpy()), f"{name} {TAG[dtype]} {key}: the block order changes the result"
                compared += 1
    print(f"attn-bwd block order: {compared} gradients bit-identical with and without FMC_SAB_XCD0")
    assert compared == 3 * len(DTYPES) * len(AB.CHILD_CASES)


# ---- e. the backward writes only what it owns --------------------------------------------------------------------------------
SENTINEL = {torch.bfloat16: (torch.int16, 0x5A5A), torch.float32: (torch.int32, 0x5A5A5A5A)}


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("name", ["self_b8_s129_d40", "cross_c8_f2"])
def test_backward_writes_only_its_outputs(K, name, dtype):
    """Raw ABI: dQ | dK | dV are views of ONE sentinel-filled buffer with 16 spare columns per row and two spare rows per batch
    entry (cross attention: also the rows / batch entries that only dQ or only dK | dV reach).  Everything outside the three views
    keeps the sentinel's bits; with dk = dv = NULL the dK | dV areas keep them too."""
    B, Bkv, H, Sq, Skv, D = AB.CASES[name]
    C, scale = H * D, D ** -0.5
    q, k, v, g = (t.to(dtype).cuda() for t in AB.make_inputs(name, dtype))
    if name in AB.SELF_CASES:                                # inputs as training has them: slices of the fused projection
        qkv = torch.cat([q, k, v], -1)
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    else:
        kv = torch.cat([k, v], -1)
        k, v = kv[..., :C], kv[..., C:]
    o, lse = K._spatial_attention_raw(q, k, v, H, scale, True)
    itype, sent = SENTINEL[dtype]
    buf = torch.empty(B, max(Sq, Skv) + 2, 3 * C + 16, dtype=dtype, device="cuda")
    bits = buf.view(itype)
    dq, dk, dv = buf[:, :Sq, :C], buf[:Bkv, :Skv, C:2 * C], buf[:Bkv, :Skv, 2 * C:3 * C]
    own_q, own_kv = torch.zeros_like(bits, dtype=torch.bool), torch.zeros_like(bits, dtype=torch.bool)
    own_q[:, :Sq, :C] = True
    own_kv[:Bkv, :Skv, C:3 * C] = True
    dvec = torch.empty(B, H, Sq, dtype=torch.float32, device="cuda")
    for t in (dq, dk, dv):
        assert t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0

    def call(with_kv):
        bits.fill_(sent)
        K._lib.check(K._lib.load().fmc_spatial_attn_bwd(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), g.data_ptr(), lse.data_ptr(), dvec.data_ptr(), dq.data_ptr(),
            dk.data_ptr() if with_kv else None, dv.data_ptr() if with_kv else None, B, H, Sq, Skv, D, q.stride(0), q.stride(1),
            k.stride(0), k.stride(1), Sq * C, C, dq.stride(0), dq.stride(1), dk.stride(0), dk.stride(1), B // Bkv, scale,
            K._dt(q), K._stream()), "fmc_spatial_attn_bwd")
        torch.cuda.synchronize()

    call(True)
    outside = ~(own_q | own_kv)
    touched = int((bits[outside] != sent).sum())
    print(f"attn-bwd {name} {TAG[dtype]} raw ABI: {touched} of {int(outside.sum())} elements outside the views touched")
    assert touched == 0
    assert not bool((bits[own_q | own_kv] == sent).any())                    # ... and every owned element was written
    full_dq = dq.clone()
    _check(name + " strided views", dtype, dict(dq=dq, dk=dk, dv=dv), _reference(name, dtype))
    call(False)
    assert int((bits[~own_q] != sent).sum()) == 0                            # the dK | dV areas included
    assert torch.equal(dq, full_dq)


# ---- f. frozen layers: backward-data on the forward kernels --------------------------------------------------------------------
def _bf16_ratio(got, ref, mag):
    """Worst error in units of `assert_bf16_close`'s bound, 2^-8 |ref| + 1e-5 |terms|."""
    got, ref, mag = got.detach().double().cpu(), ref.detach().double().cpu(), mag.detach().double().cpu()
    return float(((got - ref).abs() / (2.0 ** -8 * ref.abs() + 1e-5 * mag).clamp_min(1e-300)).max())


def _assert_bf16_close(got, ref, mag, what):
    from tests.test_gpu_kernels import assert_bf16_close
    assert_bf16_close(got, ref, mag, what)


@contextlib.contextmanager
def _own_kernels_untimed(K):
    """The library's own kernel with its own geometry, no timing loop and no vendor arm: shapes this small are in no arm table."""
    saved = K.AUTOTUNE, K.NO_VENDOR
    K.AUTOTUNE, K.NO_VENDOR = False, True
    try:
        yield
    finally:
        K.AUTOTUNE, K.NO_VENDOR = saved


@pytest.mark.parametrize("n,cin,cout,h,w,arm", [
    (2, 320, 640, 10, 32, "halo"),               # backward: 640 -> 320 on one 10 x 32 tile per image, two channel tiles
    (2, 640, 320, 10, 32, "halo"),               # ... and 320 -> 640: four channel tiles
    (3, 640, 320, 8, 16, "halo4"),               # 16 pixels wide: two images per tile, the last tile holds one
    (3, 128, 192, 7, 9, "ring"),                 # no halo form for 9 pixels: the ring kernel, ragged last 128-pixel tile
])
def test_conv3x3_frozen_backward_data(K, n, cin, cout, h, w, arm):
    """`conv3x3_frozen`: dX = conv3x3(dY, flipped filter) on the forward kernels with Cin and Cout in each other's place and no
    bias / temb / residual, against float64 autograd through `F.conv2d` on the same rounded operands.  H != W and Cin != Cout: a
    wrong flip or transpose of the filter cannot pass."""
    g = torch.Generator().manual_seed(n * 1000 + cin + h)
    cl = lambda c: torch.randn(n, h, w, c, generator=g).bfloat16().permute(0, 3, 1, 2)      # logical NCHW over channels-last storage
    x, res, dy = cl(cin), cl(cout), cl(cout)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).bfloat16().contiguous(memory_format=torch.channels_last)
    bias, temb = torch.randn(cout, generator=g).bfloat16(), torch.randn(n, cout, generator=g).bfloat16()
    xr = x.double().requires_grad_(True)
    yr = F.conv2d(xr, wt.double(), bias.double(), padding=1) + temb.double()[:, :, None, None] + res.double()
    yr.backward(dy.double())
    mag_dx = F.conv_transpose2d(dy.double().abs(), wt.double().abs(), padding=1)
    mag_y = F.conv2d(x.double().abs(), wt.double().abs(), bias.double().abs(), padding=1) + temb.double().abs()[:, :, None, None] + res.double().abs()

    xd, rd = x.cuda().requires_grad_(True), res.cuda().requires_grad_(True)
    wd, dyd = wt.cuda(), dy.cuda()
    min_tiles, K.CONV_HALO_MIN_TILES = K.CONV_HALO_MIN_TILES, 1             # (test-sized inputs: a handful of workgroups)
    try:
        with _own_kernels_untimed(K) if arm == "ring" else contextlib.nullcontext():
            y = K.conv3x3_frozen(xd, wd, bias.cuda(), temb.cuda(), rd)
            before = (dict(K.dispatch_calls["conv3x3"]), K.conv_halo_calls["conv"], K.conv_halo_calls.get("conv4", 0))
            y.backward(dyd)
            torch.cuda.synchronize()
    finally:
        K.CONV_HALO_MIN_TILES = min_tiles
    calls = {k: v - before[0][k] for k, v in K.dispatch_calls["conv3x3"].items()}
    halo, halo4 = K.conv_halo_calls["conv"] - before[1], K.conv_halo_calls.get("conv4", 0) - before[2]
    ran = "halo" if halo else ("halo4" if halo4 else "ring")
    print(f"conv3x3_frozen n {n} {cin}->{cout} {h}x{w}: backward {cout}->{cin} on the {ran} kernel {calls}; worst error in units of the bf16 bound: "
          f"dx {_bf16_ratio(xd.grad, xr.grad, mag_dx):.3f} y {_bf16_ratio(y, yr, mag_y):.3f}")
    assert calls == {"own": 1, "vendor": 0, "ineligible": 0} and halo + halo4 <= 1 and ran == arm
    _assert_bf16_close(y, yr, mag_y, "conv3x3_frozen forward")
    assert xd.grad.shape == x.shape
    _assert_bf16_close(xd.grad, xr.grad, mag_dx, "conv3x3_frozen dX")
    assert torch.equal(rd.grad, dyd)                                         # the residual's gradient is dY, bit for bit


@pytest.mark.parametrize("lead,S,Kd,N,alpha,own", [
    (3, 100, 320, 1280, 1.0, True),
    (1, 1, 1280, 320, 1.0, True),
    (2, 65, 640, 640, 0.5, True),
    (2, 32, 320, 72, 1.0, False),                # N % 64 != 0: `linear_backward_data` falls back to a matmul
])
def test_linear_frozen_backward_data(K, lead, S, Kd, N, alpha, own):
    """`linear_frozen` as a frozen 1x1 conv uses it: 3-D x, the weight a fresh `.view(N, K)` of `[N, K, 1, 1]`, dY the non-contiguous
    gradient of a transposed view of the output; dX = alpha dY W against float64."""
    g = torch.Generator().manual_seed(lead * 1000 + S + N)
    x = torch.randn(lead, S, Kd, generator=g).bfloat16()
    w4 = (torch.randn(N, Kd, 1, 1, generator=g) * Kd ** -0.5).bfloat16()
    bias, res = torch.randn(N, generator=g).bfloat16(), torch.randn(lead, S, N, generator=g).bfloat16()
    dyt = torch.randn(lead, N, S, generator=g).bfloat16()                   # gradient of y.transpose(1, 2)
    dy64, w64 = dyt.transpose(1, 2).double(), w4.view(N, Kd).double()
    dx_ref, mag_dx = alpha * dy64 @ w64, alpha * dy64.abs() @ w64.abs()
    y_ref = alpha * (x.double() @ w64.t() + bias.double()) + res.double()
    mag_y = alpha * (x.double().abs() @ w64.abs().t() + bias.double().abs()) + res.double().abs()

    xd, rd, w4d = x.cuda().requires_grad_(True), res.cuda().requires_grad_(True), w4.cuda()
    seen = []
    with _own_kernels_untimed(K):
        y = K.linear_frozen(xd, w4d.view(N, Kd), bias.cuda(), rd, alpha)
        before = dict(K.dispatch_calls["linear"])
        hook = y.register_hook(lambda grad: seen.append(grad.is_contiguous()))
        y.transpose(1, 2).backward(dyt.cuda())
        hook.remove()
        torch.cuda.synchronize()
    calls = {k: v - before[k] for k, v in K.dispatch_calls["linear"].items()}
    print(f"linear_frozen M {lead * S} K {Kd} N {N} alpha {alpha}: backward {calls}; worst error in units of the bf16 bound: "
          f"dx {_bf16_ratio(xd.grad, dx_ref, mag_dx):.3f} y {_bf16_ratio(y, y_ref, mag_y):.3f}")
    assert seen == [S == 1]                                                  # dY reached the backward as a strided view (one row: nothing to stride)
    assert calls == ({"own": 1, "vendor": 0, "ineligible": 0} if own else {"own": 0, "vendor": 0, "ineligible": 0})
    _assert_bf16_close(y, y_ref, mag_y, "linear_frozen forward")
    assert xd.grad.shape == x.shape
    _assert_bf16_close(xd.grad, dx_ref, mag_dx, "linear_frozen dX")
    assert torch.equal(rd.grad, dyt.cuda().transpose(1, 2))

"""The temporal-attention backward (`temporal_attn_bwd_kernel`, synfmc_amd/csrc/temporal_attn.hip) element by element.

Every case of tests/temporal_bwd_common.py runs through the fused entry (`self_attention_qkv(qkv, H, D**-0.5, True)` on the native
`[B, F, P, 3C]` projection) in both storage types; dq, dk and dv are compared separately with the float64 closed form on the same rounded
inputs (`assert_grad_close`: c = 2^-7 in bf16 -- two roundings, counted in temporal_bwd_common.py -- and 1e-4 in fp32 storage, relative
to the sum of |terms| behind the element).  Then: the unfused entry and the `[N, F, C]` layout give the same bits, a softmax four times
as sharp, the fp8 entry through the raw ABI against the closed form on the staged values, and a sentinel buffer around the outputs.
Every test prints its worst error in units of the bound; one run is recorded in profiles/temporal_norm_backward_bounds.md."""
import functools

import pytest
import torch

from tests import attn_bwd_common as AB
from tests import temporal_bwd_common as TB

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DTYPES = [torch.bfloat16, torch.float32]
TAG = {torch.bfloat16: "bf16", torch.float32: "fp32"}
IDS = [TB.case_id(c) for c in TB.CASES]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


@functools.lru_cache(maxsize=None)
def _reference(case, dtype, logit_scale=1.0):
    """Float64 closed form of a case in the native layout, computed once and shared (read only)."""
    return TB.reference(case, dtype, logit_scale)


def _run_fused(K, case, dtype, logit_scale=1.0):
    B, Fr, P, H, D = case
    qkv, g = TB.make_inputs(case, dtype, logit_scale)
    qkv = qkv.to(dtype).cuda().requires_grad_(True)
    K.self_attention_qkv(qkv, H, D ** -0.5, True).backward(g.to(dtype).cuda())
    return dict(zip(TB.KEYS, TB.split_qkv(qkv.grad)))


def _check(what, c, got, ref, dtype):
    """Print the worst err / |terms| of every output in units of the bound, then assert each."""
    ratios = {k: AB.grad_ratio(got[k], ref[k], ref["mag_" + k]) / c for k in TB.KEYS}
    print(f"temporal-bwd {what}: worst err / |terms| in units of c = {c:.3e}: " + " ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for k in TB.KEYS:
        assert got[k].dtype == dtype and got[k].shape == ref[k].shape
        AB.assert_grad_close(got[k], ref[k], ref["mag_" + k], c, f"{what} {k}")


# ---- a. the fused entry, every case (the head-group size each one hits: see TB.CASES) -----------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("case", list(TB.CASES), ids=IDS)
def test_temporal_attention_backward_elementwise(K, case, dtype):
    got, ref = _run_fused(K, case, dtype), _reference(case, dtype)
    _check(f"{TB.case_id(case)} {TAG[dtype]}", AB.BOUND[dtype], got, ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
def test_one_frame_is_exact(K, dtype):
    """One frame: P = 1 and dS = 0 exactly, whatever dO is -- the reference's dQ and dK are exactly zero and its dV is dO, and so must
    the kernel's be, bit for bit.  (The general kernel met this in bf16 storage only: in fp32 storage its three split-bf16 products return
    `1.0 * dO` with 16 of dO's 24 significant bits, 1239 of 1280 elements off by up to 7.2e-6 |dO|.  One frame now takes
    `temporal_attn_bwd_one_frame_kernel`, which copies dO and writes the zeros.)"""
    case = (1, 1, 4, 8, 40)
    got, ref = _run_fused(K, case, dtype), _reference(case, dtype)
    g = TB.make_inputs(case, dtype)[1].to(dtype).cuda()
    # (the float64 closed form forms rowsum(dO * O) and dP = dO V^T in two summation orders: zero to 1e-15 on fp32 inputs, exactly on bf16 ones)
    assert float(ref["dq"].abs().max()) < 1e-14 and float(ref["dk"].abs().max()) < 1e-14 and torch.equal(ref["dv"], g.double().cpu())
    nz = {k: int(torch.count_nonzero(got[k])) for k in ("dq", "dk")}
    dv_diff = int((got["dv"] != g).sum())
    print(f"temporal-bwd one frame {TAG[dtype]}: non-zero dq {nz['dq']} dk {nz['dk']} (largest |dk| {float(got['dk'].abs().max()):.3e}), "
          f"dv != dO in {dv_diff} of {g.numel()} elements (largest |dv - dO| / |dO| {float(((got['dv'] - g).abs() / g.abs().clamp_min(1e-30)).max()):.3e})")
    assert nz["dq"] == 0 and nz["dk"] == 0
    assert dv_diff == 0


# ---- b. the unfused entry and the reference layout: the same ABI call with other strides, so the same bits ------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("case", [(3, 16, 5, 8, 160), (2, 17, 3, 8, 80)], ids=TB.case_id)
def test_unfused_entry_and_reference_layout_give_the_same_bits(K, case, dtype):
    B, Fr, P, H, D = case
    C = H * D
    fused = _run_fused(K, case, dtype)
    qkv, g = (t.to(dtype).cuda() for t in TB.make_inputs(case, dtype))
    x = qkv.clone().requires_grad_(True)
    K.temporal_attention(*TB.split_qkv(x), H).backward(g)                    # three slices of the native projection
    for key, t in zip(TB.KEYS, TB.split_qkv(x.grad)):
        assert torch.equal(t, fused[key]), f"{key}: the unfused entry differs from the fused one"
    x3 = qkv.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C).contiguous().requires_grad_(True)      # `(b p) f c`
    K.temporal_attention(*TB.split_qkv(x3), H).backward(g.permute(0, 2, 1, 3).reshape(B * P, Fr, C).contiguous())
    for key, t in zip(TB.KEYS, TB.split_qkv(x3.grad)):
        assert torch.equal(TB.to_native(t, B), fused[key]), f"{key}: the [N, F, C] layout differs from the native one"
    print(f"temporal-bwd {TB.case_id(case)} {TAG[dtype]}: unfused slices and [N, F, C] layout bit-identical with the fused entry")


# ---- c. a sharper softmax (fp32 storage too: the split-bf16 x3 emulation stays within 1e-4, test_temporal_bwd_reference_host.py) -------
@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("case", TB.SHARP_CASES, ids=TB.case_id)
def test_temporal_attention_backward_sharp_softmax(K, case, dtype):
    _check(f"{TB.case_id(case)} {TAG[dtype]} logits x {TB.SHARP:g}", AB.BOUND[dtype], _run_fused(K, case, dtype, TB.SHARP),
           _reference(case, dtype, TB.SHARP), dtype)


# ---- d. fp8: e4m3 bytes dequantised while staged ------------------------------------------------------------------------------------
def _fp8_backward(K, case, q8, scales_dev, g):
    """`fmc_temporal_attn_fp8_bwd` through the raw ABI on a fused `[B, F, P, 3C]` byte tensor; returns dq, dk, dv (views of one buffer)."""
    B, Fr, P, H, D = case
    C = H * D
    q, k, v = TB.split_qkv(q8)
    dqkv = torch.empty(B, Fr, P, 3 * C, dtype=BF, device="cuda")
    dq, dk, dv = TB.split_qkv(dqkv)
    K._lib.check(K._lib.load().fmc_temporal_attn_fp8_bwd(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), scales_dev.data_ptr(), g.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
        B, P, Fr, H, D, q.stride(0), q.stride(1), q.stride(2), g.stride(0), g.stride(1), g.stride(2), dq.stride(0), dq.stride(1),
        dq.stride(2), D ** -0.5, K._stream()), "fmc_temporal_attn_fp8_bwd")
    torch.cuda.synchronize()
    return dict(dq=dq, dk=dk, dv=dv)


def _fp8_case(K, case, scales_dev, what):
    scales = scales_dev.cpu()
    q8, staged = TB.fp8_inputs(case, scales)
    g = TB.make_inputs(case, BF)[1]
    ref = TB.reference_native(*TB.split_qkv(staged), g, case[3], case[4] ** -0.5)
    got = _fp8_backward(K, case, q8.cuda(), scales_dev, g.to(BF).cuda())
    _check(f"fp8 {TB.case_id(case)} {what}", AB.C_BF16, got, ref, BF)


@pytest.mark.parametrize("case", TB.FP8_CASES, ids=TB.case_id)
def test_temporal_attention_fp8_backward_elementwise(K, case):
    """Power-of-two scales: `byte * scale` is exact in bf16, the reference is the closed form on exactly those values."""
    _fp8_case(K, case, torch.tensor(TB.FP8_POW2_SCALES, device="cuda"), "scales " + " ".join(f"{s:g}" for s in TB.FP8_POW2_SCALES))


def test_temporal_attention_fp8_backward_rolled_scales(K):
    """The scales `Fp8QKVScales.roll()` leaves (margin * amax / 448: no powers of two): the kernel stages `bf16(float(byte) * scale)`,
    an fp32 multiply and one round-to-nearest-even, and so does the reference."""
    sc = K.Fp8QKVScales(torch.device("cuda"), margin=1.25)
    sc.amax.copy_(torch.tensor([171.3, 233.1, 140.9]))
    sc.roll()
    torch.cuda.synchronize()
    scales = sc.scale.cpu()
    assert all(float(torch.frexp(s)[0]) != 0.5 for s in scales)
    _fp8_case(K, (3, 16, 5, 8, 40), sc.scale, "scales " + " ".join(f"{float(s):.6g}" for s in scales))


# ---- e. the backward writes only what it owns -----------------------------------------------------------------------------------------
SENTINEL = {torch.bfloat16: (torch.int16, 0x5A5A), torch.float32: (torch.int32, 0x5A5A5A5A)}


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("case", [(3, 16, 5, 8, 160), (2, 7, 5, 8, 40), (1, 1, 4, 8, 40)], ids=TB.case_id)      # (the last: the one-frame kernel)
def test_backward_writes_only_its_outputs(K, case, dtype):
    """Raw ABI: dQ | dK | dV are views of ONE sentinel-filled buffer with 16 spare columns per row, one spare pixel per frame and one
    spare frame per clip.  Every word outside the three views keeps the sentinel's bits, every word inside is written."""
    B, Fr, P, H, D = case
    C = H * D
    qkv, g = (t.to(dtype).cuda() for t in TB.make_inputs(case, dtype))
    q, k, v = TB.split_qkv(qkv)
    itype, sent = SENTINEL[dtype]
    buf = torch.empty(B, Fr + 1, P + 1, 3 * C + 16, dtype=dtype, device="cuda")
    bits = buf.view(itype)
    bits.fill_(sent)
    own = torch.zeros_like(bits, dtype=torch.bool)
    own[:, :Fr, :P, :3 * C] = True
    dq, dk, dv = TB.split_qkv(buf[:, :Fr, :P, :3 * C])
    for t in (dq, dk, dv):
        assert t.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in t.stride()[:3])
        assert t.data_ptr() + ((B - 1) * t.stride(0) + (Fr - 1) * t.stride(1) + (P - 1) * t.stride(2) + C) * t.element_size() \
            <= buf.data_ptr() + buf.numel() * buf.element_size()
    K._lib.check(K._lib.load().fmc_temporal_attn_bwd(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), g.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, P, Fr, H, D,
        q.stride(0), q.stride(1), q.stride(2), g.stride(0), g.stride(1), g.stride(2), dq.stride(0), dq.stride(1), dq.stride(2),
        D ** -0.5, K._dt(q), K._stream()), "fmc_temporal_attn_bwd")
    torch.cuda.synchronize()
    touched = int((bits[~own] != sent).sum())
    print(f"temporal-bwd {TB.case_id(case)} {TAG[dtype]} raw ABI: {touched} of {int((~own).sum())} words outside the views touched")
    assert touched == 0
    assert not bool((bits[own] == sent).any())                               # ... and every owned word was written
    _check(f"{TB.case_id(case)} {TAG[dtype]} strided views", AB.BOUND[dtype], dict(dq=dq, dk=dk, dv=dv), _reference(case, dtype), dtype)

"""The reference and the bounds of the temporal-attention backward tests, checked on the CPU (tests/temporal_bwd_common.py): the
closed form on the `(b p) f c` rearrangement is autograd's gradient of the native layout, the kernel's bf16 rounding chain meets
c = 2^-7 on exactly the inputs of the GPU tests (logits x 4 included), the split-bf16 x3 products meet 1e-4, and four wrong
kernels do not meet the bound."""
import functools

import pytest
import torch

from tests import attn_bwd_common as AB
from tests import temporal_bwd_common as TB

BF = torch.bfloat16
IDS = [TB.case_id(c) for c in TB.CASES]


@functools.lru_cache(maxsize=None)
def _case(case, logit_scale=1.0, dtype=BF):
    """(q, k, v, g, H, scale) in the `(b p) f c` layout and the reference in the native one (read only)."""
    qkv, g = TB.make_inputs(case, dtype, logit_scale)
    q, k, v = TB.split_qkv(qkv)
    return (TB.to_ref(q), TB.to_ref(k), TB.to_ref(v), TB.to_ref(g), case[3], case[4] ** -0.5), TB.reference(case, dtype, logit_scale)


def _native(got, case):
    return {key: TB.to_native(t, case[0]) for key, t in got.items()}


def _assert_all(got, ref, c, what):
    return {key: AB.assert_grad_close(got[key], ref[key], ref["mag_" + key], c, f"{what} {key}") for key in TB.KEYS}


@pytest.mark.parametrize("case", list(TB.CASES), ids=IDS)
def test_closed_form_is_the_autograd_gradient_of_the_native_layout(case):
    """Float64 autograd through softmax attention over the frame axis of the native `[B, F, P, 3C]` tensor, written with einsum on that
    layout (no rearrangement in common with the reference)."""
    B, Fr, P, H, D = case
    qkv, g = TB.make_inputs(case, BF)
    x = qkv.double().requires_grad_(True)
    q, k, v = (t.reshape(B, Fr, P, H, D) for t in TB.split_qkv(x))
    w = torch.softmax(torch.einsum("bfphd,bgphd->bphfg", q, k) * D ** -0.5, dim=-1)
    torch.einsum("bphfg,bgphd->bfphd", w, v).reshape(B, Fr, P, H * D).backward(g.double())
    ref = TB.reference(case, BF)
    for key, grad in zip(TB.KEYS, TB.split_qkv(x.grad)):
        assert ref[key].shape == grad.shape == (B, Fr, P, H * D)
        err = float((grad - ref[key]).abs().max() / ref["mag_" + key].max())
        assert err < 1e-12, (key, err)
        assert bool((ref["mag_" + key] >= ref[key].abs() * (1 - 1e-12)).all())            # |sum| <= sum |terms|
    if Fr == 1:                                                                           # one key: P = 1, dS = 0, dV = dO
        assert float(ref["dq"].abs().max()) == 0.0 and float(ref["dk"].abs().max()) == 0.0 and float(ref["mag_dq"].min()) > 0
        assert torch.equal(ref["dv"], g.double())


@pytest.mark.parametrize("case", list(TB.CASES), ids=IDS)
def test_bf16_rounding_chain_meets_the_bound(case):
    args, ref = _case(case)
    worst = _assert_all(_native(TB.emulate_bf16_backward(*args), case), ref, AB.C_BF16, TB.case_id(case))
    print(f"{TB.case_id(case)}: emulation, worst err / |terms| in units of 2^-7: " + " ".join(f"{k} {r:.3f}" for k, r in worst.items()))


@pytest.mark.parametrize("case", TB.SHARP_CASES, ids=TB.case_id)
def test_bf16_rounding_chain_meets_the_bound_with_a_sharp_softmax(case):
    args, ref = _case(case, TB.SHARP)
    worst = _assert_all(_native(TB.emulate_bf16_backward(*args), case), ref, AB.C_BF16, TB.case_id(case))
    print(f"{TB.case_id(case)}, logits x 4: emulation, worst err / |terms| in units of 2^-7: " + " ".join(f"{k} {r:.3f}" for k, r in worst.items()))


@pytest.mark.parametrize("logit_scale", [1.0, TB.SHARP])
@pytest.mark.parametrize("case", TB.SHARP_CASES, ids=TB.case_id)
def test_split_bf16_products_meet_the_fp32_bound(case, logit_scale):
    """fp32 storage: hi and lo bf16 pieces with lo * lo dropped stay within 1e-4 of the terms, also with logits four times as large --
    which is why the GPU file runs the sharp softmax in fp32 storage too."""
    args, ref = _case(case, logit_scale, torch.float32)
    worst = _assert_all(_native(TB.emulate_f32_backward(*args), case), ref, AB.C_F32, TB.case_id(case))
    print(f"{TB.case_id(case)}, logits x {logit_scale:g}: split-bf16 x3 emulation, worst err / |terms| in units of 1e-4: "
          + " ".join(f"{k} {r:.3f}" for k, r in worst.items()))


def _fp8_staged(case, scales):
    C = case[3] * case[4]
    _, staged = TB.fp8_inputs(case, scales)
    _, g = TB.make_inputs(case, BF)
    return TB.split_qkv(staged), g


@pytest.mark.parametrize("case", TB.FP8_CASES, ids=TB.case_id)
def test_fp8_staged_values_are_exact_and_the_chain_meets_the_bound(case):
    """Power-of-two scales: `float(byte) * scale` needs no rounding to bf16 (an e4m3 value has four significant bits), and the chain on
    the staged values meets the bf16 bound."""
    scales = torch.tensor(TB.FP8_POW2_SCALES)
    q8, staged = TB.fp8_inputs(case, scales)
    C = case[3] * case[4]
    exact = q8.view(torch.float8_e4m3fn).double() * scales.double().reshape(3, 1).expand(3, C).reshape(3 * C)
    assert torch.equal(staged.double(), exact) and bool(torch.isfinite(staged).all())
    (q, k, v), g = _fp8_staged(case, scales)
    ref = TB.reference_native(q, k, v, g, case[3], case[4] ** -0.5)
    got = TB.emulate_bf16_backward(TB.to_ref(q), TB.to_ref(k), TB.to_ref(v), TB.to_ref(g), case[3], case[4] ** -0.5)
    _assert_all(_native(got, case), ref, AB.C_BF16, "fp8 " + TB.case_id(case))


# ---- wrong kernels must not meet the bound ---------------------------------------------------------------------------------------
PARTIAL = [c for c in TB.CASES if c[1] % 16 and c[1] > 1]


@pytest.mark.parametrize("case", PARTIAL, ids=TB.case_id)
def test_fault_pad_key_left_unmasked(case):
    args, ref = _case(case)
    bad = _native(TB.emulate_bf16_backward(*args, pad_key_unmasked=True), case)
    for key in TB.KEYS:
        with pytest.raises(AssertionError, match="beyond"):
            AB.assert_grad_close(bad[key], ref[key], ref["mag_" + key], AB.C_BF16, key)


@pytest.mark.parametrize("case", PARTIAL, ids=TB.case_id)
def test_fault_rowsum_taken_over_the_pad_keys_too(case):
    """In native storage frame F of clip b is frame 0 of clip b + 1: those are the V rows behind the clip.  dV does not read the row sum."""
    args, ref = _case(case)
    v = TB.split_qkv(TB.make_inputs(case, BF)[0])[2]
    behind = TB.to_ref(torch.roll(v, -1, 0)[:, :-case[1] % 16])
    bad = _native(TB.emulate_bf16_backward(*args, v_behind=behind), case)
    for key in ("dq", "dk"):
        with pytest.raises(AssertionError, match="beyond"):
            AB.assert_grad_close(bad[key], ref[key], ref["mag_" + key], AB.C_BF16, key)


# (case, head groups in bf16 storage = H / GH): pixels != groups, or the wrong decode is the right one
@pytest.mark.parametrize("case,groups", [((3, 16, 5, 8, 160), 4), ((2, 32, 3, 8, 80), 2), ((2, 31, 3, 8, 160), 4)], ids=str)
def test_fault_pixel_and_head_group_extents_swapped_in_the_decode(case, groups):
    args, ref = _case(case)
    good = _native(TB.emulate_bf16_backward(*args), case)
    for key in TB.KEYS:
        with pytest.raises(AssertionError, match="beyond"):
            AB.assert_grad_close(TB.decode_extents_swapped(good[key], groups), ref[key], ref["mag_" + key], AB.C_BF16, key)
        assert torch.equal(TB.decode_extents_swapped(good[key], 1)[:, :, :1], good[key][:, :, :1])      # (the helper moves no value)


@pytest.mark.parametrize("case", [c for c in TB.CASES if c[1] > 1], ids=TB.case_id)
def test_fault_dk_missing_its_scale(case):
    args, ref = _case(case)
    bad = _native(TB.emulate_bf16_backward(*args, dk_unscaled=True), case)
    with pytest.raises(AssertionError, match="beyond"):
        AB.assert_grad_close(bad["dk"], ref["dk"], ref["mag_dk"], AB.C_BF16, "dk")
    _assert_all(dict(bad, dk=_native(TB.emulate_bf16_backward(*args), case)["dk"]), ref, AB.C_BF16, "the other two")

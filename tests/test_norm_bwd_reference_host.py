"""The references and bounds of the LayerNorm / GroupNorm / GEGLU backward tests, checked on the CPU (tests/norm_bwd_common.py): each
closed form is float64 autograd's gradient of the torch operator, the same formulas in plain fp32 meet the bounds, and four wrong
kernels do not."""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_bwd_common as NB

BF = torch.bfloat16
DTYPES = [torch.bfloat16, torch.float32]
TAG = {torch.bfloat16: "bf16", torch.float32: "fp32"}
LN_SMALL = NB.LN_SHAPES
GEGLU_SMALL = [s for s in NB.GEGLU_SHAPES if s[0] * s[1] <= 600000]          # (the formulas do not need the 17 M-element shape)


@pytest.mark.parametrize("shape", LN_SMALL, ids=NB.shape_id)
def test_layernorm_closed_form_is_the_autograd_gradient(shape):
    x, dy, add, gamma, beta = NB.ln_inputs(shape, BF)
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = F.layer_norm(xd, (shape[1],), gd, bd, NB.EPS)
    torch.autograd.backward([y, xd * 1.0], [dy.double(), add.double()])            # (the second use of x is the skip connection)
    ref = NB.ln_reference(x, dy, gamma, add)
    for key, grad in (("dx", xd.grad), ("dgamma", gd.grad), ("dbeta", bd.grad)):
        mag = ref["mag_" + key]
        assert float((grad - ref[key]).abs().max()) <= 1e-12 * float(mag.max()), key
        assert bool((mag >= ref[key].abs() * (1 - 1e-12)).all())                   # |sum| <= sum |terms|


@pytest.mark.parametrize("act", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("shape", NB.GN_SHAPES, ids=NB.shape_id)
def test_groupnorm_closed_form_is_the_autograd_gradient(shape, act):
    x, dy, add, gamma, beta = NB.gn_inputs(shape, BF)
    xd = x.double().requires_grad_(True)
    y = F.group_norm(xd.permute(0, 2, 1), NB.GROUPS, gamma.double(), beta.double(), NB.EPS)
    y = (F.silu(y) if act else y).permute(0, 2, 1)
    torch.autograd.backward([y, xd * 1.0], [dy.double(), add.double()])
    ref = NB.gn_reference(x, dy, gamma, beta, act, add)
    assert float((xd.grad - ref["dx"]).abs().max()) <= 1e-12 * float(ref["mag_dx"].max())
    assert bool((ref["mag_dx"] >= ref["dx"].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("shape", GEGLU_SMALL, ids=NB.shape_id)
def test_geglu_closed_form_is_the_autograd_gradient(shape):
    x, dy = NB.geglu_inputs(shape, BF)
    xd = x.double().requires_grad_(True)
    a, g = xd.chunk(2, dim=-1)
    y = a * F.gelu(g)
    y.backward(dy.double())
    ref = NB.geglu_reference(x, dy)
    assert float((y.detach() - ref["y"]).abs().max()) <= 1e-12 * float(ref["mag_y"].max())
    assert float((xd.grad - ref["dx"]).abs().max()) <= 1e-12 * float(ref["mag_dx"].max())
    assert bool((ref["mag_dx"] >= ref["dx"].abs() * (1 - 1e-12)).all()) and bool((ref["mag_y"] >= ref["y"].abs() * (1 - 1e-12)).all())


def test_geglu_magnitude_takes_the_terms_of_the_cdf_in_absolute_value():
    """At a gate of -5 fp32 forms `1 + erf` from two numbers that cancel to 2.9e-7: an error of half an ulp of 1 is a tenth of the result,
    but 3e-8 of the terms."""
    g = torch.tensor([-5.0])
    x, dy = torch.cat([torch.ones(1), g])[None], torch.ones(1, 1)
    ref = NB.geglu_reference(x, dy)
    cdf32 = 0.5 * (1.0 + torch.erf(g * 0.70710678118654752))                       # the kernel's expression, in fp32
    got = float(g * cdf32)
    assert abs(got - float(ref["y"])) > 0.01 * abs(float(ref["y"]))                # useless relative to |Phi| ...
    assert abs(got - float(ref["y"])) < 1e-6 * float(ref["mag_y"])                 # ... fine relative to its terms


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("shape", LN_SMALL, ids=NB.shape_id)
def test_layernorm_formulas_in_fp32_meet_the_bound(shape, dtype):
    x, dy, add, gamma, beta = NB.ln_inputs(shape, dtype)
    ref = NB.ln_reference(x, dy, gamma, add)
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).square().mean(-1, keepdim=True) + NB.EPS).rsqrt()
    xh, dyh = (x - mean) * rstd, dy * gamma
    dx = rstd * (dyh - dyh.mean(-1, keepdim=True) - xh * (dyh * xh).mean(-1, keepdim=True)) + add
    assert dx.dtype == torch.float32
    r = [NB.assert_close(dx.to(dtype), ref["dx"], ref["mag_dx"], dtype, "dx"),
         NB.assert_close((dy * xh).sum(0), ref["dgamma"], ref["mag_dgamma"], torch.float32, "dgamma"),
         NB.assert_close(dy.sum(0), ref["dbeta"], ref["mag_dbeta"], torch.float32, "dbeta")]
    print(f"layernorm {NB.shape_id(shape)} {TAG[dtype]}: plain fp32, worst error in units of the bound: dx {r[0]:.3f} dgamma {r[1]:.3f} dbeta {r[2]:.3f}")


# ---- wrong kernels must not meet the bound ---------------------------------------------------------------------------------------
TRIPS = (8197, 64)                     # five rows on the second trip


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
def test_fault_second_trips_rows_dropped_from_dgamma(dtype):
    x, dy, add, gamma, beta = NB.ln_inputs(TRIPS, dtype)
    ref = NB.ln_reference(x, dy, gamma, add)
    good = NB.ln_backward_by_trips(x, dy, gamma, add, dtype=dtype)
    for key in ("dgamma", "dbeta"):
        NB.assert_close(good[key], ref[key], ref["mag_" + key], torch.float32, key)
    NB.assert_close(good["dx"], ref["dx"], ref["mag_dx"], dtype, "dx")
    bad = NB.ln_backward_by_trips(x, dy, gamma, add, drop_second_trip_from_dgamma=True, dtype=dtype)
    for key in ("dgamma", "dbeta"):                          # five rows of 8197: 6e-4 of the terms, far beyond 1e-5 of them
        with pytest.raises(AssertionError, match="beyond"):
            NB.assert_close(bad[key], ref[key], ref["mag_" + key], torch.float32, key)


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
def test_fault_addend_dropped_on_the_second_trip(dtype):
    x, dy, add, gamma, beta = NB.ln_inputs(TRIPS, dtype)
    ref = NB.ln_reference(x, dy, gamma, add)
    bad = NB.ln_backward_by_trips(x, dy, gamma, add, drop_addend_after_first_trip=True, dtype=dtype)
    with pytest.raises(AssertionError, match="beyond") as info:
        NB.assert_close(bad["dx"], ref["dx"], ref["mag_dx"], dtype, "dx")
    assert "worst at (81" in str(info.value)                 # a row of the second trip (8192 .. 8196)
    NB.assert_close(bad["dx"][:NB.LN_ROWS_PER_TRIP], ref["dx"][:NB.LN_ROWS_PER_TRIP], ref["mag_dx"][:NB.LN_ROWS_PER_TRIP], dtype, "first trip")


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("shape", [(2, 97, 320), (1, 6150, 320), (1, 9, 4096)], ids=NB.shape_id)
def test_fault_last_row_of_a_split_skipped(shape, dtype):
    x, dy, add, gamma, beta = NB.gn_inputs(shape, dtype)
    ref = NB.gn_reference(x, dy, gamma, beta, True, add)
    NB.assert_close(NB.gn_backward_by_splits(x, dy, gamma, beta, True, add, dtype=dtype), ref["dx"], ref["mag_dx"], dtype, "dx")
    bad = NB.gn_backward_by_splits(x, dy, gamma, beta, True, add, skip_last_row_of_split=True, dtype=dtype)
    with pytest.raises(AssertionError, match="beyond"):
        NB.assert_close(bad, ref["dx"], ref["mag_dx"], dtype, "dx")


def test_group_split_restatement():
    assert NB.gn_split_rows(97, 320) == (49, 2) and NB.gn_split_rows(6150, 320) == (97, 64) and NB.gn_split_rows(48, 320) == (48, 1)
    assert NB.gn_split_rows(9, 4096) == (5, 2) and NB.gn_split_rows(130, 32) == (130, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("shape", [(2, 97, 320), (2, 130, 32), (2, 33, 64)], ids=NB.shape_id)
def test_fault_m2_taken_over_all_channels(shape, dtype):
    x, dy, add, gamma, beta = NB.gn_inputs(shape, dtype)
    ref = NB.gn_reference(x, dy, gamma, beta, False)
    bad = NB.gn_reference(x, dy, gamma, beta, False, group_m2=False)["dx"].float().to(dtype)
    with pytest.raises(AssertionError, match="beyond"):
        NB.assert_close(bad, ref["dx"], ref["mag_dx"], dtype, "dx")

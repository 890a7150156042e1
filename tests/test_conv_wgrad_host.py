"""CPU tests of the direct 3x3 weight gradient's test instruments (tests/conv_wgrad_common.py): the float64 reference against autograd,
the restated split plan against what each GPU case claims, the emulation of the kernel's accumulation order under both instruments, and
the wrong stand-ins, each of which both instruments must reject."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_wgrad_common as CW


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", [(2, 5, 7, 3, 4), (1, 1, 1, 2, 2), (3, 4, 6, 5, 2), (1, 2, 9, 1, 3)])
def test_reference_matches_float64_autograd(shape, stride):
    n, H, W, cin, cout = shape
    g = torch.Generator().manual_seed(H * W + stride)
    x = torch.randn(n, H, W, cin, dtype=torch.float64, generator=g)
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, None, stride, 1)
    assert tuple(y.shape[2:]) == (CW.out_size(H, stride), CW.out_size(W, stride))
    dy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    y.backward(dy)
    dw, mag = CW.reference(x, dy.permute(0, 2, 3, 1).contiguous(), stride)
    assert torch.allclose(dw, w.grad, rtol=1e-12, atol=1e-12), float((dw - w.grad).abs().max())
    assert bool((mag >= dw.abs() - 1e-12).all())
    # sum |terms| is the same loop on absolute values: the weight gradient of |x|, |dy|
    dwa, _ = CW.reference(x.abs(), dy.abs().permute(0, 2, 3, 1).contiguous(), stride)
    assert torch.allclose(mag, dwa, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", CW.CASES, ids=[c["name"] for c in CW.CASES])
def test_cases_sit_where_they_claim(case):
    pl = CW.plan(*case["shape"])
    for k, v in case["claim"].items():
        assert pl[k] == v, (case["name"], k, pl[k], v)
    assert pl["chain"] < 168, (case["name"], pl)                     # 1e-5 / 2^-24 = 167.8: the bound pays for that many half-ulp roundings
    assert (pl["ws_floats"] > 0) == (pl["splits"] > 1)
    n, H, W, cin, cout, stride = case["shape"]
    assert cin % 16 == 0 and cout % 16 == 0 and stride in (1, 2)


def test_case_table_reaches_every_edge():
    by = {c["name"]: (c, CW.plan(*c["shape"])) for c in CW.CASES}
    assert CW.CHAIN_LIMIT == 167
    assert any(p["splits"] > 1 and c["accumulate"] for c, p in by.values()) and any(p["splits"] == 1 and c["accumulate"] for c, p in by.values())
    assert {c["layout"] for c, p in by.values() if p["splits"] > 1} == {CW.OIHW, CW.OHWI}
    assert {c["layout"] for c, p in by.values() if p["splits"] == 1} == {CW.OIHW, CW.OHWI}
    assert any(p["P"] % 128 == 0 and p["splits"] == 1 for c, p in by.values()) and any(p["P"] % 128 == 1 for c, p in by.values())
    assert any(c["shape"][5] == 2 and (c["shape"][1] % 2 or c["shape"][2] % 2) for c, p in by.values())
    c, p = by["two_splits"]                                          # the split boundary is mid-row and mid-image
    first = p["chunk_slabs"] * 128
    n, H, W = c["shape"][:3]
    assert first % W != 0 and first % (H * W) != 0 and first // (H * W) == 1
    c, p = by["slab_spans_images"]
    assert 128 % (c["shape"][1] * c["shape"][2]) != 0 and c["shape"][1] * c["shape"][2] < 128


@pytest.mark.parametrize("kind", ["integer", "gaussian"])
@pytest.mark.parametrize("case", CW.CASES, ids=[c["name"] for c in CW.CASES])
def test_emulation_passes_both_instruments(case, kind):
    n, H, W, cin, cout, stride = case["shape"]
    x, dy, old = CW.operands(case, kind)
    ref, mag = CW.expected(case, x, dy, old)
    got = CW.to_oihw(CW.emulate(x, dy, stride, case["alpha"], old, case["layout"]), cout, cin, case["layout"])
    (CW.check_integer if kind == "integer" else CW.check_gaussian)(got, ref, mag, case["name"])
    if case["name"] == "one_pixel":                                  # every tap but the centre one lies outside the image
        centre = torch.zeros(3, 3, dtype=torch.bool)
        centre[1, 1] = True
        assert bool((got[:, :, ~centre] == 0).all()) and bool((got[:, :, 1, 1] != 0).any())


@pytest.mark.parametrize("kind", ["integer", "gaussian"])
@pytest.mark.parametrize("defect", CW.DEFECTS)
def test_wrong_stand_ins_are_rejected(defect, kind):
    """Each defect is caught by the instrument on at least one case of the table, and changes nothing where it cannot apply."""
    check = CW.check_integer if kind == "integer" else CW.check_gaussian
    caught = []
    for case in CW.CASES:
        n, H, W, cin, cout, stride = case["shape"]
        x, dy, old = CW.operands(case, kind)
        ref, mag = CW.expected(case, x, dy, old)
        got = CW.to_oihw(CW.emulate(x, dy, stride, case["alpha"], old, case["layout"], defect=defect), cout, cin, case["layout"])
        try:
            check(got, ref, mag, case["name"])
        except CW.Rejected:
            caught.append(case["name"])
    print(f"{defect} [{kind}]: rejected on {caught}")
    assert caught, f"{defect}: no case of the table notices it under the {kind} instrument"


def test_routing_keeps_the_measured_slower_class_on_the_old_chain():
    """`hip_ops.conv3x3_wgrad_routed` (pure Python): the trained shapes of a 16-frame 256 x 384 clip go to the direct kernel except the OMC
    Adapter's 832 -> 320 `conv_in` (profiles/conv_wgrad.md); stride 2 has no old chain and always does; outside the domain nothing does."""
    from synfmc_amd import hip_ops as K
    for cin, cout, h, w in [(384, 320, 32, 48), (320, 320, 32, 48), (640, 640, 16, 24), (1280, 1280, 8, 12), (1280, 1280, 4, 6)]:
        assert K.conv3x3_wgrad_ok(16, h, w, cin, cout, 1) and K.conv3x3_wgrad_routed(16, h, w, cin, cout, 1)
    assert K.conv3x3_wgrad_ok(16, 32, 48, 832, 320, 1) and not K.conv3x3_wgrad_routed(16, 32, 48, 832, 320, 1)
    assert K.conv3x3_wgrad_routed(16, 64, 96, 832, 320, 2)
    assert not K.conv3x3_wgrad_routed(1, 8, 8, 24, 16, 1) and not K.conv3x3_wgrad_ok(1, 8, 8, 16, 16, 3)

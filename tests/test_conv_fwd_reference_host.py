"""CPU side of tests/test_gpu_conv_forward_elementwise.py: the float64 references of tests/conv_fwd_common.py against independent restatements, a
plain-torch emulation of the kernels' documented rounding chain under both instruments at every GPU shape, and the wrong stand-ins each instrument
has to catch -- the four faults that stay below the old max-norm gate of 6e-3, and seven indexing faults the exact runs see."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_fwd_common as C

OLD_GATE = 6e-3          # `max|got - ref| / max|ref|` of tests/test_gpu_conv_halo.py, test_gpu_conv_shortcut_fold.py and test_conv_upsample_fold.py


def _id(s):
    return "-".join(str(int(v) if isinstance(v, bool) else v) or "none" for v in s[1:]) if isinstance(s, C.Spec) else str(s)


# ---- the references ---------------------------------------------------------------------------------------------------------------------------------
def _tap_loop(s, d):
    """The convolution without F.conv2d: explicit zero padding, explicit nearest 2x, a loop over the nine taps, one image at a time for temb."""
    x = d["x"].double() if d["x2"] is None else torch.cat([d["x"].double(), d["x2"].double()], -1)        # [n, hs, ws, cin]
    if s.ups:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    n, h, w, _ = x.shape
    xp = torch.zeros(n, h + 2, w + 2, s.cin, dtype=torch.float64)
    xp[:, 1:-1, 1:-1] = x
    wt = d["w"].double()
    st = 2 if s.s2 else 1
    ho, wo = C.out_hw(s)
    out = torch.zeros(n, ho, wo, s.cout, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + h:st, kx:kx + w:st][:, :ho, :wo] @ wt[:, :, ky, kx].t()
    if d["bias"] is not None:
        out += d["bias"].double()
    if d["temb"] is not None:
        for i in range(n):
            out[i] += d["temb"][i // d["tdiv"]].double()
    if d["res"] is not None:
        out += d["res"].double()
    if s.cs1:
        out += F.conv2d(d["xs"].double().permute(0, 3, 1, 2), d["wsc"].double()[:, :s.cs1, None, None]).permute(0, 2, 3, 1)
        if s.cs2:
            out += F.conv2d(d["xs2"].double().permute(0, 3, 1, 2), d["wsc"].double()[:, s.cs1:, None, None]).permute(0, 2, 3, 1)
        out += d["bsc"].double()
    return out


MODES = [
    C.spec("bf16", 2, 5, 7, 64, 24),                                            # padding at odd sizes
    C.spec("bf16", 2, 6, 10, 64, 24, ups=True, extras="b"),                     # nearest 2x
    C.spec("bf16", 2, 6, 10, 64, 24, s2=True, extras="b"),                      # stride 2
    C.spec("bf16", 2, 5, 7, 128, 24, c2=64, extras="r"),                        # two sources
    C.spec("bf16", 6, 3, 4, 64, 24, extras="t", tdiv=3),                        # per-clip temb rows
    C.spec("bf16", 2, 5, 7, 64, 32, extras="b", cs1=64, cs2=128),               # shortcut segment over two sources
]


@pytest.mark.parametrize("s", MODES, ids=_id)
def test_reference_equals_conv2d_and_a_tap_loop_in_float64(s):
    d = C.gauss_inputs(s, 3)
    r = C.reference(s, d)
    want = _tap_loop(s, d)
    assert r["ref"].dtype == torch.float64 and r["ref"].shape == want.shape == (s.n, *C.out_hw(s), s.cout)
    assert C.rel_inf(r["ref"], want) < 1e-13
    # ... and F.conv2d on the concatenated NCHW input, every addend in its broadcast form
    x = d["x"].double() if d["x2"] is None else torch.cat([d["x"].double(), d["x2"].double()], -1)
    x = x.permute(0, 3, 1, 2)
    if s.ups:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    y = F.conv2d(x, d["w"].double(), None if d["bias"] is None else d["bias"].double(), 2 if s.s2 else 1, 1)
    if d["temb"] is not None:
        y = y + d["temb"].double().repeat_interleave(s.tdiv, 0)[:, :, None, None]
    if d["res"] is not None:
        y = y + d["res"].double().permute(0, 3, 1, 2)
    if s.cs1:
        cat = torch.cat([d["xs"].double(), d["xs2"].double()], -1).permute(0, 3, 1, 2)
        y = y + F.conv2d(cat, d["wsc"].double()[:, :, None, None], d["bsc"].double())
    assert C.rel_inf(r["ref"], y.permute(0, 2, 3, 1)) < 1e-13
    assert bool((r["mag"] >= r["ref"].abs() * (1 - 1e-12)).all())


def test_groupnorm_operand_reference_pads_the_normalised_tensor_with_zeros():
    s = C.spec("bf16", 2, 4, 5, 64, 32, gn=1)
    d = C.gauss_inputs(s, 4)
    op, amb = C.operand(s, d)
    a, b = d["coef"].double()[..., 0], d["coef"].double()[..., 1]
    z = d["x"].double() * a[:, None, None] + b[:, None, None]
    assert op.shape == z.shape and amb.shape == z.shape
    assert bool(((op - F.silu(z)).abs() <= 2.0 ** -8 * F.silu(z).abs()).all())               # rounded to bf16 once
    want = F.conv2d(op.permute(0, 3, 1, 2), d["w"].double(), None, 1, 1).permute(0, 2, 3, 1)
    assert torch.equal(C.reference(s, d)["ref"], want)
    gn = F.group_norm(d["x"].double().permute(0, 3, 1, 2), 32, None, None, 1e-5).permute(0, 2, 3, 1)
    assert float(((z - b[:, None, None]) / a[:, None, None] - d["x"].double()).abs().max()) < 1e-6 and gn.shape == z.shape


def test_folded_reference_is_the_nine_tap_reference_up_to_the_filters_one_rounding():
    s = C.fold_spec(2, 3, 8, 64, 32, True)
    d = C.int_inputs(s, 5)
    assert torch.equal(C.folded_reference(s, d)["ref"], C.reference(s, d)["ref"])            # integers: the fold is exact
    d = C.gauss_inputs(s, 5)
    assert 0 < C.rel_inf(C.folded_reference(s, d)["ref"], C.reference(s, d)["ref"]) < 4e-3


def test_slot_maps_follow_the_documented_geometry():
    slot, per = C.slot_map("halo", 24, 64)
    assert per == 6 and slot[9, 31] == 0 and slot[9, 32] == 1 and slot[10, 0] == 2 and slot[23, 63] == 5
    slot, per = C.slot_map("halo4", 16, 24)                                                  # W % 16 != 0: 5 x 8 row blocks
    assert per == 12 and slot[4, 7] == 0 and slot[5, 8] == 4 and slot[15, 23] == 11
    slot, per = C.slot_map("halo4", 16, 16)                                                  # 10 x 16 row blocks, the lower one six rows high
    assert per == 2 and slot[9, 15] == 0 and slot[10, 0] == 1
    slot, per = C.slot_map("halo_fold", 26, 64)                                              # source 13 x 32: two source tiles x four phases
    assert per == 8 and slot[0, 0] == 0 and slot[0, 1] == 1 and slot[1, 0] == 2 and slot[19, 63] == 3 and slot[20, 0] == 4
    slot, per = C.slot_map("ring", 20, 16)
    assert per == 2 and slot[9, 15] == 0 and slot[10, 0] == 1


# ---- the emulation under both instruments, at every GPU shape ---------------------------------------------------------------------------------------
def _layouts(s, folded):
    """The statistics layouts a GPU test compares for this shape."""
    if s.kind != "bf16" or s.cout % 64 or s.s2:
        return []
    if folded:
        return ["halo_fold"] * (s.w % 64 == 0) + ["halo4_fold"]
    return ["halo"] * (s.w % 32 == 0) + ["halo4"] * (s.w % 8 == 0) + ["ring"] * ((s.h * s.w) % 160 == 0)


@pytest.mark.parametrize("s,folded", C.all_cases(), ids=lambda v: _id(v))
def test_emulated_rounding_chain_meets_both_instruments(s, folded):
    d, r = C.case(s, "exact", folded)                                                         # (asserts sum|terms| < 256 and sum of squares < 2^24)
    out = C.emulate(s, d, act=False)
    C.check_exact(out, r["ref"], "emulation, 9 taps")
    if folded:
        C.check_exact(C.emulate(s, d, folded=True), r["ref"], "emulation, folded")
    for layout in _layouts(s, folded):
        C.check_stats_exact(C.emulate_stats(out, layout), r["ref"], layout, layout)
    d, r = C.case(s, "rounding", folded)                                                      # (asserts the ambiguity cap)
    out = C.emulate(s, d, folded=folded)
    if s.kind == "f32":
        used = C.assert_f32_close(out, r["ref"], r["mag"], "emulation")
    else:
        used = C.assert_bf16_close(out, r["ref"], r["mag"], "emulation", extra=r["extra"])
    assert used <= 1.0 and r["amb_share"] <= C.AMBIGUOUS_CAP
    for layout in _layouts(s, folded):
        assert C.check_stats_rounding(C.emulate_stats(out, layout), out, layout, layout) <= 1.0


# ---- wrong stand-ins: the rounding instrument -----------------------------------------------------------------------------------------------------------
GN_CASE = C.spec("bf16", 2, 20, 32, 320, 320, gn=1)                    # (n, Cin, Cout, H, W) = (2, 320, 320, 20, 32), GroupNorm + SiLU operand
SC_CASE = C.spec("bf16", 2, 13, 64, 128, 320, extras="b", cs1=64, cs2=128)
TWO_SOURCE_CASE = C.spec("bf16", 2, 20, 32, 320, 320, c2=128)


def rounding_faults():
    """name -> (spec, reference, wrong result): wrong results of the kind a max-norm gate of 6e-3 passes."""
    out = {}
    d, r = C.case(GN_CASE, "rounding")
    out["output truncated to bf16 instead of rounded"] = (GN_CASE, r, C.truncate_bf16(F.conv2d(
        C.operand(GN_CASE, d)[0].float().permute(0, 3, 1, 2), d["w"].float(), None, 1, 1).permute(0, 2, 3, 1)))
    off = dict(d)
    off["coef"] = d["coef"].clone()
    off["coef"][1, 64:96, 0] *= 1.01
    out["gn_coef scale 1 % off for 32 channels of one image"] = (GN_CASE, r, C.emulate(GN_CASE, off))
    d, r = C.case(SC_CASE, "rounding")
    conv = F.conv2d(d["x"].float().permute(0, 3, 1, 2), d["w"].float(), None, 1, 1).permute(0, 2, 3, 1) + (d["bias"].float() + d["bsc"].float())
    sc = torch.cat([d["xs"].float(), d["xs2"].float()], -1) @ d["wsc"].float().t()
    out["1x1 shortcut product rounded to bf16 before it is added"] = (SC_CASE, r, (conv + sc.bfloat16().float()).bfloat16())
    d, r = C.case(TWO_SOURCE_CASE, "rounding")
    c1 = TWO_SOURCE_CASE.cin - TWO_SOURCE_CASE.c2
    p1 = F.conv2d(d["x"].float().permute(0, 3, 1, 2), d["w"].float()[:, :c1], None, 1, 1)
    p2 = F.conv2d(d["x2"].float().permute(0, 3, 1, 2), d["w"].float()[:, c1:], None, 1, 1)
    out["first source's partial sum rounded to bf16 before the second is added"] = (TWO_SOURCE_CASE, r, (p1.bfloat16().float() + p2).permute(0, 2, 3, 1).bfloat16())
    return out


def test_correct_results_of_the_fault_cases_pass():
    for s in (GN_CASE, SC_CASE, TWO_SOURCE_CASE):
        d, r = C.case(s, "rounding")
        assert C.assert_bf16_close(C.emulate(s, d), r["ref"], r["mag"], _id(s), extra=r["extra"]) <= 1.0


@pytest.mark.parametrize("name", ["output truncated to bf16 instead of rounded", "gn_coef scale 1 % off for 32 channels of one image",
                                  "1x1 shortcut product rounded to bf16 before it is added",
                                  "first source's partial sum rounded to bf16 before the second is added"])
def test_rounding_instrument_catches_what_the_max_norm_gate_passes(name):
    s, r, wrong = rounding_faults()[name]
    old = C.rel_inf(wrong, r["ref"])
    bound = 2.0 ** -8 * r["ref"].abs() + 1e-5 * r["mag"] + (0 if r["extra"] is None else r["extra"])
    beyond = int(((wrong.double() - r["ref"]).abs() > bound).sum())
    print(f"{name}: rel-inf {old:.2e} (old gate {OLD_GATE}), {beyond} of {wrong.numel()} elements beyond the element bound")
    assert old < OLD_GATE                                                 # the max-norm gate passes it
    with pytest.raises(AssertionError, match="beyond the bf16 bound"):
        C.assert_bf16_close(wrong, r["ref"], r["mag"], name, extra=r["extra"])
    assert beyond > 1000


# ---- wrong stand-ins: the exact instrument ----------------------------------------------------------------------------------------------------------------
def test_exact_instrument_catches_a_seam_tap_that_reads_the_wrong_pixel_for_one_chunk():
    """Output column 31 (the last of the first 32-pixel tile): the tap kx = +1 reads column 33 instead of 32 for channels 64 .. 127."""
    s = C.HALO[2]                                                          # (3, 10, 64, 128, 320): two column strips
    d, r = C.case(s, "exact")
    x, w = d["x"].double(), d["w"].double()
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))                                       # [n, h + 2, w + 2, c]
    delta = torch.zeros_like(r["ref"])
    for ky in range(3):
        diff = xp[:, ky:ky + s.h, 33 + 1, 64:128] - xp[:, ky:ky + s.h, 32 + 1, 64:128]       # [n, h, 64]
        delta[:, :, 31] += diff @ w[:, 64:128, ky, 2].t()
    wrong = r["ref"] + delta
    assert int((wrong != r["ref"]).sum()) > 0 and bool(((wrong != r["ref"]).nonzero()[:, 2] == 31).all())
    with pytest.raises(AssertionError, match="differ from the exact result"):
        C.check_exact(wrong, r["ref"])
    assert C.rel_inf(wrong, r["ref"]) < 1.0


def test_exact_instrument_catches_gn_coef_of_the_next_image():
    s = C.HALO[6]
    d, r = C.case(s, "exact")
    wrong = C.reference(s, {**d, "coef": d["coef"].roll(-1, 0)}, act=False)["ref"]
    with pytest.raises(AssertionError, match="differ from the exact result"):
        C.check_exact(wrong, r["ref"])


def test_exact_instrument_catches_a_border_padded_with_the_shift():
    s = C.HALO[8]
    d, r = C.case(s, "exact")
    a, b = d["coef"].double()[:, None, None, :, 0], d["coef"].double()[:, None, None, :, 1]
    op = F.pad(d["x"].double(), (0, 0, 1, 1, 1, 1)) * a + b               # the affine map applied to the padding too
    wrong = F.conv2d(op.permute(0, 3, 1, 2), d["w"].double()).permute(0, 2, 3, 1)
    bad = (wrong != r["ref"])
    assert bool(bad.any()) and torch.equal(wrong[:, 1:-1, 1:-1], r["ref"][:, 1:-1, 1:-1])        # only the border differs
    with pytest.raises(AssertionError, match="differ from the exact result"):
        C.check_exact(wrong, r["ref"])


def test_exact_instrument_catches_the_temb_row_taken_modulo():
    s = C.RING_EPILOGUE[2]                                                  # six images, two temb rows: i / 3 against i % 2
    d, r = C.case(s, "exact")
    rows = d["temb"].shape[0]
    t = d["temb"].double()
    wrong = r["ref"] - t.repeat_interleave(s.tdiv, 0)[:, None, None, :] + t[torch.arange(s.n) % rows][:, None, None, :]
    with pytest.raises(AssertionError, match="differ from the exact result"):
        C.check_exact(wrong, r["ref"])


def _stats_case():
    s = C.HALO[9]                                                           # (2, 24, 32, 64, 320): three tiles per image, the last four rows high
    d, r = C.case(s, "exact")
    return s, r, C.tile_stats(r["ref"], "halo")[0]


def test_exact_instrument_catches_a_pixel_left_out_of_a_tiles_statistics():
    s, r, parts = _stats_case()
    C.check_stats_exact(parts.float(), r["ref"], "halo")
    o = r["ref"][1, 13, 7].reshape(32, s.cout // 32)                        # image 1, tile 1
    wrong = parts.clone()
    wrong[1, 1, :, 0] -= o.sum(-1)
    wrong[1, 1, :, 1] -= (o * o).sum(-1)
    with pytest.raises(AssertionError, match="gn_partials"):
        C.check_stats_exact(wrong.float(), r["ref"], "halo")


def test_exact_instrument_catches_two_tiles_partials_swapped():
    s, r, parts = _stats_case()
    wrong = parts.clone()
    wrong[0, 0], wrong[0, 1] = parts[0, 1], parts[0, 0]
    assert torch.equal(wrong.sum(1), parts.sum(1))                          # the sum over the tiles cannot see it
    with pytest.raises(AssertionError, match="gn_partials"):
        C.check_stats_exact(wrong.float(), r["ref"], "halo")


def test_exact_instrument_catches_a_masked_row_counted_into_the_statistics():
    s, r, parts = _stats_case()
    o = r["ref"][:, 23].reshape(s.n, 32, 32, s.cout // 32)                  # the row below the image read as a copy of the last one
    wrong = parts.clone()
    wrong[:, 2, :, 0] += o.sum((1, 3))
    wrong[:, 2, :, 1] += (o * o).sum((1, 3))
    with pytest.raises(AssertionError, match="gn_partials"):
        C.check_stats_exact(wrong.float(), r["ref"], "halo")


def test_rounding_instrument_catches_the_same_statistics_faults():
    """The same three faults on Gaussian data, against `STATS_REL * sum|addends|`."""
    s = C.HALO[9]
    d, r = C.case(s, "rounding")
    out = C.emulate(s, d)
    parts = C.emulate_stats(out, "halo")
    assert C.check_stats_rounding(parts, out, "halo") <= 1.0
    o = out[1, 13, 7].float().reshape(32, s.cout // 32)
    dropped = parts.clone()
    dropped[1, 1, :, 0] -= o.sum(-1)
    dropped[1, 1, :, 1] -= (o * o).sum(-1)
    swapped = parts.clone()
    swapped[0, 0], swapped[0, 1] = parts[0, 1], parts[0, 0]
    for wrong in (dropped, swapped):
        with pytest.raises(AssertionError, match="gn_partials"):
            C.check_stats_rounding(wrong, out, "halo")

"""CPU checks of tests/gemm_fwd_common.py, the instrument tests/test_gpu_gemm_forward_elementwise.py holds the forward token GEMMs against: the float64
references are F.linear with the epilogue written out; the exact inputs meet `assert_exact_conditions`; the fp32 emulation of the documented rounding
chains equals the exact expectation bit for bit and meets every rounding bound at every GPU shape (at the device's 256 compute units); every wrong
stand-in is rejected by at least one instrument in every case it applies to, and the faults the issue names pass the gate the suite had
(`rel_inf < 1e-2`) on data whose affected part is small; the table covers C-ABI tiles 1 - 22, every `split_k` form and every entry point; the dispatch
restatement agrees with the fall-backs include/fmc_hip.h documents."""
import re

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_fwd_common as G



def _run(c, instrument, fault=None, d=None):
    """The emulation of case `c` under one instrument -> (inputs, outputs); a rounding run of the per-image form goes through the emulated fold first."""
    d = G.inputs(c, instrument) if d is None else d
    if c.entry == "linear_bf16_imgw" and instrument == "rounding":
        w_out, bias_out = G.emulate_fold(d, c.shape[1], c.shape[2])
        G.check_fold(w_out, bias_out, d, c.shape[1], c.shape[2], c.name)
        d = G.with_fold(d, w_out, bias_out)
    return d, G.emulate(c, d, G.DEVICE_CUS, fault)


def _rejected(c, instrument, fault, d=None):
    d, got = _run(c, instrument, fault, d)
    try:
        G.check(c, d, got, instrument)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", G.NAMES)
def test_emulation_meets_both_instruments_and_stand_ins_do_not(name):
    c = G.case(name)
    instruments = ["exact"] if c.entry == "linear_fp8_qkv" else ["exact", "rounding"]
    for instrument in instruments:
        d, got = _run(c, instrument)
        shares = G.check(c, d, got, instrument)
        if instrument == "rounding":
            assert shares and max(shares.values()) <= 1.0
    for fault in G.FAULTS:
        if G.applies(fault, c):
            assert any(_rejected(c, i, fault) for i in instruments), f"{name}: neither instrument rejects `{fault}` ({G.FAULTS[fault]})"


@pytest.mark.parametrize("name", ["plain-t1-bar", "plain-t5-r2", "two-source-t3", "split-k4-t2", "geglu-t7", "geglu-t16", "linear4-extras3", "x3-f32-t1-split1",
                                  "lnc-plain", "fftail-plain"])
def test_reference_is_f_linear_with_the_epilogue_written_out(name):
    c = G.case(name)
    d = G.inputs(c, "rounding")
    r = G.reference(c, d)
    x = d["x"].double() if d["x2"] is None else torch.cat([d["x"].double(), d["x2"].double()], -1)
    if "lnc" in c.form:                                                          # LayerNorm folded: rstd (x W'^T - mean c) + ln_bias
        st = d["ln_stats"].double()
        y = st[:, 1:] * (F.linear(x, d["w"].double()) - st[:, :1] * d["ln_c"].double()) + d["ln_bias"].double()
    else:
        y = d["alpha"] * F.linear(x, d["w"].double(), None if d["b"] is None else d["b"].double())
    if c.geglu:
        v, g = y.chunk(2, -1)
        y = v * 0.5 * g * (1.0 + torch.erf(g / 2.0 ** 0.5))
    for t in (d["r"], d["r2"]):
        if t is not None:
            y = y + t.double()
    assert y.shape == r["ref"].shape
    assert float((y - r["ref"]).abs().max()) <= 1e-12 * float(r["mag"].max())
    assert bool((r["mag"] + 1e-12 >= r["ref"].abs()).all()) or c.geglu


def test_rows_columns_and_k_tiles_differ():
    """A swap must show: the exact reference changes under every index permutation the stand-ins apply (rows, 8-column groups, k-tiles, 32-deep sub-tiles)."""
    c = G.case("plain-t1-bar")
    d = G.inputs(c, "exact")
    ref = G.reference(c, d)["ref"]
    x, w = d["x"].double(), d["w"].double()
    assert not torch.equal(ref[:-1], ref[1:]) and not torch.equal(ref[:, :-8], ref[:, 8:])
    for width in (32, 64):
        xs = torch.cat([x[:, width:2 * width], x[:, :width], x[:, 2 * width:]], 1)
        assert int((xs @ w.t() != x @ w.t()).sum()) > ref.numel() // 2


NINE = ["truncate", "partial_bf16", "ragged_chunk", "bias_plus8", "pad_residual", "seam_off", "alpha_after_residual", "geglu_swap16", "pe_next_frame"]
FOUR = ["gn_slots_swapped", "tilemajor_subtiles", "segment_twice", "splitk_partial_bf16"]
GAP_CASES = {"truncate": "plain-t1-bar", "partial_bf16": "k-lockstep-s3-k1088", "ragged_chunk": "split-k4-t2", "bias_plus8": "plain-t3-bar",
             "pad_residual": "plain-t2-bar", "seam_off": "two-source-t1", "alpha_after_residual": "plain-t11-bar", "geglu_swap16": "geglu-t16",
             "pe_next_frame": "ln-ln_out-bar", "gn_slots_swapped": "gn-plain-grid-tm0", "tilemajor_subtiles": "plain-t18-bar", "segment_twice": "stream-k-t13",
             "splitk_partial_bf16": "split-k8-t9"}


@pytest.mark.parametrize("fault", NINE + FOUR)
def test_the_old_gate_passes_what_the_new_instruments_reject(fault):
    """The evidence that the gap was real: on the same shapes, with the operand part the fault touches small against the tensor maximum, the faulty
    output passes `rel_inf < 1e-2` (gn_partials: the per-image sum within 1e-4) and fails the element-wise bound."""
    c = G.case(GAP_CASES[fault])
    assert G.applies(fault, c)
    d = G.gap_inputs(c, fault)
    good = G.emulate(c, d, G.DEVICE_CUS)
    G.check(c, d, good, "rounding")                                            # the gap data itself is within the bounds
    bad = G.emulate(c, d, G.DEVICE_CUS, fault)
    old = G.old_gate(c, d, bad)
    print(f"stand-in {fault} on {c.name}: the old gate {'passes' if old else 'REJECTS'} it")
    assert _rejected(c, "rounding", fault, d) or _rejected(c, "exact", fault), fault
    assert old or fault in FOUR, f"{fault}: the old gate was expected to pass this fault on the gap data"


def test_table_covers_every_tile_split_form_and_entry_point():
    cs = G.CASES
    lin = [c for c in cs if c.entry == "linear_bf16"]
    assert {c.tile for c in lin} == set(range(1, 23))
    for t in range(1, 23):                                                       # plain epilogue: bias + alpha + one residual, and two residuals
        assert any(c.tile == t and c.extras == "bar" and not c.geglu for c in lin) and any(c.tile == t and c.extras == "r2" for c in lin), t
    assert {c.tile for c in lin if c.k_split} == {1, 3, 5, 11, 13}
    assert {(c.tile, c.split_k) for c in lin if c.split_k > 1} == {(t, s) for t in (1, 2, 9) for s in (2, 4, 8)} | {(16, 2), (18, 2)}
    assert {c.tile for c in lin if c.split_k == -1 and not c.geglu} == {1, 2, 3, 4, 5, 13, 14}
    assert {c.split_k for c in lin if c.split_k < 0} == {-1, -2, -3, -18, -19, -21}                    # every split_k form of the header
    assert {c.shape[2] for c in lin if c.split_k <= -16 and not c.geglu} == {320, 1088}
    assert {c.tile for c in lin if c.geglu} == set(range(1, 15)) | {16, 17, 18}
    assert any(c.geglu and c.split_k == -1 for c in lin) and any(c.geglu and c.split_k <= -16 for c in lin)
    assert {c.entry for c in cs} == {"linear_bf16", "linear_bf16_gn", "linear_bf16_ln", "linear_bf16_lnc", "linear_bf16_ffblk", "linear_bf16_ffblk_partial",
                                     "linear_bf16_fftail", "linear_bf16_fftail_partial", "linear_bf16_imgw", "linear4_bf16", "linear_x3_f32", "linear_fp8_qkv"}
    forms = {(c.entry, c.form.replace("w_tilemajor", "").strip()) for c in cs}
    for want in (("linear_bf16_ln", "ln_out"), ("linear_bf16_ln", "ln_stats"), ("linear_bf16_ffblk", "x_blocked"), ("linear_bf16_ffblk", "out_blocked"),
                 ("linear_bf16_ffblk", "out_blocked lnc"), ("linear_bf16_fftail", "gn_partials"), ("linear_bf16_fftail", ""), ("linear_bf16_imgw", "ln_stats"),
                 ("linear_bf16_imgw", ""), ("linear_bf16_gn", "gn_partials")):
        assert want in forms, want
    assert {len(c.extras) for c in cs if c.entry == "linear4_bf16"} == {0, 1, 3, 4}
    assert {(c.tile, c.split_k) for c in cs if c.entry == "linear_x3_f32"} == {(1, 1), (13, 1), (16, 1), (2, 2)}
    header = open(G.__file__.replace("tests/gemm_fwd_common.py", "include/fmc_hip.h")).read()
    for entry in {c.entry for c in cs}:
        assert re.search(rf"\bfmc_{entry}\(", header), entry
    assert "fmc_groupnorm_fold_linear(" in header


def test_every_purpose_reaches_its_arm_at_the_device_and_at_other_cu_counts():
    for cus in (G.DEVICE_CUS, 128, 64):
        for c in G.table(cus):
            if c.want is not None:
                assert G.expected_kernel(c, cus) == tuple(c.want), (cus, c.name, G.expected_kernel(c, cus))
            if c.split_k != 1 and c.entry == "linear_bf16":
                assert G.is_split_form(c, cus), (cus, c.name)


def test_expected_kernel_agrees_with_the_documented_fall_backs():
    E = G.expected_kernel
    mk = lambda tile, shape=(257, 328, 320), **kw: G._c("probe", "linear_bf16", tile, shape, **kw)
    assert E(mk(16, (161, 328, 320))) == E(mk(13, (161, 328, 320)))              # 16 -> 13 when N % 320
    assert E(mk(17, (161, 640, 320))) == E(mk(16, (161, 640, 320)))              # 17 -> 16 (plain epilogue)
    assert E(mk(17, (257, 640, 64), geglu=True)) == E(mk(16, (257, 640, 64), geglu=True))      # ... and GEGLU with M % 256
    assert E(mk(15, (320, 320, 320), extras="r2")) == E(mk(5, (320, 320, 320), extras="r2"))   # 15 -> 5: two residuals,
    assert E(mk(15, (257, 320, 320))) == E(mk(5, (257, 320, 320)))               # M % 64,
    assert E(mk(15, (320, 320, 384))) == E(mk(5, (320, 320, 384)))               # K != 320
    assert E(mk(15, (320, 320, 320)))[0].startswith("gemm_k320_kernel")
    assert E(mk(13, k_split=128)) == E(mk(3, k_split=128))                       # 13 -> 3 for a two-source operand
    for t in (19, 20, 21, 22):                                                   # 19 - 22 -> 1: split-K, stream-K, two residuals, fp32 storage
        assert E(mk(t, extras="r2")) == E(mk(1, extras="r2"))
        assert E(mk(t, (129, 200, 1344), split_k=2)) == E(mk(1, (129, 200, 1344), split_k=2))
        assert E(mk(t, (1025, 1032, 1664), split_k=-1)) == E(mk(1, (1025, 1032, 1664), split_k=-1))
        assert E(G._c("probe", "linear_x3_f32", t, (129, 72, 64))) == E(G._c("probe", "linear_x3_f32", 1, (129, 72, 64)))
        assert E(mk(t))[0] == G.ring_name(t)
    assert E(mk(18, (161, 640, 320))) == E(mk(16, (161, 640, 320)))              # 18 = 16 on a packed weight
    # "too small a problem silently runs the plain grid"
    assert E(mk(1, (257, 328, 320), split_k=-1))[1] == "plain grid"
    assert E(mk(13, (257, 264, 320), split_k=-1))[1] == "plain grid"
    assert E(mk(13, (257, 264, 320), split_k=-2))[1] == "plain grid"
    assert E(mk(13, (257, 264, 320), split_k=-3))[1] == "plain grid"            # five k-tiles: the cost model finds no S
    for t in (7, 8, 9, 10, 12):                                                  # rings deeper than two stages have no stream-K form (launch_gemm_g, :2507)
        assert E(mk(t, (1025, 1032, 4096), split_k=-1))[1] == "plain grid"
    for sk in (-2, -3, -18):                                                     # other arms treat the 8-phase forms as -1
        assert E(mk(1, (1025, 1032, 1664), split_k=sk)) == E(mk(1, (1025, 1032, 1664), split_k=-1))
    assert E(mk(16, (160 * 257, 320, 64)))[1] == "persistent" and E(mk(16, (160 * 256, 320, 64)))[1] == "plain grid"      # more tiles than CUs

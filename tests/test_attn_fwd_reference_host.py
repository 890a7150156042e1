"""CPU checks of tests/attn_fwd_common.py, the instruments test_gpu_attn_forward_elementwise.py holds the attention forward kernels to: the float64
references against `torch.softmax` / `torch.logsumexp`, the exactness conditions of every exact run, the dispatch restatement's coverage of every kernel
and tiled instantiation, the plain-torch emulation of every rounding chain against both bounds at every GPU case, and the twelve wrong stand-ins, each
of which the exact instrument must reject.  Prints, per stand-in, what the gate the kernels had before (`rel_inf < 1e-2`, LSE within 2e-2) makes of it
(profiles/attn_forward_bounds.md records the table)."""
import math

import pytest
import torch

from tests import attn_fwd_common as A

CASES = A.all_cases()


def test_case_ids_are_unique_and_every_case_names_a_kernel():
    ids = [A.case_id(c) for c in CASES]
    assert len(ids) == len(set(ids))
    assert all(c.kernel for c in CASES)


def test_case_table_reaches_every_kernel_and_tiled_instantiation():
    """The default dispatch's kernels: the five special ones and all 50 `spatial_attn_kernel` instantiations `launch_sa` can reach."""
    reached = {c.kernel for c in A.SPATIAL}
    want = A.default_tiled_instantiations()
    assert len(want) == 50
    assert not want - reached, sorted(want - reached)
    assert not A.SPECIAL_KERNELS - reached
    assert not {k for k in reached if k.startswith("spatial_attn_kernel")} - want, "the restatement names an instantiation launch_sa cannot reach"
    assert {A.xcd_remap(c.B, c.H) for c in A.TILED} == {0, 1, 2} and {A.xcd_remap(c.B, c.H) for c in A.SA40D} == {0, 1, 2}
    temporal = {c.kernel for c in A.TEMPORAL}
    for dtype in ("bf16", "fp32"):                      # both tile counts, whole and partial, every k-step count of D in {8, 40, 80, 160}, 4 / 2 / 1 waves
        for ft in (1, 2):
            for part in (0, 1):
                for nk32, nw in ((1, 4), (2, 4), (3, 2), (5, 1)):
                    assert f"temporal_attn_kernel<{dtype},{ft},{nk32},{nw},{part}>" in temporal
    assert {c.D for c in A.GENERIC} == {64, 128, 512} and any(c.causal for c in A.GENERIC) and any(c.keep for c in A.GENERIC)


def test_expected_kernel_at_the_shapes_the_model_runs():
    assert A.expected_kernel("bf16", 16, 8, 2560, 2560, 40, 1) == "sa40d_kernel"
    assert A.expected_kernel("bf16", 16, 8, 2560, 77, 40, 16) == "xattn40_kernel"
    assert A.expected_kernel("bf16", 16, 8, 640, 640, 80, 1) == "sa_big80_kernel_w10"
    assert A.expected_kernel("bf16", 16, 8, 160, 160, 160, 1) == "sa_small160_kernel<5>"
    assert A.expected_kernel("bf16", 16, 8, 40, 77, 160, 16) == "sa_small160_kernel<3>"
    assert A.expected_kernel("fp32", 16, 8, 2560, 2560, 40, 1) == A.tiled_name("fp32", 3, False, False, 1, False, False)
    assert A.expected_kernel("bf16", 2, 8, 640, 77, 80, 1) == A.tiled_name("bf16", 5, True, True, 1, False, False)


def test_exact_scales_are_powers_of_two_in_fp32():
    for k2 in range(4):
        assert A.scale_log2(A.exact_scale(k2)) == 2.0 ** -k2


@pytest.mark.parametrize("c", CASES, ids=A.case_id)
def test_reference_is_float64_softmax_and_exact_conditions_hold(c):
    A.assert_exact_conditions(c)
    for instrument in ("exact", "rounded"):
        d, r = A.inputs(c, instrument), A.reference(c, instrument)
        k, v = d["k"].repeat_interleave(c.kvdiv, 0), d["v"].repeat_interleave(c.kvdiv, 0)
        s = torch.einsum("ghid,ghjd->ghij", d["q"], k) * (A.scale_log2(d["scale"]) * A.LN2)
        if c.causal:
            s = s.masked_fill(torch.arange(c.Skv)[None, :] > torch.arange(c.Sq)[:, None], -math.inf)
        if c.keep:
            s = s.masked_fill(~d["keep"][:, None, None, :], -math.inf)
        out = torch.softmax(s, -1) @ v
        assert torch.allclose(r["out"], out, rtol=1e-12, atol=1e-13)
        assert torch.allclose(r["lse"], torch.logsumexp(s, -1), rtol=1e-12, atol=1e-12)
        assert abs(A.scale_log2(d["scale"]) * A.LN2 / d["scale"] - 1) < 2.0 ** -23      # the ABI's fp32 scale_log2 against scale * log2(e)
        assert bool((r["exact_out" if instrument == "exact" else "rounded_out"] >= 0).all())
    A.reference.cache_clear()
    A.inputs.cache_clear()


@pytest.mark.parametrize("instrument", ["exact", "rounded"])
@pytest.mark.parametrize("c", CASES, ids=A.case_id)
def test_emulated_rounding_chain_meets_the_bound(c, instrument):
    out, lse = A.emulate(c, instrument)
    r = A.reference(c, instrument)
    key = "exact" if instrument == "exact" else "rounded"
    share = float(((out - r["out"]).abs() / r[key + "_out"].clamp_min(1e-300)).max())
    share_lse = float(((lse - r["lse"]).abs() / r[key + "_lse"].clamp_min(1e-300)).max()) if lse is not None else 0.0
    print(f"   {A.case_id(c)} {instrument}: emulation err / bound {share:.3f}, LSE {share_lse:.3f}")
    A.reference.cache_clear()
    A.inputs.cache_clear()
    assert share <= 1.0 and share_lse <= 1.0, (share, share_lse)


@pytest.mark.parametrize("fault", A.FAULTS)
def test_wrong_stand_in_fails_the_exact_instrument(fault):
    """Each stand-in is the emulated chain with one mistake; the exact instrument must find elements beyond its bound.  Printed next to it: what the
    former gate makes of the same stand-in on the Gaussian data it ran on."""
    c = A.fault_case(fault)
    good, good_lse = A.emulate(c, "exact")
    assert A.violations(c, "exact", good, good_lse) == (0.0, 0.0), "the right chain must pass where the wrong one is tried"
    out, lse = A.emulate(c, "exact", fault)
    bad_out, bad_lse = A.violations(c, "exact", out, lse)
    g_out, g_lse = A.emulate(c, "rounded", fault)
    r = A.reference(c, "rounded")
    ri = A.rel_inf(g_out, r["out"])
    dl = float((g_lse - r["lse"]).abs().max()) if g_lse is not None else 0.0
    old = "passes" if ri < 1e-2 and dl < 2e-2 else "fails"
    print(f"   {fault} at {A.case_id(c)}: {100 * bad_out:.1f} % of the outputs, {100 * bad_lse:.1f} % of the LSE beyond the exact bound; "
          f"former gate: rel_inf {ri:.2e}, LSE {dl:.2e} -> {old}")
    assert bad_out > 0 or bad_lse > 0


def test_one_perturbed_key_index_fails_the_exact_instrument():
    """The sanity check of the instrument itself: the kernel-like result against a reference in which ONE key of one (batch, head) took its
    neighbour's place."""
    c = A.fault_case("drop_last_key")
    out, lse = A.emulate(c, "exact")
    d = A.inputs(c, "exact")
    k = d["k"].clone()
    k[0, 1, 100] = d["k"][0, 1, 101]
    s2 = torch.einsum("ghid,ghjd->ghij", d["q"], k) * A.scale_log2(d["scale"])
    ref = torch.softmax(s2 * A.LN2, -1) @ d["v"]
    bound = A.reference(c, "exact")["exact_out"]
    assert bool(((out - ref).abs() > bound)[0, 1].any()) and not bool(((out - ref).abs() > bound)[0, 0].any())

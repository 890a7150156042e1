"""The instrument of tests/test_gpu_fused_block_exact.py, examined without a GPU (tests/fused_block_common.py):

  1. `assert_exact_conditions` holds for every case of the table.  The persistent-loop cases are examined on `PERIOD` pixels: their generator
     repeats after PERIOD pixels and the blocks are local to a pixel, so the PERIOD pixels are every distinct row such a case holds;
  2. the fp32 emulation of the documented chain equals the float64 expectation bit for bit in every case;
  3. every wrong stand-in differs from the expectation in at least one element of every case it applies to (`applies`), so the zero-tolerance
     comparison of the GPU file fails on each of them.  The statistics stand-in is examined on the Gaussian rows the statistics bound is for."""
import pytest
import torch

from tests import fused_block_common as FB

CASES = [FB.host_case(c) for c in FB.all_cases()]
IDS = [FB.case_id(c) for c in FB.all_cases()]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_exact_conditions_hold(c):
    FB.assert_exact_conditions(c)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_fp32_emulation_equals_the_float64_expectation(c):
    ref = FB.expectation(c)[0]
    emu = FB.chain(c, FB.Emulated)
    assert emu.dtype == torch.float32
    FB.check_exact(emu, ref, FB.case_id(c))


@pytest.mark.parametrize("fault", [f for f in FB.FAULTS if f != "stats_unrounded"])
def test_every_stand_in_is_caught_in_every_case_it_applies_to(fault):
    n, missed = 0, []
    for c in CASES:
        if not FB.applies(fault, c):
            continue
        n += 1
        ref = FB.expectation(c)[0]
        wrong = FB.chain(c, FB.Exact, fault)
        try:
            FB.check_exact(wrong, ref, FB.case_id(c))
            missed.append(FB.case_id(c))
        except AssertionError:
            pass
    assert not missed, f"{fault} ({FB.FAULTS[fault]}) passes the exact comparison in {missed}"
    assert n >= 4, f"{fault}: applies to {n} cases only"


def test_every_family_meets_its_stand_ins():
    """No stand-in of a family is switched off for the whole family by `applies`."""
    per_family = {FB.TemporalCase: {"pe_next_frame", "next_head_k", "drop_tail", "no_merge_scale", "pose_next_pixel", "no_bias", "no_residual", "v_next_pixel",
                                    "ln_no_mean"},
                  FB.TextCase: {"next_head_k", "drop_tail", "unmask_pad", "mask_last_key", "no_bias", "no_residual", "next_batch_text"},
                  FB.GegluCase: {"no_bias", "swap_value_gate", "ln_no_mean"}}
    for family, faults in per_family.items():
        for fault in faults:
            assert any(FB.applies(fault, c) for c in CASES if isinstance(c, family)), (family.__name__, fault)


def test_ties_and_masked_rows_are_in_the_table():
    for family, C in ((FB.TemporalCase, 320), (FB.TemporalCase, 640), (FB.TextCase, 320), (FB.TextCase, 640)):
        ties = {c.ties for c in CASES if isinstance(c, family) and c.C == C}
        assert {1, 2, 4} <= ties, (family.__name__, C, ties)
    assert {c.S for c in CASES if isinstance(c, FB.TextCase)} >= {77, 80, 5, 1}


def test_statistics_of_the_unrounded_output_leave_the_bound():
    """The row statistics belong to the ROUNDED output.  Statistics taken before the bf16 rounding, though computed without any error of their own,
    leave the counted bounds on Gaussian rows (the exact cases cannot show this: their outputs are representable); correct ones, evaluated in
    float32 the way the kernel does, stay inside."""
    g = torch.Generator().manual_seed(5)
    out_f = (torch.randn(640, 320, generator=g) * 1.5 + 0.2)
    out = out_f.bfloat16()
    mean, rstd, _ = FB.row_stats(out_f)
    bad_mean, bad_rstd = FB.stats_violations(torch.stack([mean, rstd], -1), out)
    assert bool(bad_mean.any()) and bool(bad_rstd.any())
    o = out.float()
    inv_c = torch.tensor(1.0) / torch.tensor(320.0)
    m32 = o.sum(-1) * inv_c
    r32 = torch.rsqrt(((o - m32[:, None]) ** 2).sum(-1) * inv_c + torch.tensor(1e-5))
    FB.check_stats(torch.stack([m32, r32], -1), out, "fp32 statistics of the rounded output")
    # a mean that is wrong by 1e-4 of the row's magnitude hides under a max-norm gate wherever the mean is small; not under this one
    off = m32 + 1e-4 * o.abs().mean(-1)
    assert bool(FB.stats_violations(torch.stack([off, r32], -1), out)[0].all())


def test_gelu_fast_is_exact_on_the_gates_the_cases_use():
    ints = torch.arange(10, 17, dtype=torch.float32)
    assert torch.equal(FB.gelu_fast_f32(ints), ints)
    assert float(FB.gelu_fast_f32(torch.zeros(1))) == 0.0
    neg = FB.gelu_fast_f32(-ints)
    assert bool((neg != 0).any()) and float(neg.abs().max()) < 1e-9      # negative gates are NOT exact: the cases use none

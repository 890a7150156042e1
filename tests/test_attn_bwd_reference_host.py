"""The reference and the bound of the spatial-attention backward tests, checked on the CPU (tests/attn_bwd_common.py): the
closed form is autograd's gradient, a correct bf16 implementation meets the bound on exactly the inputs of the GPU tests, and
three wrong ones do not."""
import functools

import pytest
import torch

from tests import attn_bwd_common as AB
from tests.test_gpu_kernels import oracle_attention          # the oracle's un-fused chain (diffusers Attention helpers)

BF = torch.bfloat16


@functools.lru_cache(maxsize=None)
def _case(name):
    B, Bkv, H, Sq, Skv, D = AB.CASES[name]
    q, k, v, g = AB.make_inputs(name, BF)
    return (q, k, v, g, H, D ** -0.5), AB.reference_backward(q, k, v, g, H, D ** -0.5)


@pytest.mark.parametrize("name", sorted(AB.CASES))
def test_closed_form_is_the_autograd_gradient(name):
    (q, k, v, g, H, scale), ref = _case(name)
    B, Bkv = q.shape[0], k.shape[0]
    qd, kd, vd = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    rep = B // Bkv
    out = oracle_attention(qd, kd.repeat_interleave(rep, dim=0), vd.repeat_interleave(rep, dim=0), H)
    out.backward(g.double())
    for key, t in (("dq", qd), ("dk", kd), ("dv", vd)):
        err = float((t.grad - ref[key]).abs().max() / ref["mag_" + key].max())
        assert err < 1e-12, (key, err)
        assert bool((ref["mag_" + key] >= ref[key].abs() * (1 - 1e-12)).all())          # |sum| <= sum |terms|
    if AB.CASES[name][4] == 1:                                                            # one key: P = 1, dS = 0
        assert float(ref["dq"].abs().max()) < 1e-14 and float(ref["dk"].abs().max()) < 1e-14 and float(ref["mag_dq"].min()) > 0


@pytest.mark.parametrize("name", sorted(AB.CASES))
def test_bf16_rounding_chain_meets_the_bound(name):
    (q, k, v, g, H, scale), ref = _case(name)
    got = AB.emulate_bf16_backward(q, k, v, g, H, scale, per_frame_partials=(k.shape[0] == 1 and q.shape[0] > 1))
    worst = {key: AB.assert_grad_close(got[key], ref[key], ref["mag_" + key], AB.C_BF16, f"{name} {key}") for key in ("dq", "dk", "dv")}
    print(f"{name}: emulation, worst err / |terms| in units of 2^-7: " + " ".join(f"{k_} {r:.3f}" for k_, r in worst.items()))


@pytest.mark.parametrize("name", ["self_b8_s129_d40", "cross_c8_f2"])
def test_bf16_rounding_chain_meets_the_bound_with_a_sharp_softmax(name):
    """Logits three times as large (a few keys take most of the weight): the bound is relative to the terms, so it still holds."""
    B, Bkv, H, Sq, Skv, D = AB.CASES[name]
    q, k, v, g = AB.make_inputs(name, BF, logit_scale=3.0)
    ref = AB.reference_backward(q, k, v, g, H, D ** -0.5)
    got = AB.emulate_bf16_backward(q, k, v, g, H, D ** -0.5)
    worst = {key: AB.assert_grad_close(got[key], ref[key], ref["mag_" + key], AB.C_BF16, f"{name} {key}") for key in ("dq", "dk", "dv")}
    print(f"{name}, logits x 3: emulation, worst err / |terms| in units of 2^-7: " + " ".join(f"{k_} {r:.3f}" for k_, r in worst.items()))


FAULT_CASES = ["self_b8_s129_d40", "self_b8_s65_d160", "cross_c8_f2"]


def _emulated(name):
    (q, k, v, g, H, scale), ref = _case(name)
    return AB.emulate_bf16_backward(q, k, v, g, H, scale)


@pytest.mark.parametrize("name", FAULT_CASES)
def test_fault_last_partial_query_tile_dropped_from_dk_dv(name):
    """dK / dV without the queries of the last partial 64-row tile: a zero dO row contributes nothing to either."""
    (q, k, v, g, H, scale), ref = _case(name)
    Sq = q.shape[1]
    assert Sq % 64
    g_cut = g.clone()
    g_cut[:, Sq // 64 * 64:] = 0
    bad = AB.emulate_bf16_backward(q, k, v, g_cut, H, scale)
    for key in ("dk", "dv"):
        with pytest.raises(AssertionError, match="beyond"):
            AB.assert_grad_close(bad[key], ref[key], ref["mag_" + key], AB.C_BF16, key)


@pytest.mark.parametrize("name", FAULT_CASES)
def test_fault_last_key_dropped_from_dq(name):
    (q, k, v, g, H, scale), ref = _case(name)
    t = AB.terms(q, k, v, g, H, scale)
    last = AB._merge(scale * t["dS"][..., -1:] @ t["k"][..., -1:, :])
    bad = (_emulated(name)["dq"] - last).to(BF)
    with pytest.raises(AssertionError, match="beyond"):
        AB.assert_grad_close(bad, ref["dq"], ref["mag_dq"], AB.C_BF16, "dq")


@pytest.mark.parametrize("name", FAULT_CASES)
def test_fault_two_batch_entries_swapped(name):
    """What an off-by-one in the block -> (batch, head) map does: every value right, two batch entries in each other's place."""
    (q, k, v, g, H, scale), ref = _case(name)
    got = _emulated(name)
    for key in ("dq", "dk", "dv"):
        bad = got[key].clone()
        bad[[0, 1]] = bad[[1, 0]]
        with pytest.raises(AssertionError, match="beyond") as info:
            AB.assert_grad_close(bad, ref[key], ref["mag_" + key], AB.C_BF16, key)
        assert "worst at (" in str(info.value)


def test_bound_holds_where_the_reference_is_zero():
    ref, mag = torch.zeros(2, 3), torch.full((2, 3), 4.0)
    assert AB.assert_grad_close(torch.full((2, 3), 4.0 * 2.0 ** -8), ref, mag, AB.C_BF16) == pytest.approx(0.5)
    with pytest.raises(AssertionError, match="1 / 6 elements"):
        got = torch.zeros(2, 3)
        got[1, 2] = 4.0 * 2.0 ** -6
        AB.assert_grad_close(got, ref, mag, AB.C_BF16, "zero reference")
    with pytest.raises(AssertionError):
        AB.assert_grad_close(torch.full((2, 3), float("nan")), ref, mag, AB.C_BF16)

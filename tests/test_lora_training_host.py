"""Domain-LoRA training (FMC stage 1) host logic on the CPU: the processor's un-merged LoRA path, the stage-1 step and the checkpoint
format against the oracle, with the kernels replaced by their contracts (`tests/fake_kernels.py` + the weight-gradient stand-in below)."""
import pytest
import torch

from synfmc_amd.configs import processor_kwargs, unet_kwargs
from tests import fake_kernels
from tests import lora_common as LC


def linear_wgrad_group(problems):
    """Contract of `fmc_linear_wgrad_bf16`: out[N, K] = alpha * a^T b (+ out), fp32, summed in fp64."""
    outs = []
    for a, b, alpha, out, acc in problems:
        g = (alpha * (a.reshape(-1, a.shape[-1]).double().t() @ b.reshape(-1, b.shape[-1]).double())).float()
        if out is None:
            out = g
        elif acc:
            out.add_(g)
        else:
            out.copy_(g)
        outs.append(out)
    return outs


@pytest.fixture
def fake(monkeypatch):
    import synfmc_amd.hip_ops as K
    fake_kernels.install(monkeypatch)
    calls = []

    def counted(problems):
        calls.append(len(problems))
        return linear_wgrad_group(problems)
    monkeypatch.setattr(K, "linear_wgrad_group", counted)
    return calls


@pytest.mark.parametrize("cross", [False, True], ids=["attn1_self", "attn2_text"])
def test_lora_processor_gradients_match_oracle(fake, cross):
    C, heads, D = 64, 4, 48
    oa, pa = LC.attention_pair(C, heads, cross_dim=D if cross else None, seed=3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 24, C, generator=g)
    text = torch.randn(2, 7, D, generator=g) if cross else None
    w = torch.randn(2, 24, C, generator=g)
    xo, xp = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ref = oa(xo, encoder_hidden_states=text)
    (ref * w).sum().backward()
    got = pa(xp, encoder_hidden_states=text)
    (got * w).sum().backward()
    assert LC.rel_inf(got, ref) < 1e-5
    assert LC.rel_inf(xp.grad, xo.grad) < 1e-5
    g_ref, g_got = LC.lora_grads(oa.processor), LC.lora_grads(pa.processor)
    assert len(g_ref) == 8 and set(g_got) == set(g_ref)
    for n in g_ref:
        assert g_ref[n].abs().max() > 0, n
        assert LC.rel_inf(g_got[n], g_ref[n]) < 1e-5, n
    # the factor gradients of one projection group are one launch: q|k|v + out (self) / q + k|v + out (text)
    assert sorted(fake) == sorted([4, 2] if not cross else [2, 3, 2])


def test_lora_processor_frozen_path_unchanged(fake):
    """Without gradients (or with a frozen LoRA) the processor keeps the merged-weight path: no weight-gradient call, same output."""
    oa, pa = LC.attention_pair(64, 4, seed=5)
    x = torch.randn(2, 24, 64, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        ref = oa(x)
        got = pa(x)
    assert LC.rel_inf(got, ref) < 1e-5 and fake == []
    assert "_fused" in pa.__dict__ and "_train_cache" not in pa.processor.__dict__


def test_stage1_training_step_matches_oracle(fake):
    ou, pu = LC.build_stage1(seed=7)
    batch = LC.stage1_batch(B=2, h=16, w=16)
    l_ref, g_ref, p_ref = LC.oracle_stage1_steps(ou, batch, steps=2)
    l_got, g_got, p_got = LC.product_stage1_steps(pu, batch, steps=2)
    assert len(g_ref) == 32 * 8 and set(g_got) == set(g_ref) and set(p_got) == set(p_ref)
    for a, b in zip(l_got, l_ref):
        assert abs(a - b) < 1e-5 * abs(b)
    err_g = LC.rel_inf_dict(g_got, g_ref)
    err_p = LC.rel_inf_dict(p_got, p_ref)
    print(f"stage-1 fp32 host: loss {l_got} vs {l_ref}, gradient rel-inf {err_g:.2e}, parameters after 2 AdamW steps {err_p:.2e}")
    assert err_g < 1e-5 and err_p < 1e-5
    assert all(p.dtype == torch.float32 for n, p in pu.named_parameters() if "_lora." in n)


def test_lora_state_dict_reference_format_round_trip():
    from synfmc_amd.training import lora_state_dict, lora_trainable_parameters
    ou, pu = LC.build_stage1(seed=9)
    params = lora_trainable_parameters(pu)
    assert len(params) == 32 * 8 and all(p.requires_grad and p.dtype == torch.float32 for p in params)
    assert all(not p.requires_grad for n, p in pu.named_parameters() if "_lora." not in n)
    sd = lora_state_dict(pu)
    ref_keys = {k for k in ou.state_dict() if "_lora." in k}
    assert set(sd) == ref_keys and len(sd) == 256
    assert "down_blocks.0.attentions.0.transformer_blocks.0.attn1.processor.to_q_lora.down.weight" in sd
    with torch.no_grad():
        for p in params:
            p.add_(0.125)
    sd = lora_state_dict(pu)
    # into the CMC + OMC product U-Net of stages 2 / 3 (train_cam_obj_ctrl.py:253-261)
    from synfmc_amd.models.unet import UNet3DConditionModelCamObjCond
    from synfmc_amd.modified_modules import patch_unet_for_omc
    pc = UNet3DConditionModelCamObjCond(**unet_kwargs(LC.W4, 64))
    pc.set_all_attn_processor(**processor_kwargs(LC.W4, True))
    patch_unet_for_omc(pc)
    missing, unexpected = pc.load_state_dict(sd, strict=False)
    assert unexpected == [] and not (set(sd) & set(missing))
    got = pc.state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k].float(), v), k


def test_motion_lora_training_still_refused():
    from synfmc_amd.models.attention_processor import LORAPoseAdaptorAttnProcessor
    from synfmc_amd.models.layers import Attention
    attn = Attention(64, heads=4, dim_head=16).requires_grad_(False)
    proc = LORAPoseAdaptorAttnProcessor(64, 64, query_condition=True, key_value_condition=True, rank=16)
    attn.set_processor(proc)
    proc.to_q_lora.up.weight.requires_grad_(True)
    x = torch.randn(1, 4, 16, 64)
    with pytest.raises(NotImplementedError, match="requires_grad_"):
        attn(x, pose_feature=torch.randn(1, 4, 16, 64), temporal=True)

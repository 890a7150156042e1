"""CPU side of the Camera-Encoder / merge / OMC-Adapter training route: the float64 closed forms against float64 autograd, every wrong
stand-in caught by the assertion written for it, and the plumbing of `camera_trainable_parameters` / `omc_trainable_parameters` on a toy."""
import pytest
import torch

from tests import camera_train_common as CC


def test_closed_forms_equal_fp64_autograd():
    CC.check_merge(CC.merge_forward, CC.merge_backward)
    CC.check_avgpool_forward(CC.avgpool_forward)
    CC.check_avgpool_backward(CC.avgpool_backward)
    CC.check_relu_backward(CC.relu_backward)
    CC.check_qkv_split(CC.split_qkv_grad)


@pytest.mark.parametrize("check,args,match", [
    (CC.check_avgpool_forward, (CC.wrong_avgpool_forward_odd_row,), "avgpool forward"),
    (CC.check_avgpool_backward, (CC.wrong_avgpool_backward_floor_unwritten,), "never written"),
    (CC.check_relu_backward, (CC.wrong_relu_backward_ge,), "relu backward"),
    (CC.check_qkv_split, (CC.wrong_split_swapped,), "split to_q"),
    (CC.check_merge, (CC.merge_forward, CC.wrong_merge_db_without_alpha), "merge db"),
    (CC.check_merge, (CC.merge_forward, CC.wrong_merge_residual_dropped), "merge dh"),
    (CC.check_merge, (CC.merge_forward, CC.wrong_merge_pose_gets_dm), "merge dpose"),
], ids=["pool_odd_row", "pool_bwd_floor_unwritten", "relu_ge", "qkv_swapped", "db_no_alpha", "residual_dropped", "pose_gets_dm"])
def test_wrong_stand_ins_are_caught(check, args, match):
    with pytest.raises(AssertionError, match=match):
        check(*args)


def test_camera_trainable_parameters_plumbing():
    """Same tensors, same order as `stage2_trainable_parameters`; fp32, requiring grad; the encoder and the merge owners marked, nothing
    else; the checkpoint has the reference's keys and split and loads into a bf16 model with no unexpected keys."""
    from synfmc_amd.models.layers import OWN_MARK
    from synfmc_amd.training import camera_state_dict, camera_trainable_parameters, stage2_trainable_parameters
    pu, pe = CC.toy_stage2()
    want = stage2_trainable_parameters(pu, pe)
    assert all(p.dtype == torch.bfloat16 and not p.requires_grad for p in want)
    got = camera_trainable_parameters(pu, pe)
    assert len(got) == len(want) > 0 and all(a is b for a, b in zip(got, want))
    assert all(p.dtype == torch.float32 and p.requires_grad for p in got)
    merges = [n for n, _ in pu.named_parameters() if "_merge." in n]
    assert merges and len(got) == len(list(pe.parameters())) + len(merges)
    assert all(m.__dict__.get(OWN_MARK) for m in pe.modules())
    marked = {n for n, m in pu.named_modules() if m.__dict__.get(OWN_MARK)}
    owners = {n.rsplit(".", 2)[0] for n in merges}                                  # `<processor>.qkv_merge.weight` -> `<processor>`
    assert marked == owners | {o + ".qkv_merge" for o in owners}
    others = [p for n, p in pu.named_parameters() if "_merge." not in n]
    assert all(p.dtype == torch.bfloat16 and not p.requires_grad for p in others)    # nothing else changes
    sd = camera_state_dict(pu, pe)
    assert set(sd) == {"pose_encoder_state_dict", "attention_processor_state_dict"}
    assert set(sd["pose_encoder_state_dict"]) == set(pe.state_dict())
    assert set(sd["attention_processor_state_dict"]) == set(merges)
    pu2, pe2 = CC.toy_stage2()
    missing, unexpected = pe2.load_state_dict(sd["pose_encoder_state_dict"], strict=False)
    assert missing == [] and unexpected == []
    missing, unexpected = pu2.load_state_dict(sd["attention_processor_state_dict"], strict=False)
    assert unexpected == [] and all(p.dtype == torch.bfloat16 for p in pu2.parameters())


def test_omc_trainable_parameters_plumbing():
    from synfmc_amd.models.layers import OWN_MARK
    from synfmc_amd.training import omc_state_dict, omc_trainable_parameters
    pa = CC.toy_adapter()
    want = list(pa.parameters())
    got = omc_trainable_parameters(pa)
    assert len(got) == len(want) and all(a is b for a, b in zip(got, want))
    assert all(p.dtype == torch.float32 and p.requires_grad for p in got)
    assert all(m.__dict__.get(OWN_MARK) for m in pa.modules())
    sd = omc_state_dict(pa)
    assert set(sd) == {"omcm_state_dict"} and set(sd["omcm_state_dict"]) == set(pa.state_dict())
    missing, unexpected = CC.toy_adapter().load_state_dict(sd["omcm_state_dict"], strict=True)
    assert missing == [] and unexpected == []


def test_cpu_and_fp32_inputs_keep_the_torch_route():
    """The mark alone changes nothing for inputs outside the new route's domain: a marked fp32 layer on CPU tensors computes what the
    unmarked layer computes (the new route is bf16 device activations only)."""
    from synfmc_amd.models.layers import Conv2d, Linear
    from synfmc_amd.training import mark_trainable_own
    torch.manual_seed(0)
    lin, conv = Linear(8, 8), Conv2d(8, 8, 3, 1, 1)
    x, x4 = torch.randn(3, 8), torch.randn(1, 8, 4, 4)
    want = lin(x), conv(x4)
    mark_trainable_own(lin)
    mark_trainable_own(conv)
    assert torch.equal(lin(x), want[0]) and torch.equal(conv(x4), want[1])


def test_partial_merges_are_refused():
    """`q_merge` / `kv_merge` processors (configurations that do not ship) have no own route: refused, nothing converted or marked."""
    from synfmc_amd.models.layers import OWN_MARK
    from synfmc_amd.training import camera_trainable_parameters
    pu, pe = CC.toy_stage2()
    proc = next(m for m in pu.modules() if hasattr(m, "qkv_merge"))
    proc.q_merge = torch.nn.Linear(4, 4)
    with pytest.raises(NotImplementedError, match="q_merge"):
        camera_trainable_parameters(pu, pe)
    assert all(p.dtype == torch.bfloat16 and not p.requires_grad for p in pe.parameters())
    assert not any(m.__dict__.get(OWN_MARK) for m in list(pu.modules()) + list(pe.modules()))


def test_shadow_twin_carries_configuration_and_follows_the_module():
    """The no-grad twin carries public attributes and plain private configuration, neither the mark nor a cache; it is reused while
    the module is unchanged and rebuilt when an attribute, the `training` flag or a replaced buffer / parameter moves."""
    from synfmc_amd.models.layers import OWN_MARK, Attention, Conv2d, shadow_twin
    from synfmc_amd.models.attention_processor import AttnProcessor
    from synfmc_amd.training import mark_trainable_own
    conv = Conv2d(8, 8, 3, 1, 1)
    mark_trainable_own(conv)
    conv.__dict__["_some_cache"] = (1, torch.zeros(1))
    twin = shadow_twin(conv)
    assert twin._reversed_padding_repeated_twice == conv._reversed_padding_repeated_twice and twin.stride == (1, 1)
    assert OWN_MARK not in twin.__dict__ and "_some_cache" not in twin.__dict__
    assert twin.weight.dtype == torch.bfloat16 and torch.equal(twin.weight.float(), conv.weight.detach().to(torch.bfloat16).float())
    assert shadow_twin(conv) is twin
    conv.train(not conv.training)
    again = shadow_twin(conv)
    assert again is not twin and again.training == conv.training
    conv.double()                                                   # parameters replaced: no fp32 master left, the twin holds them as they are
    assert shadow_twin(conv) is not again and shadow_twin(conv).weight is conv.weight
    attn = Attention(query_dim=8, heads=2, dim_head=4)
    mark_trainable_own(attn)
    t1 = shadow_twin(attn)
    assert t1.processor is attn.processor and t1.scale == attn.scale
    attn.set_processor(AttnProcessor())
    attn.scale = 0.5
    t2 = shadow_twin(attn)
    assert t2 is not t1 and t2.processor is attn.processor and t2.scale == 0.5
    with torch.no_grad():
        attn.to_q.weight.add_(1.0)                                  # a master's version moves: the same twin, the shadow refreshed in place
    t3 = shadow_twin(attn)
    assert t3 is t2 and torch.equal(t3.to_q.weight.float(), attn.to_q.weight.detach().to(torch.bfloat16).float())

"""`train_mm` host logic on the CPU: which parameters train, the checkpoint format and the clip groups of stages 2 and 3 against the
reference's rules, and the motion module's training path against the oracle with the kernels replaced by their contracts
(`tests/fake_kernels.py` + the `linear_trainable` stand-in below)."""
import pytest
import torch
import torch.nn.functional as F

from synfmc_amd.configs import processor_kwargs, unet_kwargs
from tests import fake_kernels
from tests import mm_common as MC

W4 = (64, 128, 256, 256)


def linear_trainable(x, weight, bias=None, residual=None, w_run=None, b_run=None):
    """Contract of `hip_ops.linear_trainable`: `x W^T + b + residual`, differentiable in all four (the shadows are what the kernels read)."""
    y = F.linear(x, weight.to(x.dtype), None if bias is None else bias.to(x.dtype))
    return y if residual is None else y + residual


@pytest.fixture
def fake(monkeypatch):
    import synfmc_amd.hip_ops as K
    fake_kernels.install(monkeypatch)
    calls = []

    def counted(*a, **k):
        calls.append(a[1].shape)
        return linear_trainable(*a, **k)
    monkeypatch.setattr(K, "linear_trainable", counted)
    return calls


def _product_unet():
    from synfmc_amd.models.unet import UNet3DConditionModelCamObjCond
    from synfmc_amd.modified_modules import patch_unet_for_omc
    pu = UNet3DConditionModelCamObjCond(**unet_kwargs(W4, 64))
    pu.set_all_attn_processor(**processor_kwargs(W4, True))
    patch_unet_for_omc(pu)
    return pu.requires_grad_(False)


def _oracle_unet():
    from oracle import fmc_modules as OM
    ou = OM.UNet3DConditionModelCamObjCond(**unet_kwargs(W4, 64))
    ou.set_all_attn_processor(**processor_kwargs(W4, True))
    OM.patch_down_blocks_for_omc(ou)
    return ou


def test_mm_parameter_selection_is_the_reference_rule():
    from synfmc_amd.training import motion_module_trainable_parameters
    pu, ou = _product_unet(), _oracle_unet()
    ref = MC.reference_mm_names(ou)
    assert ref == MC.reference_mm_names(pu)
    names = {id(p): n for n, p in pu.named_parameters()}
    params = motion_module_trainable_parameters(pu)
    got = [names[id(p)] for p in params]
    n_modules = sum(1 for m in pu.modules() if m.__class__.__name__ == "TemporalTransformer3DModel")
    assert got == ref and len(got) == 6 * n_modules == 120
    assert all(n.split(".temporal_transformer.")[1] in MC.MM_NAMES for n in got)
    assert all(p.dtype == torch.float32 and p.requires_grad for p in params)
    assert {n for n, p in pu.named_parameters() if p.requires_grad} == set(ref)


def test_mm_state_dict_loads_into_the_oracle_unet():
    from synfmc_amd.training import motion_module_state_dict, motion_module_trainable_parameters
    pu = _product_unet().to(torch.bfloat16)
    params = motion_module_trainable_parameters(pu)
    with torch.no_grad():
        for p in params:
            p.add_(0.25)
    sd = motion_module_state_dict(pu)
    assert len(sd) == 120 and "down_blocks.0.motion_modules.0.temporal_transformer.norm.weight" in sd
    assert all(k.split(".temporal_transformer.")[1] in MC.MM_NAMES for k in sd)
    ou = _oracle_unet()
    missing, unexpected = ou.load_state_dict(sd, strict=False)
    assert unexpected == [] and not (set(sd) & set(missing))
    got = ou.state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k], v.float()), k
    pc = _product_unet()
    missing, unexpected = pc.load_state_dict(sd, strict=False)
    assert unexpected == [] and not (set(sd) & set(missing))


class _Sched:
    def add_noise(self, latents, noise, t):
        return latents + noise


class _Toy(torch.nn.Module):
    """Stands in for the pose adaptor: a prediction that depends on every parameter handed in (so each gets a gradient)."""

    def __init__(self, params):
        super().__init__()
        self.ps = list(params)

    def forward(self, noisy, t, encoder_hidden_states=None, pose_embedding=None, traj_features=None):
        s = sum((p.float() * 1e3).sum() for p in self.ps)
        return noisy * s


def _record_clips(monkeypatch):
    groups = []
    real = torch.nn.utils.clip_grad_norm_

    def rec(params, max_norm, *a, **k):
        params = list(params)
        groups.append({id(p) for p in params})
        return real(params, max_norm, *a, **k)
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", rec)
    return groups


def _stage3_setup(train_lora: bool):
    from synfmc_amd.training import lora_trainable_parameters, motion_module_trainable_parameters
    pu = _product_unet()
    mm = motion_module_trainable_parameters(pu)
    lora = lora_trainable_parameters(pu) if train_lora else None
    omcm = torch.nn.Linear(4, 4)
    return pu, mm, lora, omcm


@pytest.mark.parametrize("train_lora", [False, True], ids=["mm_only", "mm_and_image_lora"])
def test_stage3_clip_groups_match_the_reference(monkeypatch, train_lora):
    """train_cam_obj_ctrl.py:921-927: the Adapter is clipped on its own; with `train_image_lora` every U-Net parameter that requires grad
    (LoRA + mm) is ONE more group; with `train_mm` alone the mm gradients are not clipped."""
    from synfmc_amd.training import stage3_clip_groups, stage3_training_step
    pu, mm, lora, omcm = _stage3_setup(train_lora)
    unet_trainable = {id(p) for p in pu.parameters() if p.requires_grad}
    ref = [{id(p) for p in omcm.parameters() if p.requires_grad}] + ([unet_trainable] if train_lora else [])
    assert [{id(p) for p in g} for g in stage3_clip_groups(omcm, lora, mm)] == ref
    groups = _record_clips(monkeypatch)
    toy = _Toy(list(omcm.parameters()) + mm + (lora or []))
    opt = torch.optim.SGD(list(omcm.parameters()) + mm + (lora or []), lr=0.0)
    lat = torch.randn(1, 4, 2, 4, 4)
    stage3_training_step(toy, omcm, _Sched(), opt, None, lat, torch.randn_like(lat), torch.tensor([1]), None, None,
                         lambda: None, None, lora_params=lora, mm_params=mm)
    assert sorted(groups, key=len) == sorted(ref, key=len)


def test_stage2_clips_mm_with_everything_else(monkeypatch):
    """train_cam_ctrl.py:651: stage 2 clips every trainable parameter of the pose adaptor (encoder, merge layers and, with `train_mm`,
    the motion-module parameters) as one group."""
    from synfmc_amd.training import motion_module_trainable_parameters, stage2_training_step
    pu = _product_unet()
    enc = torch.nn.Linear(4, 4)
    merge = [p for n, p in pu.named_parameters() if "_merge." in n]
    for p in merge:
        p.requires_grad_(True)
    trainable = list(enc.parameters()) + merge + motion_module_trainable_parameters(pu)
    groups = _record_clips(monkeypatch)
    toy = _Toy(trainable)
    opt = torch.optim.SGD(trainable, lr=0.0)
    lat = torch.randn(1, 4, 2, 4, 4)
    stage2_training_step(toy, trainable, _Sched(), opt, None, lat, torch.randn_like(lat), torch.tensor([1]), None, None)
    assert groups == [{id(p) for p in trainable}]


@pytest.mark.parametrize("x_grad", [False, True], ids=["input_frozen", "input_trains"])
def test_motion_module_training_path_matches_oracle(fake, x_grad):
    """The motion module with fp32-master mm parameters under a gradient: output and all six gradients against the oracle's autograd
    -- also when the input needs no gradient (the first motion module of stages 2 / 3) -- and both projections on `linear_trainable`."""
    from synfmc_amd.training import motion_module_trainable_parameters
    om, pm = MC.module_pair(C=64, seed=3)
    pm.requires_grad_(False)
    motion_module_trainable_parameters(pm)
    for p in MC.mm_params(om).values():
        p.requires_grad_(True)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 64, 16, 4, 6, generator=g)
    w = torch.randn(1, 64, 16, 4, 6, generator=g)
    ref, g_ref, dx_ref = MC.run_module(om, x, w, x_grad)
    got, g_got, dx_got = MC.run_module(pm, x, w, x_grad)
    assert MC.rel_inf(got, ref) < 1e-5
    assert set(g_got) == set(g_ref) == set(MC.MM_NAMES)
    for n in MC.MM_NAMES:
        assert g_ref[n].abs().max() > 0, n
        assert MC.rel_inf(g_got[n], g_ref[n]) < 1e-5, n
    if x_grad:
        assert MC.rel_inf(dx_got, dx_ref) < 1e-5
    assert fake == [torch.Size([64, 64]), torch.Size([64, 64])]


def test_motion_module_frozen_path_unchanged(fake):
    """Frozen mm parameters: no `linear_trainable` call, with or without a gradient."""
    om, pm = MC.module_pair(C=64, seed=5)
    pm.requires_grad_(False)
    x = torch.randn(1, 64, 16, 4, 6, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        assert MC.rel_inf(pm(x), om(x)) < 1e-5
    pm(x.clone().requires_grad_(True))
    assert fake == []

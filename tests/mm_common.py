"""Shared pieces of the `train_mm` tests (motion-module norm / proj_in / proj_out training): the reference's selection rule restated, a
motion-module pair (oracle and product with identical seeded weights) and the gradient comparison of one module."""
import copy

import torch

from synfmc_amd.configs import MMK
from tests import common_models as CM

MM_NAMES = ("norm.weight", "norm.bias", "proj_in.weight", "proj_in.bias", "proj_out.weight", "proj_out.bias")


def reference_mm_names(unet):
    """train_cam_ctrl.py:289-302 as written: module names of every TemporalTransformer3DModel + `.norm` / `.proj_in` / `.proj_out`,
    then every parameter whose name contains one of them."""
    mm_param_names = []
    for _name, _module in unet.named_modules():
        if _module.__class__.__name__ == "TemporalTransformer3DModel":
            mm_param_names.append(f"{_name}.norm")
            mm_param_names.append(f"{_name}.proj_in")
            mm_param_names.append(f"{_name}.proj_out")
    out = []
    for __name, param in unet.named_parameters():
        for _trainable_module_name in mm_param_names:
            if _trainable_module_name in __name:
                out.append(__name)
                break
    return out


def module_pair(C=256, seed=0, device="cpu", dtype=torch.float32):
    """One motion module (`VanillaTemporalModule`, configs MMK: 8 heads, one transformer block of two temporal self-attentions, PE) as
    the oracle and as the product; fan-in scaled seeded weights, the norm gains around 1."""
    from oracle import fmc_modules as OM
    from synfmc_amd.models.motion_module import VanillaTemporalModule
    kw = copy.deepcopy(MMK)
    om = OM.VanillaTemporalModule(in_channels=C, **kw)
    CM.reseed(om, seed, fan_in_gain=0.7)
    pm = VanillaTemporalModule(in_channels=C, **kw)
    pm.load_state_dict(om.state_dict(), strict=True)
    return om.eval(), pm.to(device=device, dtype=dtype).eval()


def mm_params(module):
    tt = module.temporal_transformer
    return {n: p for n, p in tt.named_parameters() if n in MM_NAMES}


def run_module(module, x, w, x_grad: bool):
    """Output and the gradients of `(module(x) * w).sum()` w.r.t. the six mm tensors (and x with `x_grad`)."""
    x = x.clone().requires_grad_(x_grad)
    out = module(x)
    (out.float() * w.to(out.device)).sum().backward()
    grads = {n: p.grad.detach().float().cpu().clone() for n, p in mm_params(module).items() if p.grad is not None}
    return out.detach().float().cpu(), grads, (x.grad.detach().float().cpu() if x_grad else None)


def rel_inf(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()

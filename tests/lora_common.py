"""Builders shared by the Domain-LoRA training tests (FMC stage 1): the oracle's un-merged `W x + s up(down(x))` against the
product's `hip_ops.lora_linear` path, on one attention module and on the motion-free U-Net."""
import torch

from oracle import diffusers_restated as OD
from oracle import fmc_modules as OM

from synfmc_amd.configs import processor_kwargs, unet_kwargs
from tests import common_models as CM
from tests.training_common import SCHED

W4 = (64, 128, 256, 256)
# AdamW's first steps move every parameter by ~lr * sign(g): with the default eps a gradient element at the rounding noise level flips
# its update between two fp-equivalent implementations.  An eps near the typical gradient size keeps the comparison about arithmetic.
ADAM_EPS = 1e-4


def attention_pair(C, heads, cross_dim=None, seed=0, device="cpu", dtype=torch.float32):
    """(oracle Attention + LoRAAttnProcessor, product Attention + LoRAAttnProcessor), rank C / 2, identical seeded weights with a
    NON-zero `up` (with the zero init every dD is trivially zero)."""
    from synfmc_amd.models.attention_processor import LoRAAttnProcessor
    from synfmc_amd.models.layers import Attention
    r = C // 2
    oa = OD.Attention(C, cross_attention_dim=cross_dim, heads=heads, dim_head=C // heads)
    oa.set_processor(OM.LoRAAttnProcessor(hidden_size=C, cross_attention_dim=cross_dim, rank=r))
    CM.reseed(oa, seed, fan_in_gain=1.0)
    pa = Attention(C, cross_attention_dim=cross_dim, heads=heads, dim_head=C // heads)
    pa.set_processor(LoRAAttnProcessor(hidden_size=C, cross_attention_dim=cross_dim, rank=r))
    pa.load_state_dict(oa.state_dict(), strict=True)
    pa = pa.to(device=device, dtype=dtype).requires_grad_(False)
    for n, p in pa.processor.named_parameters():
        p.data = p.data.float()
        p.requires_grad_(True)
    oa.requires_grad_(False)
    for p in oa.processor.parameters():
        p.requires_grad_(True)
    return oa, pa


def lora_grads(proc):
    return {n: p.grad.detach().float().cpu().clone() for n, p in proc.named_parameters()}


def build_stage1(widths=W4, cross_dim=64, seed=0, device="cpu", dtype=torch.float32):
    """The stage-1 model: the 3-D U-Net WITHOUT motion modules (`unet_kwargs(motion=False)`) with the Domain LoRA (rank C / 2) on every
    spatial attention, oracle and product with the same seeded weights (every `up` non-zero)."""
    from synfmc_amd.models.unet import UNet3DConditionModel
    ou = OM.UNet3DConditionModelCamObjCond(**unet_kwargs(widths, cross_dim, motion=False))
    ou.set_all_attn_processor(**processor_kwargs(widths, True, temporal=False))
    CM.reseed(ou, seed, fan_in_gain=0.7).eval()
    pu = UNet3DConditionModel(**unet_kwargs(widths, cross_dim, motion=False))
    pu.set_image_layer_lora(2)
    pu.load_state_dict(ou.state_dict(), strict=True)
    pu = pu.to(device=device, dtype=dtype).eval().requires_grad_(False)
    return ou, pu


def stage1_batch(B=2, h=16, w=16, cross_dim=64, seed=5, S=7):
    g = torch.Generator().manual_seed(seed)
    return dict(latents=torch.randn(B, 4, h, w, generator=g), noise=torch.randn(B, 4, h, w, generator=g),
                t=torch.randint(0, 1000, (B,), generator=g), text=torch.randn(B, S, cross_dim, generator=g))


def oracle_lora_params(ou):
    ou.requires_grad_(False)
    params = {n: p for n, p in ou.named_parameters() if "_lora." in n and "motion_modules" not in n}
    for p in params.values():
        p.requires_grad_(True)
    return params


def oracle_stage1_steps(ou, batch, steps=2, lr=1e-3, max_grad_norm=1.0):
    """train_image_lora.py:320-381 on the oracle (trains `ou` in place), `steps` times on the same batch: (losses, first-step gradients,
    parameters after)."""
    params = oracle_lora_params(ou)
    opt = torch.optim.AdamW(list(params.values()), lr=lr, eps=ADAM_EPS)
    sched = OD.DDIMScheduler(**SCHED)
    losses, grads0 = [], None
    for _ in range(steps):
        noisy = sched.add_noise(batch["latents"], batch["noise"], batch["t"])
        pred = ou(noisy.unsqueeze(2), batch["t"], batch["text"]).sample.squeeze(2)
        loss = torch.nn.functional.mse_loss(pred.float(), batch["noise"].float())
        loss.backward()
        if grads0 is None:
            grads0 = {n: p.grad.clone() for n, p in params.items()}
        torch.nn.utils.clip_grad_norm_(list(params.values()), max_grad_norm)
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(float(loss.detach()))
    return losses, grads0, {n: p.detach().clone() for n, p in params.items()}


def product_stage1_steps(pu, batch, steps=2, lr=1e-3, max_grad_norm=1.0, device="cpu", dtype=torch.float32):
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.training import lora_trainable_parameters, stage1_training_step
    trainable = lora_trainable_parameters(pu)
    opt = torch.optim.AdamW(trainable, lr=lr, eps=ADAM_EPS)
    sched = DDIMScheduler(**SCHED)
    names = {id(p): n for n, p in pu.named_parameters()}
    grads0 = {}

    def keep_first(p, n):
        def hook(param):
            if n not in grads0:
                grads0[n] = param.grad.detach().float().cpu().clone()
        return p.register_post_accumulate_grad_hook(hook)
    hooks = [keep_first(p, names[id(p)]) for p in trainable]
    dev = lambda x: x.to(device)
    losses = []
    for _ in range(steps):
        loss = stage1_training_step(pu, trainable, sched, opt, None, dev(batch["latents"]).to(dtype), dev(batch["noise"]).to(dtype),
                                    dev(batch["t"]), dev(batch["text"]).to(dtype), max_grad_norm)
        losses.append(float(loss))
    for h in hooks:
        h.remove()
    return losses, grads0, {names[id(p)]: p.detach().float().cpu().clone() for p in trainable}


def rel_inf(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rel_inf_dict(got, ref):
    r = torch.cat([ref[k].reshape(-1).double() for k in ref])
    g = torch.cat([got[k].reshape(-1).double().cpu() for k in ref])
    return ((g - r).abs().max() / r.abs().max()).item()

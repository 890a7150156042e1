"""One FMC stage-1 (Domain-LoRA) training step at the configs/lora.yaml shapes, timed on the GPU.

    python tools/lora_train_step.py --path own      [--steps 10 --warmup 3]   # hip_ops.lora_linear + fmc_linear_wgrad_bf16
    python tools/lora_train_step.py --path autograd [--steps 10 --warmup 3]   # baseline: the LoRA branch as F.linear under autograd
    python tools/lora_train_step.py --wgrad                                    # the weight-gradient kernel on the step's shapes

Workload: 16 images of 256 x 384 (32 x 48 latents), SD-1.5 widths 320 / 640 / 1280 / 1280, the motion-free 3-D U-Net with a rank C / 2
LoRA on all 32 spatial attention processors, text 16 x 77 x 768, random weights, bf16 storage with fp32 LoRA masters, AdamW.
Prints one JSON line.  The baseline keeps everything else of the step (frozen projections on the fused GEMMs, attention kernels, the
optimizer) and computes each projection as `linear(x, W) + s * F.linear(F.linear(x, D), U)` under plain autograd.
`--wgrad`: per (M, N, K) the kernel's time, TF/s and share of the dense bf16 peak (2.5 PF/s), next to the route that exists without it:
`t().contiguous()` of both operands (token dimension zero-padded to a multiple of 64), then a split-K `fmc_linear_bf16`."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BF16_TFS = 2500.0
WGRAD_SHAPES = [(24576, 320, 160), (24576, 160, 320), (24576, 480, 320), (6144, 640, 320), (6144, 960, 640), (1536, 1280, 640),
                (1536, 1920, 1280), (384, 1280, 640), (1232, 640, 768), (1232, 1280, 768)]


def _autograd_core(attn, lora, q_in, kv_in, temporal, s, residual=None):
    """Baseline processor body: frozen projections through `linear_op`, the LoRA branch through F.linear under autograd."""
    from synfmc_amd import hip_ops as K
    from synfmc_amd.models.attention_processor import _tok
    from synfmc_amd.models.layers import linear_op
    layers = [lora.to_q_lora, lora.to_k_lora, lora.to_v_lora, lora.to_out_lora]

    def proj(x, lin, i, bias=None, res=None):
        lay = layers[i]
        sc = s * (lay.network_alpha / lay.rank if lay.network_alpha is not None else 1.0)
        y = linear_op(x, lin.weight, bias, res)
        return y + sc * F.linear(F.linear(x, lay.down.weight.to(x.dtype)), lay.up.weight.to(x.dtype))
    if kv_in is None:
        qkv = torch.cat([proj(q_in, attn.to_q, 0), proj(q_in, attn.to_k, 1), proj(q_in, attn.to_v, 2)], dim=-1)
        o = K.self_attention_qkv(qkv, attn.heads, attn.scale, temporal)
    else:
        ctx = _tok(kv_in)
        q = proj(q_in, attn.to_q, 0)
        kv = torch.cat([proj(ctx, attn.to_k, 1), proj(ctx, attn.to_v, 2)], dim=-1)
        o = K.cross_attention_q_kv(q, kv, attn.heads, attn.scale)
    return proj(o, attn.to_out[0], 3, attn.to_out[0].bias, residual)


def build(seed=0):
    from synfmc_amd.configs import unet_kwargs
    from synfmc_amd.models.unet import UNet3DConditionModel
    torch.manual_seed(seed)
    pu = UNet3DConditionModel(**unet_kwargs((320, 640, 1280, 1280), 768, motion=False))
    pu.set_image_layer_lora(2)
    pu = pu.to("cuda", torch.bfloat16).requires_grad_(False)
    with torch.no_grad():
        for n, p in pu.named_parameters():
            if n.endswith("_lora.up.weight"):
                p.normal_(0, 1e-3)
    return pu


def train_step_time(path: str, steps: int, warmup: int) -> dict:
    from synfmc_amd.models import attention_processor as AP
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.training import lora_trainable_parameters, stage1_training_step
    if path == "autograd":
        AP._lora_train_core = _autograd_core
    pu = build()
    trainable = lora_trainable_parameters(pu)
    opt = torch.optim.AdamW(trainable, lr=1e-4)
    sched = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1,
                          clip_sample=False)
    g = torch.Generator(device="cuda").manual_seed(1)
    B = 16
    lat = torch.randn(B, 4, 32, 48, device="cuda", generator=g).to(torch.bfloat16)
    noise = torch.randn(B, 4, 32, 48, device="cuda", generator=g).to(torch.bfloat16)
    t = torch.randint(0, 1000, (B,), device="cuda", generator=g)
    text = torch.randn(B, 77, 768, device="cuda", generator=g).to(torch.bfloat16)

    def step():
        return stage1_training_step(pu, trainable, sched, opt, None, lat, noise, t, text)
    for _ in range(warmup):
        loss = step()
    torch.cuda.synchronize()
    torch.cuda._sleep(1000)              # a marker kernel in a kernel trace: the timed steps are what follows it
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    return {"tool": "lora_train_step", "path": path, "images": B, "latent": [32, 48], "ms_per_step": round(ms, 3),
            "steps_per_s": round(1000.0 / ms, 3), "loss": round(float(loss), 5), "steps": steps, "warmup": warmup}


def _events_ms(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _transpose_route(a, b):
    """out[N, K] = a^T b through what existed before: both operands transposed (tokens zero-padded to 64), split-K linear_bf16."""
    from synfmc_amd import hip_ops as K
    M, N = a.shape
    Kd = b.shape[1]
    Mp = (M + 63) // 64 * 64
    at = torch.zeros(N, Mp, dtype=a.dtype, device=a.device)
    bt = torch.zeros(Kd, Mp, dtype=b.dtype, device=b.device)
    at[:, :M] = a.t()
    bt[:, :M] = b.t()
    tiles = ((N + 127) // 128) * ((Kd + 127) // 128)
    split = 1
    while split < 16 and tiles * split * 2 <= 512 and Mp // 64 >= split * 4:
        split *= 2
    return K.linear_bf16(at, bt, tile=1, split_k=split)


def wgrad_table() -> dict:
    from synfmc_amd import hip_ops as K
    rows = []
    for M, N, Kd in WGRAD_SHAPES:
        a = torch.randn(M, N, device="cuda").to(torch.bfloat16)
        b = torch.randn(M, Kd, device="cuda").to(torch.bfloat16)
        out = torch.empty(N, Kd, device="cuda")
        us = _events_ms(lambda: K.linear_wgrad(a, b, out=out)) * 1e3
        us_old = _events_ms(lambda: _transpose_route(a, b)) * 1e3
        tfs = 2.0 * M * N * Kd / (us * 1e-6) / 1e12
        rows.append({"M": M, "N": N, "K": Kd, "us": round(us, 2), "tflops": round(tfs, 1), "peak_frac": round(tfs / PEAK_BF16_TFS, 4),
                     "transpose_splitk_us": round(us_old, 2), "speedup": round(us_old / us, 2)})
    return {"tool": "lora_train_step", "wgrad": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=["own", "autograd"], default="own")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--wgrad", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_train_step needs the MI355X")
    print(json.dumps(wgrad_table() if args.wgrad else train_step_time(args.path, args.steps, args.warmup)))


if __name__ == "__main__":
    main()

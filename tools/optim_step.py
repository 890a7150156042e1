"""The parameter update alone -- clip, AdamW, gradient zeroing, bf16 shadow refresh -- on the MI355X: the torch chain against `FusedAdamW`.

    python tools/optim_step.py [--updates 50 --warmup 5 --sets stage3,stage2_mm,lora]
    rocprofv3 --kernel-trace --stats -- python tools/optim_step.py --sets stage3 --updates 10      # per-kernel times (nothing else traced)

Synthetic fp32 tensors with the shapes of three trainable sets at SD-1.5 widths (from the model constructors on the meta device, no weights):
  stage3     the OMC Adapter's reached parameters (its level-3 blocks never receive a gradient and are pruned): 91.9 M elements;
  stage2_mm  stage 2 with `train_mm`: the camera encoder, the merge layers and the 120 motion-module tensors (those have bf16 shadows);
  lora       the Domain LoRA factors of stage 1.
Gradients are views of `GradAllReducer` buckets, as in training.  Two arms in one process, alternating in blocks of 10 updates, device events
around each block, each arm eager and as a replayed HIP graph:
  torch  `clip_grad_norm_` + `torch.optim.AdamW(capturable=True)` + the bucket fills + the `bf16_param` refresh of the shadowed tensors
         (`training.optimizer_update` with torch's optimizer, then the shadows as the next forward would refresh them);
  fused  `training.optimizer_update` with `FusedAdamW` (two ABI calls; shadows and zeroing inside).
After the first update the gradients are zero in both arms: the traffic is the same, the values are not the point.  Reported per set: ms per
update, algorithmic bytes / time as a share of the 6.29 TB/s copy rate (torch chain: 44 bytes per element + 12 per shadowed element; fused: 36
+ 6), and fused / torch.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WIDTHS = (320, 640, 1280, 1280)
COPY_RATE = 6.29e12
BLOCK = 10


def parameter_sets() -> dict:
    """name -> list of (shape, shadowed); built on the meta device."""
    from synfmc_amd.adapter import Adapter
    from synfmc_amd.configs import adapter_kwargs, encoder_kwargs, processor_kwargs, unet_kwargs
    from synfmc_amd.models.pose_adaptor import CameraPoseEncoder
    from synfmc_amd.models.unet import UNet3DConditionModel, UNet3DConditionModelPoseCond
    from synfmc_amd.training import _motion_module_parameters, _spatial_lora_parameters, stage2_trainable_parameters
    sets = {}
    with torch.device("meta"):
        ada = Adapter(**adapter_kwargs(WIDTHS))
        level3 = ("body.6.", "body.7.", "zero_conv_out_list.3.")         # never reached by the loss (training.GradAllReducer prunes them)
        sets["stage3"] = [(tuple(p.shape), False) for n, p in ada.named_parameters() if not n.startswith(level3)]
        pu = UNet3DConditionModelPoseCond(**unet_kwargs(WIDTHS, 768))
        pu.set_all_attn_processor(**processor_kwargs(WIDTHS))
        pe = CameraPoseEncoder(**encoder_kwargs(WIDTHS))
        mm = [p for _, p in _motion_module_parameters(pu)]
        sets["stage2_mm"] = [(tuple(p.shape), False) for p in stage2_trainable_parameters(pu, pe)] + [(tuple(p.shape), True) for p in mm]
        pl = UNet3DConditionModel(**unet_kwargs(WIDTHS, 768, motion=False))
        pl.set_image_layer_lora(2)
        sets["lora"] = [(tuple(p.shape), False) for _, p in _spatial_lora_parameters(pl)]
    return sets


class _Holder(torch.nn.Module):
    def __init__(self, p):
        super().__init__()
        self.weight = p


def _arm(shapes, fused: bool, seed=0):
    """(update(), elements, shadowed elements) of one arm."""
    from synfmc_amd.models.layers import bf16_param
    from synfmc_amd.training import FusedAdamW, GradAllReducer, optimizer_update
    gen = torch.Generator(device="cuda").manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen) * 0.05) for s, _ in shapes]
    reducer = GradAllReducer(params, find_unused=False)
    for p in params:
        p.grad.copy_(torch.randn(p.shape, device="cuda", generator=gen) * 1e-3)
    box = torch.nn.ModuleList([_Holder(p) for p, (_, sh) in zip(params, shapes) if sh])
    for h in box:
        bf16_param(h, "weight", rounded_f32=True)
    if fused:
        opt = FusedAdamW(params, lr=1e-4).attach(box)
        update = lambda: optimizer_update(params, opt, reducer, 1.0)
    else:
        opt = torch.optim.AdamW(params, lr=1e-4, capturable=True)

        def update():
            optimizer_update(params, opt, reducer, 1.0)
            for h in box:
                bf16_param(h, "weight")
    return update, sum(p.numel() for p in params), sum(h.weight.numel() for h in box), len(params)


def _graphed(update, warmup):
    for _ in range(warmup):
        update()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        update()
    return graph.replay


def measure(shapes, updates: int, warmup: int) -> dict:
    arms, alive = {}, []                     # a captured graph holds raw addresses (parameters, states, the optimizer's device tables): keep their owners
    n = n_sh = count = 0
    for name, fused in (("torch", False), ("fused", True)):
        update, n, n_sh, count = _arm(shapes, fused)
        arms[name + "_eager"] = update
    for name, fused in (("torch", False), ("fused", True)):
        update, _, _, _ = _arm(shapes, fused, seed=1)
        alive.append(update)
        arms[name + "_graph"] = _graphed(update, warmup)
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: 0.0 for k in arms}
    blocks = max(1, (updates + BLOCK - 1) // BLOCK)
    for _ in range(blocks):
        for k, fn in arms.items():                               # alternating: every arm sees the same machine state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BLOCK):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k] += e0.elapsed_time(e1)
    ms = {k: v / (blocks * BLOCK) for k, v in ms.items()}
    bytes_torch, bytes_fused = 44 * n + 12 * n_sh, 36 * n + 6 * n_sh
    out = {"tensors": count, "elements": n, "shadowed_elements": n_sh, "updates_per_arm": blocks * BLOCK}
    for k, v in ms.items():
        b = bytes_fused if k.startswith("fused") else bytes_torch
        out[k + "_ms"] = round(v, 4)
        out[k + "_copy_rate_share"] = round(b / (v * 1e-3) / COPY_RATE, 3)
    out["ratio_eager"] = round(ms["fused_eager"] / ms["torch_eager"], 3)
    out["ratio_graph"] = round(ms["fused_graph"] / ms["torch_graph"], 3)
    del arms, alive
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", default="stage3,stage2_mm,lora")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_step needs the MI355X")
    sets = parameter_sets()
    result = {"tool": "optim_step", "copy_rate_TBps": COPY_RATE / 1e12, "sets": {}}
    for name in args.sets.split(","):
        result["sets"][name] = measure(sets[name], args.updates, args.warmup)
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

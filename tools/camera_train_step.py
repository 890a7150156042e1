"""One FMC stage-2 (CMC) and one stage-3 (OMC) training step at the configs/cam.yaml shapes on the two routes of the trained layers, timed.

    python tools/camera_train_step.py [--steps 5 --warmup 2]             # both stages: parent, new, parent again (alternated in one session)
    python tools/camera_train_step.py --only stage2|stage3 --route new|parent      # one step function alone (under `rocprofv3 --kernel-trace --stats -- ...`)

Workload: one clip of 16 frames at 256 x 384 (32 x 48 latents), SD-1.5 widths 320 / 640 / 1280 / 1280, the frozen U-Net in bf16, text
1 x 77 x 768, AdamW.  Seeded NON-ZERO weights everywhere (`reseed`): the zero-initialised `qkv_merge` and zero convolutions would make the
encoder's gradients vanish.
  parent route: the Camera Encoder (stage 2) / OMC Adapter (stage 3) as fp32 modules under bf16 autocast, the merges bf16 parameters --
                torch autograd on MIOpen / hipBLASLt / at::native kernels for the trained layers;
  new route:    `camera_trainable_parameters` / `omc_trainable_parameters` -- fp32 masters, bf16 activations, no autocast, `FusedAdamW`.
    python tools/camera_train_step.py --conv-wgrad [--steps 20 --warmup 3]   # the new route with the direct 3x3 weight gradient off and on

--conv-wgrad: one model per stage on the new route; `hip_ops.CONV_WGRAD` (FMC_CONV_WGRAD) is toggled between legs of `--steps` timed steps,
off, on, off, on (every leg is printed: the two legs of a setting show its spread), then one step per setting with `hip_ops.call_log` on
and `conv3x3_weight_grad` counted: the `conv_wgrad` entries and the calls of the old chain (each is two `fmc_nhwc_to_cmajor_padded`
launches, three GEMMs, a stack and a cast).
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WIDTHS = (320, 640, 1280, 1280)
FRAMES, H, W = 16, 256, 384
SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)


def reseed(module, seed, gain=0.7):
    """Seeded fan-in scaled weights for every parameter (norm gains around 1, biases small): nothing stays zero-initialised."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.ndim >= 2:
                fan_in = p[0].numel()
                v = torch.randn(p.shape, generator=g) * (gain / fan_in ** 0.5)
            elif "norm" in name and name.endswith("weight"):
                v = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
            else:
                v = 0.05 * torch.randn(p.shape, generator=g)
            p.copy_(v.to(p.dtype))


def build_stage2(seed=0):
    """(CMC U-Net bf16, camera encoder bf16) at SD-1.5 widths, frozen, seeded non-zero weights."""
    from synfmc_amd.configs import encoder_kwargs, processor_kwargs, unet_kwargs
    from synfmc_amd.models.pose_adaptor import CameraPoseEncoder
    from synfmc_amd.models.unet import UNet3DConditionModelPoseCond
    torch.manual_seed(seed)
    pu = UNet3DConditionModelPoseCond(**unet_kwargs(WIDTHS, 768))
    pu.set_all_attn_processor(**processor_kwargs(WIDTHS))
    pe = CameraPoseEncoder(**encoder_kwargs(WIDTHS))
    reseed(pu, seed + 1)
    reseed(pe, seed + 2)
    return (pu.to("cuda", torch.bfloat16).eval().requires_grad_(False), pe.to("cuda", torch.bfloat16).eval().requires_grad_(False))


def build_stage3(seed=0):
    """(CMC + OMC U-Net bf16, camera encoder bf16, OMC Adapter bf16), frozen, seeded non-zero weights."""
    from synfmc_amd.adapter import Adapter
    from synfmc_amd.configs import adapter_kwargs, encoder_kwargs, processor_kwargs, unet_kwargs
    from synfmc_amd.models.pose_adaptor import CameraPoseEncoder
    from synfmc_amd.models.unet import UNet3DConditionModelCamObjCond
    from synfmc_amd.modified_modules import patch_unet_for_omc
    torch.manual_seed(seed)
    pu = UNet3DConditionModelCamObjCond(**unet_kwargs(WIDTHS, 768))
    pu.set_all_attn_processor(**processor_kwargs(WIDTHS))
    patch_unet_for_omc(pu)
    pe = CameraPoseEncoder(**encoder_kwargs(WIDTHS))
    pa = Adapter(**adapter_kwargs(WIDTHS))
    for i, m in enumerate((pu, pe, pa)):
        reseed(m, seed + 1 + i)
    return tuple(m.to("cuda", torch.bfloat16).eval().requires_grad_(False) for m in (pu, pe, pa))


def inputs(seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lat = torch.randn(1, 4, FRAMES, H // 8, W // 8, device="cuda", generator=g).to(torch.bfloat16)
    noise = torch.randn(lat.shape, device="cuda", generator=g).to(torch.bfloat16)
    t = torch.randint(0, 1000, (1,), device="cuda", generator=g)
    text = torch.randn(1, 77, 768, device="cuda", generator=g).to(torch.bfloat16)
    pose = torch.randn(1, 6, FRAMES, H, W, device="cuda", generator=g).to(torch.bfloat16)
    return lat, noise, t, text, pose


def stage2_step_fn(pu, pe, route: str, lr=1e-4):
    """(step(), trainable): one `stage2_training_step` at the cam.yaml shapes on the `new` or the `parent` route."""
    from synfmc_amd.models.pose_adaptor import PoseAdaptor
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.training import FusedAdamW, camera_trainable_parameters, stage2_trainable_parameters, stage2_training_step
    if route == "new":
        trainable = camera_trainable_parameters(pu, pe)
        opt = FusedAdamW(trainable, lr=lr).attach(pu, pe)
    else:
        pe.float()
        trainable = stage2_trainable_parameters(pu, pe)
        for p in trainable:
            p.requires_grad_(True)
        opt = torch.optim.AdamW(trainable, lr=lr)
    sched = DDIMScheduler(**SCHED)
    lat, noise, t, text, pose = inputs()
    adaptor = PoseAdaptor(pu, pe)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=route != "new"):
            return stage2_training_step(adaptor, trainable, sched, opt, None, lat, noise, t, text, pose)
    return step, trainable


def stage3_step_fn(pu, pe, pa, route: str, lr=1e-4):
    """(step(), trainable): one `stage3_training_step` (three synthetic objects) on the `new` or the `parent` route."""
    from synfmc_amd.configs import synthetic_clip, union_masks
    from synfmc_amd.models.pose_obj_adaptor import CamObjPoseAdaptor
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.training import FusedAdamW, omc_trainable_parameters, stage3_training_step
    from synfmc_amd.util import get_traj_features_v2
    if route == "new":
        trainable = omc_trainable_parameters(pa)
        opt = FusedAdamW(trainable, lr=lr).attach(pa)
    else:
        pa.float().requires_grad_(True)
        trainable = list(pa.parameters())
        opt = torch.optim.AdamW(trainable, lr=lr)
    sched = DDIMScheduler(**SCHED)
    lat, noise, t, text, pose = inputs()
    clip = synthetic_clip(B=1, Fr=FRAMES, H=H, W=W, cross_dim=768)
    masks = union_masks(clip).to("cuda")
    adaptor = CamObjPoseAdaptor(pu, pe)
    traj = lambda: get_traj_features_v2(clip["infos"], clip["masks"], pa, False, 0.0, [False], "cuda", torch.bfloat16)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=route != "new"):
            return stage3_training_step(adaptor, pa, sched, opt, None, lat, noise, t, text, pose, traj, masks)
    return step, trainable


def step_time(stage: str, route: str, steps: int, warmup: int) -> float:
    if stage == "stage2":
        step, _ = stage2_step_fn(*build_stage2(), route)
    else:
        step, _ = stage3_step_fn(*build_stage3(), route)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    del step
    torch.cuda.empty_cache()
    return ms


def timed_steps(step, steps: int) -> float:
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def conv_wgrad_ab(stage: str, steps: int, warmup: int) -> dict:
    """The new route of one stage with `hip_ops.CONV_WGRAD` off and on, alternated in one process on one model."""
    from synfmc_amd import hip_ops as K
    step, _ = stage2_step_fn(*build_stage2(), "new") if stage == "stage2" else stage3_step_fn(*build_stage3(), "new")
    saved = K.CONV_WGRAD
    legs = {"off_ms": [], "on_ms": []}
    counts = {}
    try:
        for on in (False, True):                       # both settings warm: autotuning, packs, workspaces
            K.CONV_WGRAD = on
            for _ in range(warmup):
                step()
        for _ in range(2):
            for on in (False, True):
                K.CONV_WGRAD = on
                legs["on_ms" if on else "off_ms"].append(round(timed_steps(step, steps), 3))
        real, old_calls = K.conv3x3_weight_grad, []
        K.conv3x3_weight_grad = lambda *a, **k: (old_calls.append(1), real(*a, **k))[1]
        try:
            for on in (False, True):
                K.CONV_WGRAD, K.call_log = on, []
                del old_calls[:]
                step()
                counts["on" if on else "off"] = {"conv_wgrad_entries": sum(1 for e in K.call_log if e[0] == "conv_wgrad"),
                                                 "old_chain_calls": len(old_calls), "logged_launches": len(K.call_log)}
        finally:
            K.conv3x3_weight_grad, K.call_log = real, None
    finally:
        K.CONV_WGRAD = saved
    del step
    torch.cuda.empty_cache()
    spread = max(legs["off_ms"]) - min(legs["off_ms"])
    return dict(legs, off_spread_ms=round(spread, 3), on_minus_off_ms=round(min(legs["on_ms"]) - min(legs["off_ms"]), 3), one_step=counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conv-wgrad", action="store_true", help="the new route with FMC_CONV_WGRAD off and on, legs alternated")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["stage2", "stage3"], help="one stage alone (for a kernel trace of it)")
    ap.add_argument("--route", choices=["new", "parent"], default="new", help="with --only: which route")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("camera_train_step needs the MI355X")
    if args.conv_wgrad:
        out = {"tool": "camera_train_step", "mode": "conv_wgrad", "frames": FRAMES, "pixels": [H, W], "steps": args.steps, "warmup": args.warmup}
        for stage in ("stage2", "stage3"):
            out[stage] = conv_wgrad_ab(stage, args.steps, args.warmup)
            print(stage, out[stage], file=sys.stderr, flush=True)
        print(json.dumps(out))
        return
    if args.only:
        ms = step_time(args.only, args.route, args.steps, args.warmup)
        print(json.dumps({"tool": "camera_train_step", "stage": args.only, "route": args.route, "ms_per_step": round(ms, 3), "steps": args.steps}))
        return
    out = {"tool": "camera_train_step", "frames": FRAMES, "pixels": [H, W], "steps": args.steps, "warmup": args.warmup}
    for stage in ("stage2", "stage3"):
        # parent, new, parent: the parent's own spread is known
        out[stage] = {name: round(step_time(stage, route, args.steps, args.warmup), 3)
                      for name, route in (("parent_ms", "parent"), ("new_ms", "new"), ("parent_again_ms", "parent"))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""One FMC stage-2 (CMC) training step at the configs/cam.yaml shapes, with and without `train_mm`, timed on the GPU.

    python tools/mm_train_step.py [--steps 5 --warmup 2]      # stage-2 step without / with train_mm + the two new kernels on its shapes
    python tools/mm_train_step.py --only on|off               # one variant alone (under `rocprofv3 --kernel-trace --stats -- ...`)

Workload: one clip of 16 frames at 256 x 384 (32 x 48 latents), SD-1.5 widths 320 / 640 / 1280 / 1280, the CMC U-Net
(`UNet3DConditionModelPoseCond`, pose-adaptor processors on the temporal attention, Domain LoRA on the spatial one, frozen) in bf16, the
camera encoder as fp32 masters under bf16 autocast, text 1 x 77 x 768, random weights, AdamW.  `train_mm` adds the 120 motion-module
tensors (norm / proj_in / proj_out of 20 modules, fp32 masters) to the trainable set.
Kernel table: per motion-module shape `fmc_groupnorm_silu_bwd_params` (with dX) against the dX-only `fmc_groupnorm_silu_bwd_add`, and
`fmc_column_sum` on the projections' dY; GB/s over the algorithmic bytes (GroupNorm backward: x and dy read, dx written; column sum: dY
read once).  Prints one JSON line."""
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
# (N = frames, HW, C) of the 20 motion modules' norms at 32 x 48 latents (levels 1536 / 384 / 96 / 24 pixels)
MM_SHAPES = [(16, 1536, 320), (16, 384, 640), (16, 96, 1280), (16, 24, 1280)]


def build_stage2(seed=0):
    """(U-Net bf16, camera encoder fp32) of the CMC stage at SD-1.5 widths, frozen; random weights."""
    from synfmc_amd.configs import encoder_kwargs, processor_kwargs, unet_kwargs
    from synfmc_amd.models.pose_adaptor import CameraPoseEncoder
    from synfmc_amd.models.unet import UNet3DConditionModelPoseCond
    torch.manual_seed(seed)
    pu = UNet3DConditionModelPoseCond(**unet_kwargs(WIDTHS, 768))
    pu.set_all_attn_processor(**processor_kwargs(WIDTHS))
    pu = pu.to("cuda", torch.bfloat16).eval().requires_grad_(False)
    pe = CameraPoseEncoder(**encoder_kwargs(WIDTHS)).to("cuda").eval().requires_grad_(False)
    return pu, pe


def stage2_inputs(seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lat = torch.randn(1, 4, FRAMES, H // 8, W // 8, device="cuda", generator=g).to(torch.bfloat16)
    noise = torch.randn(lat.shape, device="cuda", generator=g).to(torch.bfloat16)
    t = torch.randint(0, 1000, (1,), device="cuda", generator=g)
    text = torch.randn(1, 77, 768, device="cuda", generator=g).to(torch.bfloat16)
    pose = torch.randn(1, 6, FRAMES, H, W, device="cuda", generator=g)
    return lat, noise, t, text, pose


def stage2_step_fn(pu, pe, train_mm: bool, lr=1e-4):
    """(step(), trainable, mm_params): one `stage2_training_step` on the cam.yaml shapes."""
    from synfmc_amd.models.pose_adaptor import PoseAdaptor
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.training import motion_module_trainable_parameters, stage2_trainable_parameters, stage2_training_step
    trainable = stage2_trainable_parameters(pu, pe)
    for p in trainable:
        p.requires_grad_(True)
    mm = motion_module_trainable_parameters(pu) if train_mm else []
    trainable = trainable + mm
    opt = torch.optim.AdamW(trainable, lr=lr)
    sched = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1,
                          clip_sample=False)
    lat, noise, t, text, pose = stage2_inputs()
    adaptor = PoseAdaptor(pu, pe)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return stage2_training_step(adaptor, trainable, sched, opt, None, lat, noise, t, text, pose.to(torch.bfloat16))
    return step, trainable, mm


def train_step_time(train_mm: bool, steps: int, warmup: int) -> float:
    pu, pe = build_stage2()
    step, _, _ = stage2_step_fn(pu, pe, train_mm)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _events_us(fn, reps=50):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def kernel_table() -> list:
    from synfmc_amd import _lib
    from synfmc_amd import hip_ops as K
    rows = []
    for N, HW, C in MM_SHAPES:
        x = torch.randn(N, HW, C, device="cuda").to(torch.bfloat16)
        dy = torch.randn(N, HW, C, device="cuda").to(torch.bfloat16)
        gamma = torch.rand(C, device="cuda") + 0.5
        beta = torch.randn(C, device="cuda")
        _, stats = K.groupnorm_silu_raw(x, gamma, beta, 32, 1e-6, False)
        dx = torch.empty_like(x)
        lib = _lib.load()
        ws = K._workspace(x.device, lib.fmc_groupnorm_workspace_bytes(N, C, 32))

        def dx_only():
            _lib.check(lib.fmc_groupnorm_silu_bwd_add(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                      stats.data_ptr(), ws.data_ptr(), N, HW, C, 32, 0, None, K.FMC_BF16, K._stream()),
                       "fmc_groupnorm_silu_bwd_add")
        us_p = _events_us(lambda: K.groupnorm_silu_bwd_params(dy, x, gamma, beta, stats, 32, False))
        us_d = _events_us(dx_only)
        us_c = _events_us(lambda: K.column_sum(dy.view(-1, C)))
        gb = 3.0 * x.numel() * 2 / 1e9
        rows.append({"N": N, "HW": HW, "C": C, "gn_bwd_params_us": round(us_p, 2), "gn_bwd_params_gbs": round(gb / (us_p * 1e-6), 1),
                     "gn_bwd_dx_only_us": round(us_d, 2), "column_sum_us": round(us_c, 2),
                     "column_sum_gbs": round(x.numel() * 2 / 1e9 / (us_c * 1e-6), 1)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["off", "on"], help="time one variant of the step alone (for a kernel trace of it)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mm_train_step needs the MI355X")
    if args.only:
        ms = train_step_time(args.only == "on", args.steps, args.warmup)
        print(json.dumps({"tool": "mm_train_step", "train_mm": args.only == "on", "ms_per_step": round(ms, 3), "steps": args.steps}))
        return
    off = train_step_time(False, args.steps, args.warmup)
    on = train_step_time(True, args.steps, args.warmup)
    print(json.dumps({"tool": "mm_train_step", "frames": FRAMES, "pixels": [H, W], "ms_per_step": round(off, 3),
                      "ms_per_step_train_mm": round(on, 3), "ratio": round(on / off, 4), "steps": args.steps, "warmup": args.warmup,
                      "kernels": kernel_table()}))


if __name__ == "__main__":
    main()

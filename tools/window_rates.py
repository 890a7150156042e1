"""The measurements behind profiles/sliding_windows.md, on one GPU, at the bench clip's latent size (40 x 64, bench.py's `lora` model, bf16,
CFG, DDIM, captured graphs) with 2 and 3 windows of 16 frames overlapping by 12:

  per step   `AnimationPipeline` on the torch-op window loop (no `window_batch`), on `fmc_window_step` with all windows in one U-Net call
             (`window_batch=None`) and with one window per call (`window_batch=1`).  Every leg is warmed once (graphs captured), then the
             legs alternate, `--rounds` times each; a leg's time is one end-to-end call of `--steps` steps;
  kernel     the blend-and-step call alone (`hip_ops.window_step`, CFG, two copies of x_in), with the windows overlapping by 12 (one launch)
             and not at all (one `sampler_step_kernel` launch per block): device events over 2000 back-to-back calls after 20 warm-ups,
             three times.

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
F, OVERLAP = 16, 12


def _events(fn, launches=40, warmup=4):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches             # us per launch


def kernel_times(windows, dtype=torch.bfloat16):
    """Per call of `hip_ops.window_step`, 2000 back-to-back calls per sample (some 40 ms): the buffers (4 - 6 MB) stay in the caches
    between calls, so this is the time of a launch in a loop, not an HBM rate.  Overlap 12: one launch of `window_step_kernel`;
    overlap 0 (disjoint windows): B C W launches of `sampler_step_kernel`."""
    from synfmc_amd import hip_ops as K
    for overlap in (OVERLAP, 0):
        for W in windows:
            Ftot = W * (F - overlap) + overlap
            g = torch.Generator().manual_seed(0)
            eps = torch.randn(2, W, 1, 4, F, 40, 64, generator=g).to("cuda", dtype)
            x = torch.randn(1, 4, Ftot, 40, 64, generator=g).cuda()
            x_out, x_in = torch.empty_like(x), torch.empty_like(eps)
            fn = lambda: K.window_step(eps, x, overlap=overlap, guidance=8.0, m_x=1.1, m_e=-0.4, c_e=0.3, c_m=0.9, x_out=x_out, x_in=x_in)
            us = [_events(fn, launches=2000, warmup=20) for _ in range(3)]
            cover = W * F / Ftot
            moved = x.numel() * (2 * 2 * cover + 4 + 4 + 2 * 2 * cover)      # bf16 eps (2 halves) and x_in (2 copies) per covering window, fp32 x in and out
            print(json.dumps({"kernel": "window_step", "windows": W, "overlap": overlap, "frames": Ftot, "n": x.numel(),
                              "device_launches_per_call": 1 if overlap else 4 * W, "us_per_call": [round(u, 2) for u in us],
                              "bytes_per_call": int(moved)}), flush=True)


def step_times(windows, steps, rounds):
    import bench
    from synfmc_amd import schedulers as S
    from synfmc_amd.pipelines.pipeline_animation_cm_om import AnimationPipeline
    device, dtype = torch.device("cuda", 0), torch.bfloat16
    unet, _, _ = bench.build_models(device, dtype, "lora")
    _, text2 = bench.synthetic_inputs(0, device)
    legs = {"torch-op loop": {}, "window_step, all windows batched": dict(window_batch=None), "window_step, window_batch=1": dict(window_batch=1)}
    for W in windows:
        Ftot = W * (F - OVERLAP) + OVERLAP
        lat = torch.randn(1, 4, Ftot, bench.HEIGHT // 8, bench.WIDTH // 8, generator=torch.Generator().manual_seed(1)).to(device)
        pipes = {name: AnimationPipeline(None, None, None, unet, S.DDIMScheduler(**SCHED)) for name in legs}
        call = lambda name: pipes[name](None, F, height=bench.HEIGHT, width=bench.WIDTH, num_inference_steps=steps, guidance_scale=8.0,
                                        latents=lat.clone(), output_type="latent", prompt_embeds=text2.to(dtype), multidiff_total_steps=W,
                                        multidiff_overlaps=OVERLAP, **legs[name]).videos
        outs = {name: call(name) for name in legs}                               # warm: graphs captured
        torch.cuda.synchronize()
        times = {name: [] for name in legs}
        for _ in range(rounds):
            for name in legs:                                                    # the legs alternate
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(name)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / steps * 1e3)
        base = outs["torch-op loop"].float()
        for name in legs:
            dev = float((outs[name].float() - base).abs().max() / base.abs().max())
            print(json.dumps({"leg": name, "windows": W, "frames": Ftot, "steps": steps, "ms_per_step": [round(t, 2) for t in times[name]],
                              "rel_inf_vs_torch_op_loop": round(dev, 5)}), flush=True)
        del pipes


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--windows", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    if a.kernel:
        kernel_times(a.windows)
    if a.loop:
        step_times(a.windows, a.steps, a.rounds)

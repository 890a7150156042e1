"""Two measurements behind profiles/samplers.md, on one GPU:

  --kernel   per-launch time of `fmc_sampler_step` at the bench latents' n (1 x 4 x 16 x 40 x 64) in three configurations -- Euler, DPM-Solver++
             order 2 with x_in, DDIM eta = 1 -- next to `cfg_ddim_kernel`: device events over 40 back-to-back launches after 4 warm-ups;
  --loop     steps/s of the 25-step loop of `CameraObjCtrlPipeline` (bench.py's `obj` model and clip, bf16, CFG, captured graph, latents out) per
             sampler: a first call warms the graphs, the second is timed end to end.

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear")


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


def kernel_times(dtype=torch.bfloat16):
    from synfmc_amd import hip_ops as K
    shape = (1, 4, 16, 40, 64)
    n = 4 * 16 * 40 * 64
    g = torch.Generator().manual_seed(0)
    eps = torch.randn((2,) + shape[1:], generator=g).to("cuda", dtype)
    x = torch.randn(shape, generator=g).cuda()
    noise = torch.randn(shape, generator=g).to("cuda", dtype)
    h1, m_out, x_out = torch.randn_like(x), torch.empty_like(x), torch.empty_like(x)
    x_in = torch.empty((2,) + shape[1:], dtype=dtype, device="cuda")
    cases = {
        "cfg_ddim_kernel": lambda: K.cfg_ddim_step(eps, x, 8.0, 0.5, 0.6, True),
        "sampler_step euler (x_in)": lambda: K.sampler_step(eps, x, guidance=8.0, has_uncond=True, m_x=1.0, m_e=-2.0, c_x=0.9, c_m=0.1, x_out=x_out,
                                                            x_in=x_in, in_scale=0.5),
        "sampler_step dpm++ order 2 (x_in)": lambda: K.sampler_step(eps, x, guidance=8.0, has_uncond=True, m_x=1.1, m_e=-0.4, c_x=0.9, c_m=0.2,
                                                                     c_h=[-0.1], hist=[h1], m_out=m_out, x_out=x_out, x_in=x_in),
        "sampler_step ddim eta=1 (x_in)": lambda: K.sampler_step(eps, x, guidance=8.0, has_uncond=True, m_x=1.1, m_e=-0.4, c_e=0.3, c_m=0.9, c_n=0.2,
                                                                  noise=noise, x_out=x_out, x_in=x_in),
    }
    for name, fn in cases.items():
        us = [_events(fn) for _ in range(3)]
        print(json.dumps({"kernel": name, "n": n, "dtype": str(dtype), "us_per_launch": [round(u, 2) for u in us]}), flush=True)


def loop_rates(steps=25):
    import bench
    from synfmc_amd import hip_ops as K
    from synfmc_amd import schedulers as S
    from synfmc_amd.models.pose_adaptor import features_to_video
    from synfmc_amd.pipelines.pipeline_animation_cm_om import CameraObjCtrlPipeline
    from synfmc_amd.util import stack_object_inputs
    device, dtype = torch.device("cuda", 0), torch.bfloat16
    unet, enc, ada = bench.build_models(device, dtype, "obj")
    clip, text2 = bench.synthetic_inputs(0, device)
    poses, masks = stack_object_inputs(clip["infos"], clip["masks"], device)
    with torch.no_grad():
        emb = K.plucker(clip["K"].to(device), clip["c2w"].to(device), bench.HEIGHT, bench.WIDTH, "unshuffle8", dtype)
        feats, m = K.omc_rasterize(poses, masks, "unshuffle8", dtype)
        traj = features_to_video(ada(feats, m), 1)
    samplers = {
        "ddim (default, cfg_ddim_kernel)": (S.DDIMScheduler(steps_offset=1, clip_sample=False, **SCHED), {}),
        "ddim eta=1": (S.DDIMScheduler(steps_offset=1, clip_sample=False, **SCHED), dict(eta=1.0, generator=torch.Generator("cuda").manual_seed(0))),
        "euler": (S.EulerDiscreteScheduler(**SCHED), {}),
        "euler ancestral": (S.EulerAncestralDiscreteScheduler(**SCHED), dict(generator=torch.Generator("cuda").manual_seed(0))),
        "dpm-solver++ order 2": (S.DPMSolverMultistepScheduler(solver_order=2, **SCHED), {}),
    }
    for name, (sch, extra) in samplers.items():
        pipe = CameraObjCtrlPipeline(None, None, None, unet, sch, enc)
        kw = dict(prompt=None, pose_embedding=emb, video_length=bench.FRAMES, traj_features=traj, height=bench.HEIGHT, width=bench.WIDTH,
                  num_inference_steps=steps, guidance_scale=8.0, prompt_embeds=text2.to(dtype), latents=clip["latents"].to(device),
                  output_type="latent", pose_embedding_unshuffled=True, **extra)
        pipe(**kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(**kw).videos
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"sampler": name, "steps": steps, "loop_s": round(dt, 4), "steps_per_s": round(steps / dt, 3),
                          "finite": bool(torch.isfinite(out).all())}), flush=True)
        del pipe


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--steps", type=int, default=25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    if a.kernel:
        kernel_times()
    if a.loop:
        loop_rates(a.steps)

"""What the MXFP8 feed-forward (`hip_ops.FP8_FF`, csrc/gemm_mxfp8.hip) costs next to the bf16 routes (profiles/mxfp8_ff.md).

    python tools/mxfp8_ff_rates.py --kernel      the feed-forward of each U-Net level at the bench clip, today's route against the new chain
    python tools/mxfp8_ff_rates.py --loop        the 25-step CameraObjCtrlPipeline loop at 16x320x512, hip_ops.FP8_FF off and on

One GPU process per command.  Nothing is compared with a figure set in advance: the reference of every number is the other leg of the same process.

--kernel   M = 81920 / 20480 / 5120 / 1280 rows at C = 320 / 640 / 1280 / 1280 (16x320x512 at CFG batch 2).  `FeedForward.forward_ln` with the switch
           off (today's route; where it returns None, `norm.skip` + the module as the callers do) and on, each captured in a HIP graph of one call and
           replayed: 4 warm-up replays, then device events around 40.  Legs alternated, `--repeats` (>= 3) runs each; every run is printed.  Also the
           three launches of the new chain one by one.  A level counts as faster only where the SLOWEST new run beats the FASTEST run of today's route.
           `hip_ops.MXFP8_FF_SLOWER` (the widths the predicate does not route) is cleared for the measurement: every level is timed.
--loop     `bench.py`'s `obj` model through `CameraObjCtrlPipeline`, 25 steps, CFG, captured graph, latents out.  Two pipelines over the same model, one
           per switch setting; a warm-up call each, then `--repeats` timed calls per leg, legs alternated.
Both print one JSON line at the end."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

FRAMES, HEIGHT, WIDTH = 16, 320, 512
LEVELS = ((81920, 320), (20480, 640), (5120, 1280), (1280, 1280))


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def rel_inf(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-30))


def graph_time(fn, warm=4, reps=40):
    """ms per call of `fn` as a captured graph of ONE call: `warm` replays, then device events around `reps` replays."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                   # (per-shape autotuning and one-time packs happen here, outside the capture)
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(warm):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_mode(repeats, levels):
    from synfmc_amd import hip_ops as K
    from synfmc_amd.models import layers as L
    dev, bf = "cuda", torch.bfloat16
    rows = []
    K.MXFP8_FF_SLOWER = ()                                # every level is measured, whatever the predicate routes today
    with torch.no_grad():
        for M, C in levels:
            torch.manual_seed(C + M)
            ff, norm = L.FeedForward(C), L.LayerNorm(C)
            for p in ff.parameters():
                p.normal_(0, p.shape[-1] ** -0.5 if p.ndim >= 2 else 0.2)
            norm.weight.normal_(1.0, 0.2)
            norm.bias.normal_(0, 0.2)
            ff, norm = ff.to(dev, bf).eval(), norm.to(dev, bf).eval()
            h = (torch.randn(M, C) * 1.2).to(dev, bf)

            def today():
                K.FP8_FF = False
                y = ff.forward_ln(h, norm, h)
                if y is None:
                    hh, n = norm.skip(h, defer=True)
                    y = ff(n, residual=hh)
                return y

            def new():
                K.FP8_FF = True
                try:
                    assert ff.mxfp8_route(h, h)
                    return ff.forward_ln(h, norm, h)
                finally:
                    K.FP8_FF = False
            a, b = new(), today()
            torch.cuda.synchronize()
            err = rel_inf(a, b)
            t_new, t_old = [], []
            for _ in range(repeats):
                t_old.append(round(graph_time(today), 4))
                t_new.append(round(graph_time(new), 4))
            # the three launches of the new chain, one by one
            proj, out = ff.net[0].proj, ff.net[2]
            w1q, w1s = K.mxfp8_pack_weight(proj.weight, geglu=True)
            w2q, w2s = K.mxfp8_pack_weight(out.weight)
            g32, b32 = norm.weight.float(), norm.bias.float()
            xq, xs = K.layernorm_mxfp8(h, g32, b32, norm.eps)
            mq, ms = K.linear_mxfp8(xq, xs, w1q, w1s, proj.bias, geglu=True)
            parts = {"layernorm_mxfp8": graph_time(lambda: K.layernorm_mxfp8(h, g32, b32, norm.eps)),
                     "geglu_gemm": graph_time(lambda: K.linear_mxfp8(xq, xs, w1q, w1s, proj.bias, geglu=True)),
                     "output_gemm": graph_time(lambda: K.linear_mxfp8(mq, ms, w2q, w2s, out.bias, h))}
            inner = 4 * C
            tf = {"geglu_gemm": 4.0 * M * inner * C / parts["geglu_gemm"] / 1e9, "output_gemm": 2.0 * M * inner * C / parts["output_gemm"] / 1e9}
            faster = max(t_new) < min(t_old)
            log(f"M={M} C={C}: today {t_old} ms   new {t_new} ms   slowest new {'<' if faster else '>='} fastest today   rel-inf new vs today {err:.2e}")
            log(f"      new chain by launch (ms): {({k: round(v, 4) for k, v in parts.items()})}   TFLOP/s: {({k: round(v, 1) for k, v in tf.items()})}")
            rows.append({"M": M, "C": C, "today_ms": t_old, "new_ms": t_new, "faster": bool(faster), "rel_inf_new_vs_today": err,
                         "new_launches_ms": {k: round(v, 4) for k, v in parts.items()}, "new_tflops": {k: round(v, 1) for k, v in tf.items()}})
    print(json.dumps({"mode": "kernel", "clip": f"{FRAMES}x{HEIGHT}x{WIDTH}", "rows": rows}), flush=True)


def loop_mode(repeats, steps):
    import bench
    from synfmc_amd import configs as CM
    from synfmc_amd import hip_ops as K
    from synfmc_amd.models.pose_adaptor import features_to_video
    from synfmc_amd.pipelines.pipeline_animation_cm_om import CameraObjCtrlPipeline
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.util import stack_object_inputs
    dev, dtype = torch.device("cuda", 0), torch.bfloat16
    torch.cuda.set_device(0)
    K.MXFP8_FF_SLOWER = ()                                # the loop with EVERY feed-forward on the new chain, whatever the predicate routes today
    unet, enc, ada = bench.build_models(dev, dtype, "obj")
    clip = CM.synthetic_clip(B=1, Fr=FRAMES, H=HEIGHT, W=WIDTH, n_obj=3, cross_dim=bench.CROSS_DIM, seed=1234)
    uncond = torch.randn(1, 77, bench.CROSS_DIM, generator=torch.Generator().manual_seed(99))
    text2 = torch.cat([uncond, clip["text"]]).to(dev, dtype)
    poses, masks = stack_object_inputs(clip["infos"], clip["masks"], dev)
    c2w, Kin = clip["c2w"].to(dev), clip["K"].to(dev)

    def make_sched():
        return DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    with torch.no_grad():
        feats, m = K.omc_rasterize(poses, masks, "unshuffle8", dtype)
        kw = dict(prompt=None, video_length=FRAMES, height=HEIGHT, width=WIDTH, num_inference_steps=steps, guidance_scale=8.0, prompt_embeds=text2,
                  latents=clip["latents"].to(dev), output_type="latent", pose_embedding=K.plucker(Kin, c2w, HEIGHT, WIDTH, "unshuffle8", dtype),
                  pose_embedding_unshuffled=True, traj_features=features_to_video(ada(feats, m), 1))
        pipes = {False: CameraObjCtrlPipeline(None, None, None, unet, make_sched(), enc), True: CameraObjCtrlPipeline(None, None, None, unet, make_sched(), enc)}

        def call(on, **over):
            K.FP8_FF = on
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipes[on](**{**kw, **over})
                torch.cuda.synchronize()
                return time.perf_counter() - t0, torch.as_tensor(out.videos)
            finally:
                K.FP8_FF = False
        outs = {}
        for on in (False, True):                          # warm-up: autotuning, per-clip packs, graph capture
            s, outs[on] = call(on)
            log(f"warm-up, switch {'on' if on else 'off'}: {s:.2f} s")
            assert torch.isfinite(outs[on]).all()
        runs = {False: [], True: []}
        for r in range(repeats):
            for on in (False, True):
                s, o = call(on)
                runs[on].append(round(s, 4))
                assert torch.equal(o, outs[on]), "a leg is not reproducible"
                log(f"repeat {r}, switch {'on' if on else 'off'}: {s:.4f} s  ({s / steps * 1e3:.2f} ms per step)")
        diff = rel_inf(outs[True], outs[False])
        counts = {}
        for on in (False, True):
            K.call_log = []
            try:
                call(on, num_inference_steps=1, use_graph=False)
            finally:
                log_, K.call_log = K.call_log, None
            counts["on" if on else "off"] = sum(1 for fam, _, _ in log_ if fam == "mxfp8")
    off, on_ = runs[False], runs[True]
    log(f"off: {off} s   on: {on_} s   slowest on - fastest off: {max(on_) - min(off):+.4f} s   latents on vs off rel-inf {diff:.3e}   mxfp8 launches per step {counts}")
    print(json.dumps({"mode": "loop", "clip": f"{FRAMES}x{HEIGHT}x{WIDTH}", "steps": steps, "off_s": off, "on_s": on_, "faster": bool(max(on_) < min(off)),
                      "latents_on_vs_off_rel_inf": diff, "mxfp8_launches_one_eager_step": counts}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per leg (at least 3)")
    ap.add_argument("--steps", type=int, default=25, help="--loop: denoising steps per call")
    ap.add_argument("--levels", type=str, default="", help="--kernel: a subset of the widths, e.g. 320,640")
    args = ap.parse_args()
    if args.kernel == args.loop:
        raise SystemExit("one of --kernel / --loop")
    if args.repeats < 3:
        raise SystemExit("--repeats: at least 3")
    if not torch.cuda.is_available():
        raise SystemExit("tools/mxfp8_ff_rates.py measures on the MI355X: there is nothing to time without one")
    levels = [lv for lv in LEVELS if not args.levels or str(lv[1]) in args.levels.split(",")]
    kernel_mode(args.repeats, levels) if args.kernel else loop_mode(args.repeats, args.steps)


if __name__ == "__main__":
    main()

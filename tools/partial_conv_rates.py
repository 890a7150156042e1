"""What the partial-tile launches of the halo convolutions cost next to the route each shape takes without them (profiles/partial_tiles.md).

    python tools/partial_conv_rates.py [--out rates.json]

One GPU process.  Nothing is compared with a figure set in advance: the reference of every number is the other leg of the same process.

1. The shapes.  `bench.py`'s `obj` model (full-width U-Net + CMC + OMC, bf16) runs ONE eager step of the CFG-batch-2 pipeline at 16x256x384 with
   `hip_ops.PARTIAL_TILES` on and every kind of partial launch routed, and every call of `hip_ops.conv3x3` is recorded: images, size, channels,
   epilogue operands, upsample, shortcut sources.  The 16x512x768 list is the same sites at twice the height and width (the network is
   convolutional: a traced step there would add nothing but its autotuning time).  Stride-2 sites and widths that are a multiple of 32 are dropped:
   nothing changes for them.
2. Per shape, per kind of partial launch that takes it ("halo": 10 x 32 tiles; "halo4": 320 pixels of row blocks; "halo_sc": the shortcut in
   conv2's reduction; "upfold_halo" / "upfold_halo4": the phase mode of the upsample sites): the PARENT leg is `hip_ops.conv3x3` with no kind routed
   -- with the switch on that is, launch for launch, what the parent commit runs (the autotuned ring / split-K / vendor arm, or conv_halo4's whole
   row blocks); for "halo_sc" the parent leg is the shortcut GEMM followed by the convolution with the residual in its epilogue, as
   `ResnetBlock2D.forward` runs them.  The PARTIAL leg routes that one kind.  Each leg is captured in a HIP graph of one call and replayed (4 warm-up
   replays, device events around 40); the legs alternate `--rounds` times behind one uncounted round.  Outputs of the two are compared (rel-inf) before timing.
3. The rule.  A kind is routed for a shape when the partial leg's median is below the parent leg's median by more than the larger min-max spread of
   the two legs; otherwise it is not, and the table says so.  `hip_ops.partial_conv_routed` restates the decisions in closed form; the last column of the
   table (`rule`) is what it answers for the shape, so a disagreement with `routed` is visible.
Prints the table to stderr and one JSON line to stdout."""
import argparse
import inspect
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

from tools.partial_tiles_rates import FRAMES, HEIGHT, WIDTH, graph_time, log, rel_inf

ALL_KINDS = frozenset(("halo", "halo_sc", "halo4", "upfold_halo", "upfold_halo4"))


def traced_shapes():
    """{signature: call count} of the `hip_ops.conv3x3` calls of one eager CFG step at 16x256x384.  signature = (n, h, w, cin, cout, temb, residual,
    upsample, shortcut channels (cs1, cs2) or None, emit_gn), h x w the INPUT size."""
    import bench
    from synfmc_amd import configs as CM
    from synfmc_amd import hip_ops as K
    from synfmc_amd.models.pose_adaptor import features_to_video
    from synfmc_amd.pipelines.pipeline_animation_cm_om import CameraObjCtrlPipeline
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.util import stack_object_inputs
    dev, dtype = torch.device("cuda", 0), torch.bfloat16
    unet, enc, ada = bench.build_models(dev, dtype, "obj")
    clip = CM.synthetic_clip(B=1, Fr=FRAMES, H=HEIGHT, W=WIDTH, n_obj=3, cross_dim=bench.CROSS_DIM, seed=1234)
    uncond = torch.randn(1, 77, bench.CROSS_DIM, generator=torch.Generator().manual_seed(99))
    text2 = torch.cat([uncond, clip["text"]]).to(dev, dtype)
    poses, masks = stack_object_inputs(clip["infos"], clip["masks"], dev)
    seen = {}
    real = K.conv3x3
    params = inspect.signature(real)

    def recording(*a, **kw):
        b = params.bind(*a, **kw)
        b.apply_defaults()
        x, w = b.arguments["x_nchw"], b.arguments["weight_cl"]
        sc = b.arguments["shortcut"]
        if x.is_cuda and x.dtype == torch.bfloat16 and tuple(b.arguments["stride"]) == (1, 1) and tuple(w.shape[2:]) == (3, 3):
            sig = (x.shape[0], x.shape[2], x.shape[3], x.shape[1], w.shape[0], b.arguments["temb"] is not None, b.arguments["residual_nchw"] is not None,
                   bool(b.arguments["upsample"]), None if sc is None else (sc[0].shape[1], 0 if sc[1] is None else sc[1].shape[1]), bool(b.arguments["emit_gn"]))
            seen[sig] = seen.get(sig, 0) + 1
        return real(*a, **kw)
    sched = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    K.conv3x3, K.PARTIAL_TILES, routed, K.PARTIAL_CONV_ROUTED, K.PARTIAL_CONV_RULES = recording, True, K.PARTIAL_CONV_ROUTED, ALL_KINDS, False
    try:
        with torch.no_grad():
            feats, m = K.omc_rasterize(poses, masks, "unshuffle8", dtype)
            CameraObjCtrlPipeline(None, None, None, unet, sched, enc)(
                prompt=None, video_length=FRAMES, height=HEIGHT, width=WIDTH, num_inference_steps=1, guidance_scale=8.0, prompt_embeds=text2,
                latents=clip["latents"].to(dev), output_type="latent", pose_embedding=K.plucker(clip["K"].to(dev), clip["c2w"].to(dev), HEIGHT, WIDTH, "unshuffle8", dtype),
                pose_embedding_unshuffled=True, traj_features=features_to_video(ada(feats, m), 1), use_graph=False)
        torch.cuda.synchronize()
    finally:
        K.conv3x3, K.PARTIAL_TILES, K.PARTIAL_CONV_ROUTED, K.PARTIAL_CONV_RULES = real, False, routed, True
    del unet, enc, ada
    torch.cuda.empty_cache()
    return seen


def kinds_for(sig):
    """The kinds of partial launch that could take the signature, by the library's own predicates."""
    from synfmc_amd import hip_ops as K
    L = K._lib.load()
    n, h, w, cin, cout, temb, res, ups, sc, emit = sig
    if sc is not None:
        return ["halo_sc"] if w % 32 and K.conv3x3_halo_sc_partial_supported(n, h, w, cin, cout, sc[0] + sc[1], sc[0]) else []
    if ups:
        if (w % 32 == 0 and cout % 160 == 0) or (w % 8 == 0 and cout % 80 == 0):      # a whole-tile fold takes the source
            return []
        return ([k for k, ok in (("upfold_halo", L.fmc_conv3x3_halo_fold_partial_supported(n, h, w, cin, cout)),
                                 ("upfold_halo4", w % 8 and L.fmc_conv3x3_halo4_fold_partial_supported(n, h, w, cin, cout, 0))) if ok])
    out = []
    if w % 32 and K.conv3x3_halo_partial_supported(n, h, w, cin, cin, cout, False):
        out.append("halo")
    if w % 8 and K.conv3x3_halo4_partial_supported(n, h, w, cin, cin, cout, False):
        out.append("halo4")
    return out


def measure(sig, kind, rounds):
    from synfmc_amd import hip_ops as K
    n, h, w, cin, cout, temb, res, ups, sc, emit = sig
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator().manual_seed(h * 1000 + w + cin)
    ho, wo = (2 * h, 2 * w) if ups else (h, w)
    nchw = lambda *shape: torch.randn(shape[0], shape[2], shape[3], shape[1], generator=g).to(dev, bf).permute(0, 3, 1, 2)
    x = nchw(n, cin, h, w)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).to(dev, bf).contiguous(memory_format=torch.channels_last)
    bias = torch.randn(cout, generator=g).to(dev, bf)
    t = torch.randn(n, cout, generator=g).to(dev, bf) if temb else None
    r = nchw(n, cout, ho, wo) if res else None
    if sc is not None:
        xs, xs2 = nchw(n, sc[0], h, w), (nchw(n, sc[1], h, w) if sc[1] else None)
        wsc = (torch.randn(cout, sc[0] + sc[1], generator=g) * (sc[0] + sc[1]) ** -0.5).to(dev, bf)
        bsc = torch.randn(cout, generator=g).to(dev, bf)
        flat = lambda v: None if v is None else v.permute(0, 2, 3, 1).reshape(n, h * w, -1)

        def parent():                                      # the shortcut GEMM, then conv2 with the residual in its epilogue (emit_gn as the block asks)
            s = K.linear(flat(xs), wsc, bsc, x2=flat(xs2)).view(n, h, w, cout).permute(0, 3, 1, 2)
            return K.conv3x3(x, wt, bias, residual_nchw=s, emit_gn=emit)

        def partial():
            return K.conv3x3(x, wt, bias, emit_gn=emit, shortcut=(xs, xs2, wsc, bsc))
    else:
        def parent():
            return K.conv3x3(x, wt, bias, t, r, upsample=ups, emit_gn=emit)
        partial = parent

    def leg(fn, routed):
        def run():
            K.PARTIAL_TILES, keep, K.PARTIAL_CONV_ROUTED, K.PARTIAL_CONV_RULES = True, K.PARTIAL_CONV_ROUTED, routed, False
            try:
                return fn()
            finally:
                K.PARTIAL_TILES, K.PARTIAL_CONV_ROUTED, K.PARTIAL_CONV_RULES = False, keep, True
        return run
    legs = {"parent": leg(parent, frozenset()), "partial": leg(partial, frozenset((kind,)))}
    with torch.no_grad():
        routes = {}
        for name, fn in legs.items():
            fn()                                           # (autotuning and one-time packs: not part of the route)
            K.call_log = []
            try:
                out = fn()
            finally:
                lg, K.call_log = K.call_log, None
            routes[name] = [f + (" partial" if any(e == "partial" or (isinstance(e, tuple) and e and e[0] == "partial") for e in s) else "") for f, s, _ in lg]
            legs[name].out = out
        torch.cuda.synchronize()
        if not any("partial" in f for f in routes["partial"]):      # (too few workgroups for `CONV_HALO_MIN_TILES`: the dispatch keeps the parent's route)
            log(f"   {sig} [{kind}]: the dispatch does not route this shape ({routes['partial']})")
            return None
        err = rel_inf(legs["partial"].out, legs["parent"].out)
        assert err < 2e-2, (sig, kind, err)
        times = {"parent": [], "partial": []}
        for i in range(rounds + 1):                        # (round 0 is not counted: the first graph of a shape reads 5 - 10 % high, clocks and caches settling)
            for name, fn in legs.items():
                ms = graph_time(fn)
                if i:
                    times[name].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = max(max(v) - min(v) for v in times.values())
    row = {"shape": list(sig[:5]), "temb": temb, "residual": res, "upsample": ups, "shortcut": sc, "emit_gn": emit, "kind": kind, "parent_route": routes["parent"],
           "parent_ms": [round(v, 4) for v in times["parent"]], "partial_ms": [round(v, 4) for v in times["partial"]],
           "parent_median_ms": round(med["parent"], 4), "partial_median_ms": round(med["partial"], 4), "spread_ms": round(spread, 4),
           "routed": bool(med["parent"] - med["partial"] > spread), "rule": K.partial_conv_routed(kind, n, h, w, cin, cout), "rel_inf": err}
    log(f"   n={n} {h}x{w} {cin}->{cout}{' +temb' if temb else ''}{' +res' if res else ''}{' ups' if ups else ''}{f' sc {sc}' if sc else ''} [{kind}]: "
        f"parent {routes['parent']} {row['parent_ms']} ms, partial {row['partial_ms']} ms, spread {spread:.4f} -> "
        f"{'ROUTED' if row['routed'] else 'not routed'} (parent / partial {med['parent'] / med['partial']:.2f})")
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the two legs per shape")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/partial_conv_rates.py measures on the MI355X: there is nothing to time without one")
    torch.cuda.set_device(0)
    seen = traced_shapes()
    log(f"{len(seen)} stride-1 3x3 convolution signatures in one eager step at {FRAMES}x{HEIGHT}x{WIDTH}")
    result = {"mode": "conv", "rounds": args.rounds, "clips": {}}
    for scale, clip in ((1, f"{FRAMES}x{HEIGHT}x{WIDTH}"), (2, f"{FRAMES}x{2 * HEIGHT}x{2 * WIDTH}")):
        log(f"---- {clip}")
        rows = []
        for sig, count in sorted(seen.items(), key=lambda kv: (-kv[0][2], kv[0][3], kv[0][4], str(kv[0]))):
            s = (sig[0], sig[1] * scale, sig[2] * scale) + sig[3:]
            for kind in kinds_for(s):
                row = measure(s, kind, args.rounds)
                if row is not None:
                    row["calls_per_step"] = count
                    rows.append(row)
        result["clips"][clip] = rows
        saved = sum((r["parent_median_ms"] - r["partial_median_ms"]) * r["calls_per_step"] for r in rows if r["routed"])
        log(f"{clip}: {sum(r['routed'] for r in rows)} of {len(rows)} (shape, kind) pairs routed; their launches are {saved:.3f} ms per step shorter")
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()

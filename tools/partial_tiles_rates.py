"""What the partial-tile forms of the fused attention blocks and of the feed-forward chain cost at 16x256x384 (profiles/partial_tiles.md).

    python tools/partial_tiles_rates.py --kernel      the new launches next to the un-fused chain each replaces (--legs attn | ff | all)
    python tools/partial_tiles_rates.py --loop        the 25-step CameraObjCtrlPipeline loop, hip_ops.PARTIAL_TILES off and on (--switch off | on | both)

One GPU process per command.  Nothing is compared with a figure set in advance: the reference of every number is the other leg of the same
process.

--kernel   At the shapes of a 16x256x384 clip at CFG batch 2 -- temporal `[2, 16, 1536, 320]` (Camera-Adapter merge block and plain block) and
           `[2, 16, 384, 640]`, text cross-attention 32 images x 1536 rows x 320 and 32 x 384 x 640 with 16 images per text and 77 text tokens --
           the fused launch (`partial_tiles=True`) and the chain of launches the model runs in its place (LayerNorm, [merge GEMM,] q | k | v or
           to_q GEMM, attention, out-projection + residual; called through the same modules as the model calls them) are each captured in a HIP
           graph of one call and replayed: 4 warm-up replays, then device events around 40.  A graph replay leaves the launches back to back, so the
           chain's figure is the sum of its launches and not the host's enqueue time.  Outputs of the two are compared (rel-inf) before timing.
           --legs ff: the feed-forward at the same clip, M = 49152 rows x 320 and 12288 x 640 (`FeedForward.forward_ln` with the switch on): LayerNorm +
           GEGLU projection (`geglu_ln_pipe(..., partial_tiles=True)`) next to `norm.skip` + the GEGLU module; `linear_from_blocked` / `ff_tail`
           (`partial_tiles=True`) next to the output projection (+ proj_out) on the row-major intermediate; and the whole feed-forward both ways.
--loop     `bench.py`'s `obj` model (full-width U-Net + CMC + OMC, bf16) through `CameraObjCtrlPipeline`, 25 steps, CFG, captured graph, latents
           out, at 16x256x384.  Two pipelines over the same model, one called with the switch off and one with it on (a pipeline keeps one graph per
           switch setting); a warm-up call each, then `--repeats` timed calls per leg, legs alternated; every run is printed.  Then one eager
           one-step call per leg with `hip_ops.call_log` on: the launches of the GEMM-shaped front-ends by family, so that what stays un-fused at
           this size is listed.
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

FRAMES, HEIGHT, WIDTH = 16, 256, 384


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


def _init(mod, norms, seed):
    torch.manual_seed(seed)
    with torch.no_grad():
        for p in mod.parameters():
            p.normal_(0, p.shape[-1] ** -0.5 if p.ndim >= 2 else 0.2)
        for n in norms:
            n.weight.add_(1.0)


def attn_legs():
    from synfmc_amd import hip_ops as K
    from synfmc_amd.models import layers as L
    from synfmc_amd.models import motion_module as MM
    from synfmc_amd.models.attention_processor import AttnProcessor, PoseAdaptorAttnProcessor
    dev, bf = "cuda", torch.bfloat16
    rows = []
    with torch.no_grad():
        for C, hw in ((320, (HEIGHT // 8) * (WIDTH // 8)), (640, (HEIGHT // 16) * (WIDTH // 16))):
            # ---- temporal: block 0 carries the Camera-Adapter merge, block 1 is plain ----
            blk = MM.TemporalTransformerBlock(dim=C, num_attention_heads=8, attention_head_dim=C // 8, attention_block_types=("Temporal_Self", "Temporal_Self"),
                                              temporal_position_encoding=True, temporal_position_encoding_max_len=32)
            proc = PoseAdaptorAttnProcessor(hidden_size=C, pose_feature_dim=C, query_condition=True, key_value_condition=True, scale=0.8)
            blk.attention_blocks[0].set_processor(proc)
            blk.attention_blocks[1].set_processor(AttnProcessor())
            _init(blk, list(blk.norms) + [blk.ff_norm], 3)
            blk = blk.to(dev, bf).eval()
            x = (torch.randn(2, FRAMES, hw, C) * 1.2).to(dev, bf)
            pose = torch.randn(2, FRAMES, hw, C).to(dev, bf)
            assert not K.temporal_block_supported(x, 8) and K.temporal_block_partial_supported(x, 8)
            for i, merge in ((0, True), (1, False)):
                attn, norm = blk.attention_blocks[i], blk.norms[i]
                kw = {"pose_feature": pose} if merge else {}
                gamma, bpe = blk._fused_constants(i, FRAMES)
                w_qkv, w_o = blk._fused_weights(i, None, 1.0)
                fkw = {}
                if merge:
                    wm, bm = proc.merge_wb(x)
                    fkw = dict(w_merge_tm=blk._merge_packed(proc, wm), pose_term=proc._pose_term(pose, wm, bm, proc.scale), merge_scale=proc.scale)

                def fused():
                    return K.temporal_block(x, gamma, bpe, norm.eps, w_qkv, w_o, attn.to_out[0].bias, attn.scale, partial_tiles=True, **fkw)

                def chain():
                    attn.__dict__["_next_ln"], attn.__dict__["_lazy_res"] = None, False
                    h, n = norm.skip(x, pe=attn.pos_encoder.table(), pe_inner=hw, pe_frames=FRAMES)
                    return attn(n, encoder_hidden_states=None, attention_mask=None, _pe_applied=True, _residual=h, **kw)
                rows.append(_compare(f"temporal C={C} [2,16,{hw},{C}] {'merge' if merge else 'plain'}", fused, chain))
            del blk
            # ---- text cross-attention: 32 images, 16 per text, 77 text tokens ----
            sb = L.BasicTransformerBlock(C, 8, C // 8, cross_attention_dim=768)
            _init(sb, (sb.norm1, sb.norm2, sb.norm3), 5)
            sb = sb.to(dev, bf).eval()
            h3 = (torch.randn(2 * FRAMES, hw, C) * 1.2).to(dev, bf)
            text = torch.randn(2, 77, 768).to(dev, bf)
            assert not K.xattn_block_supported(h3, 77, 8) and K.xattn_block_partial_supported(h3, 77, 8)
            sb.prepare_text(text)

            def fused_x():
                return sb._xattn_fused(h3, text, {}, partial=True)

            def chain_x():
                sb.attn2.__dict__["_next_ln"], sb.attn2.__dict__["_lazy_res"] = None, False
                hh, n = sb.norm2.skip(h3, defer=True)
                return sb.attn2(n, encoder_hidden_states=text, attention_mask=None, _residual=hh)
            rows.append(_compare(f"xattn C={C} 32 x {hw} x {C}, 16 per text, S=77", fused_x, chain_x))
            del sb
    return rows


def ff_legs():
    """The feed-forward legs of --kernel: what `FeedForward.forward_ln` launches on the partial route next to what the model runs at these row counts without it."""
    from synfmc_amd import hip_ops as K
    from synfmc_amd.models import layers as L
    dev, bf = "cuda", torch.bfloat16
    rows = []
    with torch.no_grad():
        for C, hw in ((320, (HEIGHT // 8) * (WIDTH // 8)), (640, (HEIGHT // 16) * (WIDTH // 16))):
            M = 2 * FRAMES * hw
            ff, norm, po = L.FeedForward(C), L.LayerNorm(C), L.Linear(C, C)
            _init(ff, (), 7)
            _init(norm, (norm,), 8)
            _init(po, (), 9)
            ff, norm, po = ff.to(dev, bf).eval(), norm.to(dev, bf).eval(), po.to(dev, bf).eval()
            h = (torch.randn(2 * FRAMES, hw, C) * 1.2).to(dev, bf)
            x = torch.randn(2 * FRAMES, hw, C).to(dev, bf)
            w = ff.net[0].proj.weight
            assert not K.geglu_ln_direct_ok(h, w) and K.geglu_ln_partial_ok(h, w)
            var = K.geglu_pipe_partial_variant(C)
            frag = K.pack_geglu_frag(w, 16 if var == 1 else 32)
            g, b = L.f32_param(norm, "weight"), L.f32_param(norm, "bias")
            blocked = K.geglu_direct_blocked_partial_ok(h, ff.net[2].weight, h)

            def on(fn):
                def run():
                    K.PARTIAL_TILES = True
                    try:
                        return fn()
                    finally:
                        K.PARTIAL_TILES = False
                return run

            def chain_proj():
                hh, n = norm.skip(h, defer=True)
                return ff.net[0](n)

            def chain_ff():
                hh, n = norm.skip(h, defer=True)
                return ff(n, residual=hh)
            mid_rm = chain_proj()
            rows.append(_compare(f"ff C={C} M={M}: LayerNorm + GEGLU projection (pipe, variant {var})",
                                 lambda: K.geglu_ln_pipe(h, g, b, norm.eps, frag, ff.net[0].proj.bias, w.shape[0] // 2, variant=var, partial_tiles=True), chain_proj))
            if blocked:
                mid = K.geglu_ln_pipe(h, g, b, norm.eps, frag, ff.net[0].proj.bias, w.shape[0] // 2, blocked=True, variant=var, partial_tiles=True)
                out = ff.net[2]
                rows.append(_compare(f"ff C={C} M={M}: output projection + residual (linear_from_blocked)",
                                     lambda: K.linear_from_blocked(mid, out.weight, out.bias, h, partial_tiles=True), lambda: out(mid_rm, residual=h)))
                if K.ff_tail_partial_ok(h, out.weight, po.weight, x):
                    wc, bc = ff._tail_weights(po.weight, po.bias)
                    rows.append(_compare(f"ff C={C} M={M}: output projection + proj_out + residuals (ff_tail)",
                                         lambda: K.ff_tail(mid, h, wc, bc, x, partial_tiles=True), lambda: po(out(mid_rm, residual=h), residual=x)))
                    pipe = lambda blk: K.geglu_ln_pipe(h, g, b, norm.eps, frag, ff.net[0].proj.bias, w.shape[0] // 2, blocked=blk, variant=var, partial_tiles=True)
                    rows.append(_compare(f"ff C={C} M={M}: pipe (tile-major) + ff_tail | pipe (row-major) + the two projections",
                                         lambda: K.ff_tail(pipe(True), h, wc, bc, x, partial_tiles=True), lambda: po(out(pipe(False), residual=h), residual=x)))
                    rows.append(_compare(f"ff C={C} M={M}: whole feed-forward + proj_out", on(lambda: ff.forward_ln(h, norm, h, tail=(po.weight, po.bias, x, 0))),
                                         lambda: po(chain_ff(), residual=x)))
            rows.append(_compare(f"ff C={C} M={M}: whole feed-forward", on(lambda: ff.forward_ln(h, norm, h)), chain_ff))
    return rows


def kernel_mode(legs):
    rows = (attn_legs() if legs in ("attn", "all") else []) + (ff_legs() if legs in ("ff", "all") else [])
    for r in rows:
        log(f"{r['case']:58s} fused {r['fused_ms']:.4f} ms   chain {r['chain_ms']:.4f} ms   chain / fused {r['chain_ms'] / r['fused_ms']:.2f}   "
            f"rel-inf fused vs chain {r['rel_inf']:.2e}")
    print(json.dumps({"mode": "kernel", "clip": f"{FRAMES}x{HEIGHT}x{WIDTH}", "rows": rows}), flush=True)


def _compare(case, fused, chain):
    a, b = fused(), chain()
    torch.cuda.synchronize()
    err = rel_inf(a, b)
    assert err < 2e-2, (case, err)
    # chain, fused, chain, fused: the two figures of a leg show its own spread
    t = [graph_time(chain), graph_time(fused), graph_time(chain), graph_time(fused)]
    log(f"   {case}: chain {t[0]:.4f} / {t[2]:.4f} ms, fused {t[1]:.4f} / {t[3]:.4f} ms")
    return {"case": case, "fused_ms": round(min(t[1], t[3]), 4), "chain_ms": round(min(t[0], t[2]), 4), "fused_runs_ms": [round(t[1], 4), round(t[3], 4)],
            "chain_runs_ms": [round(t[0], 4), round(t[2], 4)], "rel_inf": err}


def loop_mode(repeats, steps, switch="both"):
    import bench
    from synfmc_amd import configs as CM
    from synfmc_amd import hip_ops as K
    from synfmc_amd.models.pose_adaptor import features_to_video
    from synfmc_amd.pipelines.pipeline_animation_cm_om import CameraObjCtrlPipeline
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.util import stack_object_inputs
    dev, dtype = torch.device("cuda", 0), torch.bfloat16
    torch.cuda.set_device(0)
    unet, enc, ada = bench.build_models(dev, dtype, "obj")
    clip = CM.synthetic_clip(B=1, Fr=FRAMES, H=HEIGHT, W=WIDTH, n_obj=3, cross_dim=bench.CROSS_DIM, seed=1234)
    uncond = torch.randn(1, 77, bench.CROSS_DIM, generator=torch.Generator().manual_seed(99))
    text2 = torch.cat([uncond, clip["text"]]).to(dev, dtype)
    poses, masks = stack_object_inputs(clip["infos"], clip["masks"], dev)
    c2w, Kin = clip["c2w"].to(dev), clip["K"].to(dev)

    def make_sched():
        s = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
        return s
    with torch.no_grad():
        feats, m = K.omc_rasterize(poses, masks, "unshuffle8", dtype)
        kw = dict(prompt=None, video_length=FRAMES, height=HEIGHT, width=WIDTH, num_inference_steps=steps, guidance_scale=8.0, prompt_embeds=text2,
                  latents=clip["latents"].to(dev), output_type="latent", pose_embedding=K.plucker(Kin, c2w, HEIGHT, WIDTH, "unshuffle8", dtype),
                  pose_embedding_unshuffled=True, traj_features=features_to_video(ada(feats, m), 1))
        pipes = {False: CameraObjCtrlPipeline(None, None, None, unet, make_sched(), enc), True: CameraObjCtrlPipeline(None, None, None, unet, make_sched(), enc)}

        def call(on, **over):
            K.PARTIAL_TILES = on
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipes[on](**{**kw, **over})
                torch.cuda.synchronize()
                return time.perf_counter() - t0, torch.as_tensor(out.videos)
            finally:
                K.PARTIAL_TILES = False
        legs = {"off": (False,), "on": (True,), "both": (False, True)}[switch]
        outs = {}
        for on in legs:                                   # warm-up: autotuning, per-clip packs, graph capture
            s, outs[on] = call(on)
            log(f"warm-up, switch {'on' if on else 'off'}: {s:.2f} s")
            assert torch.isfinite(outs[on]).all()
        runs = {False: [], True: []}
        for r in range(repeats):
            for on in legs:
                s, o = call(on)
                runs[on].append(round(s, 4))
                assert torch.equal(o, outs[on]), "a leg is not reproducible"
                log(f"repeat {r}, switch {'on' if on else 'off'}: {s:.4f} s  ({s / steps * 1e3:.2f} ms per step)")
        diff = rel_inf(outs[True], outs[False]) if len(legs) == 2 else None
        # ---- one eager step per leg: the launches of the GEMM-shaped front-ends by family ----
        tables = {}
        for on in legs:
            K.call_log = []
            try:
                call(on, num_inference_steps=1, use_graph=False)
            finally:
                log_, K.call_log = K.call_log, None
            fam = {}
            for family, shape, _ in log_:
                key = family if family != "fused_block" else f"fused_block {shape[0]} C={shape[2]}" + (" partial" if any(isinstance(s, tuple) for s in shape) else "")
                fam[key] = fam.get(key, 0) + 1
            tables["on" if on else "off"] = dict(sorted(fam.items()))
            log(f"one eager step, switch {'on' if on else 'off'}: {tables['on' if on else 'off']}")
    off, on_ = runs[False], runs[True]
    if len(legs) == 1:                                     # one leg (compared across processes: this commit against its parent, both with the switch on)
        import hashlib
        digest = hashlib.sha256(outs[legs[0]].float().cpu().numpy().tobytes()).hexdigest()[:16]
        log(f"switch {switch}: {runs[legs[0]]} s   latents sha256 {digest}")
        print(json.dumps({"mode": "loop", "clip": f"{FRAMES}x{HEIGHT}x{WIDTH}", "steps": steps, f"{switch}_s": runs[legs[0]], "latents_sha256_16": digest,
                          "launches_one_eager_step": tables}), flush=True)
        return
    spread = max(off) - min(off)
    log(f"off: {off} s (spread {spread:.4f} s)   on: {on_} s   slowest on - fastest off: {max(on_) - min(off):+.4f} s   latents on vs off rel-inf {diff:.3e}")
    print(json.dumps({"mode": "loop", "clip": f"{FRAMES}x{HEIGHT}x{WIDTH}", "steps": steps, "off_s": off, "on_s": on_, "off_spread_s": round(spread, 4),
                      "faster_by_more_than_the_off_spread": bool(min(off) - max(on_) > spread), "latents_on_vs_off_rel_inf": diff,
                      "launches_one_eager_step": tables}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--repeats", type=int, default=3, help="--loop: timed calls per leg")
    ap.add_argument("--steps", type=int, default=25, help="--loop: denoising steps per call")
    ap.add_argument("--legs", choices=("attn", "ff", "all"), default="all", help="--kernel: the fused attention blocks, the feed-forward, or both")
    ap.add_argument("--switch", choices=("off", "on", "both"), default="both", help="--loop: which setting of hip_ops.PARTIAL_TILES to run")
    args = ap.parse_args()
    if args.kernel == args.loop:
        raise SystemExit("one of --kernel / --loop")
    if not torch.cuda.is_available():
        raise SystemExit("tools/partial_tiles_rates.py measures on the MI355X: there is nothing to time without one")
    kernel_mode(args.legs) if args.kernel else loop_mode(args.repeats, args.steps, args.switch)


if __name__ == "__main__":
    main()

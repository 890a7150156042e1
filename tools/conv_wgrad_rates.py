"""The weight gradient of the trainable 3x3 convolutions: the old chain next to the direct fp32 kernel (profiles/conv_wgrad.md).

    python tools/conv_wgrad_rates.py [--reps 50 --runs 3]

Shapes: the trained 3x3 / stride 1 convolutions of the Camera Encoder and of the OMC Adapter for one clip of 16 frames at 256 x 384 --
`encoder_conv_in` 384 -> 320 resp. the Adapter's `conv_in` 832 -> 320 at 32 x 48, and `block1` of every `ResnetBlock`: 320 -> 320 at
32 x 48, 640 -> 640 at 16 x 24, 1280 -> 1280 at 8 x 12 and at 4 x 6 (two blocks per level: nine convolutions per adapter).
  old: `hip_ops.conv3x3_weight_grad(x, dy).to(torch.float32)` -- two layout passes, three split-K GEMMs, a stack, a cast;
  new: `hip_ops.conv3x3_wgrad(x, dy)` -- one launch, plus its combine where the pixel reduction is split.
Each leg: 5 warm-up calls, then device events around `--reps` back-to-back calls; the legs alternate old, new, old, new, ... `--runs` times
each, and every run is printed.  The calls are eager, as in a training step: at the small shapes the old chain's figure is the host issuing
its eight launches and allocations, not the device running them.  The spread of a leg is max - min over its runs.  The two results are
compared (rel-inf against float64 on the same operands) before timing.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

FRAMES = 16
# (name, Cin, Cout, H, W, convolutions of that shape in the encoder, in the OMC Adapter)
SHAPES = [("encoder conv_in", 384, 320, 32, 48, 1, 0), ("OMC conv_in", 832, 320, 32, 48, 0, 1), ("block1 level 0", 320, 320, 32, 48, 2, 2),
          ("block1 level 1", 640, 640, 16, 24, 2, 2), ("block1 level 2", 1280, 1280, 8, 12, 2, 2), ("block1 level 3", 1280, 1280, 4, 6, 2, 2)]


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def event_time(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def reference(x, dy):
    """float64 dW on the device: nine pixel-reduction products."""
    n, H, W, cin = x.shape
    xp = torch.zeros(n, H + 2, W + 2, cin, dtype=torch.float64, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x.double()
    d = dy.double().reshape(-1, dy.shape[-1])
    out = torch.empty(dy.shape[-1], cin, 3, 3, dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            out[:, :, ky, kx] = d.t() @ xp[:, ky:ky + H, kx:kx + W].reshape(-1, cin)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/conv_wgrad_rates.py measures on the MI355X: there is nothing to time without one")
    from synfmc_amd import hip_ops as K
    rows = []
    for name, cin, cout, H, W, n_enc, n_omc in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(cin + H)
        x = torch.randn(FRAMES, H, W, cin, device="cuda", generator=g).to(torch.bfloat16)
        dy = torch.randn(FRAMES, H, W, cout, device="cuda", generator=g).to(torch.bfloat16)
        old = lambda: K.conv3x3_weight_grad(x, dy).to(torch.float32)
        new = lambda: K.conv3x3_wgrad(x, dy)
        ref = reference(x, dy)
        err = {k: float((f().double() - ref).abs().max() / ref.abs().max()) for k, f in (("old", old), ("new", new))}
        del ref
        t = {"old": [], "new": []}
        for _ in range(args.runs):
            for k, f in (("old", old), ("new", new)):
                t[k].append(round(event_time(f, args.reps), 4))
        flops = 2.0 * FRAMES * H * W * 9 * cin * cout
        spread = max(t["old"]) - min(t["old"])
        row = dict(case=name, cin=cin, cout=cout, hw=[H, W], encoder_convs=n_enc, omc_convs=n_omc, old_ms=t["old"], new_ms=t["new"],
                   old_spread_ms=round(spread, 4), new_slower_than_old_by_more_than_its_spread=bool(min(t["new"]) - min(t["old"]) > spread),
                   new_tflops=round(flops / min(t["new"]) / 1e9, 1), rel_inf_vs_float64=err)
        rows.append(row)
        log(f"{name:18s} {cin:4d} -> {cout:4d} at {H}x{W}: old {t['old']} ms, new {t['new']} ms, new {row['new_tflops']} TFLOP/s; "
            f"rel-inf vs float64 old {err['old']:.2e} new {err['new']:.2e}")
    per = {k: {leg: round(sum(min(r[f"{leg}_ms"]) * r[f"{k}_convs"] for r in rows), 4) for leg in ("old", "new")} for k in ("encoder", "omc")}
    log(f"nine convolutions per adapter, ms: {per}")
    print(json.dumps({"tool": "conv_wgrad_rates", "frames": FRAMES, "reps": args.reps, "rows": rows, "nine_convs_ms": per}), flush=True)


if __name__ == "__main__":
    main()

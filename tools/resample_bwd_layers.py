"""Forward + backward of the frozen resampling convolutions and conv_out of one training clip, layer by layer: the own backward-data
(csrc/conv_resample_bwd.hip; conv_out: the stride-1 kernel on zero-padded channels) against FMC_RESAMPLE_BWD=0 (F.interpolate / F.conv2d and
torch's autograd) on the same build, alternating.  Every (layer, path) is captured once into a graph -- as the one-graph training step runs it --
and a timed window is `--replays` replays between two device events; `--rounds` windows per path, A B A B ...; the median and the spread are
printed, one JSON line per layer (profiles/resample_backward.md).

    python tools/resample_bwd_layers.py --clip 16x256x384 [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def layers_of(clip):
    f, hp, wp = (int(v) for v in clip.split("x"))
    h, w = hp // 8, wp // 8
    out = []
    for lvl, c in enumerate((320, 640, 1280)):                       # Downsample2D of down blocks 0..2
        out.append(("down", f, h >> lvl, w >> lvl, c, c))
    for lvl, c in ((3, 1280), (2, 1280), (1, 640)):                 # Upsample2D of up blocks 0..2 (source sizes)
        out.append(("up", f, h >> lvl, w >> lvl, c, c))
    out.append(("edge", f, h, w, 320, 4))                            # conv_out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip", default="16x256x384")
    ap.add_argument("--replays", type=int, default=1000)      # windows of 0.1 .. 1 s
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from synfmc_amd import hip_ops as K
    from synfmc_amd.models import layers as L
    bf16 = torch.bfloat16
    lines = []
    for kind, n, h, w, cin, cout in layers_of(args.clip):
        torch.manual_seed(1)
        m = {"down": lambda: L.Downsample2D(cin, use_conv=True, out_channels=cout), "up": lambda: L.Upsample2D(cin, use_conv=True, out_channels=cout),
             "edge": lambda: L.Conv2d(cin, cout, 3, padding=1)}[kind]().to("cuda", bf16).requires_grad_(False)
        x = torch.randn(n, h, w, cin, device="cuda").to(bf16).permute(0, 3, 1, 2).requires_grad_(True)
        with torch.no_grad():
            y0 = m(x)
        dy = torch.randn(y0.shape[0], y0.shape[2], y0.shape[3], y0.shape[1], device="cuda").to(bf16).permute(0, 3, 1, 2)

        def step():
            (gx,) = torch.autograd.grad(m(x), x, dy)
            return gx
        graphs, grads = {}, {}
        for own in (True, False):
            K.RESAMPLE_BWD = own
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                grads[own] = step()
            graphs[own] = g
        K.RESAMPLE_BWD = True
        times = {True: [], False: []}
        for _ in range(args.rounds):
            for own in (True, False):
                graphs[own].replay()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.replays):
                    graphs[own].replay()
                e1.record()
                torch.cuda.synchronize()
                times[own].append(e0.elapsed_time(e1) * 1e3 / args.replays)
        diff = float((grads[True].float() - grads[False].float()).abs().max() / grads[False].float().abs().max())
        line = dict(clip=args.clip, layer=kind, n=n, h=h, w=w, cin=cin, cout=cout,
                    own_us=round(statistics.median(times[True]), 1), own_min_max=[round(min(times[True]), 1), round(max(times[True]), 1)],
                    parent_us=round(statistics.median(times[False]), 1), parent_min_max=[round(min(times[False]), 1), round(max(times[False]), 1)],
                    grad_rel_inf_between_paths=float("%.3g" % diff))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

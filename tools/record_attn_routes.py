"""Record which kernels the attention entry points launch, from the device, into tests/golden/attn_routes.json.

    python tools/record_attn_routes.py [--commit HASH] [--out FILE]       record (on the MI355X, at the commit whose routes are to be kept)
    python tools/record_attn_routes.py --check                            the same trace on the current tree, compared with the file

Every case of the existing tables is launched once under `rocprofv3 --kernel-trace`: `attn_fwd_common.all_cases()`, the shapes of `attn_bwd_common`
(kv trainable and frozen) and `temporal_bwd_common`, and the four temporal entry points (the fp8 pair among them) at the clip lengths.  All of these run with
the switches at their defaults in ONE child process; each arm of `attn_fwd_common.SWITCH_ARMS` gets a child of its own, because csrc/spatial_attn.hip
reads its `FMC_SA_*` switches once per process.  The children run one after another, each under its own `timeout`; a child that fails ends the run
and nothing further is started.  The child launches `fmc_fp8_scales_roll` between two cases: its one-workgroup kernel is what separates the cases in
the trace.  Kept per case: the ordered (kernel name, grid in work-items, workgroup, LDS bytes) of the library's kernels (torch's own are dropped); the LDS
figure is the trace's `LDS_Block_Size`, which on this profiler holds the kernel's static allocation only.

tests/test_attn_routes.py (CPU) holds `expected_kernel` / `temporal_kernel` of tests/attn_fwd_common.py to the traced names."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_routes.json")
CLIP_LENGTHS = (1, 7, 8, 12, 15, 16, 17, 24, 25, 31, 32)
SEPARATOR = "fp8_scales_roll_kernel"
CHILD_SECONDS = 420


def child(arm, out):
    """Run the cases of `arm` ("default" or an index into SWITCH_ARMS), a separator launch after each, and write their labels in order."""
    import torch
    from synfmc_amd import hip_ops as K
    from tests import attn_bwd_common as AB
    from tests import attn_fwd_common as A
    from tests import clip_lengths_common as CL
    from tests import temporal_bwd_common as TB
    sep = [torch.zeros(3, device="cuda") for _ in range(3)]
    labels = []

    def done(label):
        torch.cuda.synchronize()
        K._lib.check(K._lib.load().fmc_fp8_scales_roll(sep[0].data_ptr(), sep[1].data_ptr(), sep[2].data_ptr(), 1.0, K._stream()), "separator")
        labels.append(label)
        A.inputs.cache_clear()

    def forward(c):
        d = A.inputs(c, "exact")
        bufs = {n: t.cuda() for n, t in A.pack(c, d).items()}
        if c.abi == "fp8":
            K._temporal_fp8_raw(bufs["qkv"], torch.tensor(A.FP8_SCALES, dtype=torch.float32, device="cuda"), c.H, d["scale"])
            return
        q, k, v = A.views(c, bufs)
        if c.abi == "spatial":
            K.spatial_attention(q, k, v, c.H, d["scale"], return_lse=True)
        elif c.abi == "temporal":
            K.temporal_attention(q, k, v, c.H, d["scale"])
        else:
            K.attention(q, k, v, c.H, d["scale"], causal=c.causal, key_keep=d["keep"].cuda() if c.keep else None)

    if arm != "default":
        env, cases = A.SWITCH_ARMS[int(arm)]
        assert all(os.environ.get(k) == v for k, v in env.items()), "the child is the run WITH the switch"
        for c in cases:
            forward(c)
            done("fwd " + A.case_id(c))
    else:
        for c in A.all_cases():
            forward(c)
            done("fwd " + A.case_id(c))
        for name in AB.CASES:
            for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
                AB.run_fused(K, name, dtype)
                done(f"bwd {name} {tag}")
                if name in AB.CROSS_CASES:
                    AB.run_fused(K, name, dtype, kv_grad=False)
                    done(f"bwd {name} {tag} frozen kv")
        for case in TB.CASES:
            H, D = case[3], case[4]
            for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
                qkv, g = (t.to(dtype).cuda() for t in TB.make_inputs(case, dtype))
                K.self_attention_qkv(qkv.requires_grad_(True), H, D ** -0.5, True).backward(g)
                done(f"temporal bwd {TB.case_id(case)} {tag}")
        for Fr in CLIP_LENGTHS:
            CL.full_tile_outputs(K, Fr)
            done(f"clip length {Fr}: fwd bf16, bwd bf16, fwd f32, bwd f32, fp8 fwd, fp8 bwd")
    torch.cuda.synchronize()
    with open(out, "w") as f:
        json.dump(labels, f)


def short(name):
    """`void (anonymous namespace)::k<unsigned short, 3>((anonymous namespace)::P) [clone .kd]` -> `k<unsigned short, 3>`"""
    name = re.sub(r"\s*\[clone[^\]]*\]$", "", name.strip()).replace("(anonymous namespace)::", "")
    name = re.sub(r"\.kd$", "", name)
    name = re.sub(r"^void\s+", "", name)
    depth = 0
    for i, ch in enumerate(name):                    # the argument list: the first "(" outside the template brackets
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def read_trace(directory, labels):
    """{label: [[kernel, grid, workgroup, lds], ...]} from the kernel-trace CSV under `directory`."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, f"one kernel trace expected under {directory}: {files}"
    with open(files[0]) as f:
        rows = list(csv.DictReader(f))
    order = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[order]))
    dims = lambda r, what: [int(r[f"{what}_Size_{a}"]) for a in "XYZ" if f"{what}_Size_{a}" in r]
    segments, cur = [], []
    for r in rows:
        name = short(r["Kernel_Name"])
        if SEPARATOR in name:
            segments.append(cur)
            cur = []
        elif "at::" not in name and not name.startswith(("Cijk", "__amd_rocclr", "hipblas")):        # torch's own kernels, runtime fills and copies
            cur.append([name, dims(r, "Grid"), dims(r, "Workgroup"), int(r.get("LDS_Block_Size", r.get("Group_Segment_Size", -1)))])
    assert not cur and len(segments) == len(labels), f"{len(segments)} separated runs for {len(labels)} cases (trailing launches: {cur})"
    assert len(set(labels)) == len(labels)
    return dict(zip(labels, segments))


def trace(tree, work):
    """Routes of `tree`: {"default": {...}, "<switch>=<value>": {...}}; children one after another, the first failure ends the run."""
    sys.path.insert(0, tree)
    from tests import attn_fwd_common as A
    arms = [("default", {})] + [(str(i), env) for i, (env, _) in enumerate(A.SWITCH_ARMS)]
    routes = {}
    for arm, env in arms:
        key = "default" if not env else ",".join(f"{k}={v}" for k, v in sorted(env.items()))
        d = os.path.join(work, "arm_" + arm)
        os.makedirs(d, exist_ok=True)
        labels = os.path.join(d, "labels.json")
        if not os.path.exists(labels):               # (a kept trace is read again, not run again)
            if not shutil.which("rocprofv3"):
                raise SystemExit("rocprofv3 not found: the routes are recorded from the device")
            cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--",
                   sys.executable, os.path.join(ROOT, "tools", "record_attn_routes.py"), "--child", arm, labels, "--tree", tree]
            run = subprocess.run(cmd, env=dict(os.environ, **env), cwd=tree, capture_output=True, text=True)
            print(f"[{key}] exit {run.returncode}", flush=True)
            if run.returncode != 0:
                sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
                raise SystemExit(f"the child of [{key}] failed ({run.returncode}): nothing further is started")
        with open(labels) as f:
            routes[key] = read_trace(d, json.load(f))
    return routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--commit", default="")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package and library are traced (default: this one)")
    ap.add_argument("--keep", default="", help="keep the raw traces in this directory")
    ap.add_argument("--child", nargs=2, metavar=("ARM", "OUT"))
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    if args.child:
        sys.path.insert(0, tree)
        return child(*args.child)
    work = args.keep or tempfile.mkdtemp(prefix="attn_routes_")
    os.makedirs(work, exist_ok=True)
    routes = trace(tree, work)
    count = sum(len(v) for v in routes.values())
    if args.check:
        with open(args.out) as f:
            want = json.load(f)["routes"]
        diff = [(arm, case) for arm in sorted(set(want) | set(routes)) for case in sorted(set(want.get(arm, {})) | set(routes.get(arm, {})))
                if want.get(arm, {}).get(case) != routes.get(arm, {}).get(case)]
        for arm, case in diff[:40]:
            print(f"[{arm}] {case}:\n    recorded {want.get(arm, {}).get(case)}\n    traced   {routes.get(arm, {}).get(case)}")
        print(f"{count} cases traced, {len(diff)} differ from {args.out}")
        return 1 if diff else 0
    data = {"recorded_at": args.commit, "source": "rocprofv3 --kernel-trace on the MI355X", "columns": ["kernel", "grid (work-items)", "workgroup", "LDS_Block_Size of the trace (the kernel's static bytes; a launch's dynamic size is not traced)"],
            "routes": routes}
    with open(args.out, "w") as f:
        json.dump(data, f, separators=(",", ":"))
        f.write("\n")
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {count} cases in {len(routes)} processes")
    return 0


if __name__ == "__main__":
    sys.exit(main())

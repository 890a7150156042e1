"""The N > 1 path over REAL RCCL: runs only where at least two GPUs are visible (`gpurun` boxes have
one: these tests skip themselves there; the driver's 8-GPU node runs them).  What they pin: `bench.py --gpus 2` starts, verifies
its world size with a collective and reports it; the training step's gradient exchange leaves bit-identical parameters on every
rank, in the default graph | all-reduce | graph form AND with the all-reduce captured inside the step's HIP graph; and
`GradAllReducer` over the `nccl` backend reproduces the mean of the per-rank gradients."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_two_gpus():
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip(f"needs >= 2 GPUs over xGMI, {torch.cuda.device_count() if torch.cuda.is_available() else 0} visible")


def _bench(*extra, timeout=1500):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", *extra], capture_output=True, text=True,
                         env=env, timeout=timeout, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_bench_infer_two_ranks_rccl():
    _need_two_gpus()
    line = _bench("--steps", "3", "--warmup", "1", "--full")
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0
    assert line["parity_rel_inf"] is None and "N > 1" in line["parity_note"]       # nobody idles behind rank 0's CPU oracle
    assert line["config"]["parallelism"].startswith("dp2")


@pytest.mark.parametrize("graph", ["split", "one", "none"])
def test_bench_train_two_ranks_rccl(graph):
    """graph | all-reduce | graph, the all-reduce captured inside ONE graph, and the eager overlapped form: each must leave the
    trained parameters bit-identical on both ranks (bench.py asserts it and reports it)."""
    _need_two_gpus()
    line = _bench("--mode", "train", "--steps", "3", "--warmup", "1", "--train-graph", graph)
    assert line["n_gpus"] == 2 and line["config"]["parameters_bit_equal_across_ranks"] is True
    assert line["config"]["hip_graph"] == graph and line["config"]["allreduce_bytes"] > 0


_NCCL_REDUCER = r'''
import os, sys, json
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
from synfmc_amd.training import GradAllReducer, broadcast_parameters
r = int(os.environ["RANK"]); torch.cuda.set_device(r); dev = torch.device("cuda", r)
dist.init_process_group("nccl", init_method="env://", device_id=dev)
w = dist.get_world_size()
torch.manual_seed(100 + r)
net = torch.nn.Sequential(torch.nn.Linear(256, 512), torch.nn.ReLU(), torch.nn.Linear(512, 64)).to(dev)
unused = torch.nn.Linear(8, 8).to(dev)
broadcast_parameters(net); broadcast_parameters(unused)
red = GradAllReducer(list(net.parameters()) + list(unused.parameters()), bucket_bytes=200_000, overlap=True)
errs = []
for step in range(3):
    x = torch.randn(32, 256, generator=torch.Generator().manual_seed(10 * step + r)).to(dev)
    net(x).pow(2).mean().backward()
    red.finish()
    got = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone()
    lo, hi = got.clone(), got.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    ref = [torch.zeros_like(p) for p in net.parameters()]
    for rr in range(w):
        xr = torch.randn(32, 256, generator=torch.Generator().manual_seed(10 * step + rr)).to(dev)
        gs = torch.autograd.grad(net(xr).pow(2).mean(), list(net.parameters()))
        ref = [a + g / w for a, g in zip(ref, gs)]
    want = torch.cat([t.reshape(-1) for t in ref])
    errs.append({"bit_equal_across_ranks": bool(torch.equal(lo, hi)), "err": float((got - want).abs().max() / want.abs().max()),
                 "n_unused": len(red.unused), "unused_none": all(p.grad is None for p in unused.parameters())})
    red.zero_grad()
if r == 0:
    print(json.dumps(errs))
dist.destroy_process_group()
'''


def test_grad_allreducer_over_rccl(tmp_path):
    _need_two_gpus()
    script = tmp_path / "nccl_reducer.py"
    script.write_text(_NCCL_REDUCER)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29751", str(script), ROOT], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("[")][-1])
    assert all(s["bit_equal_across_ranks"] and s["err"] < 1e-5 and s["n_unused"] == 2 and s["unused_none"] for s in res), res


def test_launch_lds_raised_on_second_device():
    """The dynamic-LDS attribute is raised per DEVICE: in one fresh process the 256 x 256 ring kernel with 64-deep k-tiles (tile 3,
    129 KiB and more of LDS) runs on cuda:0, then on cuda:1, each result checked on its own device against F.linear in fp32."""
    _need_two_gpus()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "launch_child.py"), ROOT, "0:3:256:256:128:0", "1:3:256:256:128:0"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    errs = json.loads(out.stdout.splitlines()[-1])
    print("rel-inf on cuda:0, cuda:1:", errs)
    assert len(errs) == 2 and all(e < 1e-2 for e in errs), errs

"""Worker of the launch-helper tests: a FRESH process, because what they test -- the dynamic-LDS size that `fmc_launch` (csrc/common.h)
has raised each kernel instantiation to on each device -- is per-process state that any earlier test would already have warmed.

    python launch_child.py ROOT CALL [CALL ...]        CALL = device:tile:M:N:K:second_residual(0|1)

runs `hip_ops.linear_bf16(x, w, None, r [, residual2=r2], tile=tile)` on seeded bf16 inputs for every CALL, in order, in this one
process, and prints one JSON list with the rel-inf error of each result against `F.linear` in fp32 on the same rounded inputs.  A
failed launch raises out of `linear_bf16` (the ABI returns a status): non-zero exit."""
import json
import sys

sys.path.insert(0, sys.argv[1])
import torch                                   # noqa: E402
import torch.nn.functional as F               # noqa: E402
from synfmc_amd import hip_ops                 # noqa: E402


def rnd(shape, seed, scale=1.0):
    x = (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.bfloat16)
    return x.float(), x


errs = []
for i, call in enumerate(sys.argv[2:]):
    dev, tile, M, N, K, second = (int(v) for v in call.split(":"))
    torch.cuda.set_device(dev)
    xo, x = rnd((M, K), 900 + 4 * i)
    wo, w = rnd((N, K), 901 + 4 * i, K ** -0.5)
    ro, r = rnd((M, N), 902 + 4 * i)
    r2o, r2 = rnd((M, N), 903 + 4 * i)
    ref = F.linear(xo, wo) + ro + (r2o if second else 0)
    out = hip_ops.linear_bf16(x.cuda(), w.cuda(), None, r.cuda(), 1.0, tile=tile, residual2=r2.cuda() if second else None)
    torch.cuda.synchronize()
    assert out.device.index == dev
    errs.append(((out.float().cpu() - ref).abs().max() / ref.abs().max()).item())
print(json.dumps(errs))

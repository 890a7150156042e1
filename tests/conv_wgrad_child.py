"""Worker of the switch test of the direct 3x3 weight gradient: a FRESH process, because `FMC_CONV_WGRAD` is read when the package is imported.

    python conv_wgrad_child.py ROOT

One marked `Conv2d(64, 128, 3, 1, 1)` with fp32 masters, forward + backward on seeded bf16 activations.  Prints one JSON line:
{"switch": the switch as the package read it, "families": `hip_ops.call_log` families of the step, "dw_err": rel-inf of `weight.grad`
against float64, "old_route_bits": whether `weight.grad` equals `conv3x3_weight_grad(x, dy).to(float32)` bit for bit}."""
import json
import sys

sys.path.insert(0, sys.argv[1])
import torch                                                   # noqa: E402
from synfmc_amd import hip_ops as K                            # noqa: E402
from tests import conv_wgrad_common as CW                      # noqa: E402

conv, x, dy = CW.marked_conv(64, 128, 1, (3, 9, 13))
K.call_log = []
xs = x.cuda().requires_grad_(True)
conv(xs).backward(dy.cuda())
torch.cuda.synchronize()
families = [e[0] for e in K.call_log]
K.call_log = None
ref, _ = CW.reference(x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1), 1)
got = conv.weight.grad
old = K.conv3x3_weight_grad(x.cuda().permute(0, 2, 3, 1).contiguous(), dy.cuda().permute(0, 2, 3, 1).contiguous()).to(torch.float32)
print(json.dumps({"switch": K.CONV_WGRAD, "families": families, "dw_err": float((got.double().cpu() - ref).abs().max() / ref.abs().max()),
                  "old_route_bits": bool(torch.equal(got, old)), "dtype": str(got.dtype)}))

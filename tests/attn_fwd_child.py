"""Worker of `test_switch_arms_every_element` (test_gpu_attn_forward_elementwise.py): a FRESH process, because csrc/spatial_attn.hip reads its A/B
switches (`FMC_SA_*`) once per process.

    FMC_SA_...=... python attn_fwd_child.py ROOT ARM OUT.json

runs the cases of `attn_fwd_common.SWITCH_ARMS[ARM]` under the exact instrument, asserts every output and LSE element against its bound and writes the
largest err / bound per case.  A failed launch or a missed bound raises: non-zero exit."""
import json
import os
import sys

sys.path.insert(0, sys.argv[1])
import torch                                         # noqa: E402
from synfmc_amd import hip_ops                       # noqa: E402
from tests import attn_fwd_common as A               # noqa: E402

env, cases = A.SWITCH_ARMS[int(sys.argv[2])]
assert all(os.environ.get(k) == v for k, v in env.items()), "the worker is the run WITH the switch"
shares = {}
for c in cases:
    d = A.inputs(c, "exact")
    q, k, v = A.views(c, {n: t.cuda() for n, t in A.pack(c, d).items()})
    out, lse = hip_ops.spatial_attention(q, k, v, c.H, d["scale"], return_lse=True)
    torch.cuda.synchronize()
    shares[A.case_id(c)] = A.check(c, "exact", out, lse, f"{env} {A.case_id(c)}")
with open(sys.argv[3], "w") as f:
    json.dump(shares, f)

"""Worker of `test_block_order_changes_no_bit` (test_gpu_attn_backward.py): a FRESH process, because the backward reads the
`FMC_SAB_XCD0` switch (plain workgroup order instead of one batch entry per XCD, csrc/spatial_attn_bwd.hip) once per process.

    FMC_SAB_XCD0=1 python attn_bwd_child.py ROOT OUTDIR

runs `attn_bwd_common.CHILD_CASES` in bf16 and fp32 through the fused entry points and writes every gradient as
`OUTDIR/<case>_<dtype>_<dq|dk|dv>.npy` (fp32 holds every bf16 value exactly).  A failed launch raises: non-zero exit."""
import os
import sys

sys.path.insert(0, sys.argv[1])
import numpy as np                                   # noqa: E402
import torch                                         # noqa: E402
from synfmc_amd import hip_ops                       # noqa: E402
from tests import attn_bwd_common as AB              # noqa: E402

assert "FMC_SAB_XCD0" in os.environ, "the worker is the run WITH the switch"
for name in AB.CHILD_CASES:
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        for key, t in AB.run_fused(hip_ops, name, dtype).items():
            np.save(os.path.join(sys.argv[2], f"{name}_{tag}_{key}.npy"), t.float().cpu().numpy())
torch.cuda.synchronize()

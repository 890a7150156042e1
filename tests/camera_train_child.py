"""Worker of the path-proof test: a FRESH process, because the A/B switch `FMC_TRAINABLE_OWN` is read when the package is imported.

    python camera_train_child.py ROOT

builds a small stage-2 stack (seeded non-zero weights, bf16), turns the stage-2 parameters into marked fp32 masters and runs one forward +
backward under `camera_train_common.torch_ops_raise`, armed inside the encoder's forward, the merges and the whole backward.  Prints one
JSON line: {"own": the switch as the package read it, "raised": the torch op that was reached, or null when the step ran to the end}."""
import json
import sys

sys.path.insert(0, sys.argv[1])
import torch                                                   # noqa: E402
from synfmc_amd.models import layers                           # noqa: E402
from synfmc_amd.training import camera_trainable_parameters    # noqa: E402
from tests import camera_train_common as CC                    # noqa: E402
from tests import common_models as CM                          # noqa: E402

W4 = (64, 128, 256, 256)
ou, oe, oa = CM.build_oracle(W4, seed=21, fan_in_gain=0.7)
pu, pe, pa = CM.build_product(ou, oe, oa, W4, dtype=torch.bfloat16)
clip = CM.synthetic_clip(B=1, Fr=16, H=64, W=64)
camera_trainable_parameters(pu, pe)
g = torch.Generator().manual_seed(3)
pose_emb = torch.randn(1, 6, 16, 64, 64, generator=g)
noise = torch.randn(clip["latents"].shape, generator=g)
raised = None
try:
    CC.path_proof(2, pu, pe, pa, clip, pose_emb, torch.tensor([500]), noise)
except CC.TorchOpReached as e:
    raised = str(e)
print(json.dumps({"own": layers.TRAINABLE_OWN, "raised": raised}))

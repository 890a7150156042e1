"""The host layer is clip-length generic: the product U-Net (CMC + OMC, the reduced widths of tests/test_host_logic.py) on the CPU
stand-ins of `tests/fake_kernels.py` at 7 and 12 frames against the oracle.  Nothing here depends on the temporal-attention
kernels (those are covered on the GPU in tests/test_gpu_clip_lengths.py); this pins channels-last plumbing, LayerNorm + PE,
the Camera-Adapter merge, the pose-term cache, the OMC injection and the `fused_blocks_ok` fall-back, so that a later change
cannot make one of them length-specific unnoticed."""
import pytest
import torch
from einops import rearrange

from oracle import conditioning as OC
from tests import common_models as CM
from tests import fake_kernels

W4 = (32, 64, 64, 64)


def rel_inf(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("Fr", [7, 12])
def test_unet_plumbing_cmc_omc_at_other_clip_lengths(monkeypatch, Fr):
    fake_kernels.install(monkeypatch)
    ou, oe, oa = CM.build_oracle(W4, cross_dim=32)
    clip = CM.synthetic_clip(B=1, Fr=Fr, H=128, W=128, cross_dim=32)
    t = torch.tensor([801])
    with torch.no_grad():
        pose_emb = rearrange(OC.to_plucker_embedding(clip["c2w"], clip["K"], (128, 128)), "b f c h w -> b c f h w")
        pose_feats = [rearrange(x, "(b f) c h w -> b c f h w", b=1) for x in oe(pose_emb)]
        traj = OC.get_traj_features(clip["infos"], clip["masks"], oa)
        ref = ou(clip["latents"], t, clip["text"], pose_embedding_features=pose_feats, traj_features=traj).sample
        ref0 = ou(clip["latents"], t, clip["text"], pose_embedding_features=pose_feats, traj_features=None).sample
    pu, pe, pa = CM.build_product(ou, oe, oa, W4, cross_dim=32, device="cpu")
    with torch.no_grad():
        out = pu(clip["latents"], t, clip["text"], pose_embedding_features=pose_feats, traj_features=traj).sample
        out0 = pu(clip["latents"], t, clip["text"], pose_embedding_features=pose_feats, traj_features=None).sample
    assert out.shape == ref.shape and out.shape[2] == Fr
    err, err0 = rel_inf(out, ref), rel_inf(out0, ref0)
    print(f"{Fr} frames: rel-inf vs the oracle {err:.3e} (with OMC), {err0:.3e} (without)")
    assert err < 1e-3 and err0 < 1e-3
    assert rel_inf(ref, ref0) > 1e-3

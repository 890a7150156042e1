"""Temporal attention at any clip length from 1 to 32 frames: the four kernels of csrc/temporal_attn.hip with a partial last frame
tile (F % 16 != 0), from the C ABI up to the pipelines.

Bounds are the project's own for the 16- / 32-frame case (tests/test_gpu_kernels.py: TOL 2e-5 / 1e-2, GTOL 1e-4 / 3e-2; the fp8 tests'
1e-2 / 2e-2 / 3e-2; tests/test_gpu_model.py: forward 1e-3 / 6e-2, stage-3 gradients 1e-4 / 6e-2, pipelines 1e-2 / 1e-3): a masked
softmax over fewer keys adds no rounding that the whole-tile case does not have.  F = 16 and F = 32 themselves must not move by one
bit (tests/golden/g8_temporal_attn_full_tiles_f*.npz, recorded with the library of the commit before this work).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from einops import rearrange

from oracle import conditioning as OC
from oracle import diffusers_restated as OD
from oracle import pipeline as OP
from tests import clip_lengths_common as CL
from tests import common_models as CM
from tests.test_gpu_kernels import GTOL, TOL, _quant, oracle_attention, rel_inf, rnd

pytestmark = pytest.mark.gpu

LENGTHS = [1, 7, 8, 12, 15, 17, 24, 25, 31]
FP8_LENGTHS = [8, 12, 24]
W4 = (64, 128, 256, 256)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


# ---- 1. forward, kernel level ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,P,H,D", [(2, 20, 8, 40), (1, 9, 8, 80), (2, 5, 8, 160), (1, 6, 8, 40), (1, 3, 8, 160), (2, 7, 4, 8),
                                     (1, 4, 8, 16)])         # the (P, H, D) classes of test_temporal_attention_native_and_reference_layouts
@pytest.mark.parametrize("Fr", LENGTHS)
def test_temporal_attention_forward_clip_lengths(K, dtype, Fr, B, P, H, D):
    C = H * D
    qkvo, qkvd = rnd((B, Fr, P, 3 * C), 20, dtype)
    ref_in = qkvo.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
    ref = oracle_attention(ref_in[..., :C], ref_in[..., C:2 * C], ref_in[..., 2 * C:], H)
    out = K.temporal_attention(qkvd[..., :C], qkvd[..., C:2 * C], qkvd[..., 2 * C:], H)       # native [B,F,P,C]
    got = out.permute(0, 2, 1, 3).reshape(B * P, Fr, C)
    r3 = qkvd.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C).contiguous()                       # reference layout in
    out3 = K.temporal_attention(r3[..., :C], r3[..., C:2 * C], r3[..., 2 * C:], H)
    e1, e3 = rel_inf(got.float(), ref), rel_inf(out3.float(), ref)
    print(f"F={Fr} {dtype}: native {e1:.3e}, reference layout {e3:.3e} (bound {TOL[dtype]})")
    assert torch.isfinite(out).all() and torch.isfinite(out3).all()
    assert e1 < TOL[dtype]
    assert e3 < TOL[dtype]


# ---- 2. backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,P,H,D", [(2, 6, 8, 40), (1, 5, 8, 160), (1, 3, 8, 80), (2, 4, 4, 8)])      # the shapes of test_temporal_attention_backward
@pytest.mark.parametrize("Fr", LENGTHS)
def test_temporal_attention_backward_clip_lengths(K, dtype, Fr, B, P, H, D):
    C = H * D
    qkvo, qkvd = rnd((B, Fr, P, 3 * C), 90, dtype)
    do, dd = rnd((B, Fr, P, C), 91, dtype)
    xr = qkvo.clone().requires_grad_(True)
    ref_in = xr.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
    out = oracle_attention(ref_in[..., :C], ref_in[..., C:2 * C], ref_in[..., 2 * C:], H)
    out.backward(do.permute(0, 2, 1, 3).reshape(B * P, Fr, C))
    xg = qkvd.clone().requires_grad_(True)
    K.temporal_attention(xg[..., :C], xg[..., C:2 * C], xg[..., 2 * C:], H).backward(dd)
    err = rel_inf(xg.grad.float(), xr.grad)
    print(f"F={Fr} {dtype}: dQ|dK|dV {err:.3e} (bound {GTOL[dtype]})")
    assert torch.isfinite(xg.grad).all()
    assert err < GTOL[dtype]


# ---- 3. fp8 forward and autograd -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P,H,D", [(2, 20, 8, 40), (1, 6, 8, 40), (1, 3, 8, 160), (1, 9, 8, 80), (2, 7, 8, 8)])
@pytest.mark.parametrize("Fr", FP8_LENGTHS)
def test_temporal_attention_fp8_forward_clip_lengths(K, Fr, B, P, H, D):
    """As test_temporal_attention_fp8_forward: the oracle on the SAME e4m3-rounded q, k, v, bound 1e-2."""
    C = H * D
    g = torch.Generator().manual_seed(72)
    qkv = torch.randn(B, Fr, P, 3 * C, generator=g)
    qkv[..., C:2 * C] *= 2.0
    scales = torch.tensor([qkv[..., :C].abs().max(), qkv[..., C:2 * C].abs().max(), qkv[..., 2 * C:].abs().max()]) * 1.25 / 448.0
    q8 = torch.cat([_quant(qkv[..., i * C:(i + 1) * C], float(scales[i])) for i in range(3)], dim=-1)
    deq = torch.cat([q8[..., i * C:(i + 1) * C].float() * float(scales[i]) for i in range(3)], dim=-1)
    ref_in = deq.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
    ref = oracle_attention(ref_in[..., :C], ref_in[..., C:2 * C], ref_in[..., 2 * C:], H)
    out = K._temporal_fp8_raw(q8.cuda(), scales.cuda(), H, D ** -0.5)
    got = out.permute(0, 2, 1, 3).reshape(B * P, Fr, C)
    err = rel_inf(got.float(), ref)
    print(f"fp8 F={Fr}: {err:.3e} (bound 1e-2)")
    assert out.dtype == torch.bfloat16 and torch.isfinite(out).all() and err < 1e-2


@pytest.mark.parametrize("Fr", FP8_LENGTHS)
def test_temporal_attention_fp8_autograd_clip_lengths(K, Fr):
    """As test_temporal_attention_fp8_autograd (projection + fp8 attention as one autograd node), its bounds."""
    B, P, H, D = 1, 12, 8, 40
    C = H * D
    xo, xd = rnd((B, Fr, P, C), 73, torch.bfloat16)
    wo, wd = rnd((3 * C, C), 74, torch.bfloat16, scale=C ** -0.5)
    do, dd = rnd((B, Fr, P, C), 75, torch.bfloat16)
    sc = K.Fp8QKVScales(xd.device)
    xg, wg = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True)
    out = K.temporal_attention_fp8(xg, wg, sc, H, D ** -0.5)
    out.backward(dd)
    scales = sc.scale.cpu()
    xr, wr = xo.clone().requires_grad_(True), wo.clone().requires_grad_(True)
    qkv = F.linear(xr, wr)
    deq = torch.cat([_quant(qkv[..., i * C:(i + 1) * C].detach(), float(scales[i])).float() * float(scales[i]) for i in range(3)], -1)
    qkv_ste = qkv + (deq - qkv).detach()
    t = qkv_ste.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
    ref = oracle_attention(t[..., :C], t[..., C:2 * C], t[..., 2 * C:], H).reshape(B, P, Fr, C).permute(0, 2, 1, 3)
    ref.backward(do)
    eo, ex, ew = rel_inf(out.float(), ref), rel_inf(xg.grad.float(), xr.grad), rel_inf(wg.grad.float(), wr.grad)
    print(f"fp8 autograd F={Fr}: out {eo:.3e} (2e-2), dx {ex:.3e} (3e-2), dW {ew:.3e} (3e-2)")
    assert eo < 2e-2
    assert ex < 3e-2
    assert ew < 3e-2


# ---- 4. pad rows are never touched -----------------------------------------------------------------------------------------
SENT = {torch.bfloat16: 0x4B1D, torch.float32: 0x4B1D5EA7}        # sentinel bit patterns (finite values nothing here computes)


def _alloc_frames(Fr):
    """Frames allocated per clip: the clip, the rest of its last 16-row tile (where a wrong row address would land), and two more."""
    return (Fr + 15) // 16 * 16 + 2


def _nan_input(values, Fa):
    """[B, Fr, P, W] values -> the `[:, :Fr]` view of a `[B, Fa, P, W]` device allocation whose other rows hold NaN."""
    B, Fr, P, W = values.shape
    if values.dtype == torch.float8_e4m3fn:
        big = torch.full((B, Fa, P, W), 0x7F, dtype=torch.uint8, device="cuda").view(torch.float8_e4m3fn)       # 0x7f = NaN in e4m3fn
        big.view(torch.uint8)[:, :Fr] = values.cuda().view(torch.uint8)
    else:
        big = torch.full((B, Fa, P, W), float("nan"), dtype=values.dtype, device="cuda")
        big[:, :Fr] = values.cuda()
    return big, big[:, :Fr]


def _sentinel_output(B, Fr, Fa, P, W, dtype):
    it = torch.int16 if dtype == torch.bfloat16 else torch.int32
    big = torch.full((B, Fa, P, W), SENT[dtype], dtype=it, device="cuda").view(dtype)
    return big, big[:, :Fr]


def _pad_rows_intact(big, Fr, dtype):
    it = torch.int16 if dtype == torch.bfloat16 else torch.int32
    return bool((big.view(it)[:, Fr:] == SENT[dtype]).all())


def _strides(t):
    return t.stride(0), t.stride(1), t.stride(2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Fr", [1, 7, 12, 17, 24, 31])
def test_pad_rows_are_never_touched(K, dtype, Fr):
    """q | k | v, o, dO and dq | dk | dv are views into larger allocations (2 clips): the frame rows behind each clip and the slack
    behind the last clip hold NaN (inputs) or a sentinel (outputs).  Results are finite and within bound; every sentinel row is
    bit-intact.  All rows a wrong address could reach are inside the test's own allocations."""
    from synfmc_amd import _lib
    B, P, H, D = 2, 5, 8, 40
    C, Fa = H * D, _alloc_frames(Fr)
    qkvo, _ = rnd((B, Fr, P, 3 * C), 120, dtype)
    do_o, _ = rnd((B, Fr, P, C), 121, dtype)
    _, qkv = _nan_input(qkvo.to(dtype), Fa)
    _, d_o = _nan_input(do_o.to(dtype), Fa)
    obig, o = _sentinel_output(B, Fr, Fa, P, C, dtype)
    gbig, dqkv = _sentinel_output(B, Fr, Fa, P, 3 * C, dtype)
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    dq, dk, dv = dqkv[..., :C], dqkv[..., C:2 * C], dqkv[..., 2 * C:]
    L, dt, scale = _lib.load(), K._dt(q), D ** -0.5
    _lib.check(L.fmc_temporal_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, P, Fr, H, D, *_strides(q), *_strides(o),
                                       scale, dt, K._stream()), "fmc_temporal_attn_fwd")
    _lib.check(L.fmc_temporal_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), d_o.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                                       B, P, Fr, H, D, *_strides(q), *_strides(d_o), *_strides(dq), scale, dt, K._stream()),
               "fmc_temporal_attn_bwd")
    torch.cuda.synchronize()
    xr = qkvo.clone().requires_grad_(True)
    ref_in = xr.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
    ref = oracle_attention(ref_in[..., :C], ref_in[..., C:2 * C], ref_in[..., 2 * C:], H)
    ref.backward(do_o.permute(0, 2, 1, 3).reshape(B * P, Fr, C))
    got = o.permute(0, 2, 1, 3).reshape(B * P, Fr, C)
    assert torch.isfinite(o).all() and torch.isfinite(dqkv).all()
    ef, eb = rel_inf(got.float(), ref), rel_inf(dqkv.float(), xr.grad)
    print(f"views, F={Fr} {dtype}: forward {ef:.3e} ({TOL[dtype]}), backward {eb:.3e} ({GTOL[dtype]})")
    assert ef < TOL[dtype]
    assert eb < GTOL[dtype]
    assert _pad_rows_intact(obig, Fr, dtype), "the forward wrote an O row >= F"
    assert _pad_rows_intact(gbig, Fr, dtype), "the backward wrote a dQ / dK / dV row >= F"


@pytest.mark.parametrize("Fr", FP8_LENGTHS)
def test_pad_rows_are_never_touched_fp8(K, Fr):
    from synfmc_amd import _lib
    B, P, H, D = 2, 5, 8, 40
    C, Fa, bf = H * D, _alloc_frames(Fr), torch.bfloat16
    g = torch.Generator().manual_seed(122)
    qkv = torch.randn(B, Fr, P, 3 * C, generator=g)
    scales = torch.tensor([qkv[..., :C].abs().max(), qkv[..., C:2 * C].abs().max(), qkv[..., 2 * C:].abs().max()]) * 1.25 / 448.0
    q8 = torch.cat([_quant(qkv[..., i * C:(i + 1) * C], float(scales[i])) for i in range(3)], dim=-1)
    deq = torch.cat([q8[..., i * C:(i + 1) * C].float() * float(scales[i]) for i in range(3)], dim=-1)
    do_o, _ = rnd((B, Fr, P, C), 123, bf)
    _, q8v = _nan_input(q8, Fa)
    _, d_o = _nan_input(do_o.to(bf), Fa)
    obig, o = _sentinel_output(B, Fr, Fa, P, C, bf)
    gbig, dqkv = _sentinel_output(B, Fr, Fa, P, 3 * C, bf)
    q, k, v = q8v[..., :C], q8v[..., C:2 * C], q8v[..., 2 * C:]
    dq, dk, dv = dqkv[..., :C], dqkv[..., C:2 * C], dqkv[..., 2 * C:]
    L, sc, scale = _lib.load(), scales.cuda(), D ** -0.5
    _lib.check(L.fmc_temporal_attn_fp8_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), sc.data_ptr(), B, P, Fr, H, D, *_strides(q),
                                           *_strides(o), scale, K._stream()), "fmc_temporal_attn_fp8_fwd")
    _lib.check(L.fmc_temporal_attn_fp8_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), sc.data_ptr(), d_o.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                           dv.data_ptr(), B, P, Fr, H, D, *_strides(q), *_strides(d_o), *_strides(dq), scale, K._stream()),
               "fmc_temporal_attn_fp8_bwd")
    torch.cuda.synchronize()
    xr = deq.clone().requires_grad_(True)
    ref_in = xr.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
    ref = oracle_attention(ref_in[..., :C], ref_in[..., C:2 * C], ref_in[..., 2 * C:], H)
    ref.backward(do_o.permute(0, 2, 1, 3).reshape(B * P, Fr, C))
    got = o.permute(0, 2, 1, 3).reshape(B * P, Fr, C)
    assert torch.isfinite(o).all() and torch.isfinite(dqkv).all()
    ef, eb = rel_inf(got.float(), ref), rel_inf(dqkv.float(), xr.grad)
    print(f"fp8 views, F={Fr}: forward {ef:.3e} (1e-2), backward {eb:.3e} (3e-2)")
    assert ef < 1e-2                                     # test_temporal_attention_fp8_forward's bound
    assert eb < 3e-2                                     # GTOL[bf16]: the backward is the bf16 kernel on the dequantised rows
    assert _pad_rows_intact(obig, Fr, bf), "the fp8 forward wrote an O row >= F"
    assert _pad_rows_intact(gbig, Fr, bf), "the fp8 backward wrote a dQ / dK / dV row >= F"


# ---- 5. whole tiles did not move -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Fr", [16, 32])
def test_full_tiles_bit_identical(K, golden_dir, Fr):
    """F = 16 and F = 32 on fixed inputs equal the recorded bits (tests/golden/make_golden_clip_lengths.py, same machine type).  The three backward
    arrays are those of the library before the partial-tile work: those paths did not move.  The three forward arrays were recorded again when the
    forward kernels moved the normalisation from the rounded p onto the PV accumulator (profiles/attn_forward_bounds.md); the backward arrays were
    bit-identical in that run."""
    gold = np.load(os.path.join(golden_dir, f"g8_temporal_attn_full_tiles_f{Fr}.npz"))
    got = CL.full_tile_outputs(K, Fr)
    for name in ("fwd_bf16", "fwd_f32", "bwd_bf16", "bwd_f32", "fp8_fwd", "fp8_bwd"):
        assert got[name].shape == gold[name].shape and got[name].dtype == gold[name].dtype, name
        diff = int((got[name] != gold[name]).sum())
        assert diff == 0, f"{name} at F = {Fr}: {diff} / {got[name].size} words differ from the recorded bits"


# ---- 6. model level --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol,gtol", [(torch.float32, 1e-3, 1e-4), (torch.bfloat16, 6e-2, 6e-2)])     # gradients measured: <= 4.9e-6 / <= 1.12e-2
@pytest.mark.parametrize("Fr", [12, 24])
def test_clip_lengths_forward_and_training(K, Fr, dtype, tol, gtol):
    """The body of test_frames32_forward_and_training at 12 and 24 frames: forward parity (fp32 1e-3 / bf16 6e-2) and stage-3 Adapter
    gradients (fp32 1e-4 / bf16 6e-2, the bounds of test_stage3_training_gradients for the same stage at 16 frames) against the
    oracle on the reduced stack.  Measured on MI355X (forward / gradient rel-inf): 12 frames fp32 1.3e-5 / 4.9e-6, bf16 1.24e-2 / 1.12e-2;
    24 frames fp32 1.5e-5 / 3.6e-6, bf16 1.44e-2 / 9.5e-3."""
    from tests import training_common as TC
    enc_len = 32 if Fr > 16 else 16                      # the camera encoder's default position table is 16 long
    ou, oe, oa = CM.build_oracle(W4, seed=30, fan_in_gain=0.7, enc_max_len=enc_len)
    clip = CM.synthetic_clip(B=1, Fr=Fr, H=128, W=128, seed=130)
    with torch.no_grad():
        plucker = OC.to_plucker_embedding(clip["c2w"], clip["K"], (128, 128))
        pose_emb = rearrange(plucker, "b f c h w -> b c f h w")
        pose_feats = [rearrange(x, "(b f) c h w -> b c f h w", b=1) for x in oe(pose_emb)]
        traj = OC.get_traj_features(clip["infos"], clip["masks"], oa)
        t = torch.tensor([801])
        ref = ou(clip["latents"], t, clip["text"], pose_embedding_features=pose_feats, traj_features=traj).sample
    pu, pe, pa = CM.build_product(ou, oe, oa, W4, dtype=dtype, enc_max_len=enc_len)
    from synfmc_amd.models.pose_obj_adaptor import CamObjPoseAdaptor
    from synfmc_amd.util import get_traj_features_v2
    with torch.no_grad():
        tf = get_traj_features_v2(clip["infos"], clip["masks"], pa, False, 0.0, [False], "cuda", dtype)
        out = CamObjPoseAdaptor(pu, pe)(clip["latents"].cuda().to(dtype), t.cuda(), clip["text"].cuda().to(dtype),
                                        pose_emb.cuda().to(dtype), tf)
    ferr = rel_inf(out.float(), ref)
    print(f"{Fr} frames, forward rel-inf vs the oracle ({dtype}): {ferr:.3e} (tolerance {tol})")
    assert out.shape == ref.shape and ferr < tol
    noise = torch.randn(clip["latents"].shape, generator=torch.Generator().manual_seed(12))
    l_ref, g_ref = TC.oracle_grads(ou, oe, oa, clip, pose_emb, t, noise)
    if dtype == torch.bfloat16:
        pa = pa.float()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        l_got, g_got = TC.product_grads(pu, pe, pa, clip, pose_emb, t, noise, "cuda", dtype)
    assert abs(float(l_ref) - float(l_got)) < (1e-4 if dtype == torch.float32 else 2e-2) * abs(float(l_ref))
    err, scale = TC.compare(g_ref, g_got)
    print(f"{Fr} frames, gradient rel-inf vs the oracle's autograd ({dtype}): {err:.3e} (tolerance {gtol})")
    assert scale > 0 and err < gtol


# ---- 7. pipelines ----------------------------------------------------------------------------------------------------------
SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
LORA_SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
                  clip_sample=False)                     # configs/lora.yaml: noise_scheduler_kwargs


@pytest.fixture(scope="module")
def stack12():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ou, oe, oa = CM.build_oracle(W4)
    clip = CM.synthetic_clip(B=1, Fr=12, H=128, W=128)
    with torch.no_grad():
        pose_emb = rearrange(OC.to_plucker_embedding(clip["c2w"], clip["K"], (128, 128)), "b f c h w -> b c f h w")
        traj = OC.get_traj_features(clip["infos"], clip["masks"], oa)
    g = torch.Generator().manual_seed(5)
    text2 = torch.cat([torch.randn(1, 77, 64, generator=g), clip["text"]])
    ref = OP.denoise(ou, OD.DDIMScheduler(**SCHED), oe, text2, pose_emb, clip["latents"], num_inference_steps=3, guidance_scale=2.0,
                     traj_features=traj, omcm_min_step=700)
    return dict(ou=ou, oe=oe, oa=oa, clip=clip, pose_emb=pose_emb, traj=traj, text2=text2, ref=ref)


@pytest.mark.parametrize("use_graph", [False, True])
def test_camera_obj_pipeline_12_frames(K, stack12, use_graph):
    """`CameraObjCtrlPipeline` at `video_length=12`: 3 DDIM steps with CFG 2.0 and `omcm_min_step=700`, eager loop and captured graph, fp32
    parity mode against `oracle.pipeline.denoise` (1e-2, as test_denoising_loop_cfg_omcm_gate).  Measured: 2.5e-5, eager and graph."""
    from synfmc_amd.pipelines.pipeline_animation_cm_om import CameraObjCtrlPipeline
    from synfmc_amd.schedulers import DDIMScheduler
    s = stack12
    pu, pe, pa = CM.build_product(s["ou"], s["oe"], s["oa"], W4)
    pipe = CameraObjCtrlPipeline(None, None, None, pu, DDIMScheduler(**SCHED), pe)
    out = pipe(None, s["pose_emb"].cuda(), 12, traj_features=[t.cuda() for t in s["traj"]], height=128, width=128,
               num_inference_steps=3, guidance_scale=2.0, latents=s["clip"]["latents"].cuda(), output_type="latent",
               prompt_embeds=s["text2"].cuda(), omcm_min_step=700, use_graph=use_graph).videos
    err = rel_inf(out, s["ref"])
    print(f"CameraObjCtrlPipeline, 12 frames, graph={use_graph}: {err:.3e} (bound 1e-2)")
    assert out.shape == s["ref"].shape and out.shape[2] == 12 and err < 1e-2


def test_animation_pipeline_multidiff_24_frame_windows(K):
    """As test_animation_pipeline_multidiff_windows with 24-frame windows: 2 windows overlapping by 20 (28 frames in all).  Measured: 9.8e-6."""
    from synfmc_amd.pipelines.pipeline_animation import AnimationPipeline
    from synfmc_amd.schedulers import DDIMScheduler
    ou, pu = CM.build_lora_only(W4, 64, seed=51, fan_in_gain=0.7, device="cuda")
    g = torch.Generator().manual_seed(4)
    lat, text2 = torch.randn(1, 4, 28, 8, 8, generator=g), torch.randn(2, 77, 64, generator=g)
    ref = OP.denoise_plain(ou, OD.DDIMScheduler(**LORA_SCHED), text2, lat, 24, 4, 3.0, multidiff_total_steps=2, multidiff_overlaps=20)
    pipe = AnimationPipeline(None, None, None, pu, DDIMScheduler(**LORA_SCHED))
    out = pipe(None, 24, height=64, width=64, num_inference_steps=4, guidance_scale=3.0, latents=lat.cuda(), output_type="latent",
               prompt_embeds=text2.cuda(), multidiff_total_steps=2, multidiff_overlaps=20).videos
    err = rel_inf(out, ref)
    print(f"AnimationPipeline, 24-frame windows: {err:.3e} (bound 1e-3)")
    assert out.shape == ref.shape and err < 1e-3


# ---- the range stays an explicit error -------------------------------------------------------------------------------------
@pytest.mark.parametrize("Fr", [33, 48])
def test_more_than_32_frames_is_a_shape_error(K, Fr):
    C, H = 64, 8
    qkv = torch.zeros(1, Fr, 2, 3 * C, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match=r"1\.\.32"):
        K.temporal_attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], H)
    xg = qkv.clone().requires_grad_(True)
    with pytest.raises(ValueError, match=r"1\.\.32"):
        K.temporal_attention(xg[..., :C], xg[..., C:2 * C], xg[..., 2 * C:], H)
    q8 = torch.zeros(1, Fr, 2, 3 * C, dtype=torch.uint8, device="cuda").view(torch.float8_e4m3fn)
    with pytest.raises(ValueError, match=r"1\.\.32"):
        K._temporal_fp8_raw(q8, torch.ones(3, device="cuda"), H, 8 ** -0.5)

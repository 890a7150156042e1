"""Domain-LoRA training (FMC stage 1; stage 3 with `train_image_lora`) on the MI355X: the weight-gradient kernel
`fmc_linear_wgrad_bf16`, the un-merged LoRA projection (`hip_ops.lora_linear`), the processor, the stage-1 step and stage 3 with the
LoRA trained along, against fp64 / the CPU oracle.  Bounds: measured x 2 where a figure was measured, capped at the stated ones."""
import pytest
import torch

from tests import common_models as CM
from tests import lora_common as LC

pytestmark = pytest.mark.gpu

W4 = LC.W4

# (M, N, K) of one stage-1 step at the configs/lora.yaml shapes (16 images, 32 x 48 latents, rank C / 2), then odd token counts
WGRAD_SHAPES = [(24576, 320, 160), (24576, 160, 320), (24576, 480, 320), (6144, 640, 320), (6144, 960, 640), (1536, 1280, 640),
                (1536, 1920, 1280), (384, 1280, 640), (1232, 640, 768), (1232, 1280, 768), (1, 320, 160), (77, 640, 768), (1000, 480, 320)]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _operands(M, N, Kd, strided, seed):
    g = torch.Generator().manual_seed(seed)
    if strided:            # column slices of fused [M, 3C]-like tensors: rows lda / ldb apart, 16-byte aligned starts
        a = torch.randn(M, 3 * N, generator=g).to(torch.bfloat16).cuda()[:, N: 2 * N]
        b = torch.randn(M, Kd + 48, generator=g).to(torch.bfloat16).cuda()[:, 16: 16 + Kd]
    else:
        a = torch.randn(M, N, generator=g).to(torch.bfloat16).cuda()
        b = torch.randn(M, Kd, generator=g).to(torch.bfloat16).cuda()
    return a, b


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "slices"])
@pytest.mark.parametrize("M,N,Kd", WGRAD_SHAPES)
def test_wgrad_kernel_matches_fp64(K, M, N, Kd, strided):
    a, b = _operands(M, N, Kd, strided, seed=M + N + Kd)
    ref = a.double().cpu().t() @ b.double().cpu()
    got = K.linear_wgrad(a, b, alpha=0.5)
    torch.cuda.synchronize()
    err = ((got.double().cpu() - 0.5 * ref).abs().max() / (0.5 * ref).abs().max()).item()
    print(f"wgrad {(M, N, Kd)} {'slices' if strided else 'dense'}: rel-inf {err:.2e}")
    assert got.shape == (N, Kd) and got.dtype == torch.float32 and err <= 1e-4
    # accumulate mode: out + alpha a^T b
    base = torch.randn(N, Kd, generator=torch.Generator().manual_seed(1)).cuda()
    acc = K.linear_wgrad(a, b, alpha=-1.0, out=base.clone(), accumulate=True)
    err_acc = ((acc.double().cpu() - (base.double().cpu() - ref)).abs().max() / ref.abs().max()).item()
    assert err_acc <= 1e-4
    # bit-reproducible
    again = K.linear_wgrad(a, b, alpha=0.5)
    assert torch.equal(got, again)


def test_wgrad_grouped_launch_equals_separate_launches(K):
    probs = [_operands(24576, 480, 320, True, 1), _operands(24576, 320, 160, False, 2), _operands(1232, 640, 768, True, 3),
             _operands(77, 160, 320, False, 4)]
    sep = [K.linear_wgrad(a, b, alpha=0.25 * (i + 1)) for i, (a, b) in enumerate(probs)]
    grp = K.linear_wgrad_group([(a, b, 0.25 * (i + 1), None, False) for i, (a, b) in enumerate(probs)])
    for s, g in zip(sep, grp):
        assert torch.equal(s, g)


def test_wgrad_rejects_what_it_does_not_take(K):
    a = torch.zeros(64, 40, dtype=torch.bfloat16, device="cuda")                      # N % 16 != 0
    b = torch.zeros(64, 32, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="N % 16"):
        K.linear_wgrad(a, b)
    a = torch.zeros(64, 36, dtype=torch.bfloat16, device="cuda")[:, 2:34]              # misaligned start
    with pytest.raises(ValueError, match="aligned"):
        K.linear_wgrad(a, b)


def test_lora_update_below_half_an_ulp_still_moves_the_output(K):
    """The trap of a merged bf16 weight: every element of s U D (2e-3) is below half a bf16 ulp of W (|W| = 1.5: ulp 2^-7), so
    bf16(W + s U D) == W, yet with positive inputs the rank-one update moves each output by ~8 of its ulps.  The training path keeps
    the LoRA branch in the fp32 accumulation: its output must move like the oracle's (within 10 % of the LoRA contribution)."""
    C, r, M = 640, 320, 512
    g = torch.Generator().manual_seed(0)
    W = (torch.randint(0, 2, (C, C), generator=g).float() * 2 - 1) * 1.5
    x = torch.rand(M, C, generator=g) * 0.5 + 0.5
    u = d = (2e-3 / r) ** 0.5
    D = torch.full((r, C), d)
    U = torch.full((C, r), u)
    assert torch.equal((W + U @ D).to(torch.bfloat16).float(), W)                           # the merged weight is blind to it
    ref = x.double() @ W.double().t()
    delta_ref = x.double() @ (U.double() @ D.double()).t()
    xb, Wb = x.to(torch.bfloat16).cuda().requires_grad_(True), W.to(torch.bfloat16).cuda()
    Dg, Ug = D.cuda().requires_grad_(True), U.cuda().requires_grad_(True)
    y = K.lora_linear(xb, [Wb], [Dg], [Ug], [1.0])
    y0 = K.lora_linear(xb, [Wb], [Dg], [torch.zeros_like(Ug).requires_grad_(True)], [1.0])
    delta = (y.double() - y0.double()).cpu()
    ulp = 2.0 ** (torch.floor(torch.log2(ref.abs())) - 7)
    assert (delta_ref / ulp).median() > 4                                                  # many output ulps
    # each output is rounded to bf16 once, so one element moves by whole ulps of itself; the coherent update shows in the mean
    err = abs(delta.mean().item() - delta_ref.mean().item()) / delta_ref.mean().item()
    print(f"LoRA contribution below half an ulp of W: outputs moved by {delta.mean():.4f} on average (oracle {delta_ref.mean():.4f}, "
          f"{(delta_ref / ulp).median():.1f} output ulps), rel err {err:.3e}")
    assert err < 0.1 and (delta > 0).double().mean() > 0.9


@pytest.mark.parametrize("cross", [False, True], ids=["attn1_self", "attn2_text"])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 5e-5), (torch.bfloat16, 2.5e-2)])      # measured 2.4e-5 / 1.3e-2
def test_lora_processor_forward_and_gradients(K, cross, dtype, tol):
    """A trainable `LoRAAttnProcessor` at C = 320 (rank 160, padded to 192 inside the GEMMs) on self attention and on the 768-wide text:
    output, input gradient and all 8 LoRA gradients against the oracle's autograd."""
    C, heads, D, S = 320, 8, 768, 77
    oa, pa = LC.attention_pair(C, heads, cross_dim=D if cross else None, seed=11, device="cuda", dtype=dtype)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 256, C, generator=g)
    text = torch.randn(2, S, D, generator=g) if cross else None
    w = torch.randn(2, 256, C, generator=g)
    xo = x.clone().requires_grad_(True)
    ref = oa(xo, encoder_hidden_states=text)
    (ref * w).sum().backward()
    xp = x.to("cuda", dtype).requires_grad_(True)
    got = pa(xp, encoder_hidden_states=None if text is None else text.to("cuda", dtype))
    (got.float() * w.cuda()).sum().backward()
    errs = [LC.rel_inf(got, ref), LC.rel_inf(xp.grad, xo.grad)]
    g_ref, g_got = LC.lora_grads(oa.processor), LC.lora_grads(pa.processor)
    errs += [LC.rel_inf(g_got[n], g_ref[n]) for n in g_ref]
    print(f"LoRA processor ({'text' if cross else 'self'}, {dtype}): output {errs[0]:.2e}, dX {errs[1]:.2e}, LoRA gradients max {max(errs[2:]):.2e}")
    assert len(g_ref) == 8 and all(g_ref[n].abs().max() > 0 for n in g_ref)
    assert max(errs) < tol


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 2e-2)])        # measured 3.5e-6 / 9.0e-3
def test_stage1_step_loss_and_lora_gradients(K, dtype, tol):
    """One stage-1 step on the reduced motion-free U-Net (W4 widths, 2 images): loss and the 256 LoRA gradients against the oracle."""
    ou, pu = LC.build_stage1(seed=7, device="cuda", dtype=dtype)
    batch = LC.stage1_batch(B=2, h=32, w=32)
    l_ref, g_ref, _ = LC.oracle_stage1_steps(ou, batch, steps=1)
    l_got, g_got, _ = LC.product_stage1_steps(pu, batch, steps=1, device="cuda", dtype=dtype)
    err = LC.rel_inf_dict(g_got, g_ref)
    lerr = abs(l_got[0] - l_ref[0]) / abs(l_ref[0])
    print(f"stage-1 step ({dtype}): loss {l_got[0]:.6f} vs {l_ref[0]:.6f} (rel {lerr:.2e}), LoRA gradient rel-inf {err:.2e}")
    assert len(g_got) == 256
    assert lerr < (1e-4 if dtype == torch.float32 else 2e-2) and err < tol


# measured: Adapter 8.5e-6 / 2.3e-2, LoRA 3.6e-6 / 9.6e-3 (fp32 / bf16)
@pytest.mark.parametrize("dtype,tol,tol_lora", [(torch.float32, 2e-5, 1e-5), (torch.bfloat16, 5e-2, 2e-2)])
def test_stage3_with_train_image_lora_gradients(K, dtype, tol, tol_lora):
    """Stage 3 with `train_image_lora` (train_cam_obj_ctrl.py:397-406): the Adapter AND the Domain LoRA train; both gradients against
    the oracle's autograd (bounds of test_stage3_training_gradients)."""
    from einops import rearrange
    from oracle import conditioning as OC
    from oracle import pipeline as OP
    from synfmc_amd.models.pose_obj_adaptor import CamObjPoseAdaptor
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.training import lora_trainable_parameters, masked_mse_loss
    from synfmc_amd.util import get_traj_features_v2
    from tests import training_common as TC
    ou, oe, oa = CM.build_oracle(W4, seed=20, fan_in_gain=0.7)
    pu, pe, pa = CM.build_product(ou, oe, oa, W4, dtype=dtype)
    clip = CM.synthetic_clip(B=1, Fr=16, H=128, W=128)
    with torch.no_grad():
        pose_emb = rearrange(OC.to_plucker_embedding(clip["c2w"], clip["K"], (128, 128)), "b f c h w -> b c f h w")
    noise = torch.randn(clip["latents"].shape, generator=torch.Generator().manual_seed(9))
    t = torch.tensor([801])
    # oracle
    ou.requires_grad_(False)
    oe.requires_grad_(False)
    oa.requires_grad_(True)
    lora_ref = {n: p for n, p in ou.named_parameters() if "_lora." in n and "motion_modules" not in n}
    for p in lora_ref.values():
        p.requires_grad_(True)
    noisy = TC.OD.DDIMScheduler(**TC.SCHED).add_noise(clip["latents"], noise, t)
    pose_feats = [rearrange(x, "(b f) c h w -> b c f h w", b=1) for x in oe(pose_emb)]
    traj = OC.get_traj_features(clip["infos"], clip["masks"], oa)
    pred = ou(noisy, t, clip["text"], pose_embedding_features=pose_feats, traj_features=traj).sample
    l_ref = OP.stage3_loss(pred, noise, TC.union_masks(clip), 0.3, 1.0)
    l_ref.backward()
    g_ref = {k: p.grad.clone() for k, p in oa.named_parameters() if p.grad is not None}
    g_ref.update({k: p.grad.clone() for k, p in lora_ref.items()})
    # product
    if dtype == torch.bfloat16:
        pa = pa.float()
    pa.requires_grad_(True)
    lora_got = dict(zip([n for n, p in pu.named_parameters() if "_lora." in n and "motion_modules" not in n], lora_trainable_parameters(pu)))
    dev = lambda v: v.to("cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        noisy = DDIMScheduler(**TC.SCHED).add_noise(dev(clip["latents"]), dev(noise), dev(t))
        tf = get_traj_features_v2(clip["infos"], clip["masks"], pa, False, 0.0, [False], "cuda", dtype)
        pred = CamObjPoseAdaptor(pu, pe)(noisy.to(dtype), dev(t), dev(clip["text"]).to(dtype), dev(pose_emb).to(dtype), tf)
        l_got = masked_mse_loss(pred, dev(noise), dev(TC.union_masks(clip)), 0.3, 1.0)
    l_got.backward()
    g_got = {k: p.grad.detach().float().cpu() for k, p in pa.named_parameters() if p.grad is not None}
    g_got.update({k: p.grad.detach().float().cpu() for k, p in lora_got.items()})
    assert set(g_ref) <= set(g_got) and len(lora_got) == 256
    lerr = abs(float(l_ref) - float(l_got)) / abs(float(l_ref))
    e_ada = LC.rel_inf_dict(g_got, {k: v for k, v in g_ref.items() if k not in lora_ref})
    e_lora = LC.rel_inf_dict(g_got, {k: g_ref[k] for k in lora_ref})
    print(f"stage 3 + train_image_lora ({dtype}): loss rel {lerr:.2e}, Adapter gradients {e_ada:.2e}, LoRA gradients {e_lora:.2e}")
    assert lerr < (1e-4 if dtype == torch.float32 else 2e-2) and e_ada < tol and e_lora < tol_lora


def test_stage1_step_full_width(K):
    """One stage-1 step at the configs/lora.yaml shapes (16 images of 256 x 384, SD-1.5 widths, rank C / 2 on all 32 processors, text
    16 x 77 x 768, random weights): finite loss, a non-zero gradient on every processor's LoRA."""
    from synfmc_amd.models.unet import UNet3DConditionModel
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.training import lora_trainable_parameters, stage1_training_step
    from tests.training_common import SCHED
    torch.manual_seed(0)
    pu = UNet3DConditionModel(**CM.unet_kwargs(CM.FULL_WIDTHS, CM.FULL_CROSS_DIM, motion=False))
    pu.set_image_layer_lora(2)
    pu = pu.to("cuda", torch.bfloat16).requires_grad_(False)
    with torch.no_grad():
        for n, p in pu.named_parameters():
            if n.endswith("_lora.up.weight"):
                p.normal_(0, 1e-3)                     # (zero-initialised up: every dD would be zero)
    trainable = lora_trainable_parameters(pu)
    assert len(trainable) == 256
    opt = torch.optim.AdamW(trainable, lr=1e-4)
    grads = {}
    names = {id(p): n for n, p in pu.named_parameters()}
    hooks = [p.register_post_accumulate_grad_hook(lambda q: grads.__setitem__(names[id(q)], q.grad.detach().abs().max().item()))
             for p in trainable]
    B = 16
    lat = torch.randn(B, 4, 32, 48, device="cuda", dtype=torch.bfloat16)
    loss = stage1_training_step(pu, trainable, DDIMScheduler(**SCHED), opt, None, lat, torch.randn_like(lat),
                                torch.randint(0, 1000, (B,), device="cuda"), torch.randn(B, 77, 768, device="cuda", dtype=torch.bfloat16))
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    procs = {n.split(".processor.")[0] for n in grads if grads[n] > 0}
    print(f"full-width stage-1 step: loss {float(loss):.4f}, processors with non-zero LoRA gradients: {len(procs)}")
    assert torch.isfinite(loss) and len(grads) == 256 and len(procs) == 32
    assert all(v > 0 and v == v for v in grads.values())

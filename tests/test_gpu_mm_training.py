"""`train_mm` on the MI355X: the GroupNorm backward with affine gradients (`fmc_groupnorm_silu_bwd_params`), the column sum
(`fmc_column_sum`), `hip_ops.linear_trainable`, one motion module and the stage-2 / stage-3 steps with trainable motion-module norm /
proj_in / proj_out against fp64 or the CPU oracle, the fp32-master inference path and one full-width stage-2 step."""
import pytest
import torch
import torch.nn.functional as F

from tests import common_models as CM
from tests import mm_common as MC

pytestmark = pytest.mark.gpu

W4 = (64, 128, 256, 256)
# (N, HW, C): the motion-module norms of the tool's stage-2 step (16 frames of 32 x 48 latents), then odd ones
GN_SHAPES = [(16, 1536, 320), (16, 384, 640), (16, 96, 1280), (16, 24, 1280), (16, 1536, 640), (16, 384, 1280), (3, 77, 64), (2, 1000, 96),
             (1, 5, 256)]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _gn_ref(x, gamma, beta, dy, act, addend):
    """fp64 autograd of F.group_norm (+SiLU) on the same (rounded) inputs: (dx, dgamma, dbeta)."""
    xd = x.double().permute(0, 2, 1).contiguous().requires_grad_(True)
    g = gamma.double().requires_grad_(True)
    b = beta.double().requires_grad_(True)
    y = F.group_norm(xd, 32, g, b, 1e-6)
    if act:
        y = F.silu(y)
    (y * dy.double().permute(0, 2, 1)).sum().backward()
    dx = xd.grad.permute(0, 2, 1)
    if addend is not None:
        dx = dx + addend.double()
    return dx, g.grad, b.grad


def _dx_only(K, dy, x, gamma, beta, stats, act, addend):
    from synfmc_amd import _lib
    N, S, C = x.shape
    lib = _lib.load()
    dx = torch.empty_like(x)
    ws = K._workspace(x.device, lib.fmc_groupnorm_workspace_bytes(N, C, 32))
    _lib.check(lib.fmc_groupnorm_silu_bwd_add(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(),
                                              ws.data_ptr(), N, S, C, 32, int(act), K._p(addend), K._dt(x), K._stream()), "bwd_add")
    return dx


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("N,HW,C", GN_SHAPES)
def test_gn_param_backward_matches_fp64(K, N, HW, C, dtype):
    g = torch.Generator(device="cuda").manual_seed(N * HW + C)
    x = (torch.randn(N, HW, C, device="cuda", generator=g) * 2 + 0.5).to(dtype)
    dy = torch.randn(N, HW, C, device="cuda", generator=g).to(dtype)
    add = torch.randn(N, HW, C, device="cuda", generator=g).to(dtype)
    gamma = torch.rand(C, device="cuda", generator=g) + 0.5
    beta = torch.randn(C, device="cuda", generator=g) * 0.5
    errs = []
    for act in (False, True):
        _, stats = K.groupnorm_silu_raw(x, gamma, beta, 32, 1e-6, act)
        for addend in (None, add):
            dx_ref, dg_ref, db_ref = _gn_ref(x, gamma, beta, dy, act, addend)
            dx, dg, db = K.groupnorm_silu_bwd_params(dy, x, gamma, beta, stats, 32, act, addend=addend)
            errs.append((MC.rel_inf(dx, dx_ref), MC.rel_inf(dg, dg_ref), MC.rel_inf(db, db_ref)))
            # dX: the bits of the dX-only backward; a second call: the same bits
            assert torch.equal(dx, _dx_only(K, dy, x, gamma, beta, stats, act, addend))
            dx2, dg2, db2 = K.groupnorm_silu_bwd_params(dy, x, gamma, beta, stats, 32, act, addend=addend)
            assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)
        # dx = NULL: the same affine gradients, nothing else; accumulate adds
        none, dg0, db0 = K.groupnorm_silu_bwd_params(dy, x, gamma, beta, stats, 32, act, want_dx=False)
        assert none is None and torch.equal(dg0, dg) and torch.equal(db0, db)
        acc_g, acc_b = torch.ones(C, device="cuda"), torch.full((C,), -2.0, device="cuda")
        K.groupnorm_silu_bwd_params(dy, x, gamma, beta, stats, 32, act, want_dx=False, dgamma=acc_g, dbeta=acc_b, accumulate=True)
        assert torch.equal(acc_g, dg + 1.0) and torch.equal(acc_b, db - 2.0)
    worst = [max(e[i] for e in errs) for i in range(3)]
    print(f"gn bwd params {(N, HW, C)} {dtype}: rel-inf dx {worst[0]:.2e} dgamma {worst[1]:.2e} dbeta {worst[2]:.2e}")
    tol_dx = 1e-2 if dtype == torch.bfloat16 else 1e-4
    assert worst[0] < tol_dx and worst[1] < 1e-4 and worst[2] < 1e-4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,N", [(24576, 320), (6144, 640), (1536, 1280), (384, 1280), (1000, 77), (1, 8), (77, 3)])
def test_column_sum_matches_fp64(K, M, N, dtype):
    g = torch.Generator(device="cuda").manual_seed(M + N)
    wide = torch.randn(M, 2 * N + 5, device="cuda", generator=g).to(dtype)
    x = wide[:, 3: 3 + N]                                                     # row-strided view, unaligned start
    ref = x.double().sum(0)
    got = K.column_sum(x, alpha=0.5)
    assert got.dtype == torch.float32 and got.shape == (N,)
    err = MC.rel_inf(got, 0.5 * ref)
    assert err < 1e-5, err
    assert torch.equal(got, K.column_sum(x, alpha=0.5))
    base = torch.randn(N, device="cuda", generator=g)
    acc = K.column_sum(x, alpha=-1.0, out=base.clone(), accumulate=True)
    assert MC.rel_inf(acc, base.double() - ref) < 1e-5
    dense = x.contiguous()
    assert torch.equal(K.column_sum(dense, alpha=0.5), got)


@pytest.mark.parametrize("M,Kd,N", [(6144, 320, 320), (1536, 640, 640), (384, 1280, 1280), (1000, 64, 128)])
@pytest.mark.parametrize("mode", ["bf16_fp32_master", "bf16_params", "fp32"])
def test_linear_trainable_matches_fp64(K, M, Kd, N, mode):
    from synfmc_amd.models.layers import bf16_param
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, Kd, generator=g)
    w = torch.randn(N, Kd, generator=g) / Kd ** 0.5
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    dy = torch.randn(M, N, generator=g)
    act = torch.float32 if mode == "fp32" else torch.bfloat16
    pdt = torch.bfloat16 if mode == "bf16_params" else torch.float32
    lin = torch.nn.Linear(Kd, N).to("cuda", pdt)
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(b)
    xs = x.to("cuda", act).requires_grad_(True)
    rs = r.to("cuda", act).requires_grad_(True)
    if mode == "bf16_fp32_master":
        y = K.linear_trainable(xs, lin.weight, lin.bias, rs, w_run=bf16_param(lin, "weight"), b_run=bf16_param(lin, "bias"))
    else:
        y = K.linear_trainable(xs, lin.weight, lin.bias, rs)
    y.backward(dy.to("cuda", act))
    wd, bd, xd, rd = (t.detach().double().cpu().requires_grad_(True) for t in (lin.weight, lin.bias, xs, rs))
    yr = xd @ wd.t() + bd + rd
    yr.backward(dy.to(act).double())
    assert lin.weight.grad.dtype == pdt and lin.bias.grad.dtype == pdt
    errs = dict(y=MC.rel_inf(y, yr.detach()), dx=MC.rel_inf(xs.grad, xd.grad), dw=MC.rel_inf(lin.weight.grad, wd.grad),
                db=MC.rel_inf(lin.bias.grad, bd.grad), dr=MC.rel_inf(rs.grad, rd.grad))
    print(f"linear_trainable {mode} {(M, Kd, N)}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    tol = 1e-5 if mode == "fp32" else 1e-2                       # bf16 activations / outputs: 2^-8 rounding of each element
    assert max(errs.values()) < tol
    assert errs["dw"] < (1e-5 if pdt == torch.float32 else 1e-2)


@pytest.mark.parametrize("x_grad", [False, True], ids=["input_frozen", "input_trains"])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 1.6e-2)])      # bf16 measured 7.95e-3, bound = measured x 2
def test_motion_module_gradients_match_oracle(K, x_grad, dtype, tol):
    """One motion module with trainable (fp32-master) norm / proj_in / proj_out against the oracle: output and all six gradients.  With the
    input frozen -- the first motion module of stages 2 / 3 -- gamma and beta still get their (non-zero) gradients."""
    from synfmc_amd.training import motion_module_trainable_parameters
    om, pm = MC.module_pair(C=128, seed=3, device="cuda", dtype=dtype)
    pm.requires_grad_(False)
    assert len(motion_module_trainable_parameters(pm)) == 6
    for p in MC.mm_params(om).values():
        p.requires_grad_(True)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 128, 16, 8, 12, generator=g)
    w = torch.randn(1, 128, 16, 8, 12, generator=g)
    ref, g_ref, dx_ref = MC.run_module(om, x, w, x_grad)
    got, g_got, dx_got = MC.run_module(pm, x.to("cuda", dtype), w, x_grad)
    errs = {"out": MC.rel_inf(got, ref)}
    assert set(g_got) == set(g_ref) == set(MC.MM_NAMES)
    errs.update({n: MC.rel_inf(g_got[n], g_ref[n]) for n in MC.MM_NAMES})
    if x_grad:
        errs["dx"] = MC.rel_inf(dx_got, dx_ref)
    print(f"motion module ({dtype}, input grad {x_grad}): " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(g_got[n].abs().max() > 0 for n in MC.MM_NAMES)
    assert max(errs.values()) < tol


# ---- stage 2 / stage 3 with train_mm on the reduced stack, against the oracle's autograd ------------------------------------------
def _oracle_step(ou, oe, oa, clip, pose_emb, t, noise, stage, lora):
    from einops import rearrange
    from oracle import conditioning as OC
    from oracle import pipeline as OP
    from tests import training_common as TC
    ou.requires_grad_(False)
    oe.requires_grad_(False)
    oa.requires_grad_(False)
    tr = {}
    if stage == 2:
        oe.requires_grad_(True)
        tr.update({"enc." + k: p for k, p in oe.named_parameters()})
        tr.update({"unet." + k: p for k, p in ou.named_parameters() if "_merge." in k})
    else:
        oa.requires_grad_(True)
        tr.update({"ada." + k: p for k, p in oa.named_parameters()})
        if lora:
            tr.update({"unet." + k: p for k, p in ou.named_parameters() if "_lora." in k and "motion_modules" not in k})
    tr.update({"unet." + k: dict(ou.named_parameters())[k] for k in MC.reference_mm_names(ou)})
    for p in tr.values():
        p.requires_grad_(True)
        p.grad = None
    noisy = TC.OD.DDIMScheduler(**TC.SCHED).add_noise(clip["latents"], noise, t)
    pose_feats = [rearrange(x, "(b f) c h w -> b c f h w", b=1) for x in oe(pose_emb)]
    if stage == 2:
        pred = ou(noisy, t, clip["text"], pose_embedding_features=pose_feats).sample
        loss = OP.stage3_loss(pred, noise, ~TC.union_masks(clip), 0.3, 1.0)
    else:
        traj = OC.get_traj_features(clip["infos"], clip["masks"], oa)
        pred = ou(noisy, t, clip["text"], pose_embedding_features=pose_feats, traj_features=traj).sample
        loss = OP.stage3_loss(pred, noise, TC.union_masks(clip), 0.3, 1.0)
    loss.backward()
    grads = {k: (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for k, p in tr.items()}
    for p in tr.values():
        p.requires_grad_(False)
    return float(loss), grads


def _product_step(pu, pe, pa, clip, pose_emb, t, noise, stage, lora, dtype):
    from synfmc_amd.models.pose_adaptor import PoseAdaptor
    from synfmc_amd.models.pose_obj_adaptor import CamObjPoseAdaptor
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.training import lora_trainable_parameters, masked_mse_loss, motion_module_trainable_parameters
    from synfmc_amd.util import get_traj_features_v2
    from tests import training_common as TC
    names = {id(p): n for n, p in pu.named_parameters()}
    tr = {}
    if stage == 2:
        pe = pe.float() if dtype == torch.bfloat16 else pe
        pe.requires_grad_(True)
        tr.update({"enc." + k: p for k, p in pe.named_parameters()})
        for k, p in pu.named_parameters():
            if "_merge." in k:
                p.requires_grad_(True)
                tr["unet." + k] = p
    else:
        pa = pa.float() if dtype == torch.bfloat16 else pa
        pa.requires_grad_(True)
        tr.update({"ada." + k: p for k, p in pa.named_parameters()})
        if lora:
            tr.update({"unet." + names[id(p)]: p for p in lora_trainable_parameters(pu)})
    mm = motion_module_trainable_parameters(pu)
    tr.update({"unet." + n: p for n, p in pu.named_parameters() if any(p is q for q in mm)})
    dev = lambda v: v.to("cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        noisy = DDIMScheduler(**TC.SCHED).add_noise(dev(clip["latents"]), dev(noise), dev(t))
        if stage == 2:
            pred = PoseAdaptor(pu, pe)(noisy.to(dtype), dev(t), dev(clip["text"]).to(dtype), dev(pose_emb).to(dtype))
            loss = masked_mse_loss(pred, dev(noise), dev(TC.union_masks(clip)), 0.3, 1.0, invert=True)
        else:
            tf = get_traj_features_v2(clip["infos"], clip["masks"], pa, False, 0.0, [False], "cuda", dtype)
            pred = CamObjPoseAdaptor(pu, pe)(noisy.to(dtype), dev(t), dev(clip["text"]).to(dtype), dev(pose_emb).to(dtype), tf)
            loss = masked_mse_loss(pred, dev(noise), dev(TC.union_masks(clip)), 0.3, 1.0)
    loss.backward()
    grads = {k: (p.grad.detach().float().cpu() if p.grad is not None else torch.zeros(p.shape)) for k, p in tr.items()}
    return float(loss), grads, len(mm)


@pytest.fixture(scope="module")
def small_clip():
    from einops import rearrange
    from oracle import conditioning as OC
    clip = CM.synthetic_clip(B=1, Fr=16, H=128, W=128)
    with torch.no_grad():
        pose_emb = rearrange(OC.to_plucker_embedding(clip["c2w"], clip["K"], (128, 128)), "b f c h w -> b c f h w")
    return clip, pose_emb


# bounds: fp32 1e-4 (measured <= 8.9e-6); bf16 measured x 2 (worst measured 1.63e-2, stage 2 mm gradients, rounded up)
# per tensor (relative to the tensor's own largest gradient): measured x 2 (worst 2.53e-5 / 3.97e-2, a deep norm's gamma)
@pytest.mark.parametrize("dtype,tol,tol_tensor", [(torch.float32, 1e-4, 5e-5), (torch.bfloat16, 3e-2, 8e-2)])
@pytest.mark.parametrize("stage,lora", [(2, False), (3, False), (3, True)], ids=["stage2", "stage3", "stage3_image_lora"])
def test_train_mm_stage_gradients_match_oracle(K, small_clip, stage, lora, dtype, tol, tol_tensor):
    clip, pose_emb = small_clip
    ou, oe, oa = CM.build_oracle(W4, seed=21 + stage, fan_in_gain=0.7)
    pu, pe, pa = CM.build_product(ou, oe, oa, W4, dtype=dtype)
    noise = torch.randn(clip["latents"].shape, generator=torch.Generator().manual_seed(11))
    t = torch.tensor([423])
    l_ref, g_ref = _oracle_step(ou, oe, oa, clip, pose_emb, t, noise, stage, lora)
    l_got, g_got, n_mm = _product_step(pu, pe, pa, clip, pose_emb, t, noise, stage, lora, dtype)
    assert n_mm == 120 and set(g_ref) == set(g_got)
    mm = {k: v for k, v in g_ref.items() if k.startswith("unet.") and ".temporal_transformer." in k and "transformer_blocks" not in k}
    rest = {k: v for k, v in g_ref.items() if k not in mm}
    assert len(mm) == 120 and rest
    first = "unet.down_blocks.0.motion_modules.0.temporal_transformer.norm."
    assert g_got[first + "weight"].abs().max() > 0 and g_got[first + "bias"].abs().max() > 0      # (its input needs no gradient)
    lerr = abs(l_ref - l_got) / abs(l_ref)
    e_mm, s_mm = CM_compare(mm, g_got)
    e_rest, s_rest = CM_compare(rest, g_got)
    e_first = max(MC.rel_inf(g_got[first + s], g_ref[first + s]) for s in ("weight", "bias"))
    # every mm tensor on its own: non-zero where the oracle's is, and within a bound relative to its OWN largest gradient
    per = {k: MC.rel_inf(g_got[k], g_ref[k]) for k in mm}
    worst = max(per, key=per.get)
    print(f"train_mm stage {stage}{' + image LoRA' if lora else ''} ({dtype}): loss rel {lerr:.2e}, mm gradients {e_mm:.3e}, "
          f"first norm {e_first:.3e}, other trainables {e_rest:.3e} (tolerance {tol}); worst single mm tensor {per[worst]:.3e} "
          f"({worst[5:]}, tolerance {tol_tensor})")
    assert all(g_ref[k].abs().max() > 0 and g_got[k].abs().max() > 0 for k in mm)
    assert lerr < (1e-4 if dtype == torch.float32 else 2e-2)
    assert s_mm > 0 and s_rest > 0 and e_mm < tol and e_rest < tol and e_first < tol
    assert per[worst] < tol_tensor


def CM_compare(ref, got):
    r = torch.cat([ref[k].reshape(-1) for k in ref]).double()
    g = torch.cat([got[k].reshape(-1).double() for k in ref])
    return ((r - g).abs().max() / r.abs().max()).item(), float(r.abs().max())


# ---- fp32 masters at inference, and one full-width step -------------------------------------------------------------------------
def _full_unet(seed=0):
    from synfmc_amd.models.unet import UNet3DConditionModel
    torch.manual_seed(seed)
    return UNet3DConditionModel(**CM.unet_kwargs(CM.FULL_WIDTHS, CM.FULL_CROSS_DIM)).to("cuda", torch.bfloat16).eval().requires_grad_(False)


def test_fp32_master_inference_is_bit_identical_and_refreshes(K):
    """No-grad output with fp32-master mm parameters == the same values stored in bf16 (bit for bit: the fused inference path reads the
    bf16 shadows); after one AdamW step (lr 1e-4) the output moves and equals a fresh model loaded with the rounded new weights -- every
    derived-weight cache (GroupNorm fold, ff_tail fold, tile-major packs) was rebuilt."""
    from synfmc_amd.training import motion_module_state_dict, motion_module_trainable_parameters
    ref_model = _full_unet()
    model = _full_unet()
    g = torch.Generator(device="cuda").manual_seed(5)
    lat = torch.randn(1, 4, 16, 32, 48, device="cuda", generator=g).to(torch.bfloat16)
    text = torch.randn(1, 77, 768, device="cuda", generator=g).to(torch.bfloat16)
    t = torch.tensor([500], device="cuda")
    run = lambda m: m(lat, t, text).sample.float()
    with torch.no_grad():
        base = run(ref_model)
        masters = motion_module_trainable_parameters(model)
        assert len(masters) == 120
        assert torch.equal(run(model), base)
        assert torch.equal(run(model), base)                  # (second call: cached derived weights)
    opt = torch.optim.AdamW(masters, lr=1e-4)
    for p in masters:
        p.grad = torch.randn(p.shape, device="cuda", generator=g)
    opt.step()
    with torch.no_grad():
        moved = run(model)
        fresh = _full_unet()
        sd = {k: v.to(torch.bfloat16) for k, v in motion_module_state_dict(model).items()}
        missing, unexpected = fresh.load_state_dict(sd, strict=False)
        assert unexpected == []
        want = run(fresh)
    diff = (moved - base).abs().max().item()
    print(f"fp32-master inference: one AdamW step moved the output by {diff:.3e} (max abs)")
    assert diff > 0 and torch.equal(moved, want)


def test_train_mm_full_width_stage2_step(K):
    """One stage-2 step at the cam.yaml shapes (tools/mm_train_step.py) with train_mm: every mm tensor gets a finite, non-zero gradient
    and every master moves."""
    from tools.mm_train_step import build_stage2, stage2_step_fn
    pu, pe = build_stage2()
    step, trainable, mm = stage2_step_fn(pu, pe, True)
    n_modules = sum(1 for m in pu.modules() if m.__class__.__name__ == "TemporalTransformer3DModel")
    assert len(mm) == 6 * n_modules == 120
    before = [p.detach().clone() for p in mm]
    grads = {}
    hooks = [p.register_post_accumulate_grad_hook(lambda q, i=i: grads.__setitem__(i, (q.grad.abs().max().item(),
                                                                                     bool(torch.isfinite(q.grad).all()))))
             for i, p in enumerate(mm)]
    loss = step()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    moved = sum(1 for p, b in zip(mm, before) if not torch.equal(p.detach(), b))
    print(f"full-width stage-2 step with train_mm: loss {float(loss):.4f}, mm tensors with gradients {len(grads)}, masters moved {moved}")
    assert torch.isfinite(loss) and len(grads) == 120
    assert all(v[0] > 0 and v[1] for v in grads.values())
    assert moved == 120 and all(p.dtype == torch.float32 for p in mm)

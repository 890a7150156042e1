"""`training.FusedAdamW` on the MI355X: the kernels of csrc/optim.hip against torch's AdamW + clip_grad_norm_ in float64 (the yardstick:
torch's own float32 run, tests/optim_common.py), bit-reproducibility, HIP-graph replay, the stale-cache guard on the full-width model and
the Domain LoRA, real stage-1 gradients, and accumulation below a bf16 ulp.

The norm bound 1e-6 is derived, not tuned: the in-chunk sum of <= 8192 squares is a TREE of depth 13 (csrc/optim.hip), so with the rounding of
the squares it is off by at most 14 * 2^-24 = 8.4e-7 relative; the square root halves that, the fp64 combine adds nothing visible."""
import pytest
import torch

from tests import common_models as CM
from tests import optim_common as OC

pytestmark = pytest.mark.gpu

HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-4)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


class _Holder(torch.nn.Module):
    def __init__(self, p):
        super().__init__()
        self.weight = p


def _with_shadows(params):
    """Modules that own `params`, their `bf16_param` shadows created as the first forward would."""
    from synfmc_amd.models.layers import bf16_param
    box = torch.nn.ModuleList([_Holder(p) for p in params])
    for h in box:
        bf16_param(h, "weight")
        bf16_param(h, "weight", rounded_f32=True)
    return box


def _shadow(box, i):
    hit = box[i].__dict__["_bf16_shadow"]["weight"]
    return hit[1], hit[2]


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


SIZES = [(1,), (7,), (4099,), (3,), (5,), (8,), (9,), (63,), (64,), (65,), (255,), (257,), (1023,), (4097,), (8191,), (8192,), (8193,),
         (16385,), (12345,), (320,), (640,), (1280,), (320, 320), (640, 641), (1280, 320), (3, 3, 64, 33), (100003,), (1000003,), (5000000,),
         (2500001,), (1280, 1280), (77, 768), (16, 9), (2, 2), (31,), (33,), (129,), (511,), (513,), (2049,)]
CANARIES = {1: (3,), 4: (5,), 9: (1,), 15: (6,), 28: (2,)}      # packed into the buckets BEHIND tensor i, absent from the optimizer


def test_kernels_against_float64(K):
    """GPU test 1: 40 tensors of 1 .. 5 M elements, gradients as GradAllReducer bucket views (only 4-byte aligned), two clip groups (one
    above max_grad_norm, one below) + unclipped tensors, two hyper-parameter groups, shadows on a third: condition 1 after 1, 3, 10 steps;
    the norms to 1e-6; shadows, zeroed gradients and untouched neighbours as integers."""
    from synfmc_amd.training import FusedAdamW, GradAllReducer
    params = OC.make_tensors(SIZES, "cuda", 0)
    n = len(params)
    canaries = {i: torch.nn.Parameter(torch.randn(s, device="cuda")) for i, s in CANARIES.items()}
    order = []
    for i, p in enumerate(params):
        order.append(p)
        if i in canaries:
            order.append(canaries[i])
    reducer = GradAllReducer(order, bucket_bytes=24 << 20, find_unused=False)
    assert len(reducer.buckets) >= 2
    offs = {p.grad.data_ptr() % 16 for p in params}
    assert offs == {0, 4, 8, 12}, offs                           # every misalignment of g occurs
    sets = [[i for i in range(n) if i % 3 == 0], [i for i in range(n) if i % 3 == 1]]
    sigma = [1e-2 if i % 3 != 1 else 1e-6 for i in range(n)]
    shadowed = [i for i in range(n) if i % 3 == 2 or i in (0, 1, 2)]
    box = _with_shadows([params[i] for i in shadowed])
    groups = [(list(range(0, n, 2)), dict(weight_decay=1e-2, **HYPER)), (list(range(1, n, 2)), dict(weight_decay=0.0, **HYPER))]
    ref64, ref32 = OC.TorchRef(params, torch.float64, groups), OC.TorchRef(params, torch.float32, groups)
    opt = FusedAdamW([dict(params=[params[i] for i in idx], **h) for idx, h in groups]).attach(box)
    canary_state = {i: [torch.randn_like(c) for _ in range(3)] for i, c in canaries.items()}       # stands for its p, m, v
    for k in range(1, 11):
        grads = [g * (s / 1e-2) for g, s in zip(OC.make_grads(SIZES, 100 + k, 1e-2), sigma)]
        for p, g in zip(params, grads):
            p.grad.copy_(g)
        for i, c in canaries.items():
            c.grad.copy_(canary_state[i][0])
        keep = {i: [_bits(c).clone(), _bits(c.grad).clone()] + [_bits(t).clone() for t in canary_state[i]] for i, c in canaries.items()}
        n64 = ref64.step(grads, sets, 1.0)
        ref32.step(grads, sets, 1.0)
        opt.step(clip_groups=[[params[i] for i in s] for s in sets], max_grad_norm=1.0, zero=True)
        norms = opt.grad_norms.cpu()
        assert float(n64[0]) > 1.0 > float(n64[1])
        for c in range(2):
            rel = abs(float(norms[c]) - float(n64[c])) / float(n64[c])
            print(f"step {k} clip group {c}: norm {float(norms[c]):.9e} float64 {float(n64[c]):.9e} rel {rel:.2e}")
            assert rel <= 1e-6
        for j, i in enumerate(shadowed):
            sb, sf = _shadow(box, j)
            want = params[i].detach().to(torch.bfloat16)
            assert torch.equal(_bits(sb), _bits(want)) and torch.equal(_bits(sf), _bits(want.float())), SIZES[i]
        assert all(int(_bits(p.grad).abs().max()) == 0 for p in params)
        for i, c in canaries.items():
            now = [_bits(c), _bits(c.grad)] + [_bits(t) for t in canary_state[i]]
            assert all(torch.equal(a, b) for a, b in zip(keep[i], now)), f"canary behind tensor {i} changed"
        if k in (1, 3, 10):
            OC.assert_condition_1(f"MI355X, step {k}", OC.fused_measures(params, opt, ref64, HYPER["lr"]),
                                  OC.torch32_measures(ref32, ref64, HYPER["lr"]))
    assert opt.rebuilds == 1
    assert all(float(opt.state[p]["step"]) == 10.0 for p in params)


def test_bit_reproducible_at_stage3_size(K):
    """GPU test 2: 91.9 M elements in 24 synthetic tensors, two runs on equal inputs: identical bits (parameters, states, norms), and the
    norm within 1e-6 of float64."""
    from synfmc_amd.training import FusedAdamW
    sizes = [(3829171 + 7 * i,) for i in range(24)]              # 91.9 M, every alignment of the tails
    assert abs(sum(s[0] for s in sizes) - 91.9e6) < 0.1e6
    results = []
    for run in range(2):
        gen = torch.Generator(device="cuda").manual_seed(11)
        params = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen) * 0.05) for s in sizes]
        opt = FusedAdamW(params, weight_decay=1e-2, **HYPER)
        for k in range(2):
            for p in params:
                g = torch.randn(p.shape, device="cuda", generator=gen) * 1e-3
                if p.grad is None:
                    p.grad = g
                else:
                    p.grad.copy_(g)
            if run == 0 and k == 0:
                n64 = sum(float(p.grad.double().pow(2).sum()) for p in params) ** 0.5
            opt.step(clip_groups=[params], max_grad_norm=1.0)
            if run == 0 and k == 0:
                rel = abs(float(opt.grad_norms[0]) - n64) / n64
                print(f"91.9 M elements: norm {float(opt.grad_norms[0]):.9e} float64 {n64:.9e} rel {rel:.2e}")
                assert n64 > 1.0 and rel <= 1e-6
        results.append(([_bits(p).clone() for p in params], [_bits(opt.state[p]["exp_avg"]).clone() for p in params],
                        [_bits(opt.state[p]["exp_avg_sq"]).clone() for p in params], _bits(opt.grad_norms).clone()))
        del params, opt
    a, b = results
    for x, y in zip(a[:3], b[:3]):
        assert all(torch.equal(s, t) for s, t in zip(x, y))
    assert torch.equal(a[3], b[3])


def _graph_arm(seed=3):
    from synfmc_amd.training import FusedAdamW, GradAllReducer
    shapes = [(4099,), (7,), (320, 320), (1,), (64, 33), (100003,)]
    params = OC.make_tensors(shapes, "cuda", seed)
    reducer = GradAllReducer(params, bucket_bytes=1 << 20, find_unused=False)
    opt = FusedAdamW(params, weight_decay=1e-2, **HYPER)
    return shapes, params, reducer, opt


def test_captured_update_replays_like_eager_steps(K):
    """GPU test 3: `optimizer_update` captured in one torch.cuda.graph, replayed three times with new gradients in the buckets and a new
    rate pushed between the replays == three eager fused steps, bit for bit.  A table rebuild under capture raises."""
    from synfmc_amd.training import FusedAdamW, optimizer_update
    shapes, pa, ra, oa = _graph_arm()
    _, pb, rb, ob = _graph_arm()
    grads = [[g.cuda() for g in OC.make_grads(shapes, 700 + k, 1e-2)] for k in range(3)]
    rates = [1e-3, 5e-4, 2.5e-4]
    norms_a, norms_b = [], []
    for k in range(3):
        for p, g in zip(pa, grads[k]):
            p.grad.copy_(g)
        oa.param_groups[0]["lr"] = rates[k]
        optimizer_update(pa, oa, ra, 1.0)
        norms_a.append(_bits(oa.grad_norms).clone())
    # arm B: one eager step builds the table and the state; the initial values are then restored IN PLACE (the addresses are the table's)
    init = [p.detach().clone() for p in pb]
    for p, g in zip(pb, grads[0]):
        p.grad.copy_(g)
    optimizer_update(pb, ob, rb, 1.0)
    with torch.no_grad():
        for p, p0 in zip(pb, init):
            p.copy_(p0)
            ob.state[p]["exp_avg"].zero_()
            ob.state[p]["exp_avg_sq"].zero_()
        ob._steps.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        optimizer_update(pb, ob, rb, 1.0)
    assert ob.rebuilds == 1
    for k in range(3):
        for p, g in zip(pb, grads[k]):
            p.grad.copy_(g)
        ob.param_groups[0]["lr"] = rates[k]
        ob.push_hyperparameters()
        graph.replay()
        norms_b.append(_bits(ob.grad_norms).clone())
    ob.mark_updated()
    torch.cuda.synchronize()
    for a, b in zip(pa, pb):
        assert torch.equal(_bits(a), _bits(b))
        for name in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(_bits(oa.state[a][name]), _bits(ob.state[b][name])), name
        assert int(_bits(b.grad).abs().max()) == 0
    assert all(torch.equal(x, y) for x, y in zip(norms_a, norms_b))
    assert float(ob.state[pb[0]]["step"]) == 3.0
    # a fresh optimizer has no table: building one under capture must raise before anything is launched
    fresh = FusedAdamW(pb, **HYPER)
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="rebuilt inside a HIP-graph capture"):
        with torch.cuda.graph(g2):
            fresh.step(clip_groups=[pb], max_grad_norm=1.0)


def _full_unet(seed=0):
    from synfmc_amd.models.unet import UNet3DConditionModel
    torch.manual_seed(seed)
    return UNet3DConditionModel(**CM.unet_kwargs(CM.FULL_WIDTHS, CM.FULL_CROSS_DIM)).to("cuda", torch.bfloat16).eval().requires_grad_(False)


def test_stale_cache_guard_full_width_mm(K, monkeypatch):
    """GPU test 4a: `test_fp32_master_inference_is_bit_identical_and_refreshes` of test_gpu_mm_training.py with FusedAdamW: after the fused
    step the no-grad output moves and equals a fresh model loaded with the new masters rounded to bf16, and the forward after the step
    performs no `bf16_param` copy for a shadow the kernel refreshed."""
    from synfmc_amd.models import layers
    from synfmc_amd.training import FusedAdamW, motion_module_state_dict, motion_module_trainable_parameters
    model = _full_unet()
    g = torch.Generator(device="cuda").manual_seed(5)
    lat = torch.randn(1, 4, 16, 32, 48, device="cuda", generator=g).to(torch.bfloat16)
    text = torch.randn(1, 77, 768, device="cuda", generator=g).to(torch.bfloat16)
    t = torch.tensor([500], device="cuda")
    run = lambda m: m(lat, t, text).sample.float()
    stale = []
    real = layers.bf16_param

    def counting(mod, name, rounded_f32=False):
        p = getattr(mod, name)
        hit = mod.__dict__.get("_bf16_shadow", {}).get(name)
        if p is not None and p.dtype == torch.float32 and (hit is None or hit[0] != (p.data_ptr(), p._version)):
            stale.append((mod.__class__.__name__, name))
        return real(mod, name, rounded_f32)
    monkeypatch.setattr(layers, "bf16_param", counting)
    with torch.no_grad():
        masters = motion_module_trainable_parameters(model)
        assert len(masters) == 120
        base = run(model)
        assert len(stale) > 0                                   # (the first forward creates the shadows)
        stale.clear()
        assert torch.equal(run(model), base) and stale == []
    opt = FusedAdamW(masters, lr=1e-4).attach(model)
    for p in masters:
        p.grad = torch.randn(p.shape, device="cuda", generator=g)
    opt.step()
    refreshed = sum(1 for e in opt._plan.entries if e["shadow_bf16"] is not None)
    assert refreshed > 0
    with torch.no_grad():
        moved = run(model)
        copies = len(stale)
        fresh = _full_unet()
        sd = {k: v.to(torch.bfloat16) for k, v in motion_module_state_dict(model).items()}
        missing, unexpected = fresh.load_state_dict(sd, strict=False)
        assert unexpected == []
        want = run(fresh)
    diff = (moved - base).abs().max().item()
    print(f"fused step on 120 masters: output moved by {diff:.3e}; shadows refreshed by the kernel {refreshed}, bf16_param copies after it {copies}")
    assert diff > 0 and torch.equal(moved, want)
    assert copies == 0


def test_stale_cache_guard_domain_lora(K, monkeypatch):
    """GPU test 4b: after a fused step on synthetic factor gradients the next forward equals a fresh model loaded with the stepped
    factors: `lora_group_weights` rebuilt from the version bump.  (Bit equality of two forwards needs a fixed arm choice: no timing-
    dependent autotuning, no vendor convolution with atomics on these small images -- the switches hip_ops documents for that.)"""
    monkeypatch.setattr(K, "AUTOTUNE", False)
    monkeypatch.setattr(K, "DETERMINISTIC", True)
    from synfmc_amd.training import FusedAdamW, lora_state_dict, lora_trainable_parameters
    from tests import lora_common as LC
    _, pu = LC.build_stage1(seed=7, device="cuda", dtype=torch.bfloat16)
    batch = LC.stage1_batch(B=2, h=32, w=32)
    x = batch["latents"].cuda().to(torch.bfloat16).unsqueeze(2)
    run = lambda m: m(x, batch["t"].cuda(), batch["text"].cuda().to(torch.bfloat16)).sample.float()
    factors = lora_trainable_parameters(pu)
    with torch.no_grad():
        base = run(pu)
        assert torch.equal(run(pu), base)
    opt = FusedAdamW(factors, lr=1e-2).attach(pu)
    g = torch.Generator(device="cuda").manual_seed(9)
    for p in factors:
        p.grad = torch.randn(p.shape, device="cuda", generator=g)
    opt.step(clip_groups=[factors], max_grad_norm=1.0)
    with torch.no_grad():
        moved = run(pu)
        _, fresh = LC.build_stage1(seed=7, device="cuda", dtype=torch.bfloat16)
        lora_trainable_parameters(fresh)
        missing, unexpected = fresh.load_state_dict(lora_state_dict(pu), strict=False)
        assert unexpected == []
        want = run(fresh)
    diff = (moved - base).abs().max().item()
    print(f"fused step on {len(factors)} LoRA factors: output moved by {diff:.3e}")
    assert diff > 0 and torch.equal(moved, want)


def test_real_stage1_gradients(K):
    """GPU test 5: one stage-1 forward / backward on the GPU; float64 torch AdamW + clip steps float64 copies with the cloned gradients,
    FusedAdamW steps the model: condition 1 at lr 1e-3."""
    import torch.nn.functional as F
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.training import FusedAdamW, lora_trainable_parameters
    from tests import lora_common as LC
    from tests.training_common import SCHED
    _, pu = LC.build_stage1(seed=7, device="cuda", dtype=torch.bfloat16)
    batch = LC.stage1_batch(B=2, h=32, w=32)
    trainable = lora_trainable_parameters(pu)
    lat, noise = batch["latents"].cuda().to(torch.bfloat16), batch["noise"].cuda().to(torch.bfloat16)
    noisy = DDIMScheduler(**SCHED).add_noise(lat, noise, batch["t"].cuda())
    pred = pu(noisy.unsqueeze(2), batch["t"].cuda(), batch["text"].cuda().to(torch.bfloat16)).sample.squeeze(2)
    F.mse_loss(pred.float(), noise.float()).backward()
    grads = [p.grad.detach().clone() for p in trainable]
    assert all(g.dtype == torch.float32 and bool(torch.isfinite(g).all()) for g in grads)
    idx = list(range(len(trainable)))
    hyper = dict(weight_decay=1e-2, **HYPER)
    ref64, ref32 = OC.TorchRef(trainable, torch.float64, [(idx, hyper)]), OC.TorchRef(trainable, torch.float32, [(idx, hyper)])
    n64 = ref64.step(grads, [idx], 1.0)[0]
    ref32.step(grads, [idx], 1.0)
    opt = FusedAdamW(trainable, **hyper).attach(pu)
    opt.step(clip_groups=[trainable], max_grad_norm=1.0)
    rel = abs(float(opt.grad_norms[0]) - float(n64)) / float(n64)
    print(f"stage-1 gradients: {len(trainable)} tensors, norm {float(n64):.4e}, rel error of the fused norm {rel:.2e}")
    assert rel <= 1e-6
    OC.assert_condition_1("stage-1 gradients, 1 step", OC.fused_measures(trainable, opt, ref64, HYPER["lr"]),
                          OC.torch32_measures(ref32, ref64, HYPER["lr"]))


def test_updates_below_a_bf16_ulp_accumulate(K):
    """GPU test 6: lr 1e-6, a master at 0.05 (bf16 ulp 2.4e-4), constant-sign gradients: 20 fused steps move the master by about
    20 * 1e-6 while the bf16 shadow changes at most once -- what the fp32-master rule exists for, through the fused path."""
    from synfmc_amd.training import FusedAdamW
    p = torch.nn.Parameter(torch.full((1000,), 0.05, device="cuda"))
    box = _with_shadows([p])
    opt = FusedAdamW([p], lr=1e-6, weight_decay=0.0).attach(box)
    p.grad = torch.full((1000,), 0.3, device="cuda")
    sb, sf = _shadow(box, 0)
    changes, last = 0, _bits(sb).clone()
    for _ in range(20):
        opt.step()
        assert torch.equal(_bits(sb), _bits(p.detach().to(torch.bfloat16))) and torch.equal(_bits(sf), _bits(p.detach().to(torch.bfloat16).float()))
        changes += int(not torch.equal(_bits(sb), last))
        last = _bits(sb).clone()
    moved = 0.05 - p.detach().double()
    print(f"20 steps at lr 1e-6: master moved by {float(moved.mean()):.4e}, bf16 shadow changed {changes} time(s)")
    assert float((moved - 20e-6).abs().max()) < 2e-6 and changes <= 1

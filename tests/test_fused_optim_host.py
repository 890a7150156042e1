"""Host-side checks of `training.FusedAdamW` and its wiring.  The two kernels are replaced by the plain-PyTorch restatement of their
contract in tests/optim_common.py (the pattern of tests/fake_kernels.py); everything above them -- the tables, clip groups, torch
semantics, the state-dict format, the reducer re-arming -- is the code under test.  The reference is torch's AdamW + clip_grad_norm_ in
float64; the yardstick torch's own float32 run (see optim_common)."""
import copy
import ctypes
import re

import pytest
import torch

from synfmc_amd import hip_ops as K
from synfmc_amd import training as T
from tests import optim_common as OC

SHAPES = [(1,), (7,), (4099,), (64, 33), (128,), (96, 160)]      # 21 871 elements: with sigma 1e-2 the norm is ~1.5, clipping is active
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-4, weight_decay=1e-2)


@pytest.fixture
def fake(monkeypatch):
    OC.install(monkeypatch)


def _set_grads(params, grads):
    """In place where a gradient exists: its address is part of what the optimizer's table is keyed on."""
    for p, g in zip(params, grads):
        if g is None:
            p.grad = None
        elif p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)


def _refs(params, hyper=HYPER):
    idx = list(range(len(params)))
    return OC.TorchRef(params, torch.float64, [(idx, hyper)]), OC.TorchRef(params, torch.float32, [(idx, hyper)])


def test_ten_steps_one_clip_group_against_float64(fake):
    """Test 1: 10 steps, one clip group, sizes 1 / 7 / 4099 among the shapes: condition 1 after 1, 3 and 10 steps, the norm to 1e-6."""
    params = OC.make_tensors(SHAPES, "cpu", 0)
    ref64, ref32 = _refs(params)
    opt = T.FusedAdamW(params, **HYPER)
    everything = list(range(len(params)))
    for k in range(1, 11):
        grads = OC.make_grads(SHAPES, 100 + k, 1e-2)
        _set_grads(params, grads)
        n64 = ref64.step(grads, [everything], 1.0)[0]
        ref32.step(grads, [everything], 1.0)
        opt.step(clip_groups=[params], max_grad_norm=1.0)
        rel = abs(float(opt.grad_norms[0]) - float(n64)) / float(n64)
        assert float(n64) > 1.0 and rel <= 1e-6, (k, float(n64), rel)
        if k in (1, 3, 10):
            OC.assert_condition_1(f"host, step {k}", OC.fused_measures(params, opt, ref64, HYPER["lr"]), OC.torch32_measures(ref32, ref64, HYPER["lr"]))
    assert opt.rebuilds == 1


def test_clip_groups_each_on_its_own(fake):
    """Test 2a: one group above max_grad_norm, one below, the rest unclipped: each equals clip_grad_norm_ per group in float64."""
    params = OC.make_tensors(SHAPES, "cpu", 1)
    ref64, ref32 = _refs(params)
    opt = T.FusedAdamW(params, **HYPER)
    sets = [[2, 3], [0, 1, 4]]                                    # tensor 5 is in no group
    sig = [1e-4, 1e-4, 1e-1, 1e-1, 1e-4, 1e-1]
    for k in range(1, 4):
        grads = [g * s / 1e-2 for g, s in zip(OC.make_grads(SHAPES, 200 + k, 1e-2), sig)]
        _set_grads(params, grads)
        n64 = ref64.step(grads, sets, 1.0)
        ref32.step(grads, sets, 1.0)
        opt.step(clip_groups=[[params[i] for i in s] for s in sets], max_grad_norm=1.0)
        assert float(n64[0]) > 1.0 > float(n64[1])
        for c in range(2):
            assert abs(float(opt.grad_norms[c]) - float(n64[c])) / float(n64[c]) <= 1e-6
        OC.assert_condition_1(f"host clip groups, step {k}", OC.fused_measures(params, opt, ref64, HYPER["lr"]),
                              OC.torch32_measures(ref32, ref64, HYPER["lr"]))
    with pytest.raises(ValueError):
        params[0].grad = torch.zeros(1)
        opt.step(clip_groups=[[params[0]], [params[0]]], max_grad_norm=1.0)


class _Sched:
    def add_noise(self, latents, noise, t):
        return latents + noise


class _Toy(torch.nn.Module):
    """Stands in for the pose adaptor: a prediction that depends on every parameter handed in (so each gets a gradient)."""

    def __init__(self, params):
        super().__init__()
        self.ps = list(params)

    def forward(self, noisy, t, encoder_hidden_states=None, pose_embedding=None, traj_features=None):
        return noisy * sum((p.float() * 1e3).sum() for p in self.ps)


@pytest.mark.parametrize("with_lora,with_mm", [(True, False), (False, True), (True, True)], ids=["lora", "mm", "lora_and_mm"])
def test_stage3_routes_the_clip_groups(fake, monkeypatch, with_lora, with_mm):
    """Test 2b: `stage3_training_step` with a FusedAdamW hands the groups of `stage3_clip_groups` to ONE step call and calls no
    clip_grad_norm_: the Adapter alone; LoRA + mm as one group with `lora_params`; `mm_params` alone unclipped."""
    omcm = torch.nn.Linear(4, 4)
    lora = [torch.nn.Parameter(torch.randn(4, 2)) for _ in range(2)] if with_lora else None
    mm = [torch.nn.Parameter(torch.randn(3)) for _ in range(3)] if with_mm else None
    everything = list(omcm.parameters()) + (lora or []) + (mm or [])
    opt = T.FusedAdamW(everything, lr=1e-3)
    seen = []
    real = T.FusedAdamW.step

    def rec(self, *a, **k):
        seen.append(([{id(p) for p in g} for g in k["clip_groups"]], k["max_grad_norm"], k["zero"]))
        return real(self, *a, **k)
    monkeypatch.setattr(T.FusedAdamW, "step", rec)
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda *a, **k: pytest.fail("clip_grad_norm_ called on the fused path"))
    before = [p.detach().clone() for p in everything]
    lat = torch.randn(1, 4, 2, 4, 4)
    T.stage3_training_step(_Toy(everything), omcm, _Sched(), opt, None, lat, torch.randn_like(lat), torch.tensor([1]), None, None,
                           lambda: None, None, max_grad_norm=0.5, lora_params=lora, mm_params=mm)
    want = [{id(p) for p in g} for g in T.stage3_clip_groups(omcm, lora, mm)]
    assert seen == [(want, 0.5, False)]
    assert len(want) == (2 if with_lora else 1)
    assert all(not torch.equal(p.detach(), b) for p, b in zip(everything, before)) and all(p.grad is None for p in everything)
    n_groups = len(want)
    assert opt.grad_norms.shape == (n_groups,)
    clipped = set().union(*want)
    table = {id(e["param"]): e["clip_group"] for e in opt._plan.entries}
    assert all((table[id(p)] >= 0) == (id(p) in clipped) for p in everything)


@pytest.mark.parametrize("direction", ["fused_to_torch", "torch_to_fused"])
def test_state_dict_both_ways(fake, direction):
    """Test 3: 3 steps under one optimizer, the state dict loaded into the other, 2 more steps under each: equal within condition 1."""
    pa, pb = OC.make_tensors(SHAPES, "cpu", 2), OC.make_tensors(SHAPES, "cpu", 2)
    ref64, ref32 = _refs(pa)
    fused_first = direction == "fused_to_torch"
    first = T.FusedAdamW(pa, **HYPER) if fused_first else torch.optim.AdamW(pa, **HYPER)
    everything = list(range(len(pa)))

    def one(opt, params, k, fused):
        grads = OC.make_grads(SHAPES, 300 + k, 1e-2)
        _set_grads(params, grads)
        if fused:
            opt.step(clip_groups=[params], max_grad_norm=1.0)
        else:
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
        return grads
    for k in range(3):
        grads = one(first, pa, k, fused_first)
        ref64.step(grads, [everything], 1.0)
        ref32.step(grads, [everything], 1.0)
    sd = first.state_dict()
    assert set(sd) == {"state", "param_groups"}
    want_keys = set(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0])
    assert set(sd["param_groups"][0]) == want_keys
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 3.0 and st["step"].device.type == "cpu"
               for st in sd["state"].values())
    with torch.no_grad():
        for a, b in zip(pa, pb):
            b.copy_(a)
    second = torch.optim.AdamW(pb, lr=7.0) if fused_first else T.FusedAdamW(pb, lr=7.0)
    second.load_state_dict(copy.deepcopy(sd))                 # (as through torch.save / torch.load: load_state_dict keeps same-dtype tensors by reference)
    assert second.param_groups[0]["lr"] == HYPER["lr"]
    for k in range(3, 5):
        grads = one(first, pa, k, fused_first)
        one(second, pb, k, not fused_first)
        ref64.step(grads, [everything], 1.0)
        ref32.step(grads, [everything], 1.0)
    fused_params, fused_opt = (pa, first) if fused_first else (pb, second)
    t32 = OC.torch32_measures(ref32, ref64, HYPER["lr"])
    OC.assert_condition_1(f"{direction}: fused arm", OC.fused_measures(fused_params, fused_opt, ref64, HYPER["lr"]), t32)
    other_params, other_opt = (pb, second) if fused_first else (pa, first)
    other = OC.measures(other_params, [other_opt.state[p]["exp_avg"] for p in other_params],
                        [other_opt.state[p]["exp_avg_sq"] for p in other_params], ref64, HYPER["lr"])
    OC.assert_condition_1(f"{direction}: torch arm", other, t32)
    assert all(float(fused_opt.state[p]["step"]) == 5.0 for p in fused_params)
    assert all(float(other_opt.state[p]["step"]) == 5.0 for p in other_params)


def test_parameter_without_gradient_is_skipped(fake):
    """Test 4: a parameter with `grad is None` on steps 2 and 3 of 5: untouched on those steps (no decay), its counter two behind, and
    over the five steps it equals torch's treatment."""
    params = OC.make_tensors(SHAPES, "cpu", 3)
    ref64, ref32 = _refs(params)
    opt = T.FusedAdamW(params, **HYPER)
    everything = list(range(len(params)))
    for k in range(5):
        grads = OC.make_grads(SHAPES, 400 + k, 1e-2)
        if k in (1, 2):
            grads[2] = None
        _set_grads(params, grads)
        before = params[2].detach().clone()
        state_before = {n: v.clone() for n, v in opt.state[params[2]].items()} if k else None
        opt.step(clip_groups=[params], max_grad_norm=1.0)
        ref64.step(grads, [everything], 1.0)
        ref32.step(grads, [everything], 1.0)
        if k in (1, 2):
            assert torch.equal(params[2].detach(), before)
            assert all(torch.equal(opt.state[params[2]][n], v) for n, v in state_before.items())
            assert all(q is not params[2] for q in opt.last_stepped)
    assert float(opt.state[params[2]]["step"]) == 3.0 and float(opt.state[params[0]]["step"]) == 5.0
    assert float(ref64.state(2, "step")) == 3.0
    OC.assert_condition_1("grad None on two of five steps", OC.fused_measures(params, opt, ref64, HYPER["lr"]),
                          OC.torch32_measures(ref32, ref64, HYPER["lr"]))
    assert opt.rebuilds == 3                                     # the set with a gradient changed twice after the first build


def test_scheduler_drives_the_rate_and_unsupported_arguments_raise(fake):
    """Test 5: under a LambdaLR the rate the kernel sees at step k is the scheduler's; amsgrad / maximize / differentiable and a bf16
    parameter raise as stated."""
    params = OC.make_tensors([(33,), (5, 5)], "cpu", 4)
    opt = T.FusedAdamW(params, lr=1e-2, eps=1e-4)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 1.0 / (1 + k))
    ref = OC.TorchRef(params, torch.float64, [([0, 1], dict(lr=1e-2, eps=1e-4))])
    rsched = torch.optim.lr_scheduler.LambdaLR(ref.opt, lambda k: 1.0 / (1 + k))
    for k in range(4):
        grads = OC.make_grads([(33,), (5, 5)], 500 + k, 1.0)
        _set_grads(params, grads)
        opt.step()
        ref.step(grads)
        assert float(opt._plan.hyper[0, 0]) == pytest.approx(1e-2 / (1 + k), rel=1e-6) and opt.param_groups[0]["lr"] == sched.get_last_lr()[0]
        sched.step()
        rsched.step()
    assert max(float((p.detach().double() - q.detach()).abs().max()) for p, q in zip(params, ref.p)) < 1e-2 * 1e-3
    for bad in ("amsgrad", "maximize", "differentiable"):
        with pytest.raises(NotImplementedError, match=bad):
            T.FusedAdamW(params, **{bad: True})
    with pytest.raises(TypeError, match="fp32"):
        T.FusedAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))])


def _bucket_views_ok(reducer):
    for b in reducer.buckets:
        off = 0
        for p in b["params"]:
            if p.grad is None or p.grad.data_ptr() != b["flat"].data_ptr() + 4 * off:
                return False
            off += p.numel()
    return True


def test_reducer_is_rearmed_without_the_fills(fake, monkeypatch):
    """Test 6: GradAllReducer at world size 1.  After `optimizer_update` the buckets are zero (by the kernel where the optimizer owns the
    whole bucket, by the fill where it does not), the .grad views are the bucket views, pending / launched are re-armed and further
    steps work; only re-bucketing rebuilds the table."""
    shapes = [(3,), (40,), (7,), (13, 5), (9,), (50,), (11,)]      # buckets of <= 80 elements, each of two parameters or more
    params = OC.make_tensors(shapes, "cpu", 5)
    outsider = params[4]                                         # trained by someone else: in a bucket, not in the optimizer
    mine = [p for p in params if p is not outsider]
    late = params[6]                                             # receives no gradient until step 6
    reducer = T.GradAllReducer(params, bucket_bytes=4 * 80, find_unused=True)
    assert len(reducer.buckets) >= 2
    opt = T.FusedAdamW(mine, **HYPER)
    fills = []
    real_zero = torch.Tensor.zero_
    monkeypatch.setattr(torch.Tensor, "zero_", lambda self: (fills.append((self.data_ptr(), self.numel())), real_zero(self))[1])
    for k in range(1, 9):
        used = [p for p in params if p is not late or k >= 6]
        x = torch.full((), float(k))
        sum((p * x).sum() for p in used).backward()
        reducer.finish()
        before = [p.detach().clone() for p in mine]
        fills.clear()
        T.optimizer_update(mine, opt, reducer, 1.0)
        assert all(bool((b["flat"] == 0).all()) for b in reducer.buckets)
        assert _bucket_views_ok(reducer) and all(len(b["params"]) >= 2 for b in reducer.buckets)
        assert all(b["pending"] == len(b["params"]) and not b["launched"] for b in reducer.buckets) and reducer._next == 0
        moved = [not torch.equal(p.detach(), b) for p, b in zip(mine, before)]
        assert moved == [p is not late or k >= 6 for p in mine]
        if k != 6:                                               # (step 6 re-admits `late`: the buckets are rebuilt, the plain path)
            flats = {(b["flat"].data_ptr(), b["flat"].numel()) for b in reducer.buckets}
            mixed = {(b["flat"].data_ptr(), b["flat"].numel()) for b in reducer.buckets if any(p is outsider for p in b["params"])}
            assert set(fills) & flats == mixed and len(mixed) == 1 and len(flats) >= 2, (k, fills, mixed)
        assert opt.rebuilds == {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 2, 7: 3, 8: 3}[k], (k, opt.rebuilds)
    assert late not in reducer.unused and reducer.readmitted == 1


def _header_symbols():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fmc_hip.h")).read()
    return sorted(set(re.findall(r"\b(fmc_optim_\w+)\s*\(", text)))


def test_new_symbols_are_bound_and_resolve():
    """Test 7: every `fmc_optim_*` function of include/fmc_hip.h is in `_lib.SIGNATURES` and resolves in the built library; the Python
    mirror of the table entry has the header's size."""
    from synfmc_amd import _lib
    names = _header_symbols()
    assert {"fmc_optim_workspace_bytes", "fmc_optim_grad_norm", "fmc_optim_adamw_step", "fmc_optim_check_tables",
            "fmc_optim_chunk_elems"} <= set(names)
    lib = _lib.load()
    for n in names:
        assert n in _lib.SIGNATURES, n
        assert getattr(lib, n) is not None
    assert lib.fmc_optim_chunk_elems() == K.OPTIM_CHUNK <= 16384
    assert ctypes.sizeof(K.OptimTensor) == 80
    assert lib.fmc_optim_workspace_bytes(3, 5, 2) == 4 * (4 + 4 + 8 + 8)
    assert lib.fmc_optim_workspace_bytes(0, 0, 0) == -1


def test_check_tables_reports_bad_tables():
    """The ABI's host-side table check: a NULL pointer, a misaligned p / m / v, a chunk map that does not cover its tensors."""
    n = K.OPTIM_CHUNK + 5
    bufs = [torch.zeros(n + 8) for _ in range(4)]
    step = torch.zeros(1)

    def row(p=0, g=0, m=0, v=0, null=None, clip=0):
        ptrs = [bufs[0].data_ptr() + p, bufs[1].data_ptr() + g, bufs[2].data_ptr() + m, bufs[3].data_ptr() + v]
        if null is not None:
            ptrs[null] = 0
        return ptrs + [0, 0, step.data_ptr(), n, (clip & 0xffffffff) | (0 << 32), 0]
    good_map = torch.tensor([[0, 1], [0, 0]], dtype=torch.int32)
    K.optim_check_tables(torch.tensor([row(g=4)], dtype=torch.int64), good_map, 1, 1)          # g only 4-byte aligned: fine
    with pytest.raises(ValueError, match="NULL"):
        K.optim_check_tables(torch.tensor([row(null=2)], dtype=torch.int64), good_map, 1, 1)
    for k in ("p", "m", "v"):
        with pytest.raises(ValueError, match="16-byte"):
            K.optim_check_tables(torch.tensor([row(**{k: 4})], dtype=torch.int64), good_map, 1, 1)
    with pytest.raises(ValueError, match="chunks"):
        K.optim_check_tables(torch.tensor([row()], dtype=torch.int64), good_map[:1], 1, 1)
    with pytest.raises(ValueError, match="twice"):
        K.optim_check_tables(torch.tensor([row()], dtype=torch.int64), torch.tensor([[0, 0], [0, 0]], dtype=torch.int32), 1, 1)
    with pytest.raises(ValueError, match="clip group"):
        K.optim_check_tables(torch.tensor([row(clip=3)], dtype=torch.int64), good_map, 1, 1)


def test_wrappers_have_no_cpu_arm():
    params = OC.make_tensors([(9,)], "cpu", 6)
    params[0].grad = torch.ones(9)
    opt = T.FusedAdamW(params)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()


def test_other_optimizers_take_the_old_path(monkeypatch):
    """Test 8: with torch.optim.AdamW `optimizer_update` still calls clip_grad_norm_, step, zero_grad, in that order, and
    `stage3_training_step` still clips the extra groups separately."""
    calls = []
    real_clip = torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda ps, mx, *a, **k: (calls.append(("clip", {id(p) for p in ps}, mx)), real_clip(list(ps), mx))[1])
    params = OC.make_tensors([(5,), (3, 3)], "cpu", 7)
    opt = torch.optim.AdamW(params, lr=1e-3)
    real_step, real_zero = opt.step, opt.zero_grad
    opt.step = lambda *a, **k: (calls.append(("step", a, k)), real_step(*a, **k))[1]
    opt.zero_grad = lambda *a, **k: (calls.append(("zero_grad", a, k)), real_zero(*a, **k))[1]
    for p in params:
        p.grad = torch.ones_like(p)
    T.optimizer_update(params, opt, None, 0.25)
    assert calls == [("clip", {id(p) for p in params}, 0.25), ("step", (), {}), ("zero_grad", (), {"set_to_none": True})]

    class _Reducer:
        def zero_grad(self):
            calls.append(("reducer.zero_grad",))
    calls.clear()
    for p in params:
        p.grad = torch.ones_like(p)
    T.optimizer_update(params, opt, _Reducer(), 1.0)
    assert [c[0] for c in calls] == ["clip", "step", "reducer.zero_grad"]
    calls.clear()
    omcm = torch.nn.Linear(4, 4)
    lora = [torch.nn.Parameter(torch.randn(4, 2))]
    everything = list(omcm.parameters()) + lora
    sgd = torch.optim.SGD(everything, lr=0.0)
    lat = torch.randn(1, 4, 2, 4, 4)
    T.stage3_training_step(_Toy(everything), omcm, _Sched(), sgd, None, lat, torch.randn_like(lat), torch.tensor([1]), None, None,
                           lambda: None, None, lora_params=lora)
    assert [c[1] for c in calls] == [{id(p) for p in lora}, {id(p) for p in omcm.parameters()}]

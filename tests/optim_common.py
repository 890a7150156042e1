"""Shared pieces of the fused-optimizer tests: a plain-PyTorch restatement of the contract of `fmc_optim_grad_norm` / `fmc_optim_adamw_step`
(the host tests run `training.FusedAdamW` on it), the float64 / float32 torch references and the error measures.

The reference of every numerical check is `torch.optim.AdamW` + `torch.nn.utils.clip_grad_norm_` in float64 on the CPU; the yardstick is
what the same two do in float32 against that run.  Measures: parameters `max |p - p64| / lr` (an update is about lr per step: the error in
units of one update); m and v: max abs error over max abs value, over all tensors; the norm: relative error."""
import torch

from synfmc_amd import hip_ops as K


# ---- the restatement (host tests only) -----------------------------------------------------------------------------
def restated_grad_norm(plan):
    hyper = plan.hyper
    for c in range(plan.n_clip_groups):
        members = [e for e in plan.entries if e["clip_group"] == c]
        total = sum(((e["g"].double() ** 2).sum() for e in members), torch.zeros((), dtype=torch.float64))
        norm = total.sqrt().float()
        if members:
            max_norm = hyper[members[0]["hyper_group"], 5]
            coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        else:
            coef = torch.ones(())
        plan.norms[c] = norm
        plan.coefs[c] = coef
    for i, e in enumerate(plan.entries):
        e["step"] += 1
        t = float(e["step"])
        b1 = 1.0 - float(hyper[e["hyper_group"], 6].double())
        b2 = 1.0 - float(hyper[e["hyper_group"], 7].double())
        plan.bias_corrections[i, 0] = 1.0 - b1 ** t
        plan.bias_corrections[i, 1] = (1.0 - b2 ** t) ** 0.5
    return plan.norms


def restated_adamw_step(plan):
    for i, e in enumerate(plan.entries):
        lr, _, b2, eps, wd, _, omb1, omb2 = plan.hyper[e["hyper_group"]].unbind()
        p, m, v = e["p"], e["m"], e["v"]
        g = e["g"] * (plan.coefs[e["clip_group"]] if e["clip_group"] >= 0 else 1.0)
        p.mul_(1.0 - lr * wd)
        m.add_((g - m) * omb1)
        v.mul_(b2).add_(omb2 * g * g)
        denom = v.sqrt() / plan.bias_corrections[i, 1] + eps
        p.sub_((lr / plan.bias_corrections[i, 0]) * (m / denom))
        if e["shadow_bf16"] is not None:
            e["shadow_bf16"].copy_(p.to(torch.bfloat16))
        if e["shadow_f32"] is not None:
            e["shadow_f32"].copy_(p.to(torch.bfloat16).float())
        if e["zero"]:
            e["g"].zero_()


def install(monkeypatch):
    monkeypatch.setattr(K, "optim_grad_norm", restated_grad_norm)
    monkeypatch.setattr(K, "optim_adamw_step", restated_adamw_step)


# ---- torch references --------------------------------------------------------------------------------------------
class TorchRef:
    """`torch.optim.AdamW` + `clip_grad_norm_` on CPU copies of `params` in `dtype`.  `groups`: list of (indices, hyper dict)."""

    def __init__(self, params, dtype, groups):
        self.dtype = dtype
        self.p = [torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in params]
        self.opt = torch.optim.AdamW([dict(params=[self.p[i] for i in idx], **h) for idx, h in groups])

    def step(self, grads, clip_sets=(), max_norm=1.0):
        """`grads[i]` or None; `clip_sets`: lists of indices, each clipped on its own.  Returns the groups' norms (before clipping)."""
        for q, g in zip(self.p, grads):
            q.grad = None if g is None else g.detach().cpu().to(self.dtype).clone()
        norms = []
        for idx in clip_sets:
            norms.append(torch.nn.utils.clip_grad_norm_([self.p[i] for i in idx if self.p[i].grad is not None], max_norm))
        self.opt.step()
        return norms

    def state(self, i, name):
        return self.opt.state[self.p[i]][name]


def measures(ps, ms, vs, ref64: TorchRef, lr: float):
    """(parameter error in updates, m error, v error) of tensors `ps`, `ms`, `vs` (None: no state yet) against the float64 reference."""
    perr, em, am, ev, av = 0.0, 0.0, 0.0, 0.0, 0.0
    for i, p in enumerate(ps):
        perr = max(perr, float((p.detach().double().cpu() - ref64.p[i].detach()).abs().max()) / lr)
        if ms[i] is None:
            continue
        m64, v64 = ref64.state(i, "exp_avg"), ref64.state(i, "exp_avg_sq")
        em = max(em, float((ms[i].double().cpu() - m64).abs().max()))
        ev = max(ev, float((vs[i].double().cpu() - v64).abs().max()))
        am, av = max(am, float(m64.abs().max())), max(av, float(v64.abs().max()))
    return perr, em / max(am, 1e-300), ev / max(av, 1e-300)


def torch32_measures(ref32: TorchRef, ref64: TorchRef, lr: float):
    n = len(ref32.p)
    has = [ref32.p[i] in ref32.opt.state and "exp_avg" in ref32.opt.state[ref32.p[i]] for i in range(n)]
    return measures(ref32.p, [ref32.state(i, "exp_avg") if has[i] else None for i in range(n)],
                    [ref32.state(i, "exp_avg_sq") if has[i] else None for i in range(n)], ref64, lr)


def fused_measures(params, opt, ref64: TorchRef, lr: float):
    ms = [opt.state[p]["exp_avg"] if "exp_avg" in opt.state.get(p, {}) else None for p in params]
    vs = [opt.state[p]["exp_avg_sq"] if "exp_avg_sq" in opt.state.get(p, {}) else None for p in params]
    return measures(params, ms, vs, ref64, lr)


def assert_condition_1(label, fused, torch32):
    """error <= 2 x torch-fp32's own error on the same case, for parameters, m and v; the pairs are printed first."""
    print(f"{label}: p/lr fused {fused[0]:.3e} torch-fp32 {torch32[0]:.3e} | m fused {fused[1]:.3e} torch-fp32 {torch32[1]:.3e} | "
          f"v fused {fused[2]:.3e} torch-fp32 {torch32[2]:.3e}")
    for name, a, b in zip(("parameters", "exp_avg", "exp_avg_sq"), fused, torch32):
        assert a <= 2.0 * b, f"{label}: {name} error {a:.3e} > 2 x torch-fp32's {b:.3e}"


def make_tensors(shapes, device, seed, w_std=0.05):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=g) * w_std).to(device)) for s in shapes]


def make_grads(shapes, seed, sigma):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * sigma for s in shapes]

"""Shared pieces of the Camera-Encoder / merge / OMC-Adapter training tests (pure torch at import; `path_proof` runs on the GPU).

* float64 closed forms of what the new route computes -- the Camera-Adapter merge `m = s ((h + pose) W^T + b) + h` and its backward,
  the 2x2 average pool (odd sizes floor) and its backward, the ReLU backward, the split of the fused q | k | v weight gradient;
* `check_*`: the assertion written for each of them against float64 autograd.  The closed forms pass them; the wrong stand-ins at the
  bottom (one defect each) must each be caught by the assertion written for it (tests/test_camera_training_host.py);
* a CPU toy of the stage-2 stack for the plumbing tests;
* the path proof: torch's linear / conv2d / avg_pool2d / relu / matmul patched to raise inside the trained layers and the backward.
"""
import torch
import torch.nn.functional as F

S = 0.37                                   # a merge scale that is not 1


# ---- closed forms -------------------------------------------------------------------------------------------------------
def merge_forward(h, pose, w, b, s):
    return s * ((h + pose) @ w.t() + b) + h


def merge_backward(dm, h, pose, w, s):
    """(dW, db, dh, dpose) of `merge_forward`: dW = s dm^T hp, db = s colsum(dm), d(hp) = s dm W feeds h and pose, h also gets dm."""
    hp = (h + pose).reshape(-1, h.shape[-1])
    dm2 = dm.reshape(-1, dm.shape[-1])
    dhp = s * (dm @ w)
    return s * dm2.t() @ hp, s * dm2.sum(0), dhp + dm, dhp


def avgpool_forward(x):
    """x `[N, H, W, C]` -> `[N, H // 2, W // 2, C]`; the last row / column of an odd size is not read."""
    ho, wo = x.shape[1] // 2, x.shape[2] // 2
    x = x[:, : 2 * ho, : 2 * wo]
    return 0.25 * (((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + x[:, 1::2, 0::2]) + x[:, 1::2, 1::2])


def avgpool_backward(dy, H, W, out=None):
    """dy `[N, H // 2, W // 2, C]` -> dx `[N, H, W, C]`, ALL of it: zeros in the uncovered last row / column."""
    n, ho, wo, c = dy.shape
    dx = dy.new_empty(n, H, W, c) if out is None else out
    dx.zero_()
    dx[:, : 2 * ho, : 2 * wo] = 0.25 * dy.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return dx


def relu_backward(dy, y):
    return torch.where(y > 0, dy, torch.zeros_like(dy))


def split_qkv_grad(dw_fused):
    """The fused `[3C, C]` weight gradient back into (to_q, to_k, to_v): row blocks in that order."""
    c = dw_fused.shape[0] // 3
    return dw_fused[:c], dw_fused[c: 2 * c], dw_fused[2 * c:]


# ---- the assertions -----------------------------------------------------------------------------------------------------
def _close(a, b, what):
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} != {tuple(b.shape)}"
    assert torch.allclose(a, b, rtol=1e-12, atol=1e-12), f"{what}: max abs difference {float((a - b).abs().max()):.3e}"


def check_merge(forward, backward, seed=0):
    g = torch.Generator().manual_seed(seed)
    h, pose = (torch.randn(2, 5, 8, dtype=torch.float64, generator=g).requires_grad_(True) for _ in range(2))
    w = torch.randn(8, 8, dtype=torch.float64, generator=g).requires_grad_(True)
    b = torch.randn(8, dtype=torch.float64, generator=g).requires_grad_(True)
    dm = torch.randn(2, 5, 8, dtype=torch.float64, generator=g)
    ref = S * F.linear(h + pose, w, b) + h
    ref.backward(dm)
    with torch.no_grad():
        _close(forward(h, pose, w, b, S), ref, "merge forward")
        dw, db, dh, dpose = backward(dm, h, pose, w, S)
        _close(dw, w.grad, "merge dW")
        _close(db, b.grad, "merge db")
        _close(dh, h.grad, "merge dh")
        _close(dpose, pose.grad, "merge dpose")


AVGPOOL_SHAPES = [(2, 6, 10, 8), (1, 5, 7, 8), (1, 3, 9, 16), (2, 4, 3, 8)]      # (torch refuses an empty output: H, W >= 2)


def check_avgpool_forward(forward, seed=1):
    g = torch.Generator().manual_seed(seed)
    for shape in AVGPOOL_SHAPES:
        x = torch.randn(shape, dtype=torch.float64, generator=g)
        ref = F.avg_pool2d(x.permute(0, 3, 1, 2), kernel_size=2, stride=2).permute(0, 2, 3, 1)
        _close(forward(x), ref, f"avgpool forward {shape}")


def check_avgpool_backward(backward, seed=2):
    """Against autograd of `AvgPool2d(2, 2)`; the output buffer starts as NaN: every element must be written, the floor row / column with zeros."""
    g = torch.Generator().manual_seed(seed)
    for n, H, W, c in AVGPOOL_SHAPES:
        x = torch.randn(n, H, W, c, dtype=torch.float64, generator=g).requires_grad_(True)
        y = F.avg_pool2d(x.permute(0, 3, 1, 2), kernel_size=2, stride=2).permute(0, 2, 3, 1)
        dy = torch.randn(y.shape, dtype=torch.float64, generator=g)
        y.backward(dy)
        buf = torch.full((n, H, W, c), float("nan"), dtype=torch.float64)
        dx = backward(dy, H, W, out=buf)
        assert not bool(torch.isnan(dx).any()), f"avgpool backward {(n, H, W, c)}: {int(torch.isnan(dx).sum())} elements of dX were never written"
        _close(dx, x.grad, f"avgpool backward {(n, H, W, c)}")


def check_relu_backward(backward, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(257, dtype=torch.float64, generator=g)
    x[::5] = 0.0                                                 # exact zeros: the gradient there is 0
    x[1::10] = -0.0
    x = x.requires_grad_(True)
    y = torch.relu(x)
    dy = torch.randn(257, dtype=torch.float64, generator=g) + 3.0
    y.backward(dy)
    _close(backward(dy, y.detach()), x.grad, "relu backward")


def check_qkv_split(split, seed=4):
    g = torch.Generator().manual_seed(seed)
    wq, wk, wv = (torch.randn(4, 4, dtype=torch.float64, generator=g).requires_grad_(True) for _ in range(3))
    x = torch.randn(7, 4, dtype=torch.float64, generator=g)
    dy = torch.randn(7, 12, dtype=torch.float64, generator=g)
    fused = torch.cat([wq, wk, wv], dim=0).detach().requires_grad_(True)
    F.linear(x, fused).backward(dy)
    F.linear(x, torch.cat([wq, wk, wv], dim=0)).backward(dy)
    for got, want, name in zip(split(fused.grad), (wq.grad, wk.grad, wv.grad), ("to_q", "to_k", "to_v")):
        _close(got, want, f"q | k | v split {name}")


# ---- wrong stand-ins: one defect each -------------------------------------------------------------------------------------
def wrong_avgpool_forward_odd_row(x):
    """Pools the odd last row / column too (ceil mode)."""
    return F.avg_pool2d(x.permute(0, 3, 1, 2), kernel_size=2, stride=2, ceil_mode=True).permute(0, 2, 3, 1)


def wrong_avgpool_backward_floor_unwritten(dy, H, W, out=None):
    """Writes only what lies under a window."""
    n, ho, wo, c = dy.shape
    dx = dy.new_empty(n, H, W, c) if out is None else out
    dx[:, : 2 * ho, : 2 * wo] = 0.25 * dy.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return dx


def wrong_relu_backward_ge(dy, y):
    return torch.where(y >= 0, dy, torch.zeros_like(dy))


def wrong_split_swapped(dw_fused):
    q, k, v = split_qkv_grad(dw_fused)
    return k, q, v


def wrong_merge_db_without_alpha(dm, h, pose, w, s):
    dw, db, dh, dpose = merge_backward(dm, h, pose, w, s)
    return dw, db / s, dh, dpose


def wrong_merge_residual_dropped(dm, h, pose, w, s):
    dw, db, dh, dpose = merge_backward(dm, h, pose, w, s)
    return dw, db, dh - dm, dpose


def wrong_merge_pose_gets_dm(dm, h, pose, w, s):
    dw, db, dh, dpose = merge_backward(dm, h, pose, w, s)
    return dw, db, dh, dpose + dm


# ---- a CPU toy of the stage-2 stack ---------------------------------------------------------------------------------------
TOY_WIDTHS = (32, 32, 64, 64)


def toy_stage2(dtype=torch.bfloat16):
    """(CMC U-Net, camera encoder) at toy widths on the CPU, frozen, stored in `dtype`."""
    from synfmc_amd.configs import encoder_kwargs, processor_kwargs, unet_kwargs
    from synfmc_amd.models.pose_adaptor import CameraPoseEncoder
    from synfmc_amd.models.unet import UNet3DConditionModelPoseCond
    torch.manual_seed(0)
    pu = UNet3DConditionModelPoseCond(**unet_kwargs(TOY_WIDTHS, 32))
    pu.set_all_attn_processor(**processor_kwargs(TOY_WIDTHS))
    pe = CameraPoseEncoder(**encoder_kwargs(TOY_WIDTHS))
    return pu.to(dtype).eval().requires_grad_(False), pe.to(dtype).eval().requires_grad_(False)


def toy_adapter(dtype=torch.bfloat16):
    from synfmc_amd.adapter import Adapter
    from synfmc_amd.configs import adapter_kwargs
    torch.manual_seed(1)
    return Adapter(**adapter_kwargs(TOY_WIDTHS)).to(dtype).eval().requires_grad_(False)


# ---- the path proof: torch's own linear / conv / pool / relu / matmul raise inside the trained layers and the backward -------------------
class TorchOpReached(RuntimeError):
    pass


class torch_ops_raise:
    """Context manager: `torch.nn.functional.linear`, `conv2d`, `avg_pool2d`, `relu` and `torch.matmul` raise `TorchOpReached` while
    `state["armed"]`.  (The frozen U-Net's time embedding and edge layers are plain torch modules: the proof arms the patch inside the
    forward of the TRAINED modules and for the whole backward.)"""

    def __enter__(self):
        self.state = {"armed": False}
        self.saved = [(F, n, getattr(F, n)) for n in ("linear", "conv2d", "avg_pool2d", "relu")] + [(torch, "matmul", torch.matmul)]
        for mod, name, orig in self.saved:
            def wrapped(*a, _orig=orig, _name=name, **k):
                if self.state["armed"]:
                    raise TorchOpReached(_name)
                return _orig(*a, **k)
            setattr(mod, name, wrapped)
        return self.state

    def __exit__(self, *exc):
        for mod, name, orig in self.saved:
            setattr(mod, name, orig)
        return False


def arm_inside(state, modules, merge_owners=()):
    """Arm the patch inside the forward of `modules` and inside `_merge` of `merge_owners`; returns an undo function."""
    handles = []
    for m in modules:
        handles.append(m.register_forward_pre_hook(lambda *_: state.__setitem__("armed", True)))
        handles.append(m.register_forward_hook(lambda *_: state.__setitem__("armed", False)))
    for proc in merge_owners:
        inner = proc._merge

        def merged(*a, _inner=inner, **k):
            state["armed"] = True
            try:
                return _inner(*a, **k)
            finally:
                state["armed"] = False
        proc.__dict__["_merge"] = merged

    def undo():
        for h in handles:
            h.remove()
        for proc in merge_owners:
            proc.__dict__.pop("_merge", None)
    return undo


def path_proof(stage, pu, pe, pa, clip, pose_emb, t, noise):
    """One stage-2 / stage-3 forward + backward of marked modules (bf16, no autocast, the vendor arms off) with the patch armed inside the
    trained modules' forward and for the whole backward.  Returns (families of `hip_ops.call_log`, the change of `dispatch_calls`)."""
    import copy
    from synfmc_amd import hip_ops as K
    from synfmc_amd.models.layers import OWN_MARK
    from tests import training_common as TC
    owners = [m for m in pu.modules() if hasattr(m, "qkv_merge") and m.__dict__.get(OWN_MARK)]
    saved = (K.NO_VENDOR, K.call_log)
    K.NO_VENDOR, K.call_log = True, []
    before = copy.deepcopy(K.dispatch_calls)
    try:
        with torch_ops_raise() as state:
            undo = arm_inside(state, [pe] if stage == 2 else [pa], owners if stage == 2 else ())
            try:
                real = torch.Tensor.backward

                def armed_backward(self, *a, **k):
                    state["armed"] = True
                    try:
                        return real(self, *a, **k)
                    finally:
                        state["armed"] = False
                torch.Tensor.backward = armed_backward
                if stage == 2:
                    TC.product_grads_stage2(pu, pe, clip, pose_emb, t, noise, "cuda", torch.bfloat16)
                else:
                    TC.product_grads(pu, pe, pa, clip, pose_emb, t, noise, "cuda", torch.bfloat16)
            finally:
                torch.Tensor.backward = real
                undo()
        torch.cuda.synchronize()
        delta = {k: {a: K.dispatch_calls[k][a] - before[k][a] for a in v} for k, v in before.items()}
        return [e[0] for e in K.call_log], delta
    finally:
        K.NO_VENDOR, K.call_log = saved

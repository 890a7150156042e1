"""Training-step pieces of the FMC hot path.

Mirrors what `train_cam_obj_ctrl.py:782-943` (stage 3, OMC) and `train_cam_ctrl.py:540-665` (stage 2, CMC) do around
`pose_adaptor(...)`: biased timestep sampling, `add_noise`, the `sd_w * MSE + mask_w * masked-MSE` loss, gradient
clipping and the optimizer step -- plus the one exchange step of the path, the gradient all-reduce, done here by
`GradAllReducer` over RCCL (`torch.distributed`, backend "nccl" on ROCm) instead of `DistributedDataParallel`:

* gradients live in a few large flat buckets (views are installed as `p.grad`, nothing is copied);
* a bucket is all-reduced asynchronously the moment its last gradient has been accumulated, so the transfers overlap
  the rest of the backward (the U-Net activation backward is ~95 % of it and produces no parameter gradients);
* buckets are sized for xGMI (default 128 MiB: 7 point-to-point links per GPU, large messages amortise the ring
  latency; the whole OMC stage is 610 MB = 5 buckets) rather than DDP's 25 MiB NVSwitch default;
* parameters that never receive a gradient (the Adapter's level-3 blocks, 60.6 M of 152.5 M params: hence the
  reference's `find_unused_parameters=True`, train_cam_obj_ctrl.py:556) are found in a discovery step and dropped from
  the buckets (`grad = None`, as under DDP): they are neither shipped nor weight-decayed;
* optional bf16 compression of the buckets on the wire.
"""
from __future__ import annotations

from typing import Iterable, List, Optional

import torch
import torch.distributed as dist
import torch.nn.functional as F


def biased_timesteps(bsz: int, num_train_timesteps: int, omcm_min_step: int, min_step_prob: float, device,
                     generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """train_cam_obj_ctrl.py:793-800: with probability `min_step_prob` draw t from [omcm_min_step, T), else [0, omcm_min_step)."""
    if omcm_min_step > 0:
        t_rand = torch.rand(bsz, device=device, generator=generator)
        hi = torch.randint(omcm_min_step, num_train_timesteps, (bsz,), device=device, generator=generator)
        lo = torch.randint(0, omcm_min_step, (bsz,), device=device, generator=generator)
        return torch.where(t_rand < min_step_prob, hi, lo).long()
    return torch.randint(0, num_train_timesteps, (bsz,), device=device, generator=generator).long()


def masked_mse_loss(model_pred: torch.Tensor, target: torch.Tensor, obj_masks: Optional[torch.Tensor],
                    sd_loss_weight: float = 0.3, mask_loss_weight: float = 1.0, invert: bool = False) -> torch.Tensor:
    """`sd_w * MSE(pred, target) + mask_w * MSE(mask*pred, mask*target)` (train_cam_obj_ctrl.py:878-908).
    obj_masks: `[B, F, H, W]` union of the object masks at pixel resolution (bool / 0-1), brought to latent size with
    nearest interpolation (:897-899).  `invert=True` is stage 2's `1 - mask` (train_cam_ctrl.py:624)."""
    sd = F.mse_loss(model_pred.float(), target.float(), reduction="mean")
    if obj_masks is None:
        return sd
    b, f = obj_masks.shape[:2]
    m = obj_masks.to(model_pred.dtype).reshape(b * f, 1, *obj_masks.shape[2:])
    m = F.interpolate(m, size=model_pred.shape[-2:])
    m = m.reshape(b, f, 1, *m.shape[2:]).permute(0, 2, 1, 3, 4)
    if invert:
        m = 1 - m
    ml = F.mse_loss((m * model_pred).float(), (m * target).float(), reduction="mean")
    return mask_loss_weight * ml + sd_loss_weight * sd


class GradAllReducer:
    """Bucketed, overlapped gradient all-reduce (mean over ranks) for the trainable subset of a model.

    * `find_unused=True` (the reference's `DDP(find_unused_parameters=True)`, train_cam_obj_ctrl.py:556): the FIRST step is
      a discovery step -- a parameter counts as used when its gradient hook fired on ANY rank (one all-reduce of a
      bitmap); unused parameters (the Adapter's level-3 blocks: 60.6 M of 152.5 M) are dropped from the buckets and get
      `grad = None`, so they are neither shipped (242 MB of zeros per step) nor touched by AdamW's weight decay --
      exactly what happens to them under DDP.
    * `compress_dtype=torch.bfloat16`: the buckets travel as bf16 (half the xGMI bytes); accumulation, clipping and the
      optimizer stay fp32.
    * `overlap=False`: nothing is launched from inside `backward()`; `finish()` reduces the buckets afterwards.  This is
      the mode for a HIP-graph-captured forward/backward (graph | all-reduce | graph, see bench.py --mode train).
    * a second `backward()` before `zero_grad()` raises instead of silently using un-reduced gradients.
    * a pruned parameter that IS reached on a later step (DDP re-detects unused parameters every iteration) is noticed by
      `finish()` -- its `.grad` is no longer None on some rank; one 1-element MAX all-reduce per step is the price -- its
      gradient is averaged over the ranks in a one-off collective for that step, and `zero_grad()` re-admits it to the buckets
      for good.  Ranks therefore never step on a rank-local gradient.  Build the optimizer over ALL trainable parameters (as the
      reference does): it skips `grad is None`; a HIP-graph-captured step needs a static set and cannot re-admit -- there the
      check fires at capture time.
    * the discovery step must run EAGERLY: under capture / replay the hooks do not fire and everything would look unused."""

    def __init__(self, params: Iterable[torch.nn.Parameter], bucket_bytes: int = 128 << 20, group=None,
                 overlap: bool = True, compress_dtype: Optional[torch.dtype] = None, find_unused: bool = True):
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.bucket_bytes, self.overlap, self.compress_dtype = bucket_bytes, overlap, compress_dtype
        self._all = [p for p in params if p.requires_grad]
        self._discovering = find_unused
        self._fired = set()
        self._next = 0                              # first bucket not yet handed to the collective (launch order = index)
        self.unused: List[torch.nn.Parameter] = []
        self.buckets: List[dict] = []
        self._hooks = []
        self._readmit: List[torch.nn.Parameter] = []     # pruned parameters that received a gradient after all (see finish)
        self.readmitted = 0                             # how many were ever re-admitted (reported / tested)
        self._build(self._all)

    # ---- bucket construction ---------------------------------------------------------------------------
    def _build(self, params, old_grads=None):
        for h in self._hooks:
            h.remove()
        self._hooks, self.buckets = [], []
        cur, cur_bytes = [], 0
        for p in reversed(params):                  # gradients become ready roughly in reverse registration order
            nbytes = p.numel() * p.element_size()
            if cur and (cur_bytes + nbytes > self.bucket_bytes or cur[0].dtype != p.dtype or cur[0].device != p.device):
                self._add_bucket(cur, old_grads)
                cur, cur_bytes = [], 0
            cur.append(p)
            cur_bytes += nbytes
        if cur:
            self._add_bucket(cur, old_grads)
        for bi, b in enumerate(self.buckets):
            for p in b["params"]:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._make_hook(bi)))

    def _add_bucket(self, params, old_grads=None):
        flat = torch.zeros(sum(p.numel() for p in params), dtype=params[0].dtype, device=params[0].device)
        off = 0
        for p in params:
            view = flat[off: off + p.numel()].view_as(p)
            if old_grads is not None and id(p) in old_grads:
                view.copy_(old_grads[id(p)])
            p.grad = view                                         # autograd accumulates in place into this view
            off += p.numel()
        self.buckets.append({"params": params, "flat": flat, "pending": len(params), "work": None, "launched": False,
                             "comp": None})

    def _make_hook(self, bi):
        def hook(p):
            b = self.buckets[bi]
            if b["launched"]:
                raise RuntimeError("GradAllReducer: a gradient arrived for a bucket that was already reduced -- several "
                                   "backward() passes per step (gradient accumulation) are not supported; call zero_grad()")
            self._fired.add(id(p))
            b["pending"] -= 1
            if self.overlap and not self._discovering:
                # collectives must be issued in the same order on every rank, and a parameter may be reached on some ranks
                # only: buckets go out strictly in index order, a ready bucket waits for its predecessors
                while self._next < len(self.buckets) and self.buckets[self._next]["pending"] == 0:
                    self._launch(self.buckets[self._next])
                    self._next += 1
        return hook

    # ---- the exchange ----------------------------------------------------------------------------------
    def _launch(self, b, async_op: bool = True):
        if b["launched"]:
            return
        b["launched"] = True
        if self.world > 1:
            buf = b["flat"]
            if self.compress_dtype is not None and buf.dtype != self.compress_dtype:
                b["comp"] = buf = b["flat"].to(self.compress_dtype)
            b["work"] = dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=async_op)

    def _prune_unused(self):
        """End of the discovery step: used = hook fired on any rank."""
        if self._all[0].is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GradAllReducer: the discovery step (first finish()) must run eagerly -- gradient hooks do not "
                               "fire under HIP-graph capture, every parameter would be classified unused")
        self._discovering = False
        used = torch.tensor([1.0 if id(p) in self._fired else 0.0 for p in self._all], device=self._all[0].device)
        if self.world > 1:
            dist.all_reduce(used, op=dist.ReduceOp.MAX, group=self.group)
        used = used.bool().tolist()
        if not any(used):
            raise RuntimeError("GradAllReducer: no gradient hook fired on any rank in the discovery step (was backward() run, "
                               "eagerly, before finish()?)")
        self.unused = [p for p, u in zip(self._all, used) if not u]
        if not self.unused:
            return
        keep = [p for p, u in zip(self._all, used) if u]
        old = {id(p): p.grad.detach().clone() for p in keep}
        for p in self.unused:
            p.grad = None
        self._build(keep, old)
        for b in self.buckets:                                    # this step's gradients are complete: nothing pending
            b["pending"] = 0

    def finish(self) -> None:
        """Call after `loss.backward()`: flush buckets whose parameters never got a gradient, wait, average."""
        if self._discovering:
            self._prune_unused()
        for b in self.buckets:
            self._launch(b)
        for b in self.buckets:
            if b["work"] is not None:
                if hasattr(b["work"], "wait"):
                    b["work"].wait()
                b["work"] = None
            if self.world > 1:
                if b["comp"] is not None:
                    b["flat"].copy_(b["comp"])
                    b["comp"] = None
                b["flat"].mul_(1.0 / self.world)
        if self.unused:
            self._reduce_late_gradients()

    def _reduce_late_gradients(self) -> None:
        """A pruned parameter has a gradient on some rank (autograd gave it a fresh rank-local `.grad`): average it over the ranks now,
        re-admit it to the buckets at the next `zero_grad()`.  Same collectives in the same order on every rank."""
        capturing = self._all[0].is_cuda and torch.cuda.is_current_stream_capturing()
        late_here = any(p.grad is not None for p in self.unused)
        if capturing:
            if late_here:
                raise RuntimeError("GradAllReducer: a parameter pruned as unused received a gradient inside a HIP-graph capture; a "
                                   "captured step needs a static parameter set -- run this step eagerly so that it is re-admitted")
            return                                               # (a captured step cannot negotiate: the check above is the guard)
        dev = self._all[0].device
        if self.world > 1:
            flag = torch.tensor([1.0 if late_here else 0.0], device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=self.group)
            late_any = bool(flag.item() > 0)
        else:
            late_any = late_here
        if not late_any:
            return
        bits = torch.tensor([1.0 if p.grad is not None else 0.0 for p in self.unused], device=dev)
        if self.world > 1:
            dist.all_reduce(bits, op=dist.ReduceOp.MAX, group=self.group)
        bits = bits.bool().tolist()
        readmit = [p for p, u in zip(self.unused, bits) if u]
        for p in readmit:
            g = p.grad if p.grad is not None else torch.zeros_like(p)
            if self.world > 1:
                dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.group)
                g.mul_(1.0 / self.world)
            p.grad = g
        self._readmit = readmit
        self.readmitted += len(readmit)

    def zero_grad(self) -> None:
        if self._readmit:                                        # rebuild the buckets with the re-admitted parameters (original order)
            ids = {id(p) for p in self._readmit} | {id(p) for b in self.buckets for p in b["params"]}
            self.unused = [p for p in self.unused if id(p) not in ids]
            self._readmit = []
            self._build([p for p in self._all if id(p) in ids])
        for p in self.unused:
            p.grad = None
        for b in self.buckets:
            b["flat"].zero_()
            b["pending"] = len(b["params"])
            b["launched"] = False
        self._next = 0
        self._reinstall_views()      # an optimizer's zero_grad(set_to_none=True) may have dropped the views

    def rearm(self, zeroed: Iterable[torch.nn.Parameter]) -> None:
        """`zero_grad()` after an update that has already zeroed the gradients of `zeroed` in place (`FusedAdamW.step(zero=True)`): a
        bucket whose parameters were ALL zeroed through their bucket views skips its fill, every other bucket is filled as usual."""
        if self._readmit:
            return self.zero_grad()                              # the buckets are rebuilt: the plain path
        done = {id(p) for p in zeroed}
        for p in self.unused:
            p.grad = None
        for b in self.buckets:
            off, covered, esz = 0, True, b["flat"].element_size()
            for p in b["params"]:
                covered = covered and id(p) in done and p.grad is not None and p.grad.data_ptr() == b["flat"].data_ptr() + esz * off
                off += p.numel()
            if not covered:
                b["flat"].zero_()
            b["pending"] = len(b["params"])
            b["launched"] = False
        self._next = 0
        self._reinstall_views()

    def _reinstall_views(self):
        for b in self.buckets:
            off = 0
            for p in b["params"]:
                view = b["flat"][off: off + p.numel()].view_as(p)
                if p.grad is None or p.grad.data_ptr() != view.data_ptr():
                    p.grad = view
                off += p.numel()

    def parameters(self):
        return [p for b in self.buckets for p in b["params"]]

    def allreduce_bytes(self) -> int:
        """bytes one step puts on the wire per rank (after pruning / compression)"""
        e = torch.empty((), dtype=self.compress_dtype).element_size() if self.compress_dtype is not None else None
        return sum(b["flat"].numel() * (e or b["flat"].element_size()) for b in self.buckets)


def broadcast_parameters(module: torch.nn.Module, src: int = 0, group=None) -> None:
    """Rank-0 -> all copy of the module state (what the DDP constructor does once).  c10d
    collectives write their output without touching the tensor's version counter, and every derived-weight cache of the
    models (fused QKV, channels-last / flipped filters, fp32 affine copies, interleaved GEGLU rows, batched temb) is keyed
    on it: the received values therefore land through `copy_`, which bumps it."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return
    with torch.no_grad():
        for t in list(module.parameters()) + list(module.buffers()):
            buf = t.detach().clone()
            dist.broadcast(buf, src=src, group=group)
            t.copy_(buf)


def training_target(noise_scheduler, latents, noise, timesteps):
    """What the model's output is compared with (train_cam_obj_ctrl.py:870-875): the noise under epsilon prediction (the tensor
    itself, untouched), `get_velocity` under v-prediction."""
    cfg = getattr(noise_scheduler, "config", None)
    kind = (cfg.get("prediction_type", "epsilon") if isinstance(cfg, dict) else getattr(cfg, "prediction_type", "epsilon"))
    if kind == "epsilon":
        return noise
    if kind == "v_prediction":
        return noise_scheduler.get_velocity(latents, noise, timesteps)
    raise ValueError(f"Unknown prediction type {kind}")


def stage3_forward_backward(pose_adaptor, noise_scheduler, latents, noise, timesteps, encoder_hidden_states,
                            plucker_embedding, traj_features_fn, obj_masks, sd_loss_weight=0.3, mask_loss_weight=1.0):
    """add_noise -> Adapter -> U-Net -> loss -> backward (train_cam_obj_ctrl.py:802-915); returns the detached loss."""
    noisy_latents = noise_scheduler.add_noise(latents, noise, timesteps)
    traj_features = traj_features_fn()
    model_pred = pose_adaptor(noisy_latents, timesteps, encoder_hidden_states=encoder_hidden_states,
                              pose_embedding=plucker_embedding, traj_features=traj_features)
    target = training_target(noise_scheduler, latents, noise, timesteps)
    loss = masked_mse_loss(model_pred, target, obj_masks, sd_loss_weight, mask_loss_weight)
    loss.backward()
    return loss.detach()


def _capturing(t: torch.Tensor) -> bool:
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


class FusedAdamW(torch.optim.Optimizer):
    """`torch.optim.AdamW` (amsgrad=False, maximize=False) on this library's kernels: gradient clipping per group, the update, the bf16
    shadows of the fp32 masters (`layers.bf16_param`) and the zeroing of the gradients in two ABI calls (`fmc_optim_grad_norm`,
    `fmc_optim_adamw_step`) for all tensors.  Constructor arguments, `param_groups` and the `state_dict()` format are AdamW's: schedulers
    drive `param_groups[i]["lr"]` as ever, and a checkpoint written under either optimizer resumes under the other.

    * fp32 parameters only (masters are fp32); a parameter whose `.grad is None` is skipped entirely -- no decay, its step counter does not move.
    * The device tables are rebuilt only when the set of parameters with a gradient, an address (gradient, shadow, state) or the clip grouping
      changes; inside a HIP-graph capture a rebuild raises: a captured step needs a static set.  `rebuilds` counts them.
    * Hyper-parameters travel through a small device record: every eager `step` refreshes it, a captured step replays with what
      `push_hyperparameters()` copied there between the replays.  The graph holds the addresses of the optimizer's tables: keep the
      optimizer alive as long as the graph.
    * The kernels write through raw pointers; `step` bumps the version counter of everything they wrote and re-keys the shadows it refreshed
      (every derived-weight cache of the models is keyed on `(data_ptr, _version)`).  A REPLAYED step runs no Python: call `mark_updated()`
      after the replays, before the next eager forward.
    * `attach(model)` tells the optimizer where the shadows live; a master without a shadow simply gets none."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None):
        if amsgrad:
            raise NotImplementedError("FusedAdamW: amsgrad is not implemented (the reference's trainers do not use it; the kernel keeps no max of v)")
        if maximize:
            raise NotImplementedError("FusedAdamW: maximize is not implemented (negate the loss instead)")
        if differentiable:
            raise NotImplementedError("FusedAdamW: the update runs in a HIP kernel outside autograd, it cannot be differentiable")
        if not 0.0 <= float(lr) or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not 0.0 <= weight_decay:
            raise ValueError(f"FusedAdamW: invalid hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None, decoupled_weight_decay=True)
        self._steps = None                 # one flat fp32 device tensor: state[p]["step"] is a 0-d view of it
        self._slot = {}
        self._owners = {}                  # id(p) -> (module, name): where layers.bf16_param keeps p's shadows
        self._plan, self._plan_key, self._hyper = None, None, None
        self._max_grad_norm, self._pushed = float("inf"), None
        self.rebuilds = 0
        self.grad_norms = None             # per clip group, a device tensor, after step()
        self.last_stepped: List[torch.nn.Parameter] = []
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            if p.dtype != torch.float32:
                raise TypeError(f"FusedAdamW: fp32 parameters only (masters are fp32 by this project's rule), got {p.dtype}")
        self._plan_key = None

    def attach(self, *models: torch.nn.Module) -> "FusedAdamW":
        """Find the modules that own this optimizer's parameters: their `bf16_param` shadows are refreshed by `step` from then on."""
        from .models.layers import bf16_shadow_owners
        mine = [p for g in self.param_groups for p in g["params"]]
        for model in models:
            self._owners.update(bf16_shadow_owners(model, mine))
        self._plan_key = None
        return self

    # ---- state -------------------------------------------------------------------------------------------
    def _step_slot(self, p: torch.Tensor) -> torch.Tensor:
        if id(p) not in self._slot:
            params = [q for g in self.param_groups for q in g["params"]]
            flat = torch.zeros(len(params), dtype=torch.float32, device=p.device)
            self._slot = {id(q): i for i, q in enumerate(params)}
            for q in params:
                st = self.state.get(q)
                if st is not None and "step" in st:
                    flat[self._slot[id(q)]] = float(st["step"])
                    st["step"] = flat[self._slot[id(q)]]
            self._steps = flat
        return self._steps[self._slot[id(p)]]

    def _state_of(self, p):
        st = self.state[p]
        if "exp_avg" not in st:
            st["step"] = self._step_slot(p)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    def state_dict(self):
        """AdamW's format; `step` as the CPU fp32 scalar tensors torch's own AdamW writes."""
        sd = super().state_dict()
        sd["state"] = {k: {n: (v.detach().cpu().clone() if n == "step" and torch.is_tensor(v) else v) for n, v in st.items()}
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._steps, self._slot = None, {}
        for p, st in list(self.state.items()):
            if "exp_avg" not in st:
                continue
            step = st.get("step", 0.0)
            st.pop("step", None)
            slot = self._step_slot(p)
            slot.fill_(float(step))
            st["step"] = slot
            for n in ("exp_avg", "exp_avg_sq"):
                st[n] = st[n].to(device=p.device, dtype=torch.float32).contiguous()
        self._plan_key = None

    # ---- the tables --------------------------------------------------------------------------------------
    def _shadows(self, p):
        own = self._owners.get(id(p))
        if own is None:
            return None
        from .models.layers import bf16_shadow_tensors
        return bf16_shadow_tensors(*own)

    def _prepare(self, clip_groups, zero):
        group_of = {}
        for ci, grp in enumerate(clip_groups or []):
            for p in grp:
                if group_of.setdefault(id(p), ci) != ci:
                    raise ValueError("FusedAdamW: a parameter is in two clip groups")
        entries, key = [], [len(clip_groups or []), bool(zero)]
        for hi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("FusedAdamW does not support sparse gradients")
                sh = self._shadows(p)
                st = self._state_of(p)
                entries.append((p, hi, group_of.get(id(p), -1), sh))
                key += [id(p), p.data_ptr(), p.grad.data_ptr(), hi, group_of.get(id(p), -1),
                        sh[0].data_ptr() if sh else 0, sh[1].data_ptr() if sh else 0,
                        st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr()]
        return entries, key

    def _build(self, entries, n_clip_groups, zero):
        from . import hip_ops as K
        dev = entries[0][0].device
        rows = []
        for p, hi, ci, sh in entries:
            if p.device != dev:
                raise RuntimeError("FusedAdamW: all parameters must live on one device")
            if not p.is_contiguous() or not p.grad.is_contiguous() or p.grad.dtype != torch.float32:
                raise RuntimeError("FusedAdamW: parameters and gradients must be contiguous fp32 tensors")
            st = self._state_of(p)
            rows.append(dict(p=p.detach(), g=p.grad, m=st["exp_avg"], v=st["exp_avg_sq"], step=st["step"],
                             shadow_bf16=sh[0] if sh else None, shadow_f32=sh[1] if sh else None, clip_group=ci, hyper_group=hi, zero=zero,
                             param=p))
        if self._hyper is None or self._hyper.shape[0] != len(self.param_groups) or self._hyper.device != dev:
            self._hyper = torch.zeros(len(self.param_groups), K.OPTIM_HYPER, dtype=torch.float32, device=dev)
            self._pushed = None
        self.rebuilds += 1
        return K.OptimPlan(rows, n_clip_groups, self._hyper)

    def push_hyperparameters(self, max_grad_norm: Optional[float] = None) -> None:
        """Copy `param_groups` (lr, betas, eps, weight_decay) and the clip threshold into the device record the kernels read.  Every eager
        `step` does it; around a captured step call it between the replays (after `scheduler.step()`)."""
        if max_grad_norm is not None:
            self._max_grad_norm = float(max_grad_norm)
        if self._hyper is None:
            return
        rows = [[float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), self._max_grad_norm,
                 1.0 - float(g["betas"][0]), 1.0 - float(g["betas"][1])] for g in self.param_groups]
        if rows != self._pushed:                                 # a constant schedule costs no copy
            self._hyper.copy_(torch.tensor(rows, dtype=torch.float64).to(torch.float32))
            self._pushed = rows

    def mark_updated(self) -> None:
        """Tell torch what the kernels wrote: bump the version counter of every master, state, shadow and zeroed gradient of the current
        table and re-key the refreshed shadows.  `step` calls it; after REPLAYS of a captured step the caller does."""
        if self._plan is None:
            return
        from .models.layers import bf16_shadow_mark_fresh
        wrote = []
        for e in self._plan.entries:
            wrote += [e["param"], e["m"], e["v"], e["step"]]
            wrote += [t for t in (e["shadow_bf16"], e["shadow_f32"]) if t is not None]
            if e["zero"]:
                wrote.append(e["g"])
        torch._C._increment_version(wrote)                        # wants a LIST (a bare tensor would be iterated row by row)
        for e in self._plan.entries:
            if e["shadow_bf16"] is not None:
                bf16_shadow_mark_fresh(*self._owners[id(e["param"])])

    @torch.no_grad()
    def step(self, closure=None, clip_groups=None, max_grad_norm: Optional[float] = None, zero: bool = False):
        """clip per group -> AdamW -> shadows -> (zero) in two ABI calls.  `clip_groups`: a list of parameter lists, each clipped to
        `max_grad_norm` on its own (`clip_grad_norm_` semantics); parameters in no group are not clipped.  `zero`: the gradients are zeroed
        in place.  Afterwards `grad_norms` holds the groups' norms (device tensor) and `last_stepped` the parameters that were updated."""
        if closure is not None:
            raise NotImplementedError("FusedAdamW.step takes no closure")
        if clip_groups and max_grad_norm is None:
            raise ValueError("FusedAdamW.step: clip_groups need a max_grad_norm")
        from . import hip_ops as K
        rebuild_in_capture = ("FusedAdamW: the tensor table would have to be rebuilt inside a HIP-graph capture (the set of parameters with a "
                              "gradient, an address or the clip grouping changed) -- run one eager step with the same arguments first")
        first = next((p for g in self.param_groups for p in g["params"] if p.grad is not None), None)
        capturing = first is not None and _capturing(first)
        if capturing and self._plan_key is None:
            raise RuntimeError(rebuild_in_capture)               # (before any state is allocated on the capturing stream)
        entries, key = self._prepare(clip_groups, zero)
        if not entries:
            self.last_stepped, self.grad_norms = [], None
            return None
        if key != self._plan_key:
            if capturing:
                raise RuntimeError(rebuild_in_capture)
            self._plan = self._build(entries, len(clip_groups or []), zero)
            self._plan_key = key
        if capturing:
            if self._pushed is None or (max_grad_norm is not None and float(max_grad_norm) != self._pushed[0][5]):
                raise RuntimeError("FusedAdamW: max_grad_norm differs from the value in the device record; push_hyperparameters(max_grad_norm) "
                                   "before the capture")
        else:
            self.push_hyperparameters(max_grad_norm)
        K.optim_grad_norm(self._plan)
        K.optim_adamw_step(self._plan)
        self.mark_updated()
        self.grad_norms = self._plan.norms
        self.last_stepped = [e["param"] for e in self._plan.entries]
        return None


def optimizer_update(trainable: Iterable[torch.nn.Parameter], optimizer, reducer: Optional["GradAllReducer"],
                     max_grad_norm: float = 1.0, extra_clip_groups=None) -> None:
    """clip -> step -> zero (train_cam_obj_ctrl.py:917-943), on already averaged gradients.  With a `FusedAdamW` the three are its two
    kernel passes: `trainable` and each of `extra_clip_groups` are clipped on their own, the kernel zeroes the gradients it used and the
    reducer is re-armed without the fills of the buckets that are already zero."""
    params = [p for p in trainable if p.requires_grad and p.grad is not None]
    if isinstance(optimizer, FusedAdamW):
        groups = [params] + [[p for p in g if p.grad is not None] for g in (extra_clip_groups or [])]
        optimizer.step(clip_groups=groups, max_grad_norm=max_grad_norm, zero=reducer is not None)
        if reducer is not None:
            reducer.rearm(optimizer.last_stepped)
        else:
            optimizer.zero_grad(set_to_none=True)
        return
    torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
    optimizer.step()
    if reducer is not None:
        reducer.zero_grad()
    else:
        optimizer.zero_grad(set_to_none=True)


def stage3_clip_groups(omcm, lora_params=None, mm_params=None) -> List[List[torch.nn.Parameter]]:
    """The parameter groups stage 3 clips, each to `max_grad_norm` on its own (train_cam_obj_ctrl.py:921-927): the Adapter; with
    `train_image_lora` every U-Net parameter that requires grad -- the Domain LoRA and, with `train_mm` too, the motion-module
    parameters -- as ONE group.  With `train_mm` alone the motion-module gradients are not clipped at all."""
    groups = [[p for p in omcm.parameters() if p.requires_grad]]
    if lora_params is not None:
        groups.append([p for p in list(lora_params) + list(mm_params or []) if p.requires_grad])
    return groups


def stage3_training_step(pose_adaptor, omcm, noise_scheduler, optimizer, reducer: Optional[GradAllReducer], latents,
                         noise, timesteps, encoder_hidden_states, plucker_embedding, traj_features_fn, obj_masks,
                         sd_loss_weight=0.3, mask_loss_weight=1.0, max_grad_norm=1.0, lora_params=None, mm_params=None):
    """One OMC-stage optimisation step (train_cam_obj_ctrl.py:802-943 minus data loading, VAE and CLIP).

    `traj_features_fn()` must run the (trainable) Adapter, e.g. `lambda: get_traj_features_v2(infos, masks, omcm, ...)`.
    `lora_params` (`train_image_lora`, :397-406): the Domain-LoRA parameters trained along (`lora_trainable_parameters`).
    `mm_params` (`train_mm`, :367-384): the motion-module parameters trained along (`motion_module_trainable_parameters`).  Clipping
    follows `stage3_clip_groups`.  Returns the loss value (a 0-d tensor)."""
    loss = stage3_forward_backward(pose_adaptor, noise_scheduler, latents, noise, timesteps, encoder_hidden_states,
                                   plucker_embedding, traj_features_fn, obj_masks, sd_loss_weight, mask_loss_weight)
    if reducer is not None:
        reducer.finish()
    extra = stage3_clip_groups(omcm, lora_params, mm_params)[1:]
    if isinstance(optimizer, FusedAdamW):
        optimizer_update(omcm.parameters(), optimizer, reducer, max_grad_norm, extra_clip_groups=extra)
        return loss
    for group in extra:
        torch.nn.utils.clip_grad_norm_([p for p in group if p.grad is not None], max_grad_norm)
    optimizer_update(omcm.parameters(), optimizer, reducer, max_grad_norm)
    return loss


def stage2_trainable_parameters(unet, pose_encoder) -> List[torch.nn.Parameter]:
    """The CMC stage trains the camera encoder and the Camera-Adapter merge layers of the temporal attention
    processors (`qkv_merge` / `q_merge` / `kv_merge`), everything else is frozen (train_cam_ctrl.py:262-283)."""
    params = list(pose_encoder.parameters())
    params += [p for n, p in unet.named_parameters() if "_merge." in n]
    return params


def stage2_training_step(pose_adaptor, trainable: Iterable[torch.nn.Parameter], noise_scheduler, optimizer,
                         reducer: Optional[GradAllReducer], latents, noise, timesteps, encoder_hidden_states,
                         plucker_embedding, obj_masks=None, sd_loss_weight=0.3, mask_loss_weight=1.0, max_grad_norm=1.0):
    """One CMC-stage optimisation step (train_cam_ctrl.py:540-665 minus data loading, VAE and CLIP): the camera
    encoder runs inside `pose_adaptor` with gradients, the loss weights the background (`1 - object mask`, :624)."""
    noisy_latents = noise_scheduler.add_noise(latents, noise, timesteps)
    model_pred = pose_adaptor(noisy_latents, timesteps, encoder_hidden_states=encoder_hidden_states,
                              pose_embedding=plucker_embedding)
    target = training_target(noise_scheduler, latents, noise, timesteps)
    loss = masked_mse_loss(model_pred, target, obj_masks, sd_loss_weight, mask_loss_weight, invert=True)
    loss.backward()
    if reducer is not None:
        reducer.finish()
    optimizer_update(trainable, optimizer, reducer, max_grad_norm)
    return loss.detach()


# ---- FMC stage 1: the Domain LoRA (train_image_lora.py) --------------------------------------------------------------------
def _spatial_lora_parameters(unet):
    return [(f"{name}.{k}", p) for name, proc in unet.attn_processors.items() if isinstance(proc, torch.nn.Module)
            for k, p in proc.named_parameters() if "_lora." in k]


def lora_trainable_parameters(unet) -> List[torch.nn.Parameter]:
    """The Domain-LoRA factors of the spatial attention processors (`LoRAAttnProcessor`, attn1 / attn2 of every transformer block;
    train_image_lora.py:170-180): turned into fp32 master parameters that require grad, and returned.  Nothing else changes: the
    motion-module LoRA and every other parameter keep their dtype and `requires_grad`."""
    params = []
    for _, p in _spatial_lora_parameters(unet):
        if p.dtype != torch.float32:
            p.data = p.data.float()
        p.requires_grad_(True)
        params.append(p)
    if not params:
        raise ValueError("the U-Net has no spatial LoRA processors (set_image_layer_lora / add_spatial_lora)")
    return params


def lora_state_dict(unet) -> dict:
    """The Domain-LoRA checkpoint in the key format of the reference's `AttnProcsLayers(unet.attn_processors).state_dict()`
    (train_image_lora.py:178, :392), e.g. `down_blocks.0.attentions.0.transformer_blocks.0.attn1.processor.to_q_lora.down.weight`:
    it loads into the stage-2 / stage-3 U-Nets with `load_state_dict(..., strict=False)` and no unexpected keys
    (train_cam_obj_ctrl.py:253-261)."""
    return {name: p.detach().clone() for name, p in _spatial_lora_parameters(unet)}


def stage1_training_step(unet, trainable: Iterable[torch.nn.Parameter], noise_scheduler, optimizer, reducer: Optional[GradAllReducer],
                         latents, noise, timesteps, encoder_hidden_states, max_grad_norm=1.0):
    """One Domain-LoRA optimisation step (train_image_lora.py:320-381 minus data loading, VAE and CLIP): `add_noise`, the
    epsilon-target MSE in fp32, clip, step, zero.  latents / noise `[B, 4, h, w]`, timesteps `[B]`, encoder_hidden_states `[B, 77, D]`.
    The images run as clips of one frame through the 3-D U-Net built without motion modules (`unet_kwargs(..., motion=False)`,
    loadable with `from_pretrained_2d`): per frame the arithmetic of the reference's `UNet2DConditionModel`.  Returns the loss."""
    noisy_latents = noise_scheduler.add_noise(latents, noise, timesteps)
    model_pred = unet(noisy_latents.unsqueeze(2), timesteps, encoder_hidden_states).sample.squeeze(2)
    target = training_target(noise_scheduler, latents, noise, timesteps)
    loss = F.mse_loss(model_pred.float(), target.float(), reduction="mean")
    loss.backward()
    if reducer is not None:
        reducer.finish()
    optimizer_update(trainable, optimizer, reducer, max_grad_norm)
    return loss.detach()


# ---- `train_mm`: the motion modules' norm / proj_in / proj_out (train_cam_ctrl.py:289-305, train_cam_obj_ctrl.py:367-384) ----------
def _motion_module_parameters(unet):
    """(name, parameter) exactly as the reference selects them: for every `TemporalTransformer3DModel` the prefixes `<module>.norm`,
    `<module>.proj_in`, `<module>.proj_out`, and every U-Net parameter whose name CONTAINS one of them (a substring rule)."""
    prefixes = []
    for name, module in unet.named_modules():
        if module.__class__.__name__ == "TemporalTransformer3DModel":
            prefixes += [f"{name}.norm", f"{name}.proj_in", f"{name}.proj_out"]
    out = []
    for name, p in unet.named_parameters():
        if any(pre in name for pre in prefixes):
            out.append((name, p))
    return out


def motion_module_trainable_parameters(unet) -> List[torch.nn.Parameter]:
    """The `train_mm` parameters (20 motion modules x 6 tensors at the SD-1.5 configs): turned into fp32 master parameters that require
    grad, and returned.  The bf16 kernels read the projections through bf16 shadows (`layers.bf16_param`), so AdamW updates below half a
    bf16 ulp of a weight accumulate in the master instead of being rounded away.  Nothing else changes."""
    params = []
    for _, p in _motion_module_parameters(unet):
        if p.dtype != torch.float32:
            p.data = p.data.float()
        p.requires_grad_(True)
        params.append(p)
    if not params:
        raise ValueError("the U-Net has no motion modules (TemporalTransformer3DModel)")
    return params


def motion_module_state_dict(unet) -> dict:
    """The `train_mm` checkpoint: `...temporal_transformer.{norm,proj_in,proj_out}.{weight,bias}` keys, loadable into the U-Net with
    `load_state_dict(..., strict=False)` and no unexpected keys.  (The reference's `mm_state_dict`, train_cam_ctrl.py:679-681, compares
    state-dict keys with module names and therefore saves an empty dict; this writes what it evidently intends.)"""
    return {name: p.detach().clone() for name, p in _motion_module_parameters(unet)}


# ---- stages 2 and 3 on the own kernels: Camera Encoder, Camera-Adapter merges, OMC Adapter as fp32 masters ------------------------------
def mark_trainable_own(module: torch.nn.Module) -> None:
    """Set the mark (`layers.OWN_MARK`) on `module` and every module below it: their forward then takes the own training route for bf16
    device activations -- fp32 masters read through bf16 shadows, no autocast (`layers.own_trainable`).  `FMC_TRAINABLE_OWN=0` sends
    the marked modules back to torch ops on cast weights."""
    from .models.layers import OWN_MARK
    for m in module.modules():
        m.__dict__[OWN_MARK] = True


def _masters(params) -> List[torch.nn.Parameter]:
    for p in params:
        if p.dtype != torch.float32:
            p.data = p.data.float()
        p.requires_grad_(True)
    return params


def camera_trainable_parameters(unet, pose_encoder) -> List[torch.nn.Parameter]:
    """The stage-2 parameters -- the same tensors in the same order as `stage2_trainable_parameters` -- turned into fp32 masters that
    require grad, and their modules (the whole Camera Encoder, every attention processor that owns a merge layer) marked for the own
    training route: run the step with bf16 activations and NO autocast.  The encoder then casts its input to bf16; forward, dX, dW and db of
    every projection, 1x1 and 3x3 convolution, the GEGLU feed-forwards, the average pools, ReLUs and the merges run on this library's
    kernels, reading cached bf16 shadows (`layers.bf16_param`) that `FusedAdamW.attach(unet, pose_encoder)` refreshes in its update.
    Buffers keep their dtype.  Not covered: a `Downsample(use_conv=True)` on an odd-sized input and 3x3 convolutions whose channel counts are no multiples of 64 (torch ops on cast weights), fp32 activations (the torch route as before); a U-Net with `q_merge` / `kv_merge`
    processors is refused."""
    partial = [n for n, m in unet.named_modules() if hasattr(m, "q_merge") or hasattr(m, "kv_merge")]
    if partial:
        raise NotImplementedError("camera_trainable_parameters: the q-only / kv-only Camera-Adapter merges (`q_merge` / `kv_merge`, configurations "
                                  f"that do not ship) have no own training route, e.g. {partial[0]}; train them with `stage2_trainable_parameters` "
                                  "under autocast")
    params = _masters(stage2_trainable_parameters(unet, pose_encoder))
    mark_trainable_own(pose_encoder)
    for m in unet.modules():
        if hasattr(m, "qkv_merge"):
            mark_trainable_own(m)
    return params


def omc_trainable_parameters(omcm) -> List[torch.nn.Parameter]:
    """The OMC Adapter's parameters (stage 3) as fp32 masters that require grad, the Adapter marked for the own training route (see
    `camera_trainable_parameters`): `get_traj_features_v2(..., omcm, ..., dtype=torch.bfloat16)` without autocast."""
    params = _masters(list(omcm.parameters()))
    mark_trainable_own(omcm)
    return params


def camera_state_dict(unet, pose_encoder) -> dict:
    """The stage-2 checkpoint in the reference's keys and split (train_cam_ctrl.py:671-678): `pose_encoder_state_dict` is the encoder's
    `state_dict()`, `attention_processor_state_dict` the U-Net entries of the trainable merge layers (names containing `merge`, no
    `lora`).  Both load into a bf16 model with `load_state_dict(..., strict=False)` and no unexpected keys."""
    return {"pose_encoder_state_dict": {k: v.detach().clone() for k, v in pose_encoder.state_dict().items()},
            "attention_processor_state_dict": {k: v.detach().clone() for k, v in unet.state_dict().items() if "merge" in k and "lora" not in k}}


def omc_state_dict(omcm) -> dict:
    """The stage-3 checkpoint entry `omcm_state_dict` (train_cam_obj_ctrl.py:963-968): the Adapter's `state_dict()`."""
    return {"omcm_state_dict": {k: v.detach().clone() for k, v in omcm.state_dict().items()}}

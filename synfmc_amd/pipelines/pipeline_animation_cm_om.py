"""Denoising pipelines of FMC (`fmc/pipelines/pipeline_animation_cm_om.py`) on the gfx950 path.

`CameraObjCtrlPipeline(vae, text_encoder, tokenizer, unet, scheduler, pose_encoder)(prompt, pose_embedding,
video_length, traj_features, height, width, num_inference_steps, guidance_scale, generator, omcm_min_step, ...)`
keeps the reference's constructor and call signature (:442-738).  The VAE and the CLIP text encoder are frozen
third-party models outside the metric: they are used through duck typing when given,
and `prompt_embeds=` / `output_type="latent"` let the loop run without them.

What changes under the hood (one denoising step = one U-Net forward at CFG batch 2 + the DDIM update):
  * camera features are computed once per clip and stay channels-last; they are NOT duplicated for the
    unconditional branch by a concat per level per step -- one `cat` per level per clip (reference :668-669);
  * OMC features are NOT zero-padded for the unconditional half (reference :671-676): `fmc_feature_add_fwd` simply
    skips that half;
  * `omcm_min_step` gating (:682-685) picks between two captured HIP graphs (with / without OMC features);
  * CFG combine + DDIM update are one fused kernel on fp32 latents (:711-720); with any other sampler of `synfmc_amd.schedulers` (DDIM
    with eta / clipping / v-prediction, Euler, Euler-ancestral, DPM-Solver++) the step is `fmc_sampler_step`, which also writes the next
    step's model input, so the loop launches no `cat` and no cast; `eta` and `generator` reach the scheduler (:335-351);
  * the captured graphs are kept on the pipeline between calls: text, camera and OMC features are copied into the
    graph's static buffers per clip (and the per-clip Camera-Adapter pose terms recomputed in place), so a second clip
    of the same shape costs no warm-up and no capture.

`AnimationPipeline` (:40-440) is the plain text-to-video loop of the LoRA-only configuration (BASELINE configs[1]):
base U-Net, no pose encoder, sliding-window "multidiff" blending included.

Sliding windows (`multidiff_total_steps > 1`) run under camera and object control too: the reference stops at an assert (:690)
because it never slices `traj_features`; here the windows go through the U-Net as batch entries with per-window text, camera and
OMC features gathered once per clip, and `fmc_window_step` averages the guided predictions over the overlaps, steps the full
latents and writes every window's next model input (`_window_loop`; `window_batch` caps the windows per U-Net call).
"""
from __future__ import annotations

import os
from typing import Callable, List, Optional, Union

import numpy as np
import torch

from ..models.pose_adaptor import features_to_video


class AnimationPipelineOutput:
    def __init__(self, videos):
        self.videos = videos


class _GraphedUNet:
    """Captures `unet(x, t, text[, pose_feats, traj])` into a HIP graph whose inputs are static buffers owned here;
    `set_conditioning` refills them for a new clip, `__call__` replays with new latents / timestep."""

    def __init__(self, unet, latents_shape, text, pose_feats, traj_feats, dtype, cfg_shared_input: bool = False, t_float: bool = False):
        self.unet = unet
        self.t_float = bool(t_float)                        # a timestep table with a fractional entry (Euler, linspace spacing): a float32 scalar
        self.cfg_shared_input = bool(cfg_shared_input)      # the caller feeds `cat([latents] * 2)`: the U-Net may compute the shared prefix once
        dev = text.device
        self.x = torch.zeros(latents_shape, dtype=dtype, device=dev)
        self.t = torch.zeros((), dtype=torch.float32 if self.t_float else torch.int64, device=dev)
        own = lambda v: v.detach().clone(memory_format=torch.preserve_format)
        self.text = own(text if text.dtype == dtype else text.to(dtype))   # (model dtype: the U-Net then hands THIS buffer to its cross-attention layers)
        self.pose = None if pose_feats is None else [own(p) for p in pose_feats]
        self.traj = None if traj_feats is None else [own(p) for p in traj_feats]
        self.graph = None
        self.out = None
        self._pose_terms = []

    def _call(self):
        kw = {}
        if self.pose is not None:
            kw = dict(pose_embedding_features=self.pose)
            if self.traj is not None or getattr(self.unet, "_pass_traj_none", False):   # (the CMC-only model takes no traj_features)
                kw["traj_features"] = self.traj
        if self.cfg_shared_input:
            kw["cfg_shared_input"] = True
        return self.unet(self.x, self.t, encoder_hidden_states=self.text, **kw).sample

    def capture(self):
        from .. import hip_ops as K
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._call()
        torch.cuda.current_stream().wait_stream(side)
        if getattr(self, "_cap_stream", None) is not None:     # re-capture (`set_conditioning` on a non-refillable runner): the old graph dies
            self.graph = None                                  # with its stream's stream-K workspace (~0.5 GB), not only the last one in __del__
            K.release_streamk_workspace(self._cap_stream)
        self._cap_stream = torch.cuda.Stream()
        K.prepare_streamk_workspace(self._cap_stream)      # allocated and zeroed eagerly, not inside the capture
        self.graph = torch.cuda.CUDAGraph()
        self._cap_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(self.graph, stream=self._cap_stream):
            self.out = self._call()
        torch.cuda.current_stream().wait_stream(self._cap_stream)
        # per-clip constants the processors computed during the warm-up (Camera-Adapter pose terms `s (W pose + b)`): the
        # graph reads them by address, so this runner keeps them alive and refreshes them in place for a new clip
        self._pose_terms = [(m, m.__dict__["_pose_term_cache"]) for m in self.unet.modules()
                            if m.__dict__.get("_pose_term_cache") is not None]
        # (the inner levels read the pose term through the q | k | v projection: `_PoseMerge._qkv_fold` -- its per-clip tensor is kept and refreshed too)
        self._qkv_folds = {id(m): m.__dict__["_qkv_fold_cache"] for m in self.unet.modules() if m.__dict__.get("_qkv_fold_cache") is not None}
        # ... and the text's k | v projections + fragment packs of the cross-attention layers (`Attention.text_kv`, once per clip): computed by the
        # warm-up calls from `self.text`, read by the graph by address, refreshed in place by `set_conditioning`
        self._text_kvs = [(m, m.__dict__["_text_kv"]) for m in self.unet.modules()
                          if m.__dict__.get("_text_kv") is not None and m.__dict__["_text_kv"][3] is self.text]
        # `set_conditioning` recomputes the pose terms from the `pose_view` tensors: that is only right while they ALIAS this runner's
        # static camera buffers (channels-last storage: the token view is free).  A layout that forced a private copy would replay the
        # next clip with this clip's camera term -- such a runner re-captures instead of refilling.
        mine = {p.untyped_storage().data_ptr() for p in (self.pose or [])}
        self._refillable = all(view.untyped_storage().data_ptr() in mine for _, (_, _, view) in self._pose_terms)

    def __del__(self):
        try:
            from .. import hip_ops as K
            if getattr(self, "_cap_stream", None) is not None:
                K.release_streamk_workspace(self._cap_stream)
        except Exception:
            pass

    def set_conditioning(self, text, pose_feats, traj_feats):
        """New clip, same shapes: refill the static buffers, recompute the pose terms into the tensors the graph reads."""
        from .. import hip_ops as K
        self.text.copy_(text)
        for dst, src in zip(self.pose or [], pose_feats or []):
            dst.copy_(src)
        for dst, src in zip(self.traj or [], traj_feats or []):
            dst.copy_(src)
        if not getattr(self, "_refillable", True):           # (pose terms were computed from private copies: capture again on the new buffers)
            for mod, _ in self._pose_terms:
                mod.__dict__.pop("_pose_term_cache", None)
                mod.__dict__.pop("_qkv_fold_cache", None)
            self.capture()
            return
        self._text_kvs = [(mod, mod.refresh_text_kv(entry)) for mod, entry in getattr(self, "_text_kvs", [])]
        for mod, (key, term, pose_view) in self._pose_terms:
            pf = pose_view if pose_view.is_contiguous() else pose_view.contiguous()
            term.copy_(K.linear(pf, mod.qkv_merge.weight, mod.qkv_merge.bias, None, key[-1]))
            fold = getattr(self, "_qkv_folds", {}).get(id(mod))    # the merge folded into q | k | v (inner levels): its per-clip term follows the pose term
            if fold is not None:
                assert fold[4] is term, "internal: the folded q | k | v term was built from another pose term"
                fold[2].copy_(K.linear(term, fold[3]))

    def __call__(self, x, t):
        self.x.copy_(x)
        self.t.fill_(float(t) if self.t_float else int(t))
        self.graph.replay()
        return self.out


_CLIP_PRODUCTS = ("_pose_term_cache", "_qkv_fold_cache", "_text_kv")      # what the modules keep per clip, one entry each
_LEGACY_WINDOWS = object()             # `AnimationPipeline(window_batch=...)` not given: the torch-op window loop and its bits


def _weights_version(module) -> int:
    """Fingerprint of everything a captured graph of `module` reads by address or was specialised on: identity, storage and version of
    every parameter and buffer (`p.data = ...`, `load_state_dict(assign=True)`, in-place updates), the attention-processor classes, and
    the module flags that change the launched kernels (fp8 temporal attention, LoRA / pose scales)."""
    items = [(id(t), t.data_ptr(), t._version) for t in list(module.parameters()) + list(module.buffers())]
    flags = []
    for m in module.modules():
        proc = m.__dict__.get("processor") or m._modules.get("processor") if hasattr(m, "_modules") else None
        if proc is not None:
            flags.append((type(proc).__name__, getattr(proc, "scale", None), getattr(proc, "lora_scale", None)))
        for name in ("_fp8_scales", "lora_scale", "motion_lora_scale"):
            v = m.__dict__.get(name)
            if v is not None:
                flags.append((name, id(v) if not isinstance(v, (int, float)) else v))
    return hash((tuple(items), tuple(flags)))


class AnimationPipeline:
    """Plain text-to-video loop.  Reference: pipeline_animation_cm_om.py:40-440 --
    `AnimationPipeline(vae, text_encoder, tokenizer, unet, scheduler)(prompt, video_length, height, width,
    num_inference_steps, guidance_scale, ...)`.  One denoising step = the base U-Net at CFG batch 2 on every sliding
    window (`multidiff_total_steps` windows of `video_length` frames overlapping by `multidiff_overlaps`, noise predictions
    averaged where windows overlap, :399-421) + the DDIM update."""
    vae_scale_factor = 8

    def __init__(self, vae, text_encoder, tokenizer, unet, scheduler):
        from ..schedulers import coerce_scheduler
        self.vae, self.text_encoder, self.tokenizer = vae, text_encoder, tokenizer
        self.unet, self.scheduler = unet, coerce_scheduler(scheduler)       # accepts a diffusers DDIM / Euler / Euler-ancestral / DPM-Solver++ scheduler as well
        self._runners = {}

    # ---- pieces outside the metric ------------------------------------------------------------------
    def _encode_prompt(self, prompt, device, num_videos_per_prompt, do_classifier_free_guidance, negative_prompt):
        if self.tokenizer is None or self.text_encoder is None:
            raise RuntimeError("no tokenizer / text_encoder attached: pass `prompt_embeds=` "
                               "([2B,77,C] = uncond || cond when guidance_scale > 1)")
        def enc(texts):
            ids = self.tokenizer(texts, padding="max_length", max_length=self.tokenizer.model_max_length,
                                 truncation=True, return_tensors="pt").input_ids.to(device)
            return self.text_encoder(ids)[0]
        text = enc(prompt).repeat_interleave(num_videos_per_prompt, dim=0)
        if not do_classifier_free_guidance:
            return text
        neg = [""] * len(prompt) if negative_prompt is None else negative_prompt
        return torch.cat([enc(neg).repeat_interleave(num_videos_per_prompt, dim=0), text])

    def decode_latents(self, latents):
        if self.vae is None:
            raise RuntimeError("no VAE attached: call with output_type='latent'")
        video_length = latents.shape[2]
        latents = 1 / 0.18215 * latents
        b = latents.shape[0]
        frames = latents.permute(0, 2, 1, 3, 4).reshape(b * video_length, *latents.shape[1:2], *latents.shape[3:])
        video = torch.cat([self.vae.decode(frames[i:i + 1]).sample for i in range(frames.shape[0])])
        video = video.reshape(b, video_length, *video.shape[1:]).permute(0, 2, 1, 3, 4)
        return ((video / 2 + 0.5).clamp(0, 1)).cpu().float().numpy()

    def check_inputs(self, prompt, height, width, callback_steps):
        if prompt is not None and not isinstance(prompt, (str, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_steps is None or not isinstance(callback_steps, int) or callback_steps <= 0:
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type"
                             f" {type(callback_steps)}.")

    def prepare_latents(self, batch_size, num_channels_latents, video_length, height, width, dtype, device, generator,
                        latents=None):
        shape = (batch_size, num_channels_latents, video_length, height // self.vae_scale_factor,
                 width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective"
                             f" batch size of {batch_size}.")
        if latents is None:
            if isinstance(generator, list):
                latents = torch.cat([torch.randn((1,) + shape[1:], generator=g, device=g.device, dtype=torch.float32)
                                     .to(device) for g in generator])
            else:
                gen_dev = generator.device if isinstance(generator, torch.Generator) else torch.device(device)
                latents = torch.randn(shape, generator=generator, device=gen_dev, dtype=torch.float32).to(device)
        else:
            if latents.shape != shape:
                raise ValueError(f"Unexpected latents shape, got {latents.shape}, expected {shape}")
            latents = latents.to(device)
        return latents.float() * self.scheduler.init_noise_sigma

    # ---- shared machinery of the two loops -----------------------------------------------------------
    def _prologue(self, prompt, height, width, callback_steps, latents, num_videos_per_prompt, guidance_scale,
                  negative_prompt, prompt_embeds, device, eta):
        unet = self.unet
        self._slot_products = {}                    # (the eager window chunks' per-clip products: `_runner`)
        if hasattr(unet, "invalidate_text_conditioning"):
            unet.invalidate_text_conditioning()     # a new clip: no text k | v of the previous prompt survives (they are re-made once below / by the runner)
        height = height or unet.config.sample_size * self.vae_scale_factor
        width = width or unet.config.sample_size * self.vae_scale_factor
        self.check_inputs(prompt, height, width, callback_steps)
        do_cfg = guidance_scale > 1.0
        # the loops below feed the U-Net `cat([latents] * 2)` under classifier-free guidance: its two halves are identical until the
        # first text cross-attention, and the U-Net may compute that prefix once (the `cfg_shared_input` keyword of its forward, passed per call:
        # nothing sticky on the module; FMC_CFG_SHARED=0: A/B)
        self._cfg_shared = bool(do_cfg) and os.environ.get("FMC_CFG_SHARED", "1") != "0"
        batch_size = 1
        if latents is not None:
            batch_size = latents.shape[0]
        if isinstance(prompt, list):
            batch_size = len(prompt)
        if prompt_embeds is None:
            prompt = prompt if isinstance(prompt, list) else [prompt] * batch_size
            if negative_prompt is not None and not isinstance(negative_prompt, list):
                negative_prompt = [negative_prompt] * batch_size
            prompt_embeds = self._encode_prompt(prompt, device, num_videos_per_prompt, do_cfg, negative_prompt)
        text = prompt_embeds.to(device=device, dtype=unet.dtype)
        return height, width, do_cfg, batch_size, text

    def _runner(self, x_shape, text, pose_feats, traj, use_graph, t_float: bool = False, slot=None):
        """The U-Net step as a callable `(x, t) -> eps`: a cached HIP graph (refilled with this clip's conditioning) or eager.
        `t_float`: the timestep table has a fractional entry, which has to reach the U-Net untruncated.  `slot`: the chunk of windows
        this runner serves when a clip's windows go through the U-Net in several calls, each with conditioning of its own: a graph of
        its own per slot, and on the eager path the modules' per-clip products (pose terms, folded q | k | v terms, the text's k | v)
        of the slot's first call are put back before every later one, so that they are computed once per clip and slot."""
        unet = self.unet
        shared = bool(getattr(self, "_cfg_shared", False)) and getattr(unet, "_accepts_cfg_shared_input", False)   # (a foreign U-Net never sees the keyword)
        skw = {"cfg_shared_input": True} if shared else {}
        if not use_graph:
            if slot is None and hasattr(unet, "prepare_text_conditioning") and not torch.is_grad_enabled():
                unet.prepare_text_conditioning(text)     # once per clip, before the loop -- not inside step 1
            # (a slot's text k | v are made by its first call and kept with its other per-clip products: preparing every slot here would
            # only overwrite the modules' one entry slot after slot)
            kept = None if slot is None else self._slot_products.setdefault(slot, {})
            def eager(x, t):
                kw = {}
                if pose_feats is not None:
                    kw["pose_embedding_features"] = pose_feats
                    if traj is not None or getattr(unet, "_pass_traj_none", False):    # (UNet3DConditionModelPoseCond takes no traj_features)
                        kw["traj_features"] = traj
                tt = torch.tensor(float(t), dtype=torch.float32, device=x.device) if t_float else torch.tensor(int(t), device=x.device)
                for m, entries in (kept or {}).items():
                    m.__dict__.update(entries)
                out = unet(x, tt, encoder_hidden_states=text, **skw, **kw).sample
                if kept is not None and not kept:
                    kept.update({m: {k: m.__dict__[k] for k in _CLIP_PRODUCTS if m.__dict__.get(k) is not None} for m in unet.modules()
                                 if any(m.__dict__.get(k) is not None for k in _CLIP_PRODUCTS)})
                return out
            return eager
        from .. import hip_ops as K
        # (`hip_ops.PARTIAL_TILES` and `hip_ops.FP8_FF` decide launches that a captured graph replays: a graph captured under another setting is not this step's)
        key = (tuple(x_shape), tuple(text.shape), unet.dtype, pose_feats is not None, traj is not None,
               shared, bool(t_float), bool(K.PARTIAL_TILES), bool(K.FP8_FF), slot, _weights_version(unet))
        r = self._runners.get(key)
        if r is None:
            for k in [k for k in self._runners if k[:-1] == key[:-1]]:      # same shapes, stale weights: drop the graph
                del self._runners[k]
            r = _GraphedUNet(unet, x_shape, text, pose_feats, traj, unet.dtype, cfg_shared_input=shared, t_float=t_float)
            r.capture()
            self._runners[key] = r
        else:
            r.set_conditioning(text, pose_feats, traj)
        return r

    def _sampler_path(self, eta, generator, timesteps, x_shape, latents, do_cfg):
        """`(fused, t_float, step keywords, x_in)`.  Every configuration but the plain DDIM one steps through `fmc_sampler_step`, which
        also writes the next model input (scaled, CFG-duplicated, in the model's dtype) into `x_in`: only the first input of a clip is
        made by torch ops.  `eta` and `generator` go to the scheduler, which uses what its family takes (reference :335-351)."""
        sch = self.scheduler
        t_float = any(not float(t).is_integer() for t in timesteps)
        if not (hasattr(sch, "fused_input") and sch.fused_input(eta)):
            if eta != 0.0:
                raise NotImplementedError(f"{type(sch).__name__} takes no eta")
            return False, t_float, {}, None
        x_in = torch.empty(x_shape, dtype=self.unet.dtype, device=latents.device)
        if tuple(x_shape) == (latents.shape[0] * (2 if do_cfg else 1),) + tuple(latents.shape[1:]):
            first = sch.scale_model_input(latents, timesteps[0])
            x_in.copy_(torch.cat([first] * 2) if do_cfg else first)
        else:
            x_in = None                                     # sliding windows: the inputs are slices, made per window
        return True, t_float, dict(eta=eta, generator=generator), x_in

    def _window_loop(self, latents, single, overlap, windows, text, pose_w, traj_w, window_batch, use_graph, timesteps, guidance_scale,
                     do_cfg, eta, generator, omcm_min_step, callback, callback_steps):
        """Sliding windows on `fmc_window_step`.  The windows go through the U-Net as batch entries `[R][W_chunk][B]` (R: uncond,
        cond), `window_batch` of them per call (None: all); text, camera (`pose_w`: per window, per level `[B, c, F, h, w]`, or None)
        and OMC features (`traj_w`, likewise) are gathered per chunk ONCE per clip, and every chunk has a runner of its own, so that
        its pose terms, folded q | k | v terms and text k | v are made once per clip.  The kernel averages the guided predictions
        over the overlaps, steps the full latents and writes every window's next model input (reference :687-720)."""
        unet, sch = self.unet, self.scheduler
        if not hasattr(sch, "step_windows"):
            raise NotImplementedError(f"{type(sch).__name__} has no step_windows")
        if window_batch is not None and (not isinstance(window_batch, int) or window_batch < 1):
            raise ValueError(f"window_batch {window_batch!r}: None (all windows in one U-Net call) or a positive int")
        B, R, W = latents.shape[0], 2 if do_cfg else 1, windows
        stride = single - overlap
        per = W if window_batch is None else min(window_batch, W)
        chunks = [(k, min(k + per, W)) for k in range(0, W, per)]
        blk = (B, latents.shape[1], single) + tuple(latents.shape[3:])
        # one buffer for every window's model input and one for the predictions, addressed by (stride_r, stride_w): [R][W][B] storage is
        # one U-Net batch; with one window per call [W][R][B] storage makes every call's batch dense
        per_window = per == 1 and W > 1
        def buffer():
            store = torch.empty(((W, R) if per_window else (R, W)) + blk, dtype=unet.dtype, device=latents.device)
            return store.transpose(0, 1) if per_window else store
        x_in = buffer()
        eps = buffer() if len(chunks) > 1 else None
        first = sch.scale_model_input(latents, timesteps[0])
        for w in range(W):
            x_in[:, w] = first[:, :, w * stride:w * stride + single]
        t_float = any(not float(t).is_integer() for t in timesteps)
        uses_traj = [traj_w is not None and not (omcm_min_step > 0 and t < omcm_min_step) for t in timesteps]      # reference :682-685
        cl3d = lambda v: v.contiguous(memory_format=torch.channels_last_3d)
        runs = {}
        for ci, (k0, k1) in enumerate(chunks):              # every runner of the clip before its first step
            n = k1 - k0
            text_c = text.reshape((R, 1, B) + tuple(text.shape[1:])).expand((R, n, B) + tuple(text.shape[1:])) \
                .reshape((R * n * B,) + tuple(text.shape[1:])).contiguous()
            pose_c = traj_c = None
            if pose_w is not None:
                pose_c = [cl3d(torch.cat([torch.cat([pose_w[w][lv] for w in range(k0, k1)])] * R)) for lv in range(len(pose_w[0]))]
            if traj_w is not None:
                traj_c = [cl3d(torch.cat([traj_w[w][lv] for w in range(k0, k1)]).to(unet.dtype)) for lv in range(len(traj_w[0]))]
            for key in sorted(set(uses_traj)):
                runs[ci, key] = self._runner((R * n * B,) + blk[1:], text_c, pose_c, traj_c if key else None, use_graph, t_float,
                                             slot=ci if len(chunks) > 1 else None)
        for i, t in enumerate(timesteps):
            for ci, (k0, k1) in enumerate(chunks):
                out = runs[ci, uses_traj[i]](x_in[:, k0:k1].reshape((R * (k1 - k0) * B,) + blk[1:]), t)
                if eps is not None:
                    eps[:, k0:k1].copy_(out.reshape((R, k1 - k0) + blk))
            e = eps if eps is not None else out.contiguous().view((R, W) + blk)
            latents = sch.step_windows(e, t, latents, guidance_scale, overlap, eta=eta, generator=generator, x_in=x_in)
            if callback is not None and i % callback_steps == 0:
                callback(i, t, latents)
        self._slot_products = {}                            # (the chunks' per-clip tensors are not kept beyond the clip)
        return latents

    def _finish(self, latents, output_type, return_dict):
        if output_type == "latent":
            video = latents
        else:
            video = self.decode_latents(latents)
            if output_type == "tensor":
                video = torch.from_numpy(video)
        if not return_dict:
            return video
        return AnimationPipelineOutput(videos=video)

    # ---- the plain denoising loop (BASELINE configs[1]) ----------------------------------------------
    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None], video_length: Optional[int], height: Optional[int] = None,
                 width: Optional[int] = None, num_inference_steps: int = 50, guidance_scale: float = 7.5,
                 negative_prompt=None, num_videos_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None,
                 latents: Optional[torch.Tensor] = None, output_type: Optional[str] = "tensor",
                 return_dict: bool = True, callback: Optional[Callable] = None, callback_steps: Optional[int] = 1,
                 multidiff_total_steps: int = 1, multidiff_overlaps: int = 12, prompt_embeds=None,
                 use_graph: bool = True, window_batch=_LEGACY_WINDOWS, **kwargs):
        """`window_batch` (None: all windows in one U-Net call, or an int: at most that many per call) moves the sliding windows onto
        `fmc_window_step` (`_window_loop`); not given, the windows run one after another on torch ops, with the bits they always had."""
        unet = self.unet
        device = next(unet.parameters()).device
        height, width, do_cfg, batch_size, text = self._prologue(
            prompt, height, width, callback_steps, latents, num_videos_per_prompt, guidance_scale, negative_prompt,
            prompt_embeds, device, eta)
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        timesteps = self.scheduler._timesteps_host
        single = video_length
        video_length = multidiff_total_steps * (video_length - multidiff_overlaps) + multidiff_overlaps       # :369
        latents = self.prepare_latents(batch_size * num_videos_per_prompt, unet.in_channels, video_length, height,
                                       width, text.dtype, device, generator, latents).contiguous()
        if multidiff_total_steps > 1 and window_batch is not _LEGACY_WINDOWS:
            if not 0 <= multidiff_overlaps < single:
                raise ValueError(f"multidiff_overlaps {multidiff_overlaps}: windows of {single} frames overlap by 0 .. {single - 1}")
            latents = self._window_loop(latents, single, multidiff_overlaps, multidiff_total_steps, text, None, None, window_batch,
                                        use_graph, timesteps, guidance_scale, do_cfg, eta, generator, 0, callback, callback_steps)
            return self._finish(latents, output_type, return_dict)
        x_shape = (latents.shape[0] * (2 if do_cfg else 1), latents.shape[1], single) + tuple(latents.shape[3:])
        fused, t_float, step_kw, x_in = self._sampler_path(eta, generator, timesteps, x_shape, latents, do_cfg)
        run = self._runner(x_shape, text, None, None, use_graph, t_float)
        stride = single - multidiff_overlaps
        for i, t in enumerate(timesteps):
            if multidiff_total_steps == 1 and fused:
                latents = self.scheduler.step_cfg(run(x_in, t), t, latents, guidance_scale, do_cfg, x_in=x_in, **step_kw)
            elif multidiff_total_steps == 1:
                x = torch.cat([latents] * 2) if do_cfg else latents
                eps = run(x.to(unet.dtype), t)
                latents = self.scheduler.step_cfg(eps, t, latents, guidance_scale, do_cfg)
            else:                                       # sliding windows: average the guided predictions (:399-421)
                full = torch.zeros_like(latents)
                count = torch.zeros_like(latents)
                for w in range(multidiff_total_steps):
                    s0 = w * stride
                    part = latents[:, :, s0:s0 + single].contiguous()
                    if fused:
                        part = self.scheduler.scale_model_input(part, t)
                    x = torch.cat([part] * 2) if do_cfg else part
                    eps = run(x.to(unet.dtype), t).float()
                    if do_cfg:
                        eu, ec = eps.chunk(2)
                        eps = eu + guidance_scale * (ec - eu)
                    full[:, :, s0:s0 + single] += eps
                    count[:, :, s0:s0 + single] += 1
                latents = self.scheduler.step_cfg((full / count).contiguous(), t, latents, 1.0, False, **step_kw)
            if callback is not None and i % callback_steps == 0:
                callback(i, t, latents)
        return self._finish(latents, output_type, return_dict)


class CameraObjCtrlPipeline(AnimationPipeline):
    """Reference: pipeline_animation_cm_om.py:442-738 (a subclass of `AnimationPipeline` there too)."""

    def __init__(self, vae, text_encoder, tokenizer, unet, scheduler, pose_encoder):
        super().__init__(vae, text_encoder, tokenizer, unet, scheduler)
        self.pose_encoder = pose_encoder

    def _frame_limit(self):
        """Frames the Camera Encoder can see at once: the length of its temporal positional table (None: it has none)."""
        from ..models.motion_module import PositionalEncoding
        mods = self.pose_encoder.modules() if hasattr(self.pose_encoder, "modules") else []
        sizes = [int(m.pe.shape[1]) for m in mods if isinstance(m, PositionalEncoding)]
        return min(sizes) if sizes else None

    def _window_conditioning(self, pose_embedding, traj_features, single, overlap, windows, batch):
        """Camera and OMC features per window: `(pose_w, traj_w)`, each a list over the windows of per-level `[B, c, F, h, w]`
        tensors (`traj_w` None without OMC features).  Tensor forms cover all `Ftot` frames and are sliced (reference :700); list
        forms hold one entry per window (reference :646-653)."""
        stride = single - overlap
        total = (windows - 1) * stride + single
        cut = lambda levels: [[x[:, :, w * stride:w * stride + single] for x in levels] for w in range(windows)]
        if isinstance(pose_embedding, (list, tuple)):
            for pe in pose_embedding:
                if pe.ndim != 5 or pe.shape[2] != single:
                    raise ValueError(f"every pose embedding of the list is [B, 6, {single}, H, W]: got {tuple(pe.shape)}")
            bs = pose_embedding[0].shape[0]
            pose_w = [features_to_video(self.pose_encoder(pe), bs) for pe in pose_embedding]
        else:
            if pose_embedding.ndim != 5 or pose_embedding.shape[2] != total:
                raise ValueError(f"pose_embedding covers {tuple(pose_embedding.shape)}: {windows} windows of {single} frames overlapping "
                                 f"by {overlap} need [B, 6, {total}, H, W] (or a list of one embedding per window)")
            limit = self._frame_limit()
            if limit is not None and total > limit:
                raise ValueError(f"pose_embedding as one tensor is encoded in one pass over {total} frames, and the Camera Encoder's "
                                 f"positional table holds {limit}: pass a list of one embedding per window")
            bs = pose_embedding.shape[0]
            pose_w = cut(features_to_video(self.pose_encoder(pose_embedding), bs))
        traj_w = None
        if traj_features is not None:
            if isinstance(traj_features[0], (list, tuple)):
                if len(traj_features) != windows:
                    raise ValueError(f"traj_features lists {len(traj_features)} windows, multidiff_total_steps is {windows}")
                traj_w = [list(levels) for levels in traj_features]
                frames = {int(x.shape[2]) for levels in traj_w for x in levels}
                if frames != {single}:
                    raise ValueError(f"every window's traj_features cover {single} frames: got {sorted(frames)}")
            else:
                frames = {int(x.shape[2]) for x in traj_features}
                if frames != {total}:
                    raise ValueError(f"traj_features cover {sorted(frames)} frames: {windows} windows of {single} frames overlapping by "
                                     f"{overlap} need {total} (or a list of one per-level list per window)")
                traj_w = cut(list(traj_features))
            if any(x.shape[0] != batch for levels in traj_w for x in levels):
                raise ValueError(f"OMC features do not cover the {batch} clips of the latents")
        if bs != batch:
            raise ValueError(f"camera features cover {bs} clips but the latents hold {batch} "
                             "(num_videos_per_prompt > 1 needs the conditioning repeated by the caller)")
        return pose_w, traj_w

    # ---- the denoising loop (the metric's unit) ------------------------------------------------------
    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None], pose_embedding: torch.Tensor, video_length: Optional[int],
                 traj_features=None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, negative_prompt=None,
                 num_videos_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None,
                 latents: Optional[torch.Tensor] = None, output_type: Optional[str] = "tensor",
                 return_dict: bool = True, callback: Optional[Callable] = None, callback_steps: Optional[int] = 1,
                 multidiff_total_steps: int = 1, multidiff_overlaps: int = 12, prompt_embeds=None,
                 use_graph: bool = True, pose_embedding_unshuffled: bool = False, window_batch: Optional[int] = None, **kwargs):
        """`multidiff_total_steps > 1`: sliding windows of `video_length` frames overlapping by `multidiff_overlaps` (the reference
        stops at an assert, :690, because it never slices `traj_features`; its slicing of the camera features, :646-653 and :697-701,
        and its average, :715-717, are what runs here).  `pose_embedding`: a 5-d tensor over all frames, encoded once and sliced per
        window, or a list of one tensor per window, each encoded on its own.  `traj_features`: per-level tensors over all frames, or a
        list of one per-level list per window.  `window_batch`: windows per U-Net call (None: all)."""
        unet = self.unet
        windows = int(multidiff_total_steps)
        pose_list = isinstance(pose_embedding, (list, tuple))
        if windows > 1:
            if not 0 <= multidiff_overlaps < video_length:
                raise ValueError(f"multidiff_overlaps {multidiff_overlaps}: windows of {video_length} frames overlap by 0 .. {video_length - 1}")
            if pose_embedding_unshuffled:
                raise ValueError("pose_embedding_unshuffled takes one window (multidiff_total_steps=1)")
            if pose_list and len(pose_embedding) != windows:
                raise ValueError(f"pose_embedding lists {len(pose_embedding)} windows, multidiff_total_steps is {windows}")
        elif pose_list:
            raise ValueError("a list of pose embeddings is one per window: it needs multidiff_total_steps > 1")
        device = (pose_embedding[0] if pose_list else pose_embedding).device
        height, width, do_cfg, batch_size, text = self._prologue(
            prompt, height, width, callback_steps, latents, num_videos_per_prompt, guidance_scale, negative_prompt,
            prompt_embeds, device, eta)

        self.scheduler.set_timesteps(num_inference_steps, device=device)
        timesteps = self.scheduler._timesteps_host
        single = video_length
        video_length = windows * (single - multidiff_overlaps) + multidiff_overlaps if windows > 1 else single      # :369
        latents = self.prepare_latents(batch_size * num_videos_per_prompt, unet.in_channels, video_length, height,
                                       width, text.dtype, device, generator, latents).contiguous()
        if windows > 1:
            pose_w, traj_w = self._window_conditioning(pose_embedding, traj_features, single, multidiff_overlaps, windows, latents.shape[0])
            latents = self._window_loop(latents, single, multidiff_overlaps, windows, text, pose_w, traj_w, window_batch, use_graph,
                                        timesteps, guidance_scale, do_cfg, eta, generator, kwargs.get("omcm_min_step", 0), callback,
                                        callback_steps)
            return self._finish(latents, output_type, return_dict)

        # camera features: once per clip (reference :657-669)
        if pose_embedding_unshuffled:
            bs = pose_embedding.shape[0] // video_length
            feats = self.pose_encoder.forward_unshuffled(pose_embedding, bs)
        else:
            assert pose_embedding.ndim == 5
            bs = pose_embedding.shape[0]
            feats = self.pose_encoder(pose_embedding)
        if bs != latents.shape[0] or (traj_features is not None and traj_features[0].shape[0] != latents.shape[0]):
            # the reference fails here too (`hidden_states + traj_features[idx]` / the pose merge on mismatched batches)
            raise ValueError(f"camera / OMC features cover {bs} clips but the latents hold {latents.shape[0]} "
                             "(num_videos_per_prompt > 1 needs the conditioning repeated by the caller)")
        pose_feats = features_to_video(feats, bs)
        if do_cfg:
            pose_feats = [torch.cat([x, x], dim=0) for x in pose_feats]
        pose_feats = [x.contiguous(memory_format=torch.channels_last_3d) for x in pose_feats]
        if traj_features is not None:
            traj_features = [t.to(unet.dtype).contiguous(memory_format=torch.channels_last_3d) for t in traj_features]

        omcm_min_step = kwargs.get("omcm_min_step", 0)
        x_shape = (latents.shape[0] * (2 if do_cfg else 1),) + tuple(latents.shape[1:])
        runs = {}
        fused, t_float, step_kw, x_in = self._sampler_path(eta, generator, timesteps, x_shape, latents, do_cfg)

        for i, t in enumerate(timesteps):
            traj = traj_features
            if traj_features is not None and omcm_min_step > 0 and t < omcm_min_step:      # reference :682-685
                traj = None
            key = traj is not None
            if key not in runs:
                runs[key] = self._runner(x_shape, text, pose_feats, traj, use_graph, t_float)
            if fused:
                latents = self.scheduler.step_cfg(runs[key](x_in, t), t, latents, guidance_scale, do_cfg, x_in=x_in, **step_kw)
            else:
                x = torch.cat([latents] * 2) if do_cfg else latents
                eps = runs[key](x.to(unet.dtype), t)
                latents = self.scheduler.step_cfg(eps, t, latents, guidance_scale, do_cfg)
            if callback is not None and i % callback_steps == 0:
                callback(i, t, latents)
        return self._finish(latents, output_type, return_dict)

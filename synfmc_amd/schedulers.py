"""Samplers of the FMC denoising loop.  The reference takes them from `diffusers` (`train_cam_obj_ctrl.py:231,802`,
`pipeline_animation_cm_om.py:624,705,720`; kwargs from `configs/*.yaml: noise_scheduler_kwargs`); its pipelines are typed for
DDIM, PNDM, LMS, Euler, Euler-ancestral and DPM-Solver multistep.  Built here: `DDIMScheduler`, `EulerDiscreteScheduler`,
`EulerAncestralDiscreteScheduler` and `DPMSolverMultistepScheduler` (dpmsolver++, midpoint, orders 1-3).

Host side: the beta schedule, the timestep and sigma tables and the coefficients of one step (tiny; float64 from the float32
tables diffusers keeps).  Device side: `step_cfg` runs the classifier-free-guidance combine and the update as ONE launch on fp32
latents -- `fmc_cfg_ddim_step` for the configuration the FMC configs use (DDIM, eta = 0, epsilon, no clipping, leading spacing),
`fmc_sampler_step` for everything else: every update here is `x' = c_x x + c_e e + c_m m + sum c_h[j] hist[j] + c_n noise` with
`m = clamp(m_x x + m_e e)` the x0 prediction, and the kernel also writes the next step's model input.  `step_windows` is the same step
for sliding windows: one prediction per window, averaged where windows overlap, on `fmc_window_step` with the same coefficients.

The timestep and sigma tables follow diffusers 0.24.0 as read, not as run: no copy of the library was at hand."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import hip_ops as K


class DDIMSchedulerOutput:
    def __init__(self, prev_sample, pred_original_sample=None):
        self.prev_sample = prev_sample
        self.pred_original_sample = pred_original_sample


SchedulerOutput = DDIMSchedulerOutput


class _Config:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def get(self, k, d=None):
        return self.__dict__.get(k, d)


def _make_betas(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas, cls):
    if trained_betas is not None:
        return torch.as_tensor(np.asarray(trained_betas, dtype=np.float32))
    if beta_schedule == "linear":
        return torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)      # (diffusers 0.24.0 scheduling_ddim.py: torch.linspace, fp32)
    if beta_schedule == "scaled_linear":
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    raise NotImplementedError(f"{beta_schedule} is not implemented for {cls}")


def _draw_noise(latents, eps, generator):
    """diffusers' `randn_tensor`: the shape of the combined prediction, the model dtype, drawn on the generator's device."""
    if isinstance(generator, (list, tuple)):              # one generator per sample, as randn_tensor draws them
        return torch.cat([torch.randn((1,) + tuple(latents.shape[1:]), generator=g, device=g.device, dtype=eps.dtype).to(latents.device)
                          for g in generator]).contiguous()
    gen_dev = generator.device if isinstance(generator, torch.Generator) else latents.device
    return torch.randn(latents.shape, generator=generator, device=gen_dev, dtype=eps.dtype).to(latents.device).contiguous()


def _add_noise_ac(self, original_samples, noise, timesteps):
    key = (original_samples.device, original_samples.dtype)
    cache = self.__dict__.setdefault("_ac_dev", {})
    ac = cache.get(key)
    if ac is None:                 # one host-to-device copy per (device, dtype): capturable in a HIP graph afterwards
        ac = cache[key] = self.alphas_cumprod.to(device=original_samples.device, dtype=original_samples.dtype)
    timesteps = timesteps.to(original_samples.device)
    a = ac[timesteps] ** 0.5
    s = (1 - ac[timesteps]) ** 0.5
    while a.ndim < original_samples.ndim:
        a, s = a.unsqueeze(-1), s.unsqueeze(-1)
    return a, s


class DDIMScheduler:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0,
                 prediction_type="epsilon", thresholding=False, timestep_spacing="leading", clip_sample_range=1.0, **_unused):
        betas = _make_betas(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas, self.__class__)
        if prediction_type not in ("epsilon", "sample", "v_prediction"):
            raise ValueError(f"prediction_type {prediction_type!r}: epsilon, sample or v_prediction")
        if thresholding:
            raise NotImplementedError("dynamic thresholding is not built (clip_sample with clip_sample_range is)")
        if timestep_spacing not in ("leading", "linspace", "trailing"):
            raise ValueError(f"timestep_spacing {timestep_spacing!r}: leading, linspace or trailing")
        self.betas = betas
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.config = _Config(num_train_timesteps=num_train_timesteps, steps_offset=steps_offset, prediction_type=prediction_type,
                              clip_sample=clip_sample, beta_schedule=beta_schedule, clip_sample_range=clip_sample_range,
                              timestep_spacing=timestep_spacing, thresholding=thresholding)
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        # the configuration of configs/*.yaml keeps its own kernel (bench.py and the trace tools find step boundaries by its name)
        self._plain = prediction_type == "epsilon" and not clip_sample and timestep_spacing == "leading"

    def set_timesteps(self, num_inference_steps: int, device=None):
        T = self.config.num_train_timesteps
        if num_inference_steps > T:
            raise ValueError("num_inference_steps cannot exceed num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        spacing = self.config.timestep_spacing
        if spacing == "leading":
            ratio = T // num_inference_steps
            ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.config.steps_offset
        elif spacing == "linspace":
            ts = np.linspace(0, T - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        else:
            ts = np.round(np.arange(T, 0, -T / num_inference_steps)).astype(np.int64) - 1
        self._timesteps_host = ts.tolist()
        self.timesteps = torch.tensor(self._timesteps_host, dtype=torch.int64, device=device)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def fused_input(self, eta: float = 0.0) -> bool:
        """Whether `step_cfg` goes through `fmc_sampler_step` (and can emit the next model input) for this configuration."""
        return not (self._plain and eta == 0.0)

    def next_input_scale(self) -> float:
        return 1.0

    def _alphas(self, t: int):
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else float(self.final_alpha_cumprod)
        return a_t, a_prev

    def add_noise(self, original_samples, noise, timesteps):
        a, s = _add_noise_ac(self, original_samples, noise, timesteps)
        return a * original_samples + s * noise

    def get_velocity(self, sample, noise, timesteps):
        a, s = _add_noise_ac(self, sample, noise, timesteps)
        return a * noise - s * sample

    def _coefs(self, t: int, eta: float, use_clipped_model_output: bool):
        a_t, a_prev = self._alphas(t)
        sa, sb = math.sqrt(a_t), math.sqrt(1.0 - a_t)
        kind = self.config.prediction_type
        if kind == "epsilon":
            m_x, m_e, p = 1.0 / sa, -sb / sa, (0.0, 1.0, 0.0)
        elif kind == "sample":
            m_x, m_e, p = 0.0, 1.0, (1.0 / sb, -sa / sb, 0.0)
        else:
            m_x, m_e, p = sa, -sb, (sb, sa, 0.0)
        if use_clipped_model_output:            # the noise prediction re-derived from the (clipped) x0
            p = (1.0 / sb, 0.0, -sa / sb)
        std = eta * math.sqrt((1.0 - a_prev) / (1.0 - a_t) * (1.0 - a_t / a_prev)) if eta > 0.0 else 0.0
        d = math.sqrt(max(1.0 - a_prev - std * std, 0.0))
        return dict(m_x=m_x, m_e=m_e, m_clamp=float(self.config.clip_sample_range) if self.config.clip_sample else 0.0,
                    c_x=d * p[0], c_e=d * p[1], c_m=math.sqrt(a_prev) + d * p[2], c_n=std)

    def step_cfg(self, eps: torch.Tensor, timestep: int, latents: torch.Tensor, guidance_scale: float,
                 has_uncond: bool, eta: float = 0.0, generator=None, x_in=None, use_clipped_model_output: bool = False,
                 variance_noise=None) -> torch.Tensor:
        """eps `[2B, ...]` (uncond || cond) or `[B, ...]`, latents fp32 `[B, ...]` -> new fp32 latents.  `x_in` (model dtype,
        `[2B or B, ...]`): receives the next step's model input when the step runs on `fmc_sampler_step`."""
        if self._plain and eta == 0.0 and not use_clipped_model_output:
            a_t, a_prev = self._alphas(int(timestep))
            return K.cfg_ddim_step(eps.contiguous(), latents, guidance_scale, a_t, a_prev, has_uncond)
        eps = eps.contiguous()
        c = self._coefs(int(timestep), float(eta), use_clipped_model_output)
        noise = None
        if eta > 0.0:
            noise = variance_noise.to(eps.dtype).contiguous() if variance_noise is not None else _draw_noise(latents, eps, generator)
        return K.sampler_step(eps, latents, guidance=guidance_scale, has_uncond=has_uncond, noise=noise, x_in=x_in, **c)

    def step_windows(self, eps: torch.Tensor, timestep: int, latents: torch.Tensor, guidance_scale: float, overlap: int,
                     eta: float = 0.0, generator=None, x_in=None, use_clipped_model_output: bool = False, variance_noise=None) -> torch.Tensor:
        """Sliding windows: eps `[R, W, B, C, F, ...]` (R = 2: uncond, cond), one prediction per window of F frames overlapping by
        `overlap`; latents fp32 `[B, C, Ftot, ...]`.  The blend and the step are one `fmc_window_step` launch (the plain
        configuration included); `x_in` `[R', W, B, C, F, ...]` receives every window's next model input."""
        c = self._coefs(int(timestep), float(eta), use_clipped_model_output)
        noise = None
        if eta > 0.0:
            noise = variance_noise.to(eps.dtype).contiguous() if variance_noise is not None else _draw_noise(latents, eps, generator)
        return K.window_step(eps, latents, overlap=overlap, guidance=guidance_scale, noise=noise, x_in=x_in, **c)

    def step(self, model_output, timestep, sample, eta: float = 0.0, use_clipped_model_output: bool = False, generator=None,
             variance_noise=None, **kwargs):
        x = sample.float().contiguous()
        out = self.step_cfg(model_output.to(torch.float32).contiguous(), int(timestep), x, 1.0, False, eta=eta, generator=generator,
                            use_clipped_model_output=use_clipped_model_output, variance_noise=variance_noise)
        return DDIMSchedulerOutput(out.to(sample.dtype))


class _SigmaScheduler:
    """What the sigma-table samplers share: betas, the step counter and its check, plumbing of `step`."""
    order = 1
    _default_spacing = "linspace"

    def _init_common(self, num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas, prediction_type, timestep_spacing,
                     steps_offset, **extra):
        self.betas = _make_betas(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas, self.__class__)
        if prediction_type not in ("epsilon", "sample", "v_prediction"):
            raise ValueError(f"prediction_type {prediction_type!r}: epsilon, sample or v_prediction")
        if timestep_spacing not in ("leading", "linspace", "trailing"):
            raise ValueError(f"timestep_spacing {timestep_spacing!r}: leading, linspace or trailing")
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self._train_sigmas = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()          # float32, as diffusers
        self.config = _Config(num_train_timesteps=num_train_timesteps, steps_offset=steps_offset, prediction_type=prediction_type,
                              beta_schedule=beta_schedule, timestep_spacing=timestep_spacing, **extra)
        self.num_inference_steps = None
        self._step_index = 0
        self._hist = []

    def _set_tables(self, ts: np.ndarray, sigmas: np.ndarray, device):
        """`ts`: the timesteps handed to the U-Net; `sigmas`: float32, one more entry than `ts`."""
        self.sigmas = torch.from_numpy(sigmas.astype(np.float32))
        self._sigmas_host = [float(s) for s in sigmas.astype(np.float32)]
        if all(float(t).is_integer() for t in ts):
            self._timesteps_host = [int(t) for t in ts]
            self.timesteps = torch.tensor(self._timesteps_host, dtype=torch.int64 if ts.dtype.kind == "i" else torch.float32, device=device)
        else:                                   # fractional timesteps (Euler, linspace spacing) reach the U-Net as they are
            self._timesteps_host = [float(t) for t in ts]
            self.timesteps = torch.tensor(self._timesteps_host, dtype=torch.float32, device=device)
        self._step_index = 0                    # a new trajectory: the counter and the multistep history start over
        self._hist = []

    def _index_for(self, timestep) -> int:
        i = self._step_index
        if self.num_inference_steps is None:
            raise RuntimeError("call set_timesteps before step")
        if i >= len(self._timesteps_host) or float(timestep) != float(self._timesteps_host[i]):
            raise ValueError(f"step {i} of {len(self._timesteps_host)}: got timestep {timestep!r}, the table holds "
                             f"{self._timesteps_host[i] if i < len(self._timesteps_host) else 'no more entries'} "
                             "(steps run in table order; set_timesteps starts a new trajectory)")
        return i

    def fused_input(self, eta: float = 0.0) -> bool:
        return True

    def _model_to_x0(self, sigma: float):
        """(m_x, m_e) of the x0 prediction `m = m_x x + m_e e` at noise level sigma, x the UNSCALED sample (x0 + sigma noise)."""
        kind = self.config.prediction_type
        if kind == "epsilon":
            return 1.0, -sigma
        if kind == "sample":
            return 0.0, 1.0
        return 1.0 / (sigma * sigma + 1.0), -sigma / math.sqrt(sigma * sigma + 1.0)

    def step(self, model_output, timestep, sample, generator=None, **kwargs):
        x = sample.float().contiguous()
        out = self.step_cfg(model_output.to(torch.float32).contiguous(), timestep, x, 1.0, False, generator=generator)
        return SchedulerOutput(out.to(sample.dtype))


class EulerDiscreteScheduler(_SigmaScheduler):
    """diffusers 0.24.0 `EulerDiscreteScheduler` with `s_churn = 0`, no Karras sigmas, linear sigma interpolation."""
    _stochastic = False

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 prediction_type="epsilon", interpolation_type="linear", use_karras_sigmas=False, timestep_spacing="linspace",
                 steps_offset=0, **_unused):
        if use_karras_sigmas or interpolation_type != "linear":
            raise NotImplementedError("use_karras_sigmas / log_linear interpolation are not built (linear sigma interpolation is)")
        self._init_common(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas, prediction_type, timestep_spacing,
                          steps_offset)
        ts = np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=np.float32)[::-1].copy()
        self.timesteps = torch.from_numpy(ts)
        self.sigmas = torch.from_numpy(np.concatenate([self._train_sigmas[::-1], [0.0]]).astype(np.float32))

    @property
    def init_noise_sigma(self):
        smax = float(self.sigmas.max())
        return smax if self.config.timestep_spacing in ("linspace", "trailing") else math.sqrt(smax * smax + 1.0)

    def set_timesteps(self, num_inference_steps: int, device=None):
        T, n = self.config.num_train_timesteps, num_inference_steps
        if n > T:
            raise ValueError("num_inference_steps cannot exceed num_train_timesteps")
        self.num_inference_steps = n
        spacing = self.config.timestep_spacing
        if spacing == "linspace":
            ts = np.linspace(0, T - 1, n, dtype=np.float32)[::-1].copy()
        elif spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float32) + self.config.steps_offset
        else:
            ts = (np.arange(T, 0, -T / n).round() - 1).astype(np.float32)
        sig = np.interp(ts, np.arange(0, T), self._train_sigmas)
        self._set_tables(ts, np.concatenate([sig, [0.0]]).astype(np.float32), device)

    def scale_model_input(self, sample, timestep=None):
        s = self._sigmas_host[self._step_index]
        return sample / math.sqrt(s * s + 1.0)

    def next_input_scale(self) -> float:
        """`scale_model_input` of the step AFTER the one about to run (1 after the last: sigma = 0)."""
        s = self._sigmas_host[min(self._step_index + 1, len(self._sigmas_host) - 1)]
        return 1.0 / math.sqrt(s * s + 1.0)

    def add_noise(self, original_samples, noise, timesteps):
        ts = [float(t) for t in (timesteps.reshape(-1).tolist() if torch.is_tensor(timesteps) else np.atleast_1d(timesteps))]
        table = [float(t) for t in self.timesteps.tolist()]
        sig = torch.tensor([float(self.sigmas[table.index(t)]) for t in ts], dtype=original_samples.dtype, device=original_samples.device)
        while sig.ndim < original_samples.ndim:
            sig = sig.unsqueeze(-1)
        return original_samples + noise * sig

    def _coefs(self, i: int):
        s, s_next = self._sigmas_host[i], self._sigmas_host[i + 1]
        c_n = 0.0
        if self._stochastic:
            up = math.sqrt(s_next * s_next * (s * s - s_next * s_next) / (s * s))
            c_n, s_next = up, math.sqrt(s_next * s_next - up * up)
        m_x, m_e = self._model_to_x0(s)
        r = (s_next - s) / s                     # x' = x + (x - m) / sigma * dt
        return dict(m_x=m_x, m_e=m_e, c_x=1.0 + r, c_m=-r, c_n=c_n)

    def step_cfg(self, eps, timestep, latents, guidance_scale, has_uncond, eta: float = 0.0, generator=None, x_in=None,
                 noise=None) -> torch.Tensor:
        """As `DDIMScheduler.step_cfg`; `latents` are the UNSCALED sample, `eps` the model's output on `scale_model_input(latents)`.
        `eta` is accepted and ignored, as the reference's `prepare_extra_step_kwargs` never passes it to this family."""
        i = self._index_for(timestep)
        eps = eps.contiguous()
        c = self._coefs(i)
        if self._stochastic:
            noise = noise.to(eps.dtype).contiguous() if noise is not None else _draw_noise(latents, eps, generator)
        else:
            noise = None
        scale = self.next_input_scale()
        out = K.sampler_step(eps, latents, guidance=guidance_scale, has_uncond=has_uncond, noise=noise, x_in=x_in, in_scale=scale, **c)
        self._step_index = i + 1
        return out

    def step_windows(self, eps, timestep, latents, guidance_scale, overlap, eta: float = 0.0, generator=None, x_in=None,
                     noise=None) -> torch.Tensor:
        """As `DDIMScheduler.step_windows`; the windows' predictions were made on `scale_model_input` of their frames."""
        i = self._index_for(timestep)
        c = self._coefs(i)
        if self._stochastic:
            noise = noise.to(eps.dtype).contiguous() if noise is not None else _draw_noise(latents, eps, generator)
        else:
            noise = None
        out = K.window_step(eps, latents, overlap=overlap, guidance=guidance_scale, noise=noise, x_in=x_in,
                            in_scale=self.next_input_scale(), **c)
        self._step_index = i + 1
        return out


class EulerAncestralDiscreteScheduler(EulerDiscreteScheduler):
    """diffusers 0.24.0 `EulerAncestralDiscreteScheduler`: the Euler step to `sigma_down`, plus `sigma_up` of fresh noise."""
    _stochastic = True


class DPMSolverMultistepScheduler(_SigmaScheduler):
    """diffusers 0.24.0 `DPMSolverMultistepScheduler`, `algorithm_type="dpmsolver++"`, `solver_type="midpoint"`, orders 1-3.  The
    converted model outputs (x0 predictions) of the last `solver_order` steps live in fp32 buffers of the latents' shape, written
    by the step kernel itself (`m_out`) over the oldest one."""

    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 solver_order=2, prediction_type="epsilon", thresholding=False, algorithm_type="dpmsolver++", solver_type="midpoint",
                 lower_order_final=True, euler_at_final=False, use_karras_sigmas=False, use_lu_lambdas=False,
                 lambda_min_clipped=-float("inf"), variance_type=None, timestep_spacing="linspace", steps_offset=0, **_unused):
        if algorithm_type != "dpmsolver++" or solver_type != "midpoint":
            raise NotImplementedError(f"algorithm_type {algorithm_type!r} / solver_type {solver_type!r}: dpmsolver++ with midpoint is built")
        if thresholding or use_karras_sigmas or use_lu_lambdas or variance_type in ("learned", "learned_range"):
            raise NotImplementedError("thresholding, Karras sigmas, Lu lambdas and learned variances are not built")
        if solver_order not in (1, 2, 3):
            raise ValueError(f"solver_order {solver_order}: 1, 2 or 3")
        self._init_common(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas, prediction_type, timestep_spacing,
                          steps_offset, solver_order=solver_order, lower_order_final=lower_order_final, euler_at_final=euler_at_final,
                          lambda_min_clipped=lambda_min_clipped, algorithm_type=algorithm_type, solver_type=solver_type)
        self.alpha_t = torch.sqrt(self.alphas_cumprod)
        self.sigma_t = torch.sqrt(1 - self.alphas_cumprod)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self.timesteps = torch.from_numpy(np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=np.float32)[::-1].copy())
        self.sigmas = torch.from_numpy(self._train_sigmas.copy())
        self._lower_order_nums = 0

    def set_timesteps(self, num_inference_steps: int, device=None):
        T, n = self.config.num_train_timesteps, num_inference_steps
        if n > T:
            raise ValueError("num_inference_steps cannot exceed num_train_timesteps")
        clipped = int(torch.searchsorted(torch.flip(self.lambda_t, [0]), torch.tensor(float(self.config.lambda_min_clipped))))
        last = T - clipped
        spacing = self.config.timestep_spacing
        if spacing == "linspace":
            ts = np.linspace(0, last - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif spacing == "leading":
            ts = (np.arange(0, n + 1) * (last // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + self.config.steps_offset
        else:
            ts = (np.arange(last, 0, -T / n).round() - 1).astype(np.int64)
        self.num_inference_steps = len(ts)
        sig = np.interp(ts, np.arange(0, T), self._train_sigmas)
        ac0 = float(self.alphas_cumprod[0])
        self._set_tables(ts, np.concatenate([sig, [((1 - ac0) / ac0) ** 0.5]]).astype(np.float32), device)
        self._lower_order_nums = 0

    def scale_model_input(self, sample, timestep=None):
        return sample

    def next_input_scale(self) -> float:
        return 1.0

    def add_noise(self, original_samples, noise, timesteps):
        a, s = _add_noise_ac(self, original_samples, noise, timesteps)
        return a * original_samples + s * noise

    @staticmethod
    def _alpha_sigma_lambda(sigma: float):
        alpha = 1.0 / math.sqrt(sigma * sigma + 1.0)
        sig = sigma * alpha
        return alpha, sig, math.log(alpha) - math.log(sig)

    def _order_at(self, i: int) -> int:
        n, cfg = len(self._timesteps_host), self.config
        final = i == n - 1 and (cfg.euler_at_final or (cfg.lower_order_final and n < 15))
        second = i == n - 2 and cfg.lower_order_final and n < 15
        if cfg.solver_order == 1 or self._lower_order_nums < 1 or final:
            return 1
        if cfg.solver_order == 2 or self._lower_order_nums < 2 or second:
            return 2
        return 3

    def _coefs(self, i: int, order: int):
        """x0 conversion at sigma_i, then the update to sigma_{i+1}; `c_h` weigh the x0 predictions of steps i-1, i-2."""
        sg = self._sigmas_host
        a_s0, s_s0, l_s0 = self._alpha_sigma_lambda(sg[i])
        a_t, s_t, l_t = self._alpha_sigma_lambda(sg[i + 1])
        kind = self.config.prediction_type
        if kind == "epsilon":
            m_x, m_e = 1.0 / a_s0, -s_s0 / a_s0
        elif kind == "sample":
            m_x, m_e = 0.0, 1.0
        else:
            m_x, m_e = a_s0, -s_s0
        h = l_t - l_s0
        E = math.expm1(-h)
        c_m, c_h = -a_t * E, []
        if order >= 2:
            l_s1 = self._alpha_sigma_lambda(sg[i - 1])[2]
            r0 = (l_s0 - l_s1) / h
        if order == 2:
            c_m += -0.5 * a_t * E / r0
            c_h = [0.5 * a_t * E / r0]
        elif order == 3:
            l_s2 = self._alpha_sigma_lambda(sg[i - 2])[2]
            r1 = (l_s1 - l_s2) / h
            k1 = a_t * (E / h + 1.0)
            k2 = -a_t * ((E + h) / (h * h) - 0.5)
            q, s = r0 / (r0 + r1), 1.0 / (r0 + r1)
            P = k1 * (1.0 + q) + k2 * s              # weight of D1_0 = (m0 - m1) / r0
            Q = -k1 * q - k2 * s                     # weight of D1_1 = (m1 - m2) / r1
            c_m += P / r0
            c_h = [-P / r0 + Q / r1, -Q / r1]
        return dict(m_x=m_x, m_e=m_e, c_x=s_t / s_s0, c_m=c_m, c_h=c_h)

    def step_cfg(self, eps, timestep, latents, guidance_scale, has_uncond, eta: float = 0.0, generator=None, x_in=None) -> torch.Tensor:
        """As `DDIMScheduler.step_cfg`.  `eta` and `generator` are accepted and ignored (a deterministic solver)."""
        return self._multistep(eps.contiguous(), timestep, latents, x_in,
                               lambda e, **kw: K.sampler_step(e, latents, guidance=guidance_scale, has_uncond=has_uncond, **kw))

    def step_windows(self, eps, timestep, latents, guidance_scale, overlap, eta: float = 0.0, generator=None, x_in=None) -> torch.Tensor:
        """As `DDIMScheduler.step_windows`; the history holds x0 predictions of the full latents' shape."""
        return self._multistep(eps, timestep, latents, x_in,
                               lambda e, **kw: K.window_step(e, latents, overlap=overlap, guidance=guidance_scale, **kw))

    def _multistep(self, eps, timestep, latents, x_in, launch) -> torch.Tensor:
        i = self._index_for(timestep)
        order_max = self.config.solver_order
        if i == 0 or len(self._hist) != order_max or self._hist[0].shape != latents.shape or self._hist[0].device != latents.device:
            self._hist = [torch.empty_like(latents) for _ in range(order_max)]       # (first step after set_timesteps)
        order = self._order_at(i)
        c = self._coefs(i, order)
        hist = [self._hist[(i - 1 - j) % order_max] for j in range(order - 1)]
        m_out = self._hist[i % order_max] if order_max > 1 else None           # over the oldest slot; order 1 keeps no history
        out = launch(eps, hist=hist, m_out=m_out, x_in=x_in, **c)
        if self._lower_order_nums < order_max:
            self._lower_order_nums += 1
        self._step_index = i + 1
        return out


_FAMILIES = "DDIMScheduler, EulerDiscreteScheduler, EulerAncestralDiscreteScheduler and DPMSolverMultistepScheduler (dpmsolver++, midpoint)"


def coerce_scheduler(scheduler):
    """The reference's trainers hand the pipelines a `diffusers` scheduler object (train_cam_obj_ctrl.py:231, :497); the loops here
    call `step_cfg` (the fused CFG + update kernels).  A foreign scheduler is therefore re-expressed as this module's class of the
    same family from its class name and `.config` (same betas, offset, spacing, prediction type); anything this path does not
    implement raises here rather than producing other numbers."""
    if scheduler is None or hasattr(scheduler, "step_cfg"):
        return scheduler
    cfg = getattr(scheduler, "config", None)
    if cfg is None:
        raise TypeError(f"cannot use {type(scheduler).__name__} as the scheduler of the FMC pipelines")
    get = (lambda k, d=None: cfg.get(k, d)) if hasattr(cfg, "get") else (lambda k, d=None: getattr(cfg, k, d))
    name = type(scheduler).__name__
    common = dict(num_train_timesteps=get("num_train_timesteps", 1000), beta_start=get("beta_start", 0.0001),
                  beta_end=get("beta_end", 0.02), beta_schedule=get("beta_schedule", "linear"), trained_betas=get("trained_betas"),
                  steps_offset=get("steps_offset", 0), prediction_type=get("prediction_type", "epsilon"))
    if get("thresholding", False) or get("use_karras_sigmas", False):
        raise NotImplementedError(f"{name}: thresholding / use_karras_sigmas are not built; supported: {_FAMILIES}")
    if "DDIM" in name:
        return DDIMScheduler(clip_sample=get("clip_sample", True), set_alpha_to_one=get("set_alpha_to_one", True),
                             timestep_spacing=get("timestep_spacing", "leading"), clip_sample_range=get("clip_sample_range", 1.0), **common)
    if "EulerAncestral" in name:
        return EulerAncestralDiscreteScheduler(timestep_spacing=get("timestep_spacing", "linspace"), **common)
    if "EulerDiscrete" in name:
        return EulerDiscreteScheduler(timestep_spacing=get("timestep_spacing", "linspace"),
                                      interpolation_type=get("interpolation_type", "linear"), **common)
    if "DPMSolverMultistep" in name and "Inverse" not in name:
        if get("algorithm_type", "dpmsolver++") != "dpmsolver++":
            raise NotImplementedError(f"{name}: algorithm_type {get('algorithm_type')!r} is not built; supported: {_FAMILIES}")
        return DPMSolverMultistepScheduler(solver_order=get("solver_order", 2), algorithm_type="dpmsolver++",
                                           solver_type=get("solver_type", "midpoint"), lower_order_final=get("lower_order_final", True),
                                           euler_at_final=get("euler_at_final", False), use_lu_lambdas=get("use_lu_lambdas", False),
                                           lambda_min_clipped=get("lambda_min_clipped", -float("inf")), variance_type=get("variance_type"),
                                           timestep_spacing=get("timestep_spacing", "linspace"), **common)
    raise NotImplementedError(f"{name} is not built (PNDM and LMS among them); supported: {_FAMILIES}")

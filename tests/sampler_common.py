"""Shared by test_sampler_host.py (CPU) and test_gpu_sampler.py: a float64 closed form of `fmc_sampler_step` with the magnitude
behind every output, float64 restatements of the four samplers written from the formulas of diffusers 0.24.0 (in the library's own
form -- x0 prediction, derivative, dt, lambda -- not the coefficient form of synfmc_amd/schedulers.py), and the bound.

The bound.  The kernel (csrc/sampler_step.hip) computes, in fp32, with at most one rounding per operation (hipcc may contract a
multiply and an add into one fma, which only removes roundings):

    e   = eu + g * (ec - eu)                         3 roundings: the subtraction, the product, the sum
    m   = m_x * x + m_e * e                          +2 on the chain through e: the product m_e * e, the sum       -> R_M  = 5
    acc = c_x * x + c_e * e ; acc += c_m * m         +2 on the chain through m: the product c_m * m, the add
    acc += c_h[j] * hist[j]  (j < 3) ; acc += c_n * noise          +4 adds                                        -> R_X  = 11
    x_in = in_scale * acc                            +1                                                            -> R_IN = 12

The clamp is exact and 1-Lipschitz, so m carries its unclamped magnitude on.  Every rounding is relative 2^-24 on a partial sum that the
sum of |terms| bounds, so |fp32 - exact| <= R * 2^-24 * sum|terms| along the longest chain R of each output; a bf16 `x_in` adds its
own rounding, 2^-8 |in_scale x'| (the issue's figure; half an ulp is 2^-9).  Inputs are exact: bf16 and fp32 values are fp32 values,
and the closed form takes the coefficients as the fp32 numbers the kernel receives.  `R = 12`, the longest chain, is the figure the
profile quotes.
"""
import math

import numpy as np
import torch

R_M, R_X, R_IN = 5, 11, 12
R = R_IN
U32 = 2.0 ** -24
BF16_REL = 2.0 ** -8

COEF_KEYS = ("m_x", "m_e", "m_clamp", "c_x", "c_e", "c_m", "c_n", "in_scale")


def f32(v):
    """The fp32 value a coefficient has inside the kernel, as a Python float."""
    return float(np.float32(v))


def closed_form(eps, x, *, guidance=1.0, has_uncond=False, m_x=0.0, m_e=0.0, m_clamp=0.0, c_x=1.0, c_e=0.0, c_m=0.0, c_n=0.0,
                c_h=(), hist=(), noise=None, in_scale=1.0):
    """float64, element-wise, on flat tensors; coefficients rounded to fp32 first.  Returns {name: (value, sum|terms|)} for
    x_out, m_out, x_in (one copy)."""
    d = lambda t: t.detach().double().cpu().reshape(-1)
    g, m_x, m_e, m_clamp, c_x, c_e, c_m, c_n, in_scale = (f32(v) for v in (guidance, m_x, m_e, m_clamp, c_x, c_e, c_m, c_n, in_scale))
    c_h = [f32(c) for c in c_h]
    x, e_all = d(x), d(eps)
    n = x.numel()
    if has_uncond:
        eu, ec = e_all[:n], e_all[n:]
        e = eu + g * ec - g * eu
        s_e = eu.abs() + abs(g) * ec.abs() + abs(g) * eu.abs()
    else:
        e, s_e = e_all, e_all.abs()
    m = m_x * x + m_e * e
    s_m = (m_x * x).abs() + abs(m_e) * s_e
    if m_clamp > 0:
        m = m.clamp(-m_clamp, m_clamp)
    xn = c_x * x + c_e * e + c_m * m
    s_x = (c_x * x).abs() + abs(c_e) * s_e + abs(c_m) * s_m
    for c, h in zip(c_h, hist):
        xn = xn + c * d(h)
        s_x = s_x + (c * d(h)).abs()
    if noise is not None:
        xn = xn + c_n * d(noise)
        s_x = s_x + (c_n * d(noise)).abs()
    return {"x_out": (xn, s_x), "m_out": (m, s_m), "x_in": (in_scale * xn, abs(in_scale) * s_x)}


def bound(name, value, mag, dtype=torch.float32):
    r = {"x_out": R_X, "m_out": R_M, "x_in": R_IN}[name]
    b = r * U32 * mag
    if dtype == torch.bfloat16:
        b = b + BF16_REL * value.abs()
    return b


def worst_ratio(got, name, value, mag, dtype=torch.float32):
    """max over elements of |got - value| / bound (a tiny floor keeps 0 / 0 out: exact zeros must come out as exact zeros)."""
    err = (got.detach().double().cpu().reshape(-1) - value).abs()
    b = bound(name, value, mag, dtype)
    return float((err / b.clamp_min(1e-300)).max()) if err.numel() else 0.0


def fp32_emulation(eps, x, *, guidance=1.0, has_uncond=False, m_x=0.0, m_e=0.0, m_clamp=0.0, c_x=1.0, c_e=0.0, c_m=0.0, c_n=0.0,
                   c_h=(), hist=(), noise=None, in_scale=1.0, in_dtype=torch.float32):
    """The kernel's chain in torch fp32 ops, one rounding per operation, in the kernel's order."""
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    x = x.float().reshape(-1)
    e_all = eps.float().reshape(-1)
    n = x.numel()
    e = e_all[:n] + t(guidance) * (e_all[n:] - e_all[:n]) if has_uncond else e_all
    m = t(m_x) * x + t(m_e) * e
    if m_clamp > 0:
        m = torch.minimum(torch.maximum(m, t(-m_clamp)), t(m_clamp))
    acc = t(c_x) * x + t(c_e) * e
    acc = acc + t(c_m) * m
    for c, h in zip(c_h, hist):
        acc = acc + t(c) * h.float().reshape(-1)
    if noise is not None:
        acc = acc + t(c_n) * noise.float().reshape(-1)
    return {"x_out": acc, "m_out": m, "x_in": (t(in_scale) * acc).to(in_dtype)}


def standin_sampler_step(eps, x, *, guidance=1.0, has_uncond=False, m_x=0.0, m_e=0.0, m_clamp=0.0, c_x=1.0, c_e=0.0, c_m=0.0, c_n=0.0,
                         c_h=(), hist=(), noise=None, x_out=None, m_out=None, x_in=None, in_scale=1.0):
    """`hip_ops.sampler_step` in plain torch, float64 arithmetic with the coefficients as given (NOT rounded to fp32: the host
    identities are about the scheduler's float64 numbers).  Honours x_out / m_out / x_in like the kernel: every input is read
    before any output is written."""
    n = x.numel()
    xd, ed = x.double().reshape(-1), eps.double().reshape(-1)
    e = ed[:n] + guidance * (ed[n:] - ed[:n]) if has_uncond else ed
    m = m_x * xd + m_e * e
    if m_clamp > 0:
        m = m.clamp(-m_clamp, m_clamp)
    xn = c_x * xd + c_e * e + c_m * m
    for c, h in zip(c_h, hist):
        xn = xn + c * h.double().reshape(-1)
    if noise is not None:
        xn = xn + c_n * noise.double().reshape(-1)
    if x_out is None:
        x_out = torch.empty_like(x)
    x_out.copy_(xn.reshape(x.shape).to(x_out.dtype))
    if m_out is not None:
        m_out.copy_(m.reshape(m_out.shape).to(m_out.dtype))
    if x_in is not None:
        reps = x_in.numel() // n
        x_in.copy_((in_scale * xn).repeat(reps).reshape(x_in.shape).to(x_in.dtype))
    return x_out


def standin_cfg_ddim_step(eps, x, guidance, alpha_t, alpha_prev, has_uncond):
    e = eps.double()
    if has_uncond:
        eu, ec = e.chunk(2)
        e = eu + guidance * (ec - eu)
    x0 = (x.double() - (1 - alpha_t) ** 0.5 * e) / alpha_t ** 0.5
    return (alpha_prev ** 0.5 * x0 + (1 - alpha_prev) ** 0.5 * e).to(x.dtype)


# ---- the tables, restated (diffusers 0.24.0 as read) ------------------------------------------------------------------------------
def alphas_cumprod(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012, T=1000):
    """float64 view of the float32 table the library keeps."""
    if beta_schedule == "linear":
        betas = torch.linspace(beta_start, beta_end, T, dtype=torch.float32)
    else:
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, 0).double().numpy()


def _sigma_table(ac):
    return np.sqrt((1 - ac.astype(np.float32)) / ac.astype(np.float32)).astype(np.float32)


def interp_ac(ac, t):
    return float(np.interp(float(t), np.arange(len(ac)), ac))


class _Out:
    def __init__(self, prev_sample, pred_original_sample=None):
        self.prev_sample, self.pred_original_sample = prev_sample, pred_original_sample


class RefDDIM:
    """DDIMScheduler.step as the library writes it: x0, optional clip, variance, the direction pointing to x_t, noise."""

    def __init__(self, ac, spacing="leading", steps_offset=0, prediction_type="epsilon", clip_sample=False, clip_sample_range=1.0,
                 eta=0.0, use_clipped_model_output=False, set_alpha_to_one=True):
        self.ac, self.T = ac, len(ac)
        self.spacing, self.offset, self.kind = spacing, steps_offset, prediction_type
        self.clip, self.clip_range, self.eta, self.use_clipped = clip_sample, clip_sample_range, eta, use_clipped_model_output
        self.final_ac = 1.0 if set_alpha_to_one else float(ac[0])
        self.init_noise_sigma = 1.0
        self.noises = None                     # list of noise tensors, one per step, when eta > 0

    def set_timesteps(self, n):
        T = self.T
        self.n, self.i = n, 0
        if self.spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].astype(np.int64) + self.offset
        elif self.spacing == "linspace":
            ts = np.linspace(0, T - 1, n).round()[::-1].astype(np.int64)
        else:
            ts = np.round(np.arange(T, 0, -T / n)).astype(np.int64) - 1
        self.timesteps = torch.tensor(ts.tolist(), dtype=torch.int64)

    def pairs(self):
        out = []
        for t in self.timesteps.tolist():
            p = t - self.T // self.n
            out.append((float(self.ac[t]), float(self.ac[p]) if p >= 0 else self.final_ac))
        return out

    def scale_model_input(self, x, t=None):
        return x

    def step(self, e, t, x, noise=None):
        a_t, a_p = self.pairs()[self.i]
        b_t = 1 - a_t
        if self.kind == "epsilon":
            x0, pe = (x - b_t ** 0.5 * e) / a_t ** 0.5, e
        elif self.kind == "sample":
            x0, pe = e, (x - a_t ** 0.5 * e) / b_t ** 0.5
        else:
            x0, pe = a_t ** 0.5 * x - b_t ** 0.5 * e, a_t ** 0.5 * e + b_t ** 0.5 * x
        if self.clip:
            x0 = x0.clamp(-self.clip_range, self.clip_range)
        var = (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
        std = self.eta * var ** 0.5
        if self.use_clipped:
            pe = (x - a_t ** 0.5 * x0) / b_t ** 0.5
        prev = a_p ** 0.5 * x0 + (1 - a_p - std ** 2) ** 0.5 * pe
        if self.eta > 0:
            noise = self.noises[self.i] if noise is None else noise
            prev = prev + std * noise.to(prev.dtype)
        self.i += 1
        return _Out(prev, x0)


class RefEuler:
    """EulerDiscreteScheduler / EulerAncestralDiscreteScheduler (s_churn = 0)."""

    def __init__(self, ac, spacing="linspace", steps_offset=0, prediction_type="epsilon", ancestral=False):
        self.ac, self.T = ac, len(ac)
        self.spacing, self.offset, self.kind, self.ancestral = spacing, steps_offset, prediction_type, ancestral
        self.train_sigmas = _sigma_table(ac)
        self.sigmas = np.concatenate([self.train_sigmas[::-1], [0.0]]).astype(np.float32)
        self.noises = None

    @property
    def init_noise_sigma(self):
        smax = float(self.sigmas.max())
        return smax if self.spacing in ("linspace", "trailing") else (smax ** 2 + 1) ** 0.5

    def set_timesteps(self, n):
        T = self.T
        self.n, self.i = n, 0
        if self.spacing == "linspace":
            ts = np.linspace(0, T - 1, n, dtype=np.float32)[::-1].copy()
        elif self.spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float32) + self.offset
        else:
            ts = (np.arange(T, 0, -T / n).round() - 1).astype(np.float32)
        sig = np.interp(ts, np.arange(0, T), self.train_sigmas)
        self.sigmas = np.concatenate([sig, [0.0]]).astype(np.float32)
        self.timesteps = torch.tensor([float(t) for t in ts], dtype=torch.float32)

    def scale_model_input(self, x, t=None):
        s = float(self.sigmas[self.i])
        return x / (s ** 2 + 1) ** 0.5

    def step(self, e, t, x, noise=None):
        s, s_to = float(self.sigmas[self.i]), float(self.sigmas[self.i + 1])
        if self.kind == "epsilon":
            x0 = x - s * e
        elif self.kind == "sample":
            x0 = e
        else:
            x0 = e * (-s / (s ** 2 + 1) ** 0.5) + x / (s ** 2 + 1)
        deriv = (x - x0) / s
        if self.ancestral:
            up = (s_to ** 2 * (s ** 2 - s_to ** 2) / s ** 2) ** 0.5
            down = (s_to ** 2 - up ** 2) ** 0.5
            prev = x + deriv * (down - s)
            noise = self.noises[self.i] if noise is None else noise
            prev = prev + noise.to(prev.dtype) * up
        else:
            prev = x + deriv * (s_to - s)
        self.i += 1
        return _Out(prev, x0)


class RefDPM:
    """DPMSolverMultistepScheduler, dpmsolver++ / midpoint, orders 1-3."""
    init_noise_sigma = 1.0

    def __init__(self, ac, solver_order=2, spacing="linspace", steps_offset=0, prediction_type="epsilon", lower_order_final=True,
                 euler_at_final=False, lambda_min_clipped=-float("inf")):
        self.ac, self.T = ac, len(ac)
        self.order, self.spacing, self.offset, self.kind = solver_order, spacing, steps_offset, prediction_type
        self.lof, self.eaf, self.lmc = lower_order_final, euler_at_final, lambda_min_clipped
        self.train_sigmas = _sigma_table(ac)

    def set_timesteps(self, n):
        T = self.T
        acf = torch.tensor(self.ac, dtype=torch.float32)
        lam = torch.log(acf.sqrt()) - torch.log((1 - acf).sqrt())
        last = T - int(torch.searchsorted(torch.flip(lam, [0]), torch.tensor(float(self.lmc))))
        if self.spacing == "linspace":
            ts = np.linspace(0, last - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif self.spacing == "leading":
            ts = (np.arange(0, n + 1) * (last // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + self.offset
        else:
            ts = (np.arange(last, 0, -T / n).round() - 1).astype(np.int64)
        sig = np.interp(ts, np.arange(0, T), self.train_sigmas)
        self.sigmas = np.concatenate([sig, [((1 - self.ac[0]) / self.ac[0]) ** 0.5]]).astype(np.float32)
        self.timesteps = torch.tensor(ts.tolist(), dtype=torch.int64)
        self.n, self.i, self.outs, self.lower = len(ts), 0, [], 0

    def scale_model_input(self, x, t=None):
        return x

    @staticmethod
    def _asl(sigma):
        a = 1 / (sigma ** 2 + 1) ** 0.5
        return a, sigma * a, math.log(a) - math.log(sigma * a)

    def pairs(self):
        """(alphas_cumprod at the step's sigma, at the next sigma): alpha^2 of the scheduler's own table."""
        return [(self._asl(float(s))[0] ** 2, self._asl(float(sn))[0] ** 2) for s, sn in zip(self.sigmas[:-1], self.sigmas[1:])]

    def step(self, e, t, x, noise=None):
        i, sg = self.i, [float(s) for s in self.sigmas]
        a_s, s_s, l_s = self._asl(sg[i])
        if self.kind == "epsilon":
            x0 = (x - s_s * e) / a_s
        elif self.kind == "sample":
            x0 = e
        else:
            x0 = a_s * x - s_s * e
        self.outs = ([x0] + self.outs)[:self.order]
        final = i == self.n - 1 and (self.eaf or (self.lof and self.n < 15))
        second = i == self.n - 2 and self.lof and self.n < 15
        a_t, s_t, l_t = self._asl(sg[i + 1])
        h = l_t - l_s
        if self.order == 1 or self.lower < 1 or final:
            prev = (s_t / s_s) * x - a_t * (math.exp(-h) - 1.0) * x0
        elif self.order == 2 or self.lower < 2 or second:
            m0, m1 = self.outs[0], self.outs[1]
            r0 = (l_s - self._asl(sg[i - 1])[2]) / h
            d1 = (1.0 / r0) * (m0 - m1)
            prev = (s_t / s_s) * x - a_t * (math.exp(-h) - 1.0) * m0 - 0.5 * a_t * (math.exp(-h) - 1.0) * d1
        else:
            m0, m1, m2 = self.outs
            l1, l2 = self._asl(sg[i - 1])[2], self._asl(sg[i - 2])[2]
            r0, r1 = (l_s - l1) / h, (l1 - l2) / h
            d1_0, d1_1 = (1.0 / r0) * (m0 - m1), (1.0 / r1) * (m1 - m2)
            d1 = d1_0 + (r0 / (r0 + r1)) * (d1_0 - d1_1)
            d2 = (1.0 / (r0 + r1)) * (d1_0 - d1_1)
            prev = ((s_t / s_s) * x - a_t * (math.exp(-h) - 1.0) * m0 + a_t * ((math.exp(-h) - 1.0) / h + 1.0) * d1
                    - a_t * ((math.exp(-h) - 1.0 + h) / h ** 2 - 0.5) * d2)
        if self.lower < self.order:
            self.lower += 1
        self.i += 1
        return _Out(prev, x0)


def run_reference(ref, n_steps, x, model, guidance=1.0, dtype=torch.float64):
    """The loop of the pipelines on a restated scheduler: `model(x_in, t) -> eps` on the (CFG-duplicated) scaled input.  Returns the
    latents after every step."""
    ref.set_timesteps(n_steps)
    x = x.to(dtype)
    out = []
    cfg = guidance > 1.0
    for t in ref.timesteps.tolist():
        xi = ref.scale_model_input(torch.cat([x] * 2) if cfg else x, t)
        e = model(xi, t)
        if cfg:
            eu, ec = e.chunk(2)
            e = eu + guidance * (ec - eu)
        x = ref.step(e, t, x).prev_sample
        out.append(x)
    return out


def run_product(sch, n_steps, x, model, guidance=1.0, eta=0.0, noises=None, in_dtype=None):
    """The same loop on a scheduler of synfmc_amd.schedulers through `step_cfg`, feeding the model the `x_in` the step emitted."""
    sch.set_timesteps(n_steps)
    cfg = guidance > 1.0
    first = sch.scale_model_input(x, sch._timesteps_host[0])
    x_in = (torch.cat([first] * 2) if cfg else first).to(in_dtype or x.dtype).clone()
    out = []
    for k, t in enumerate(sch._timesteps_host):
        e = model(x_in, t).to(x_in.dtype)
        kw = {}
        if noises is not None:
            kw = {"variance_noise": noises[k]} if type(sch).__name__ == "DDIMScheduler" else {"noise": noises[k]}
        if sch.fused_input(eta):
            x = sch.step_cfg(e, t, x, guidance, cfg, eta=eta, x_in=x_in, **kw)
        else:
            x = sch.step_cfg(e, t, x, guidance, cfg)
            x_in = (torch.cat([x] * 2) if cfg else x).to(x_in.dtype)
        out.append(x)
    return out

"""CPU checks of the samplers: the bound of tests/sampler_common.py against an fp32 emulation of the kernel's chain and against wrong
kernels, float64 identities between the samplers, the order of DPM-Solver++, the tables, the plumbing through both pipelines and the
training target.  `hip_ops.sampler_step` / `cfg_ddim_step` are replaced by the float64 stand-ins of sampler_common.py.

The identities hold at 1e-10 on the noise levels the sampler itself works with: the sigma tables are rounded to float32 as the
library rounds them, so the DDIM side of a comparison is the DDIM closed form on the sampler's own (ac_t, ac_next) = 1 / (sigma^2 + 1)
pairs, and the point-mass denoiser sits at the sampler's own ac_t.  Against `DDIMScheduler`'s own float32 alphas_cumprod table the
same comparison is held to 1e-5: each table entry carries a relative 2^-24, and a trajectory from t = 999 scales the latents by
1 / sqrt(ac_999) ~ 15.
"""
import types

import numpy as np
import pytest
import torch

from tests import sampler_common as SC

BETAS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


@pytest.fixture
def K(monkeypatch):
    import synfmc_amd.hip_ops as K
    calls = {"sampler_step": [], "cfg_ddim_step": []}

    def sampler_step(eps, x, **kw):
        calls["sampler_step"].append(kw)
        return SC.standin_sampler_step(eps, x, **kw)

    def cfg_ddim_step(*a):
        calls["cfg_ddim_step"].append(a)
        return SC.standin_cfg_ddim_step(*a)

    monkeypatch.setattr(K, "sampler_step", sampler_step)
    monkeypatch.setattr(K, "cfg_ddim_step", cfg_ddim_step)
    K._sampler_calls = calls
    yield K
    del K._sampler_calls


# ---- 1. the bound ----------------------------------------------------------------------------------------------------------------
def _case(n=4099, seed=0, has_uncond=True, n_hist=3, clamp=0.8, noise=True, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    eps = r((2 if has_uncond else 1) * n).to(dtype)
    kw = dict(guidance=7.5, has_uncond=has_uncond, m_x=1.31, m_e=-0.77, m_clamp=clamp, c_x=0.93, c_e=0.21, c_m=-0.35, c_n=0.4,
              c_h=[0.6, -0.45, 0.3][:n_hist], hist=[r(n) for _ in range(n_hist)], noise=r(n).to(dtype) if noise else None, in_scale=0.37)
    return eps, r(n), kw


def _ratios(outs, eps, x, kw, in_dtype=torch.float32):
    ref = SC.closed_form(eps, x, **kw)
    return {k: SC.worst_ratio(outs[k], k, *ref[k], dtype=in_dtype if k == "x_in" else torch.float32) for k in ("x_out", "m_out", "x_in")}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("has_uncond,n_hist,clamp,noise", [(True, 3, 0.8, True), (False, 0, 0.0, False), (True, 2, 0.0, True), (False, 1, 2.5, False)])
def test_fp32_emulation_meets_the_bound(dtype, has_uncond, n_hist, clamp, noise):
    eps, x, kw = _case(has_uncond=has_uncond, n_hist=n_hist, clamp=clamp, noise=noise, dtype=dtype)
    rat = _ratios(SC.fp32_emulation(eps, x, in_dtype=dtype, **kw), eps, x, kw, dtype)
    print(f"fp32 emulation, {dtype}: share of the bound used {rat}")
    assert max(rat.values()) <= 1.0


def _wrong(name, eps, x, kw):
    """The emulation with one defect of a plausible wrong kernel."""
    n = x.numel()
    k = dict(kw)
    if name == "swapped halves":
        eps = torch.cat([eps[n:], eps[:n]])
    elif name == "guidance on the wrong half":              # e = g eu + (ec - eu)
        return SC.fp32_emulation(k["guidance"] * eps[:n] + (eps[n:] - eps[:n]), x, **dict(k, has_uncond=False))
    elif name == "one history slot dropped":
        k["c_h"], k["hist"] = k["c_h"][:-1], k["hist"][:-1]
    elif name == "history order reversed":
        k["hist"] = k["hist"][::-1]
    elif name == "noise ignored":
        k["noise"] = None
    elif name == "clamp skipped":
        k["m_clamp"] = 0.0
    out = SC.fp32_emulation(eps, x, **k)
    if name == "clamp applied to x'":
        out = SC.fp32_emulation(eps, x, **dict(kw, m_clamp=0.0))
        out["x_out"] = out["x_out"].clamp(-kw["m_clamp"], kw["m_clamp"])
        out["m_out"] = SC.fp32_emulation(eps, x, **kw)["m_out"]
    elif name == "x_in unscaled":
        out["x_in"] = out["x_out"].clone()
    elif name == "last n % 8 elements dropped":
        for v in out.values():
            v[n - n % 8:] = 0.0
    return out


WRONG = ["swapped halves", "guidance on the wrong half", "one history slot dropped", "history order reversed", "noise ignored", "clamp skipped",
         "clamp applied to x'", "x_in unscaled", "last n % 8 elements dropped"]


@pytest.mark.parametrize("name", WRONG)
def test_wrong_kernels_fail_the_bound(name):
    eps, x, kw = _case()
    assert x.numel() % 8 == 3
    rat = _ratios(_wrong(name, eps, x, kw), eps, x, kw)
    print(f"{name}: worst error / bound {rat}")
    assert max(rat.values()) > 1.0


def test_missing_second_x_in_copy_and_early_m_out_fail():
    """The two defects that need the buffers: the second CFG copy of x_in left unwritten, and m_out stored to an aliased history slot
    before that slot was read."""
    eps, x, kw = _case()
    n = x.numel()
    ref = SC.closed_form(eps, x, **kw)
    good = SC.fp32_emulation(eps, x, **kw)
    x_in = torch.full((2, n), float("nan"))
    x_in[0] = good["x_in"]                                  # (the defect: row 1 never written)
    ratios = [SC.worst_ratio(torch.nan_to_num(x_in[r], nan=0.0), "x_in", *ref["x_in"]) for r in range(2)]
    assert ratios[0] <= 1.0 < ratios[1]
    early = dict(kw, hist=[h.clone() for h in kw["hist"]])
    early["hist"][1] = good["m_out"].clone()                # (the defect: slot 1 already holds m when the sum reads it)
    assert SC.worst_ratio(SC.fp32_emulation(eps, x, **early)["x_out"], "x_out", *ref["x_out"]) > 1.0
    # ... and the stand-in used below reads before it writes
    hist = [h.clone() for h in kw["hist"]]
    out = SC.standin_sampler_step(eps, x, **dict(kw, hist=hist, m_out=hist[1]))
    assert SC.worst_ratio(out, "x_out", *ref["x_out"]) <= 1.0 and SC.worst_ratio(hist[1], "m_out", *ref["m_out"]) <= 1.0


# ---- 2. identities (float64) -----------------------------------------------------------------------------------------------------
def _tanh_model(x_in, t):
    return torch.tanh(0.7 * x_in + 0.3 * np.sin(float(t) / 100.0))


def _ddim_closed(x, e, a_t, a_p, eta=0.0, noise=None):
    x0 = (x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5
    std = eta * ((1 - a_p) / (1 - a_t) * (1 - a_t / a_p)) ** 0.5
    out = a_p ** 0.5 * x0 + (1 - a_p - std * std) ** 0.5 * e
    return out if noise is None else out + std * noise


def _own_pairs(sch):
    ac = [1.0 / (s * s + 1.0) for s in sch._sigmas_host]
    return list(zip(ac[:-1], ac[1:]))


def _relmax(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("ancestral", [False, True])
def test_euler_is_ddim_in_sigma_space(K, ancestral):
    from synfmc_amd.schedulers import DDIMScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    g = torch.Generator().manual_seed(0)
    z = torch.randn(64, generator=g, dtype=torch.float64)
    noises = [torch.randn(64, generator=g, dtype=torch.float64) for _ in range(10)] if ancestral else None
    cls = EulerAncestralDiscreteScheduler if ancestral else EulerDiscreteScheduler
    eu = cls(timestep_spacing="leading", steps_offset=1, **BETAS)
    eu.set_timesteps(10)
    assert eu.init_noise_sigma == pytest.approx((max(eu._sigmas_host) ** 2 + 1) ** 0.5)
    xs = SC.run_product(eu, 10, z * eu.init_noise_sigma, _tanh_model, noises=noises)
    dd = DDIMScheduler(steps_offset=1, clip_sample=False, **BETAS)
    ys = SC.run_product(dd, 10, z.clone(), _tanh_model, eta=1.0 if ancestral else 0.0, noises=noises)
    assert dd._timesteps_host == eu._timesteps_host
    y = z.clone()                                           # the DDIM closed form on Euler's own noise levels
    for k, ((a_t, a_p), t) in enumerate(zip(_own_pairs(eu), eu._timesteps_host)):
        y = _ddim_closed(y, _tanh_model(y, t), a_t, a_p, 1.0 if ancestral else 0.0, noises[k] if ancestral else None)
        s_next = eu._sigmas_host[k + 1]
        scaled = xs[k] / (s_next ** 2 + 1) ** 0.5
        assert _relmax(scaled, y) < 1e-10, (k, _relmax(scaled, y))
        assert _relmax(scaled, ys[k]) < 1e-5, (k, _relmax(scaled, ys[k]))
    assert len(K._sampler_calls["sampler_step"]) == (20 if ancestral else 10)
    assert len(K._sampler_calls["cfg_ddim_step"]) == (0 if ancestral else 10)


def test_dpm_order_1_is_ddim_on_its_own_pairs(K):
    from synfmc_amd.schedulers import DPMSolverMultistepScheduler
    z = torch.randn(64, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    sch = DPMSolverMultistepScheduler(solver_order=1, **BETAS)
    xs = SC.run_product(sch, 10, z, _tanh_model)
    y = z.clone()
    for k, ((a_t, a_p), t) in enumerate(zip(_own_pairs(sch), sch._timesteps_host)):
        y = _ddim_closed(y, _tanh_model(y, t), a_t, a_p)
        assert _relmax(xs[k], y) < 1e-10, (k, _relmax(xs[k], y))


SAMPLERS = [("ddim", dict(steps_offset=1, clip_sample=False)), ("ddim", dict(clip_sample=False, timestep_spacing="trailing", prediction_type="v_prediction")),    # (DDIM's previous timestep is
            # t - T // n under every spacing: with "linspace" that is not the next table entry, so the line is left there by construction)
            ("euler", dict()), ("euler", dict(timestep_spacing="trailing", prediction_type="v_prediction")),
            ("dpm", dict(solver_order=1)), ("dpm", dict(solver_order=2)), ("dpm", dict(solver_order=3)),
            ("dpm", dict(solver_order=3, lower_order_final=False, timestep_spacing="trailing")), ("dpm", dict(solver_order=2, euler_at_final=True))]


def _make(kind, kw):
    from synfmc_amd import schedulers as S
    cls = {"ddim": S.DDIMScheduler, "euler": S.EulerDiscreteScheduler, "ancestral": S.EulerAncestralDiscreteScheduler,
           "dpm": S.DPMSolverMultistepScheduler}[kind]
    return cls(**BETAS, **kw)


@pytest.mark.parametrize("kind,kw", SAMPLERS)
def test_point_mass_denoiser_stays_on_the_line(K, kind, kw):
    """eps (or v) of a data distribution that is one point x0: every deterministic sampler keeps x on alpha x0 + sigma n0."""
    g = torch.Generator().manual_seed(0)
    x0, n0 = torch.randn(64, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
    sch = _make(kind, kw)
    sch.set_timesteps(10)
    if kind == "ddim":
        levels = [sch._alphas(t) for t in sch._timesteps_host]
        acs = [a for a, _ in levels] + [levels[-1][1]]
        line = lambda a: a ** 0.5 * x0 + (1 - a) ** 0.5 * n0
    else:
        acs = [1.0 / (s * s + 1.0) for s in sch._sigmas_host]
        line = (lambda a: x0 + ((1 - a) / a) ** 0.5 * n0) if kind == "euler" else (lambda a: a ** 0.5 * x0 + (1 - a) ** 0.5 * n0)
    step = {"k": 0}

    def model(x_in, t):
        a = acs[step["k"]]
        step["k"] += 1
        e = (x_in - a ** 0.5 * x0) / (1 - a) ** 0.5
        if kw.get("prediction_type") == "v_prediction":
            return a ** 0.5 * e - (1 - a) ** 0.5 * x0
        return e

    xs = SC.run_product(sch, 10, line(acs[0]), model)
    for k, x in enumerate(xs):
        assert _relmax(x, line(acs[k + 1])) < 1e-10, (k, _relmax(x, line(acs[k + 1])))
    if kind in ("ddim", "euler"):
        assert _relmax(xs[-1], x0) < 1e-10


# ---- 3. order --------------------------------------------------------------------------------------------------------------------
def _dpm_on_pairs(K, order, n):
    from synfmc_amd.schedulers import DPMSolverMultistepScheduler
    ac = SC.alphas_cumprod()
    ts = np.linspace(999, 0, n + 1).round().astype(np.int64)
    sch = DPMSolverMultistepScheduler(solver_order=order, lower_order_final=False, **BETAS)
    sch.set_timesteps(n)
    sch._set_tables(ts[:-1], np.sqrt((1 - ac[ts]) / ac[ts]), None)
    sch.num_inference_steps = n
    x = torch.randn(64, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    for t in sch._timesteps_host:
        x = sch.step_cfg(torch.tanh(0.7 * x + 0.3 * float(ac[t])), t, x, 1.0, False)
    return x


def test_dpm_second_order_converges_faster(K):
    ref = _dpm_on_pairs(K, 1, 999)
    err = {o: {n: float((_dpm_on_pairs(K, o, n) - ref).abs().max()) for n in (10, 20, 40)} for o in (1, 2)}
    print(f"DPM-Solver++ max error against 999 first-order steps: order 1 {err[1]}, order 2 {err[2]}")
    for n in (10, 20):
        assert err[2][n] < err[1][n]
        assert err[2][n] / err[2][2 * n] > err[1][n] / err[1][2 * n]


# ---- 4. the product against the restatements, float64 ----------------------------------------------------------------------------
REFS = [("ddim", dict(steps_offset=1, clip_sample=False), lambda ac: SC.RefDDIM(ac, steps_offset=1), 0.0),
        ("ddim", dict(clip_sample=True, clip_sample_range=0.9, timestep_spacing="trailing", prediction_type="v_prediction"),
         lambda ac: SC.RefDDIM(ac, spacing="trailing", prediction_type="v_prediction", clip_sample=True, clip_sample_range=0.9, eta=0.6), 0.6),
        ("ddim", dict(clip_sample=False, timestep_spacing="linspace", prediction_type="sample"),
         lambda ac: SC.RefDDIM(ac, spacing="linspace", prediction_type="sample"), 0.0),
        ("euler", dict(), lambda ac: SC.RefEuler(ac), 0.0),
        ("euler", dict(timestep_spacing="leading", steps_offset=1, prediction_type="v_prediction"),
         lambda ac: SC.RefEuler(ac, spacing="leading", steps_offset=1, prediction_type="v_prediction"), 0.0),
        ("ancestral", dict(timestep_spacing="trailing"), lambda ac: SC.RefEuler(ac, spacing="trailing", ancestral=True), 0.0),
        ("dpm", dict(solver_order=1), lambda ac: SC.RefDPM(ac, solver_order=1), 0.0),
        ("dpm", dict(solver_order=2), lambda ac: SC.RefDPM(ac, solver_order=2), 0.0),
        ("dpm", dict(solver_order=3, timestep_spacing="leading", steps_offset=1), lambda ac: SC.RefDPM(ac, solver_order=3, spacing="leading", steps_offset=1), 0.0),
        ("dpm", dict(solver_order=3, lower_order_final=False, prediction_type="v_prediction"),
         lambda ac: SC.RefDPM(ac, solver_order=3, lower_order_final=False, prediction_type="v_prediction"), 0.0)]


@pytest.mark.parametrize("n_steps", [7, 16])
@pytest.mark.parametrize("kind,kw,make_ref,eta", REFS)
def test_product_schedulers_match_the_restatements(K, kind, kw, make_ref, eta, n_steps):
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, 48, generator=g, dtype=torch.float64)
    noises = [torch.randn(2, 48, generator=g, dtype=torch.float64) for _ in range(n_steps)]
    sch, ref = _make(kind, kw), make_ref(SC.alphas_cumprod())
    ref.noises = noises

    def model(x_in, t):                                     # two CFG halves that differ
        e = _tanh_model(x_in, t)
        e[e.shape[0] // 2:] += 0.2
        return e

    stochastic = kind == "ancestral" or eta > 0
    got = SC.run_product(sch, n_steps, z * sch.init_noise_sigma, model, guidance=2.0, eta=eta, noises=noises if stochastic else None)
    want = SC.run_reference(ref, n_steps, z * ref.init_noise_sigma, model, guidance=2.0)
    assert [float(t) for t in sch._timesteps_host] == [float(t) for t in ref.timesteps.tolist()]
    assert sch.init_noise_sigma == pytest.approx(ref.init_noise_sigma, rel=1e-12)
    for k in range(n_steps):
        assert _relmax(got[k], want[k]) < 1e-10, (k, _relmax(got[k], want[k]))


# ---- 5. tables and plumbing ------------------------------------------------------------------------------------------------------
def test_tables_lengths_dtypes_and_reset(K):
    from synfmc_amd import schedulers as S
    eu = S.EulerDiscreteScheduler(**BETAS)
    smax = float(eu.sigmas.max())
    assert eu.init_noise_sigma == smax == pytest.approx(((1 - SC.alphas_cumprod()[-1]) / SC.alphas_cumprod()[-1]) ** 0.5, rel=1e-6)
    assert S.EulerDiscreteScheduler(timestep_spacing="leading", **BETAS).init_noise_sigma == pytest.approx((smax ** 2 + 1) ** 0.5)
    eu.set_timesteps(3)
    assert eu._timesteps_host == [999.0, 499.5, 0.0] and eu.timesteps.dtype == torch.float32
    assert eu.sigmas.dtype == torch.float32 and eu.sigmas.shape == (4,) and float(eu.sigmas[-1]) == 0.0
    eu.set_timesteps(10)
    assert eu._timesteps_host == [999, 888, 777, 666, 555, 444, 333, 222, 111, 0] and all(isinstance(t, int) for t in eu._timesteps_host)
    dpm = S.DPMSolverMultistepScheduler(solver_order=3, **BETAS)
    assert dpm.init_noise_sigma == 1.0
    dpm.set_timesteps(5)
    assert dpm.timesteps.dtype == torch.int64 and len(dpm._timesteps_host) == 5 and dpm.sigmas.shape == (6,)
    assert dpm._timesteps_host == np.linspace(0, 999, 6).round()[::-1][:-1].astype(int).tolist()
    x = torch.randn(1, 8, dtype=torch.float64)
    for t in dpm._timesteps_host[:3]:
        x = dpm.step_cfg(torch.zeros_like(x), t, x, 1.0, False)
    assert dpm._step_index == 3 and len(dpm._hist) == 3 and dpm._lower_order_nums == 3
    with pytest.raises(ValueError, match="timestep"):
        dpm.step_cfg(torch.zeros_like(x), dpm._timesteps_host[0], x, 1.0, False)       # not the table's entry at the counter
    old = dpm._hist
    dpm.set_timesteps(5)
    assert dpm._step_index == 0 and dpm._hist == [] and dpm._lower_order_nums == 0
    dpm.step_cfg(torch.zeros_like(x), dpm._timesteps_host[0], x, 1.0, False)
    assert len(dpm._hist) == 3 and all(a is not b for a in dpm._hist for b in old)
    assert [len(kw["hist"]) for kw in K._sampler_calls["sampler_step"]] == [0, 1, 2, 0]
    dd = S.DDIMScheduler(clip_sample=False, timestep_spacing="trailing", **BETAS)
    dd.set_timesteps(4)
    assert dd._timesteps_host == [999, 749, 499, 249] and dd.timesteps.dtype == torch.int64
    dd = S.DDIMScheduler(clip_sample=False, timestep_spacing="linspace", **BETAS)
    dd.set_timesteps(4)
    assert dd._timesteps_host == [999, 666, 333, 0]
    x0, nz, t = torch.randn(2, 3), torch.randn(2, 3), torch.tensor([5, 700])
    ac = dd.alphas_cumprod[t][:, None]
    assert torch.allclose(dd.get_velocity(x0, nz, t), ac.sqrt() * nz - (1 - ac).sqrt() * x0, atol=1e-7)


class _FakeUNet(torch.nn.Module):
    in_channels = 4
    dtype = torch.float32

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.config = types.SimpleNamespace(sample_size=8)
        self.seen = []

    def forward(self, x, t, encoder_hidden_states=None, **kw):
        self.seen.append((t.dtype, float(t)))
        return types.SimpleNamespace(sample=torch.tanh(0.7 * x + 0.3 * torch.sin(t.double() / 100.0).float()))


def _pipes(scheduler):
    from synfmc_amd.pipelines.pipeline_animation_cm_om import AnimationPipeline, CameraObjCtrlPipeline
    unet = _FakeUNet()
    text = torch.zeros(2, 77, 8)
    lat = torch.randn(1, 4, 2, 8, 8, generator=torch.Generator().manual_seed(1))
    plain = AnimationPipeline(None, None, None, unet, scheduler)
    cam = CameraObjCtrlPipeline(None, None, None, unet, scheduler, lambda emb: [torch.zeros(2, 4, 8, 8)])
    kw = dict(height=64, width=64, guidance_scale=2.0, output_type="latent", prompt_embeds=text, use_graph=False)
    run_plain = lambda **k: plain(None, 2, latents=lat.clone(), multidiff_overlaps=0, **kw, **k).videos
    run_cam = lambda **k: cam(None, torch.zeros(1, 6, 2, 64, 64), 2, latents=lat.clone(), **kw, **k).videos
    return unet, run_plain, run_cam


def test_fractional_timesteps_reach_the_unet(K):
    from synfmc_amd.schedulers import EulerDiscreteScheduler
    for which in (1, 2):
        unet, *runs = _pipes(EulerDiscreteScheduler(**BETAS))
        runs[which - 1](num_inference_steps=3)
        assert unet.seen == [(torch.float32, 999.0), (torch.float32, 499.5), (torch.float32, 0.0)]


def test_eta_and_generator_through_both_pipelines(K):
    from synfmc_amd import schedulers as S
    kw = dict(clip_sample=False, steps_offset=1, **BETAS)
    for which in (0, 1):
        gen = lambda s: torch.Generator().manual_seed(s)
        run = lambda sch, **k: _pipes(sch)[1 + which](num_inference_steps=3, **k)
        K._sampler_calls["sampler_step"].clear()
        K._sampler_calls["cfg_ddim_step"].clear()
        base = run(S.DDIMScheduler(**kw))
        assert len(K._sampler_calls["cfg_ddim_step"]) == 3 and not K._sampler_calls["sampler_step"]       # the default: its own kernel
        a, b, c = (run(S.DDIMScheduler(**kw), eta=0.5, generator=gen(s)) for s in (7, 7, 8))
        assert all(k["c_n"] > 0 and k["noise"] is not None for k in K._sampler_calls["sampler_step"][:2])  # (the last step lands on alpha = 1)
        assert len(K._sampler_calls["cfg_ddim_step"]) == 3
        assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, base)
        e0, e1 = run(S.EulerDiscreteScheduler(**BETAS)), run(S.EulerDiscreteScheduler(**BETAS), eta=0.5, generator=gen(7))
        assert torch.equal(e0, e1)                                                                          # eta and the generator change nothing
        d0, d1 = run(S.DPMSolverMultistepScheduler(**BETAS)), run(S.DPMSolverMultistepScheduler(**BETAS), eta=0.5)
        assert torch.equal(d0, d1)
        a, b, c = (run(S.EulerAncestralDiscreteScheduler(**BETAS), generator=gen(s)) for s in (7, 7, 8))
        assert torch.equal(a, b) and not torch.equal(a, c)


def test_multidiff_windows_on_the_new_path(K):
    """Sliding windows with Euler: scaled window inputs, the averaged guided prediction with has_uncond=False, no x_in."""
    from synfmc_amd.pipelines.pipeline_animation_cm_om import AnimationPipeline
    from synfmc_amd.schedulers import EulerDiscreteScheduler
    unet = _FakeUNet()
    pipe = AnimationPipeline(None, None, None, unet, EulerDiscreteScheduler(**BETAS))
    lat = torch.randn(1, 4, 6, 8, 8, generator=torch.Generator().manual_seed(1))
    out = pipe(None, 4, height=64, width=64, num_inference_steps=3, guidance_scale=2.0, latents=lat, output_type="latent",
               prompt_embeds=torch.zeros(2, 77, 8), use_graph=False, multidiff_total_steps=2, multidiff_overlaps=2).videos
    calls = K._sampler_calls["sampler_step"]
    assert out.shape == lat.shape and len(calls) == 3 and all(not c["has_uncond"] and c["x_in"] is None for c in calls)
    assert torch.isfinite(out).all()


def _foreign(name, **cfg):
    base = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1)
    return type(name, (), {"config": types.SimpleNamespace(**dict(base, **cfg))})()


def test_coerce_scheduler_families():
    from synfmc_amd import schedulers as S
    got = S.coerce_scheduler(_foreign("DDIMScheduler", clip_sample=False, prediction_type="v_prediction", timestep_spacing="trailing"))
    assert type(got) is S.DDIMScheduler and got.config.prediction_type == "v_prediction" and got.config.timestep_spacing == "trailing"
    got = S.coerce_scheduler(_foreign("EulerDiscreteScheduler", timestep_spacing="leading"))
    assert type(got) is S.EulerDiscreteScheduler and got.config.timestep_spacing == "leading" and got.config.steps_offset == 1
    assert type(S.coerce_scheduler(_foreign("EulerAncestralDiscreteScheduler"))) is S.EulerAncestralDiscreteScheduler
    got = S.coerce_scheduler(_foreign("DPMSolverMultistepScheduler", solver_order=3, euler_at_final=True))
    assert type(got) is S.DPMSolverMultistepScheduler and got.config.solver_order == 3 and got.config.euler_at_final
    for bad in (_foreign("PNDMScheduler"), _foreign("LMSDiscreteScheduler"), _foreign("DPMSolverMultistepScheduler", algorithm_type="sde-dpmsolver++"),
                _foreign("EulerDiscreteScheduler", use_karras_sigmas=True), _foreign("DPMSolverMultistepScheduler", thresholding=True)):
        with pytest.raises(NotImplementedError, match="DDIMScheduler, EulerDiscreteScheduler"):
            S.coerce_scheduler(bad)
    mine = S.EulerDiscreteScheduler(**BETAS)
    assert S.coerce_scheduler(mine) is mine


# ---- 6. training target ----------------------------------------------------------------------------------------------------------
def test_training_target_by_prediction_type():
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.training import training_target
    g = torch.Generator().manual_seed(2)
    x0, nz, t = torch.randn(2, 4, 3, 4, 4, generator=g), torch.randn(2, 4, 3, 4, 4, generator=g), torch.tensor([3, 870])
    eps_s = DDIMScheduler(clip_sample=False, **BETAS)
    assert training_target(eps_s, x0, nz, t) is nz                                      # epsilon: the very tensor, as before
    v_s = DDIMScheduler(clip_sample=False, prediction_type="v_prediction", **BETAS)
    ac = v_s.alphas_cumprod[t].view(2, 1, 1, 1, 1)
    assert torch.allclose(training_target(v_s, x0, nz, t), ac.sqrt() * nz - (1 - ac).sqrt() * x0, atol=1e-7)
    with pytest.raises(ValueError, match="prediction type"):
        training_target(DDIMScheduler(clip_sample=False, prediction_type="sample", **BETAS), x0, nz, t)


def test_stage1_step_uses_the_target(monkeypatch):
    """The v-prediction target reaches the loss of a training step: a model that returns the velocity has zero loss."""
    from synfmc_amd import training as T
    from synfmc_amd.schedulers import DDIMScheduler
    g = torch.Generator().manual_seed(4)
    x0, nz, t = torch.randn(2, 4, 4, 4, generator=g), torch.randn(2, 4, 4, 4, generator=g), torch.tensor([10, 600])
    monkeypatch.setattr(T, "optimizer_update", lambda *a, **k: None)
    for kind in ("epsilon", "v_prediction"):
        sch = DDIMScheduler(clip_sample=False, prediction_type=kind, **BETAS)
        want = nz if kind == "epsilon" else sch.get_velocity(x0, nz, t)
        w = torch.nn.Parameter(torch.zeros(()))
        unet = lambda x, tt, text: types.SimpleNamespace(sample=want.unsqueeze(2) + w)
        loss = T.stage1_training_step(unet, [w], sch, None, None, x0, nz, t, None)
        assert float(loss) == 0.0

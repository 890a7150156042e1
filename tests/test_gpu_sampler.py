"""`fmc_sampler_step` and the samplers built on it, on the GPU: the raw C ABI against the float64 closed form element by element
(bound and rounding count: tests/sampler_common.py), inside guarded arenas, the four schedulers against their float64 restatements,
and Euler / DPM-Solver++ through `CameraObjCtrlPipeline` against the oracle U-Net driven by the restated scheduler.

Shapes: n = 1, 7, 8, 9 (below, at and above one 8-element run), 4097 (several workgroups, a tail), one and two trips of the capped
grid plus a ragged rest.  Odd n with has_uncond puts the conditional half of a bf16 eps_uc, and the second copy of x_in, on a 2-byte
boundary; `skew` moves the fp32 streams off 16 bytes (together: a scalar head; each differently: the element-wise path).
"""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch
from einops import rearrange

from oracle import conditioning as OC
from oracle import pipeline as OP
from tests import common_models as CM
from tests import edge_guard_common as EG
from tests import sampler_common as SC
from tests.test_gpu_kernels import rel_inf

pytestmark = pytest.mark.gpu

BETAS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
COEF = dict(guidance=7.5, m_x=1.31, m_e=-0.77, c_x=0.93, c_e=0.21, c_m=-0.35, c_n=0.4, in_scale=0.37)
C_H = [0.6, -0.45, 0.3]
CLAMP = {True: 5.0, False: 1.0}                             # by has_uncond: m = 1.31 x - 0.77 e has a standard deviation of 7.8 under guidance 7.5
                                                            # and 1.5 without, so about half of the elements lie beyond the clamp either way


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _coef(K, clamp, n_hist, **over):
    from synfmc_amd._lib import SamplerCoef
    c = dict(COEF, **over)
    return SamplerCoef(c["guidance"], c["m_x"], c["m_e"], clamp, c["c_x"], c["c_e"], c["c_m"], c["c_n"], (ctypes.c_float * 3)(*C_H), c["in_scale"])


def _raw(K, eps, x, noise, hist, x_out, m_out, x_in, n, has_uncond, n_hist, in_reps, coef, dtype, in_dtype):
    from synfmc_amd import _lib
    p = lambda t: None if t is None else t.data_ptr()
    h = [p(t) for t in hist] + [None] * (3 - len(hist))
    return _lib.load().fmc_sampler_step(p(eps), p(x), p(noise), h[0], h[1], h[2], p(x_out), p(m_out), p(x_in), n, int(has_uncond), n_hist,
                                        in_reps, coef, K._DT[dtype], K._DT[in_dtype], K._stream())


class _Inputs:
    """One set of host inputs per (n, dtype), shared by every configuration of the case and left unchanged."""

    def __init__(self, n, dtype):
        g = torch.Generator().manual_seed(n % 9973)
        self.n, self.dtype = n, dtype
        self.eps = torch.randn(2 * n, generator=g).to(dtype)
        self.noise = torch.randn(n, generator=g).to(dtype)
        self.x = torch.randn(n, generator=g)
        self.hist = [torch.randn(n, generator=g) for _ in range(3)]
        self.dev = {k: v.cuda() for k, v in dict(eps=self.eps, noise=self.noise, x=self.x).items()}
        self.dev["hist"] = [h.cuda() for h in self.hist]
        self._ref = {}

    def reference(self, has_uncond, n_hist, clamp, noise):
        key = (has_uncond, n_hist, clamp, noise)
        if key not in self._ref:
            n = self.n
            self._ref[key] = SC.closed_form(self.eps if has_uncond else self.eps[:n], self.x, has_uncond=has_uncond, m_clamp=clamp,
                                            c_h=C_H[:n_hist], hist=self.hist[:n_hist], noise=self.noise if noise else None, **COEF)
        return self._ref[key]


def _place(t, off, pad=8):
    """A copy of `t` that starts `off` elements into a fresh buffer (off = 0: 16-byte aligned like any tensor)."""
    buf = torch.zeros(t.numel() + pad, dtype=t.dtype, device="cuda")
    v = buf[off:off + t.numel()]
    v.copy_(t)
    return v


def _run_config(K, inp, has_uncond, n_hist, clamp, noise, m_mode, alias_x, in_reps, skew, in_dtype=None):
    """One launch; returns the worst error / bound of every output.  m_mode: None, "own" or the history slot m_out aliases."""
    n, dtype = inp.n, inp.dtype
    clamp = CLAMP[has_uncond] if clamp else 0.0
    in_dtype = in_dtype or dtype
    offs = {"x": 0, "h": [0, 0, 0], "xo": 0, "mo": 0, "eps": 0, "nz": 0, "xin": 0}
    if skew == 1:
        offs = {"x": 1, "h": [1, 1, 1], "xo": 1, "mo": 1, "eps": 0, "nz": 0, "xin": 0}
    elif skew == 2:
        offs = {"x": 3, "h": [1, 2, 0], "xo": 2, "mo": 1, "eps": 1, "nz": 3, "xin": 1}
    d = inp.dev
    eps = _place(d["eps"] if has_uncond else d["eps"][:n], offs["eps"])
    nz = _place(d["noise"], offs["nz"]) if noise else None
    x = _place(d["x"], offs["x"])
    hist = [_place(d["hist"][j], offs["h"][j]) for j in range(n_hist)]
    x_out = x if alias_x else _place(torch.full((n,), float("nan"), device="cuda"), offs["xo"])
    m_out = None if m_mode is None else (_place(torch.full((n,), float("nan"), device="cuda"), offs["mo"]) if m_mode == "own" else hist[m_mode])
    x_in = _place(torch.full((in_reps * n,), float("nan"), device="cuda").to(in_dtype), offs["xin"]) if in_reps else None
    rc = _raw(K, eps, x, nz, hist, x_out, m_out, x_in, n, has_uncond, n_hist, in_reps, _coef(K, clamp, n_hist), dtype, in_dtype)
    assert rc == 0, K._lib.load().fmc_last_error()
    ref = inp.reference(has_uncond, n_hist, clamp, noise)
    rat = {"x_out": SC.worst_ratio(x_out, "x_out", *ref["x_out"])}
    if m_out is not None:
        rat["m_out"] = SC.worst_ratio(m_out, "m_out", *ref["m_out"])
    for r in range(in_reps):
        rat[f"x_in{r}"] = SC.worst_ratio(x_in[r * n:(r + 1) * n], "x_in", *ref["x_in"], dtype=in_dtype)
    for j in range(n_hist):                                  # an input the launch must not have written
        if m_mode != j:
            assert torch.equal(hist[j], d["hist"][j])
    assert clamp == 0 or 0.1 < float((ref["m_out"][0].abs() == SC.f32(clamp)).double().mean()) < 0.9 or n < 64
    return rat


def _m_modes(n_hist):
    return [None, "own"] + list(range(n_hist))


def _trip(K):
    return K.sampler_step_elems_per_trip()


SIZES = [1, 7, 8, 9, 4097, "trip+3", "2trip+5"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("size", SIZES)
def test_raw_abi_against_closed_form(K, size, dtype):
    trip = _trip(K)
    n = size if isinstance(size, int) else {"trip+3": trip + 3, "2trip+5": 2 * trip + 5}[size]
    inp = _Inputs(n, dtype)
    if n <= 4097:                                           # the full product of the options
        configs = [(u, nh, cl, nz, mm, ax, reps, 0) for u, nh, cl, nz, ax, reps in
                   itertools.product((False, True), range(4), (False, True), (False, True), (False, True), (0, 1, 2)) for mm in _m_modes(nh)]
        configs = configs[::3] if n > 9 else configs        # all 672 up to n = 9, every third of them at 4097
        configs += [(True, 3, True, True, 1, True, 2, skew) for skew in (1, 2)] + [(False, 1, False, False, "own", False, 1, skew) for skew in (1, 2)]
    else:                                                   # the trips of the capped grid: everything on, and the barest launch
        configs = [(True, 3, True, True, 2, True, 2, 0), (False, 0, False, False, None, False, 0, 0), (True, 2, False, False, "own", False, 1, 1)]
    worst = {}
    for cfg in configs:
        for k, v in _run_config(K, inp, *cfg).items():
            worst[k[:4]] = max(worst.get(k[:4], 0.0), v)
            assert v <= 1.0, (cfg, k, v)
    if n == 4097:                                           # the model dtype of x_in need not be that of eps
        other = torch.bfloat16 if dtype == torch.float32 else torch.float32
        for k, v in _run_config(K, inp, True, 2, True, True, "own", False, 2, 0, in_dtype=other).items():
            assert v <= 1.0, ("in_dtype", k, v)
    print(f"n={n} {dtype}: {len(configs)} configurations, share of the bound used {({k: round(v, 3) for k, v in worst.items()})}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [9, 4099])
def test_guarded_arenas(K, n, dtype):
    """Zeros, NaN and +Inf around every input, sentinels around every output: same bits, nothing outside written, everything inside written."""
    inp = _Inputs(n, dtype)
    coef = _coef(K, CLAMP[True], 3)

    def fn(g):
        eps = g.inp(inp.eps, 1, name="eps_uc")
        nz = g.inp(inp.noise, 1, name="noise")
        x = g.inp(inp.x, 1, name="x")
        hist = [g.inp(inp.hist[j], 1, name=f"hist{j}") for j in range(3)]
        x_out = g.out((n,), torch.float32, 1, name="x_out")
        m_out = g.out((n,), torch.float32, 1, name="m_out")
        x_in = g.out((2 * n,), dtype, 1, name="x_in")
        assert _raw(K, eps, x, nz, hist, x_out, m_out, x_in, n, True, 3, 2, coef, dtype, dtype) == 0
        return {"x_out": x_out, "m_out": m_out, "x_in": x_in}

    outs = EG.run_surroundings(fn, device="cuda", what=f"sampler_step n={n} {dtype}", sync=torch.cuda.synchronize)
    ref = inp.reference(True, 3, CLAMP[True], True)
    assert SC.worst_ratio(outs["x_out"], "x_out", *ref["x_out"]) <= 1.0 and SC.worst_ratio(outs["m_out"], "m_out", *ref["m_out"]) <= 1.0
    for r in range(2):
        assert SC.worst_ratio(outs["x_in"][r * n:(r + 1) * n], "x_in", *ref["x_in"], dtype=dtype) <= 1.0


def test_argument_errors(K):
    from synfmc_amd import _lib
    n = 16
    f = lambda: torch.zeros(2 * n, device="cuda")
    eps, x, out, xin = f(), f(), f(), f()
    coef = _coef(K, 0.0, 0)
    call = lambda **k: _raw(K, **dict(dict(eps=eps, x=x, noise=None, hist=[], x_out=out, m_out=None, x_in=None, n=n, has_uncond=False, n_hist=0,
                                          in_reps=0, coef=coef, dtype=torch.float32, in_dtype=torch.float32), **k))
    assert call() == 0
    assert call(eps=None) == -5 and call(x=None) == -5 and call(x_out=None) == -5
    assert b"NULL" in _lib.load().fmc_last_error()
    assert call(n_hist=2, hist=[x]) == -5                   # hist[1] missing
    assert call(in_reps=1) == -5                            # x_in missing
    assert call(n=0) == -1 and call(n=-3) == -1 and call(n_hist=4, hist=[x, x, x]) == -1 and call(in_reps=3, x_in=xin) == -1
    lib = _lib.load()
    p = lambda t: t.data_ptr()
    assert lib.fmc_sampler_step(p(eps), p(x), None, None, None, None, p(out), None, None, n, 0, 0, 0, coef, 7, 0, K._stream()) == -2
    assert lib.fmc_sampler_step(p(eps), p(x), None, None, None, None, p(out), None, p(xin), n, 0, 0, 1, coef, 1, 7, K._stream()) == -2
    assert lib.fmc_sampler_step(p(eps), p(x) + 2, None, None, None, None, p(out), None, None, n, 0, 0, 0, coef, 1, 1, K._stream()) == -3
    with pytest.raises(ValueError, match="bad n"):
        _lib.check(call(n=0), "fmc_sampler_step")
    torch.cuda.synchronize()
    assert K.sampler_step_elems_per_trip() % 8 == 0 and K.sampler_step_elems_per_trip() >= 8 * 256


# ---- the schedulers --------------------------------------------------------------------------------------------------------------
GUIDE = 2.0
SCHEDULERS = [("ddim", dict(clip_sample=True, clip_sample_range=1.5, timestep_spacing="trailing"),
               lambda ac: SC.RefDDIM(ac, spacing="trailing", clip_sample=True, clip_sample_range=1.5, eta=0.7), 0.7),
              ("euler", dict(), lambda ac: SC.RefEuler(ac), 0.0),
              ("ancestral", dict(), lambda ac: SC.RefEuler(ac, ancestral=True), 0.0),
              ("dpm", dict(solver_order=3, lower_order_final=False), lambda ac: SC.RefDPM(ac, solver_order=3, lower_order_final=False), 0.0)]


def _model64(x_in, t):
    e = torch.tanh(0.7 * x_in.double() + 0.3 * math.sin(float(t) / 100.0))
    e[e.shape[0] // 2:] += 0.2
    return e


@pytest.mark.parametrize("kind,kw,make_ref,eta", SCHEDULERS, ids=[s[0] for s in SCHEDULERS])
def test_schedulers_against_restatements(K, monkeypatch, kind, kw, make_ref, eta):
    """4 steps on [1, 4, 2, 8, 8] latents with CFG.  The model is evaluated in float64 on the x_in the kernel wrote and rounded to fp32.

    The bound of step k, element-wise: the kernel's own rounding bound b_k (closed form, with the coefficients and buffers of the
    launch) plus what the deviation D_k of the state does to this step's exact result:
        D_{k+1} = b_k + (|c_x| + |c_m m_x|) D_k + (|c_e| + |c_m m_e|) E_k + sum_j |c_h[j]| M_{k-1-j}
        E_k = L (in_scale_{k-1} D_k + 2 * 2^-24 |x_in|) + 2^-24 (1 + 2 g) max|e|
              (model slope <= 0.7, CFG combine <= 1 + 2 g: L = 0.7 (1 + 2 g); x_in is x' scaled and rounded; eps is rounded to fp32)
        M_k = R_M 2^-24 sum|terms of m| + |m_x| D_k + |m_e| E_k  (the deviation of the stored x0 prediction)
    -- a recursion linear in the step count for coefficients of size one, evaluated with the launches' own numbers.
    Measured share of it: at most 0.08 at step 1, falling to 0.005 and less by step 4 (profiles/samplers.md)."""
    from synfmc_amd import schedulers as S
    cls = {"ddim": S.DDIMScheduler, "euler": S.EulerDiscreteScheduler, "ancestral": S.EulerAncestralDiscreteScheduler,
           "dpm": S.DPMSolverMultistepScheduler}[kind]
    g = torch.Generator().manual_seed(11)
    z = torch.randn(1, 4, 2, 8, 8, generator=g)
    noises = [torch.randn(1, 4, 2, 8, 8, generator=g) for _ in range(4)]
    sch, ref = cls(**BETAS, **kw), make_ref(SC.alphas_cumprod())
    ref.noises = [nz.double() for nz in noises]
    launches = []
    real = K.sampler_step

    def spy(eps, x, **k):
        rec = dict(k, eps=eps.clone(), x=x.clone(), hist=[h.clone() for h in k.get("hist", ())])
        launches.append(rec)
        return real(eps, x, **k)

    monkeypatch.setattr(K, "sampler_step", spy)
    stochastic = kind == "ancestral" or eta > 0
    seen = []

    def model(x_in, t):
        seen.append(x_in[:x_in.shape[0] // 2].double().cpu().reshape(-1).abs())
        return _model64(x_in.cpu(), t).float().cuda()

    got = SC.run_product(sch, 4, (z * sch.init_noise_sigma).cuda(), model, guidance=GUIDE, eta=eta,
                         noises=[nz.cuda() for nz in noises] if stochastic else None)
    want = SC.run_reference(ref, 4, z.double() * ref.init_noise_sigma, _model64, guidance=GUIDE)
    assert len(launches) == 4
    L = 0.7 * (1 + 2 * GUIDE)
    D = torch.zeros(z.numel(), dtype=torch.float64)
    M, scale_prev, used = [], 1.0 if kind in ("ddim", "dpm") else 1.0 / math.sqrt(sch._sigmas_host[0] ** 2 + 1), []
    for k, rec in enumerate(launches):
        c = {key: rec.get(key, 0.0) for key in ("m_x", "m_e", "m_clamp", "c_x", "c_e", "c_m", "c_n")}
        cf = SC.closed_form(rec["eps"], rec["x"], guidance=GUIDE, has_uncond=True, c_h=rec.get("c_h", ()), hist=rec["hist"], noise=rec.get("noise"),
                            in_scale=rec.get("in_scale", 1.0), **c)
        E = L * (scale_prev * D + 2 * SC.U32 * seen[k]) + SC.U32 * (1 + 2 * GUIDE) * float(rec["eps"].abs().max())
        b = SC.bound("x_out", *cf["x_out"])
        nxt = b + (abs(c["c_x"]) + abs(c["c_m"] * c["m_x"])) * D + (abs(c["c_e"]) + abs(c["c_m"] * c["m_e"])) * E
        for j, ch in enumerate(rec.get("c_h", ())):
            nxt = nxt + abs(ch) * M[k - 1 - j]
        M.append(SC.bound("m_out", *cf["m_out"]) + abs(c["m_x"]) * D + abs(c["m_e"]) * E)
        D, scale_prev = nxt, rec.get("in_scale", 1.0)
        err = (got[k].double().cpu().reshape(-1) - want[k].reshape(-1)).abs()
        used.append(float((err / D).max()))
        assert bool((err <= D).all()), (kind, k, used)
    print(f"{kind}: share of the bound used per step {[round(u, 3) for u in used]}; final rel-inf {rel_inf(got[-1], want[-1]):.2e}")


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
W4 = (64, 128, 256, 256)


@pytest.fixture(scope="module")
def stack8():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ou, oe, oa = CM.build_oracle(W4)
    clip = CM.synthetic_clip(B=1, Fr=8, H=64, W=64)
    with torch.no_grad():
        pose_emb = rearrange(OC.to_plucker_embedding(clip["c2w"], clip["K"], (64, 64)), "b f c h w -> b c f h w")
        traj = OC.get_traj_features(clip["infos"], clip["masks"], oa)
    g = torch.Generator().manual_seed(5)
    text2 = torch.cat([torch.randn(1, 77, 64, generator=g), clip["text"]])
    pu, pe, pa = CM.build_product(ou, oe, oa, W4)
    return dict(ou=ou, oe=oe, clip=clip, pose_emb=pose_emb, traj=traj, text2=text2, pu=pu, pe=pe)


def _pipe_run(s, scheduler, use_graph, **kw):
    from synfmc_amd.pipelines.pipeline_animation_cm_om import CameraObjCtrlPipeline
    pipe = CameraObjCtrlPipeline(None, None, None, s["pu"], scheduler, s["pe"])
    return pipe(None, s["pose_emb"].cuda(), 8, traj_features=[t.cuda() for t in s["traj"]], height=64, width=64, num_inference_steps=3,
                guidance_scale=2.0, latents=s["clip"]["latents"].cuda(), output_type="latent", prompt_embeds=s["text2"].cuda(),
                omcm_min_step=700, use_graph=use_graph, **kw).videos


@pytest.mark.parametrize("kind", ["euler", "dpm2"])
def test_pipeline_euler_and_dpm_against_the_oracle(K, stack8, kind):
    """`CameraObjCtrlPipeline`, 3 steps, CFG 2.0, fp32 storage, against `oracle.pipeline.denoise` on the oracle U-Net with the restated
    scheduler (1e-2, the bound of test_camera_obj_pipeline_12_frames); Euler with linspace spacing hands the U-Net 999, 499.5, 0.
    Measured: Euler 2.5e-5, DPM-Solver++ order 2 2.3e-5; graph and eager bit-identical."""
    from synfmc_amd import schedulers as S
    s = stack8
    ac = SC.alphas_cumprod()
    if kind == "euler":
        make, ref = (lambda: S.EulerDiscreteScheduler(**BETAS)), SC.RefEuler(ac)
    else:
        make, ref = (lambda: S.DPMSolverMultistepScheduler(solver_order=2, **BETAS)), SC.RefDPM(ac, solver_order=2)
    ref.set_timesteps(3)
    want = OP.denoise(s["ou"], ref, s["oe"], s["text2"], s["pose_emb"], s["clip"]["latents"] * ref.init_noise_sigma, num_inference_steps=3,
                      guidance_scale=2.0, traj_features=s["traj"], omcm_min_step=700)
    eager, graph = _pipe_run(s, make(), False), _pipe_run(s, make(), True)
    err = rel_inf(eager, want)
    print(f"CameraObjCtrlPipeline with {kind}: {err:.3e} against the oracle loop (bound 1e-2); graph == eager: {torch.equal(eager, graph)}")
    assert eager.shape == want.shape and err < 1e-2
    assert torch.equal(eager, graph)


def test_default_ddim_keeps_its_kernel(K, stack8, monkeypatch):
    from synfmc_amd.schedulers import DDIMScheduler
    count = {"ddim": 0, "sampler": 0}
    real_d, real_s = K.cfg_ddim_step, K.sampler_step
    monkeypatch.setattr(K, "cfg_ddim_step", lambda *a, **k: (count.__setitem__("ddim", count["ddim"] + 1), real_d(*a, **k))[1])
    monkeypatch.setattr(K, "sampler_step", lambda *a, **k: (count.__setitem__("sampler", count["sampler"] + 1), real_s(*a, **k))[1])
    sched = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    out = _pipe_run(stack8, DDIMScheduler(**sched), False)
    assert count == {"ddim": 3, "sampler": 0} and torch.isfinite(out).all()
    out = _pipe_run(stack8, DDIMScheduler(**sched), False, eta=0.5, generator=torch.Generator().manual_seed(1))
    assert count == {"ddim": 3, "sampler": 3} and torch.isfinite(out).all()

"""CPU checks of the sliding-window step: the closed form of tests/window_common.py against a literal transcription of the reference
loop, the count formula against a brute-force mask, the fp32 emulation and eleven wrong stand-ins under both instruments at every
GPU case, `step_windows` of every scheduler family, and the plumbing of both pipelines (tensor and list conditioning, chunking by
`window_batch`, the refusals) on a fake U-Net with `hip_ops.window_step` replaced by the float64 stand-in."""
import types

import numpy as np
import pytest
import torch

from tests import sampler_common as SC
from tests import window_common as WC

BETAS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


# ---- 1. the closed form and the count --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("F,overlap,W", [(4, 0, 3), (4, 1, 2), (4, 3, 5), (5, 2, 4), (16, 12, 3)])
def test_closed_form_is_the_reference_loop(R, F, overlap, W):
    """`sum_w (e_w / mask)` of the reference and `(sum_w e_w) / cnt` of the kernel: mask == cnt on every frame and the division
    distributes over the sum, so float64 evaluations differ by roundings only (1e-12)."""
    g = torch.Generator().manual_seed(F * 100 + overlap * 10 + W)
    eps = torch.randn(R, W, 2, 3, F, 5, generator=g, dtype=torch.float64)
    x = torch.randn(2, 3, WC.total_frames(F, overlap, W), 5, generator=g, dtype=torch.float64)
    want, mask = WC.reference_transcription(eps, x, overlap=overlap, guidance=7.5)
    got = WC.closed_form(eps, x, overlap=overlap, guidance=7.5, c_x=0.0, c_e=1.0)["x_out"]          # x' = e
    assert torch.equal(mask[0, 0, :, 0].long(), WC.counts(F, overlap, W))
    assert float((got[0] - want).abs().max() / want.abs().max()) < 1e-12


def test_count_formula_against_a_brute_force_mask():
    checked = 0
    for F in range(1, 7):
        for overlap in range(F):
            for W in range(1, 7):
                stride, Ftot = F - overlap, WC.total_frames(F, overlap, W)
                assert Ftot == (W - 1) * stride + F
                cover = [[w for w in range(W) if w * stride <= f < w * stride + F] for f in range(Ftot)]
                for f, ws in enumerate(cover):
                    lo, hi = WC.covering(f, F, overlap, W)
                    assert ws == list(range(lo, hi + 1)) and len(ws) >= 1, (F, overlap, W, f)
                    checked += 1
                assert WC.counts(F, overlap, W).tolist() == [len(ws) for ws in cover]
    assert checked > 1000


# ---- 2. the instruments at every GPU case ----------------------------------------------------------------------------------------
def _run(case, kind, defect=None):
    eps, x, kw = WC.make_inputs(case, kind)
    in_dt = torch.bfloat16 if case["in_bf16"] else torch.float32
    outs = WC.chain(eps, x, in_reps=case["in_reps"], in_dtype=in_dt, defect=defect, **kw)
    return outs, WC.closed_form(eps, x, **kw), in_dt


def test_case_table_reaches_every_option():
    seen = {k: {c[k] for c in WC.CASES} for k in WC.CASES[0]}
    assert seen["B"] == {1, 2} and seen["C"] == {3, 4} and seen["overlap"] == {0, 1, 2, 3} and seen["W"] == {1, 2, 3, 5}
    assert seen["hw"] == {1, 7, 8, 15, 67} and seen["in_reps"] == {0, 1, 2} and seen["n_hist"] == {0, 1, 2, 3}
    assert seen["m_mode"] == {None, "own", 0, 1, 2} and seen["layout"] == {"rw", "wr"}
    for k in ("e_bf16", "in_bf16", "cfg", "noise", "clamp", "alias_x"):
        assert seen[k] == {False, True}, k
    assert len({WC.case_id(c) for c in WC.CASES}) == len(WC.CASES) == 80


def test_fp32_emulation_meets_both_instruments():
    worst = 0.0
    for case in WC.CASES:
        outs, ref, in_dt = _run(case, "gauss")
        rat = WC.rounded_ratios(outs, ref, case, in_dt)
        worst = max(worst, *rat.values())
        assert max(rat.values()) <= 1.0, (WC.case_id(case), rat)
        outs, ref, in_dt = _run(case, "exact")
        assert WC.exact_equal(outs, ref, case, in_dt), WC.case_id(case)
    print(f"fp32 emulation over {len(WC.CASES)} cases: largest share of the bound used {worst:.3f}")


@pytest.mark.parametrize("defect", WC.DEFECTS)
def test_wrong_stand_ins_are_rejected(defect):
    cases = [c for c in WC.CASES if WC.applies(defect, c)]
    assert len(cases) >= 5, defect
    for case in cases:
        outs, ref, in_dt = _run(case, "gauss", defect)
        assert max(WC.rounded_ratios(outs, ref, case, in_dt).values()) > 1.0, ("rounded", defect, WC.case_id(case))
        outs, ref, in_dt = _run(case, "exact", defect)
        assert not WC.exact_equal(outs, ref, case, in_dt), ("exact", defect, WC.case_id(case))


def test_unwritten_x_in_is_rejected():
    case = next(c for c in WC.CASES if c["in_reps"] == 2 and c["W"] > 1)
    outs, ref, in_dt = _run(case, "gauss")
    outs["x_in"][1, -1, ..., -1] = float("nan")             # the last element of the last window of the second rep never written
    assert max(WC.rounded_ratios(outs, ref, case, in_dt).values()) > 1.0


# ---- 3. the schedulers -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def K(monkeypatch):
    import synfmc_amd.hip_ops as K
    calls = {"window_step": [], "sampler_step": [], "cfg_ddim_step": []}

    def window_step(eps, x, **kw):
        calls["window_step"].append(dict(kw, eps_shape=tuple(eps.shape)))
        return WC.standin_window_step(eps, x, **kw)

    def sampler_step(eps, x, **kw):
        calls["sampler_step"].append(kw)
        return SC.standin_sampler_step(eps, x, **kw)

    def cfg_ddim_step(*a):
        calls["cfg_ddim_step"].append(a)
        return SC.standin_cfg_ddim_step(*a)

    monkeypatch.setattr(K, "window_step", window_step)
    monkeypatch.setattr(K, "sampler_step", sampler_step)
    monkeypatch.setattr(K, "cfg_ddim_step", cfg_ddim_step)
    K._window_calls = calls
    yield K
    del K._window_calls


FAMILIES = [("ddim", dict(steps_offset=1, clip_sample=False), 0.0), ("ddim", dict(clip_sample=True, timestep_spacing="trailing"), 0.6),
            ("euler", dict(), 0.0), ("ancestral", dict(), 0.0), ("dpm", dict(solver_order=3, lower_order_final=False), 0.0)]


def _make(kind, kw):
    from synfmc_amd import schedulers as S
    cls = {"ddim": S.DDIMScheduler, "euler": S.EulerDiscreteScheduler, "ancestral": S.EulerAncestralDiscreteScheduler,
           "dpm": S.DPMSolverMultistepScheduler}[kind]
    return cls(**BETAS, **kw)


@pytest.mark.parametrize("kind,kw,eta", FAMILIES, ids=[f"{k}-{e}" for k, _, e in FAMILIES])
def test_step_windows_of_one_window_is_step_cfg(K, kind, kw, eta):
    """One window is no window: `step_windows` hands `fmc_window_step` the coefficients, the history, the noise and the next input
    scale that `step_cfg` hands `fmc_sampler_step` (the plain DDIM configuration: those of `fmc_cfg_ddim_step`)."""
    g = torch.Generator().manual_seed(3)
    z = torch.randn(1, 4, 3, 2, 2, generator=g, dtype=torch.float64)
    noises = [torch.randn(z.shape, generator=g, dtype=torch.float64) for _ in range(5)]
    a, b = _make(kind, kw), _make(kind, kw)
    a.set_timesteps(5)
    b.set_timesteps(5)
    xa = xb = z * a.init_noise_sigma
    nkw = (lambda k: {"variance_noise": noises[k]} if kind == "ddim" else {"noise": noises[k]}) if (kind == "ancestral" or eta > 0) else (lambda k: {})
    for k, t in enumerate(a._timesteps_host):
        e = torch.tanh(torch.cat([xa * 0.7, xa * 0.7 + 0.2]))
        xin_a, xin_b = torch.empty(2, *z.shape[1:], dtype=torch.float64), torch.empty(2, 1, *z.shape, dtype=torch.float64)
        fused = a.fused_input(eta)
        xa = a.step_cfg(e, t, xa, 2.0, True, **(dict(eta=eta, x_in=xin_a, **nkw(k)) if fused else {}))
        xb = b.step_windows(e.view(2, 1, *z.shape), t, xb, 2.0, 0, eta=eta, x_in=xin_b, **nkw(k))
        assert float((xa - xb).abs().max()) <= 1e-12 * float(xa.abs().max()), (kind, k)
        if fused:
            assert float((xin_a - xin_b.view(xin_a.shape)).abs().max()) <= 1e-12 * float(xin_a.abs().max())
    assert len(K._window_calls["window_step"]) == 5
    if kind == "dpm":
        assert [len(c["hist"]) for c in K._window_calls["window_step"]] == [0, 1, 2, 2, 2]


# ---- 4. the pipelines ------------------------------------------------------------------------------------------------------------
def _fake_eps(x, t, pose, traj):
    """Per sample and per frame: what a U-Net batch of windows must be indifferent to."""
    e = torch.tanh(0.7 * x + 0.3 * np.sin(float(t) / 100.0))
    if pose is not None:
        e = e + 0.1 * pose.to(e.dtype)
    if traj is not None:                                    # the OMC features reach the conditional half only
        e = torch.cat([e[:e.shape[0] - traj.shape[0]], e[e.shape[0] - traj.shape[0]:] + 0.05 * traj.to(e.dtype)])
    return e


class _FakeUNet(torch.nn.Module):
    in_channels = 4
    dtype = torch.float32

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.config = types.SimpleNamespace(sample_size=8)
        self.seen = []

    def forward(self, x, t, encoder_hidden_states=None, pose_embedding_features=None, traj_features=None):
        self.seen.append(dict(batch=x.shape[0], text=tuple(encoder_hidden_states.shape), traj=traj_features is not None, t=float(t),
                              pose=None if pose_embedding_features is None else pose_embedding_features[0].clone()))
        assert encoder_hidden_states.shape[0] == x.shape[0]
        return types.SimpleNamespace(sample=_fake_eps(x, t, None if pose_embedding_features is None else pose_embedding_features[0],
                                                      None if traj_features is None else traj_features[0]))


class _FakeEncoder(torch.nn.Module):
    """One level; a frame's feature is a function of that frame's embedding alone, so that slicing features and slicing
    embeddings agree.  Carries the positional table of the Camera Encoder's temporal blocks."""

    def __init__(self, max_len=16):
        from synfmc_amd.models.motion_module import PositionalEncoding
        super().__init__()
        self.pos = PositionalEncoding(8, max_len=max_len)

    def forward(self, emb):
        b, c, f, h, w = emb.shape
        return [emb.mean(dim=(1, 3, 4)).reshape(b * f, 1, 1, 1).expand(b * f, 4, 8, 8).contiguous()]


F1, OV = 4, 2


def _clip(W, B=1, seed=1):
    g = torch.Generator().manual_seed(seed)
    Ftot = WC.total_frames(F1, OV, W)
    return dict(lat=torch.randn(B, 4, Ftot, 8, 8, generator=g), emb=torch.randn(B, 6, Ftot, 64, 64, generator=g),
                traj=[torch.randn(B, 4, Ftot, 8, 8, generator=g)], text=torch.randn(2 * B, 77, 8, generator=g))


def _cam(scheduler, unet=None, enc=None):
    from synfmc_amd.pipelines.pipeline_animation_cm_om import CameraObjCtrlPipeline
    return CameraObjCtrlPipeline(None, None, None, unet or _FakeUNet(), scheduler, enc or _FakeEncoder())


def _call(pipe, clip, W, emb=None, traj="tensor", **kw):
    args = dict(height=64, width=64, num_inference_steps=4, guidance_scale=2.0, output_type="latent", prompt_embeds=clip["text"],
                use_graph=False, multidiff_total_steps=W, multidiff_overlaps=OV, omcm_min_step=500, latents=clip["lat"].clone())
    args.update(kw)
    tf = clip["traj"] if traj == "tensor" else traj
    return pipe(None, clip["emb"] if emb is None else emb, F1, traj_features=tf, **args).videos


def _slices(t, W):
    return [t[:, :, w * (F1 - OV):w * (F1 - OV) + F1] for w in range(W)]


def _reference_loop(clip, W, ref, n_steps=4, guidance=2.0, min_step=500):
    """The reference's loop (:679-720) in float64 with the slicing its intent implies: camera features and OMC features per window."""
    ref.set_timesteps(n_steps)
    lat = clip["lat"].double() * ref.init_noise_sigma
    feat = _FakeEncoder()(clip["emb"].double())[0]
    B = lat.shape[0]
    pose = feat.view(B, -1, 4, 8, 8).permute(0, 2, 1, 3, 4)
    for t in ref.timesteps.tolist():
        full, mask, preds = torch.zeros_like(lat), torch.zeros_like(lat), []
        for w in range(W):
            s0 = w * (F1 - OV)
            mask[:, :, s0:s0 + F1] += 1
            x = ref.scale_model_input(torch.cat([lat[:, :, s0:s0 + F1]] * 2), t)
            traj = None if t < min_step else clip["traj"][0][:, :, s0:s0 + F1].double()
            eu, ec = _fake_eps(x, t, torch.cat([pose[:, :, s0:s0 + F1]] * 2), traj).chunk(2)
            preds.append(eu + guidance * (ec - eu))
        for w, p in enumerate(preds):
            s0 = w * (F1 - OV)
            full[:, :, s0:s0 + F1] += p / mask[:, :, s0:s0 + F1]
        lat = ref.step(full, t, lat).prev_sample
    return lat


def test_camera_pipeline_runs_more_than_one_window(K):
    """Fails without the feature: the pipeline stopped at `assert multidiff_total_steps == 1`."""
    from synfmc_amd.schedulers import EulerDiscreteScheduler
    clip = _clip(2)
    out = _call(_cam(EulerDiscreteScheduler(**BETAS)), clip, 2)
    want = _reference_loop(clip, 2, SC.RefEuler(SC.alphas_cumprod()))
    err = float((out.double() - want).abs().max() / want.abs().max())
    assert out.shape == clip["lat"].shape and err < 1e-5, err                  # (the fake U-Net computes in fp32)
    assert len(K._window_calls["window_step"]) == 4 and not K._window_calls["sampler_step"] and not K._window_calls["cfg_ddim_step"]


@pytest.mark.parametrize("W", [2, 3])
def test_tensor_and_list_conditioning_agree(K, W):
    from synfmc_amd.schedulers import DDIMScheduler
    clip = _clip(W, B=2)
    sched = lambda: DDIMScheduler(steps_offset=1, clip_sample=False, **BETAS)
    a = _call(_cam(sched()), clip, W)
    b = _call(_cam(sched()), clip, W, emb=_slices(clip["emb"], W), traj=[[s] for s in _slices(clip["traj"][0], W)])
    c = _call(_cam(sched()), clip, W, emb=_slices(clip["emb"], W))
    assert torch.equal(a, b) and torch.equal(a, c)
    want = _reference_loop(clip, W, SC.RefDDIM(SC.alphas_cumprod(), steps_offset=1))
    assert float((a.double() - want).abs().max() / want.abs().max()) < 1e-5
    no_traj = _call(_cam(sched()), clip, W, traj=None)
    assert not torch.equal(a, no_traj)


@pytest.mark.parametrize("window_batch,batches", [(None, [6]), (1, [2, 2, 2]), (2, [4, 2]), (3, [6]), (7, [6])])
def test_window_batch_chunks_the_unet_calls(K, window_batch, batches):
    from synfmc_amd.schedulers import EulerDiscreteScheduler
    clip = _clip(3)
    unet = _FakeUNet()
    out = _call(_cam(EulerDiscreteScheduler(**BETAS), unet), clip, 3, window_batch=window_batch)
    base = _call(_cam(EulerDiscreteScheduler(**BETAS)), clip, 3)
    assert torch.equal(out, base)
    assert [s["batch"] for s in unet.seen] == batches * 4
    steps = [unet.seen[i * len(batches):(i + 1) * len(batches)] for i in range(4)]
    assert [s[0]["traj"] for s in steps] == [t >= 500 for t in (999, 666, 333, 0)]          # omcm_min_step, as before
    feat = _FakeEncoder()(clip["emb"])[0].view(1, -1, 4, 8, 8).permute(0, 2, 1, 3, 4)
    k0 = 0
    for call, n in zip(steps[0], batches):                  # every chunk got its own windows' camera features, [R][W_chunk][B]
        want = torch.cat([torch.cat(_slices(feat, 3)[k0:k0 + n // 2])] * 2)
        assert torch.equal(call["pose"], want) and call["text"] == (n, 77, 8)
        k0 += n // 2
    layouts = {c["eps_shape"][:2] for c in K._window_calls["window_step"]}
    assert layouts == {(2, 3)}


def test_refusals(K):
    from synfmc_amd.schedulers import EulerDiscreteScheduler
    pipe = _cam(EulerDiscreteScheduler(**BETAS))
    clip = _clip(2)
    with pytest.raises(ValueError, match="overlap"):
        _call(pipe, clip, 2, multidiff_overlaps=F1)
    with pytest.raises(ValueError, match="lists 3 windows"):
        _call(pipe, clip, 2, emb=_slices(_clip(3)["emb"], 3))
    with pytest.raises(ValueError, match="traj_features lists 1 windows"):
        _call(pipe, clip, 2, traj=[[clip["traj"][0][:, :, :F1]]])
    with pytest.raises(ValueError, match="need 6"):
        _call(pipe, clip, 2, traj=[clip["traj"][0][:, :, :5]])
    with pytest.raises(ValueError, match=r"\[B, 6, 6, H, W\]"):
        _call(pipe, clip, 2, emb=clip["emb"][:, :, :5])
    with pytest.raises(ValueError, match="window_batch"):
        _call(pipe, clip, 2, window_batch=0)
    with pytest.raises(ValueError, match="one per window"):
        _call(pipe, clip, 1, emb=[clip["emb"][:, :, :F1]], latents=clip["lat"][:, :, :F1].clone())
    with pytest.raises(ValueError, match="2 clips"):
        _call(pipe, clip, 2, latents=torch.cat([clip["lat"]] * 2), prompt_embeds=torch.cat([clip["text"]] * 2))
    short = _cam(EulerDiscreteScheduler(**BETAS), enc=_FakeEncoder(max_len=5))
    with pytest.raises(ValueError, match="positional table holds 5"):
        _call(short, clip, 2)
    out = _call(short, clip, 2, emb=_slices(clip["emb"], 2))                   # the list form has no such limit
    assert torch.equal(out, _call(pipe, clip, 2))


def test_one_window_keeps_its_path(K):
    from synfmc_amd.schedulers import EulerDiscreteScheduler
    clip = _clip(1)
    out = _call(_cam(EulerDiscreteScheduler(**BETAS)), clip, 1, window_batch=1)
    assert len(K._window_calls["sampler_step"]) == 4 and not K._window_calls["window_step"] and torch.isfinite(out).all()


def test_animation_pipeline_takes_the_new_path_only_when_asked(K):
    from synfmc_amd.pipelines.pipeline_animation_cm_om import AnimationPipeline
    from synfmc_amd.schedulers import DDIMScheduler, EulerDiscreteScheduler
    clip = _clip(3)
    for make in (lambda: EulerDiscreteScheduler(**BETAS), lambda: DDIMScheduler(steps_offset=1, clip_sample=False, **BETAS)):
        kw = dict(height=64, width=64, num_inference_steps=4, guidance_scale=2.0, output_type="latent", prompt_embeds=clip["text"], use_graph=False,
                  multidiff_total_steps=3, multidiff_overlaps=OV)
        run = lambda **k: AnimationPipeline(None, None, None, _FakeUNet(), make())(None, F1, latents=clip["lat"].clone(), **kw, **k).videos
        for c in K._window_calls.values():
            c.clear()
        old = run()
        assert not K._window_calls["window_step"] and len(K._window_calls["sampler_step"]) + len(K._window_calls["cfg_ddim_step"]) == 4
        new = [run(window_batch=wb) for wb in (None, 1, 2)]
        assert len(K._window_calls["window_step"]) == 12
        assert torch.equal(new[0], new[1]) and torch.equal(new[0], new[2])
        assert float((new[0] - old).abs().max() / old.abs().max()) < 1e-5

"""Sliding windows through `CameraObjCtrlPipeline` and `AnimationPipeline` on the GPU, on the reduced stack of tests/test_gpu_model.py
(widths 64 / 128 / 256 / 256) at 64 x 64 pixels:

  * windows that do not overlap are independent clips: bit for bit the single-window pipeline, eager and captured, bf16 and fp32;
  * 2 and 3 windows of 16 frames overlapping by 12 against a loop over the oracle U-Net, the oracle encoder and the restated DDIM
    scheduler that slices camera and OMC features as the reference's loop intends (:687-720);
  * one bf16 step against the float64 blend of the product U-Net's own per-window predictions, within the kernel's element bound;
  * no Camera-Adapter pose term is computed after the first step of a clip, with one U-Net call per window as well;
  * `AnimationPipeline(window_batch=...)` against `oracle.pipeline.denoise_plain`.
"""
import pytest
import torch
from einops import rearrange

from oracle import conditioning as OC
from oracle import diffusers_restated as OD
from oracle import pipeline as OP
from tests import common_models as CM
from tests import window_common as WC
from tests.test_gpu_kernels import rel_inf

pytestmark = pytest.mark.gpu
W4 = (64, 128, 256, 256)
BETAS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
DDIM = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
F16, OV12 = 16, 12


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def stack(K):
    """The oracle stack (Camera Encoder with a 32-entry positional table: the tensor form encodes all frames at once) and one
    24-frame clip; shorter clips are its leading frames."""
    ou, oe, oa = CM.build_oracle(W4, enc_max_len=32)
    clip = CM.synthetic_clip(B=1, Fr=24, H=64, W=64)
    with torch.no_grad():
        pose_emb = rearrange(OC.to_plucker_embedding(clip["c2w"], clip["K"], (64, 64)), "b f c h w -> b c f h w")
        traj = OC.get_traj_features(clip["infos"], clip["masks"], oa)
    g = torch.Generator().manual_seed(5)
    text2 = torch.cat([torch.randn(1, 77, 64, generator=g), clip["text"]])
    return dict(ou=ou, oe=oe, oa=oa, lat=clip["latents"], pose_emb=pose_emb, traj=traj, text2=text2, products={}, refs={})


def _product(stack, dtype):
    if dtype not in stack["products"]:
        stack["products"][dtype] = CM.build_product(stack["ou"], stack["oe"], stack["oa"], W4, dtype=dtype, enc_max_len=32)
    return stack["products"][dtype]


def _frames(stack, f0, f1):
    """Latents, embedding and OMC features of frames [f0, f1) on the device."""
    cut = lambda t: t[:, :, f0:f1].contiguous().cuda()
    return cut(stack["lat"]), cut(stack["pose_emb"]), [cut(t) for t in stack["traj"]]


def _pipe(stack, dtype, scheduler):
    from synfmc_amd.pipelines.pipeline_animation_cm_om import CameraObjCtrlPipeline
    pu, pe, _ = _product(stack, dtype)
    return CameraObjCtrlPipeline(None, None, None, pu, scheduler, pe)


def _call(pipe, stack, lat, emb, traj, frames, steps, **kw):
    dt = pipe.unet.dtype
    emb = [e.to(dt) for e in emb] if isinstance(emb, list) else emb.to(dt)
    return pipe(None, emb, frames, traj_features=traj, height=64, width=64, num_inference_steps=steps, guidance_scale=2.0, latents=lat,
                output_type="latent", prompt_embeds=stack["text2"].cuda(), omcm_min_step=700, **kw).videos.clone()


# ---- windows that do not overlap -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_disjoint_windows_are_independent_clips(K, stack, monkeypatch, dtype, use_graph):
    """Two windows of 8 frames, no overlap, list form, one window per U-Net call, Euler, 3 steps: every window's frames equal, bit
    for bit, the pipeline run on that window alone with `multidiff_total_steps=1`.  No tolerance.

    The single-window pipeline steps on `sampler_step_kernel`; hipcc contracts the `a x + b e` sums of the shared `sampler_update`
    into fma with a different product fused in `window_step_kernel`, lane by lane (measured through that kernel: rel-inf 6.0e-8 with
    bf16 storage, 1.2e-6 with fp32, after 3 steps).  `fmc_window_step` therefore runs windows that do not overlap on
    `sampler_step_kernel` itself, one launch per contiguous block (profiles/sliding_windows.md)."""
    from synfmc_amd.schedulers import EulerDiscreteScheduler
    monkeypatch.setattr(K, "DETERMINISTIC", True)
    lat, emb, traj = _frames(stack, 0, 16)
    halves = [_frames(stack, 0, 8), _frames(stack, 8, 16)]
    pipe = _pipe(stack, dtype, EulerDiscreteScheduler(**BETAS))
    out = _call(pipe, stack, lat, [h[1] for h in halves], [h[2] for h in halves], 8, 3, multidiff_total_steps=2, multidiff_overlaps=0,
                window_batch=1, use_graph=use_graph)
    assert out.shape == lat.shape and torch.isfinite(out).all()
    for w, (l, e, t) in enumerate(halves):
        alone = _call(_pipe(stack, dtype, EulerDiscreteScheduler(**BETAS)), stack, l, e, t, 8, 3, use_graph=use_graph)
        assert torch.equal(out[:, :, 8 * w:8 * w + 8], alone), (w, rel_inf(out[:, :, 8 * w:8 * w + 8], alone))
    assert not torch.equal(out[:, :, :8], out[:, :, 8:])


# ---- overlapping windows against the oracle --------------------------------------------------------------------------------------
def _oracle_windows(stack, W):
    """The reference's loop (:679-720) on the oracle U-Net, encoder and `OD.DDIMScheduler`, with `traj_features` sliced like the
    camera features (:700): 6 steps, guidance 2.0, `omcm_min_step=700`."""
    if W in stack["refs"]:
        return stack["refs"][W]
    Ftot = WC.total_frames(F16, OV12, W)
    ou, sch, g = stack["ou"], OD.DDIMScheduler(**DDIM), 2.0
    lat, emb, traj = stack["lat"][:, :, :Ftot], stack["pose_emb"][:, :, :Ftot], [t[:, :, :Ftot] for t in stack["traj"]]
    with torch.no_grad():
        sch.set_timesteps(6)
        feats = [torch.cat([rearrange(x, "(b f) c h w -> b c f h w", b=1)] * 2) for x in stack["oe"](emb)]
        traj2 = [torch.cat([torch.zeros_like(t), t]) for t in traj]
        for t in sch.timesteps:
            full, mask, preds = torch.zeros_like(lat), torch.zeros_like(lat), []
            for w in range(W):
                s0 = w * (F16 - OV12)
                mask[:, :, s0:s0 + F16] += 1
                x = sch.scale_model_input(torch.cat([lat[:, :, s0:s0 + F16]] * 2), t)
                tw = None if t < 700 else [v[:, :, s0:s0 + F16] for v in traj2]
                eu, ec = ou(x, t, encoder_hidden_states=stack["text2"], pose_embedding_features=[v[:, :, s0:s0 + F16] for v in feats],
                            traj_features=tw).sample.chunk(2)
                preds.append(eu + g * (ec - eu))
            for w, p in enumerate(preds):
                s0 = w * (F16 - OV12)
                full[:, :, s0:s0 + F16] += p / mask[:, :, s0:s0 + F16]
            lat = sch.step(full, t, lat).prev_sample
    stack["refs"][W] = lat
    return lat


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("window_batch", [None, 1], ids=["batched", "one-per-call"])
@pytest.mark.parametrize("W", [2, 3])
def test_overlapping_windows_against_the_oracle(K, stack, W, window_batch, use_graph):
    """2 and 3 windows of 16 frames overlapping by 12 (20 and 24 frames), tensor-form conditioning, fp32 parity mode, 6 DDIM steps at
    guidance 2.0 with `omcm_min_step=700`; the gate is the 1e-2 of `test_denoising_loop_cfg_omcm_gate` (same step count and
    guidance).  Measured on the MI355X: 1.36e-5 with 2 windows, 1.68e-5 - 1.74e-5 with 3, the same batched and one window per call,
    eager and captured."""
    from synfmc_amd.schedulers import DDIMScheduler
    want = _oracle_windows(stack, W)
    lat, emb, traj = _frames(stack, 0, WC.total_frames(F16, OV12, W))
    out = _call(_pipe(stack, torch.float32, DDIMScheduler(**DDIM)), stack, lat, emb, traj, F16, 6, multidiff_total_steps=W,
                multidiff_overlaps=OV12, window_batch=window_batch, use_graph=use_graph)
    err = rel_inf(out, want)
    print(f"{W} windows, window_batch={window_batch}, {'captured' if use_graph else 'eager'}: {err:.3e} against the oracle loop (gate 1e-2)")
    assert out.shape == want.shape and err < 1e-2


# ---- one step in bf16 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window_batch", [None, 1], ids=["batched", "one-per-call"])
def test_one_bf16_step_is_the_blend_of_the_unets_own_predictions(K, stack, monkeypatch, window_batch):
    """The new latents of one bf16 step lie within the kernel's element bound (tests/window_common.py) of the float64 blend of the
    per-window predictions the eager product U-Net made, and every window's next model input within its own."""
    from synfmc_amd.schedulers import EulerDiscreteScheduler
    seen = []
    real = K.window_step

    def spy(eps, x, **kw):
        seen.append((eps.clone(), x.clone(), dict(kw)))
        return real(eps, x, **kw)

    monkeypatch.setattr(K, "window_step", spy)
    lat, emb, traj = _frames(stack, 0, 20)
    out = _call(_pipe(stack, torch.bfloat16, EulerDiscreteScheduler(**BETAS)), stack, lat, emb, traj, F16, 1, multidiff_total_steps=2,
                multidiff_overlaps=OV12, window_batch=window_batch, use_graph=False)
    assert len(seen) == 1
    eps, x, kw = seen[0]
    assert eps.dtype == torch.bfloat16 and tuple(eps.shape) == (2, 2, 1, 4, 16, 8, 8) and float(eps.float().abs().max()) > 0
    x_in = kw.pop("x_in")
    flat = lambda t: t.reshape(tuple(t.shape[:-2]) + (-1,)).cpu()
    ref = WC.closed_form(flat(eps), flat(x), **kw)
    case = dict(F=F16, overlap=OV12, W=2)
    rat = WC.rounded_ratios({"x_out": flat(out), "x_in": flat(x_in)}, ref, case, torch.bfloat16)
    print(f"one bf16 step, window_batch={window_batch}: share of the bound used {rat}")
    assert max(rat.values()) <= 1.0


# ---- pose terms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("window_batch", [None, 1], ids=["batched", "one-per-call"])
def test_pose_terms_are_computed_in_the_first_step_only(K, stack, monkeypatch, window_batch, use_graph):
    """Counters of the test's own, each event with the step it happened in (the pipeline's callback moves the step on), over two
    clips through one pipeline (the second refills the runners of the first):

      pose    a `hip_ops.linear` launched inside `_PoseMerge._pose_term`: a miss of a module's per-clip pose term;
      fold    a `hip_ops.linear` launched inside `_PoseMerge._qkv_fold` outside `_pose_term`: a folded q | k | v term made anew
              (the fold is switched on for every temporal block, as in `test_pipeline_graph_reuse_across_clips`);
      refill  a `hip_ops.linear` launched inside `_GraphedUNet.set_conditioning`: the merge GEMMs and folded terms of a refill;
      runner  a call of `_GraphedUNet.set_conditioning` or `_GraphedUNet.capture` itself;
      text    a text k | v projection computed (`layers.text_kv_calls`) or refreshed (`Attention.refresh_text_kv`).

    Every event lies in step 0 of its clip, and each kind that the path can produce is seen at all.  Graph replays launch nothing
    from Python: what a captured run could do wrong after step 0 is to make, capture or refill a runner, which `runner` records."""
    from synfmc_amd.models import attention_processor as AP
    from synfmc_amd.models import layers as L
    from synfmc_amd.pipelines import pipeline_animation_cm_om as P
    from synfmc_amd.schedulers import DDIMScheduler
    monkeypatch.setattr(AP, "MERGE_FOLD_MIN_DIM", 0)
    state = {"step": 0, "pose": 0, "fold": 0, "refill": 0}
    events = []
    real_linear = K.linear

    def linear(*a, **k):
        for kind in ("pose", "fold", "refill"):             # innermost first: `_qkv_fold` calls `_pose_term`
            if state[kind]:
                events.append((kind, state["step"]))
                break
        return real_linear(*a, **k)

    def scoped(kind, real, record=None):
        def wrapper(self, *a, **k):
            if record:
                events.append((record, state["step"]))
            outer = {n: state[n] for n in ("pose", "fold", "refill")}
            state.update(pose=0, fold=0, refill=0)
            state[kind] = 1
            try:
                return real(self, *a, **k)
            finally:
                state.update(outer)
        return wrapper

    monkeypatch.setattr(K, "linear", linear)
    monkeypatch.setattr(AP._PoseMerge, "_pose_term", scoped("pose", AP._PoseMerge._pose_term))
    monkeypatch.setattr(AP._PoseMerge, "_qkv_fold", scoped("fold", AP._PoseMerge._qkv_fold))
    monkeypatch.setattr(P._GraphedUNet, "set_conditioning", scoped("refill", P._GraphedUNet.set_conditioning, "runner"))
    real_capture, real_refresh = P._GraphedUNet.capture, L.Attention.refresh_text_kv
    monkeypatch.setattr(P._GraphedUNet, "capture", lambda self: (events.append(("runner", state["step"])), real_capture(self))[1])
    monkeypatch.setattr(L.Attention, "refresh_text_kv", lambda self, *a: (events.append(("text", state["step"])), real_refresh(self, *a))[1])
    lat, emb, traj = _frames(stack, 0, 20)
    pipe = _pipe(stack, torch.bfloat16, DDIMScheduler(**DDIM))
    text_after_first = []
    for clip in range(2):
        state["step"] = 0
        first = {}

        def callback(i, t, x):
            if i == 0:
                first["text"] = L.text_kv_calls["computed"]
            state["step"] = i + 1

        n0, t0 = len(events), L.text_kv_calls["computed"]
        _call(pipe, stack, lat, emb * (1.0 + clip), traj, F16, 4, multidiff_total_steps=2, multidiff_overlaps=OV12, window_batch=window_batch,
              use_graph=use_graph, callback=callback)
        text_after_first.append(L.text_kv_calls["computed"] - first["text"])
        mine = events[n0:]
        late = sorted({e for e in mine if e[1] != 0})
        assert not late, (clip, late)
        kinds = {k for k, _ in mine}
        assert "pose" in kinds or clip == 1 and use_graph, (clip, kinds)              # (a refilled runner recomputes in `refill`)
        if use_graph:
            assert "runner" in kinds and (clip == 0 or {"refill", "text"} <= kinds), (clip, kinds)
        else:
            assert "fold" in kinds and first["text"] > t0, (clip, kinds)
    assert text_after_first == [0, 0], text_after_first
    merges = sum(m.__dict__.get("_pose_term_cache") is not None for m in pipe.unet.modules())
    folds = sum(m.__dict__.get("_qkv_fold_cache") is not None for m in pipe.unet.modules())
    assert merges > 0 and folds > 0
    if not use_graph:                                       # eager: once per module, chunk and clip, not once per step
        chunks = 1 if window_batch is None else 2
        assert sum(k == "pose" for k, _ in events) == 2 * merges * chunks, (sum(k == "pose" for k, _ in events), merges, chunks)


# ---- the plain pipeline ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window_batch", [None, 1], ids=["batched", "one-per-call"])
def test_animation_pipeline_windows_on_the_fused_step(K, window_batch):
    """`AnimationPipeline(window_batch=...)`: the case and the gate (1e-3) of `test_animation_pipeline_multidiff_windows`."""
    from synfmc_amd.pipelines.pipeline_animation import AnimationPipeline
    from synfmc_amd.schedulers import DDIMScheduler
    sched = dict(BETAS, steps_offset=1, clip_sample=False)                     # configs/lora.yaml: noise_scheduler_kwargs
    ou, pu = CM.build_lora_only(W4, 64, seed=51, fan_in_gain=0.7, device="cuda")
    g = torch.Generator().manual_seed(4)
    lat, text2 = torch.randn(1, 4, 20, 8, 8, generator=g), torch.randn(2, 77, 64, generator=g)
    ref = OP.denoise_plain(ou, OD.DDIMScheduler(**sched), text2, lat, 16, 4, 3.0, multidiff_total_steps=2, multidiff_overlaps=12)
    pipe = AnimationPipeline(None, None, None, pu, DDIMScheduler(**sched))
    out = pipe(None, 16, height=64, width=64, num_inference_steps=4, guidance_scale=3.0, latents=lat.cuda(), output_type="latent",
               prompt_embeds=text2.cuda(), multidiff_total_steps=2, multidiff_overlaps=12, window_batch=window_batch).videos
    err = rel_inf(out, ref)
    print(f"AnimationPipeline, window_batch={window_batch}: {err:.3e} against denoise_plain (gate 1e-3)")
    assert out.shape == ref.shape and err < 1e-3

"""Shared by test_window_host.py (CPU) and test_gpu_window_step.py: the float64 closed form of `fmc_window_step` with the magnitude
behind every output, the count formula, an fp32 emulation of the kernel's chain, the case table, two instruments and the wrong
stand-ins that both instruments have to reject.

Shapes.  eps and x_in are `[R, W, B, C, F, hw]` views (R: unconditional, conditional), the latents `[B, C, Ftot, hw]` with
`Ftot = (W - 1) stride + F`, `stride = F - overlap`.  Window w covers frames `[w stride, w stride + F)`; frame f is covered by
`w_lo = max(0, ceil((f - F + 1) / stride)) .. w_hi = min(W - 1, floor(f / stride))`.

The identity behind the closed form.  The reference (pipeline_animation_cm_om.py:687-720) accumulates `e_w / mask` over the windows,
mask being the number of windows over each frame; the kernel computes `(sum_w e_w) / cnt`.  `mask == cnt` on every frame (brute force
in test_window_host.py) and division by a constant distributes over the sum, so the two are the same real number; in float64 they
differ by a few 2^-53 relative, which the host test holds to 1e-12.

The bound.  The kernel (csrc/sampler_step.hip, `window_step_kernel`) computes, in fp32, at most one rounding per operation:

    e_w = eu_w + g * (ec_w - eu_w)                   3 roundings per window, in parallel chains
    e   = e_{w_lo} + ... + e_{w_hi}                  + (cnt - 1) adds
    e   = e / cnt                                    + 1                                                       -> 3 + cnt
    m   = m_x * x + m_e * e                          + 2: the product m_e * e, the sum                         -> R_M  = 5 + cnt
    acc = c_x * x + c_e * e ; acc += c_m * m         + 2 on the chain through m
    acc += c_h[j] * hist[j]  (j < 3) ; acc += c_n * noise          + 4 adds                                    -> R_X  = 11 + cnt
    x_in = in_scale * acc                            + 1                                                       -> R_IN = 12 + cnt

that is the chain of tests/sampler_common.py (5 / 11 / 12) plus `cnt`: the `cnt - 1` adds and the division.  The rest is as there:
every rounding is relative 2^-24 on a partial sum that the sum of |terms| bounds, a bf16 `x_in` adds 2^-8 |in_scale x'|, the clamp
is exact and 1-Lipschitz.  `cnt <= F` (4 in the GPU cases, so R <= 16).
"""
import itertools

import torch

from tests import sampler_common as SC

U32, BF16_REL, f32 = SC.U32, SC.BF16_REL, SC.f32


# ---- the windows -----------------------------------------------------------------------------------------------------------------
def covering(f, F, overlap, W):
    """(w_lo, w_hi) of frame f: the formula of the kernel."""
    stride = F - overlap
    return max(0, -(-(f - F + 1) // stride)), min(W - 1, f // stride)


def total_frames(F, overlap, W):
    return W * (F - overlap) + overlap


def counts(F, overlap, W):
    """cnt per frame, from the formula."""
    return torch.tensor([b - a + 1 for a, b in (covering(f, F, overlap, W) for f in range(total_frames(F, overlap, W)))])


def windows_of(full, F, overlap, W):
    """`[B, C, Ftot, hw]` -> `[W, B, C, F, hw]`: every window's own frames."""
    stride = F - overlap
    return torch.stack([full[:, :, w * stride:w * stride + F] for w in range(W)])


# ---- the float64 closed form -----------------------------------------------------------------------------------------------------
def closed_form(eps, x, *, overlap, guidance=1.0, m_x=0.0, m_e=0.0, m_clamp=0.0, c_x=1.0, c_e=0.0, c_m=0.0, c_n=0.0, c_h=(), hist=(),
                noise=None, in_scale=1.0):
    """float64, coefficients rounded to fp32 first.  Returns {name: (value, sum|terms|, cnt)} with x_out / m_out / x_in of the
    latents' shape and cnt broadcastable to it (x_in per window: `windows_of`)."""
    d = lambda t: t.detach().double().cpu()
    g, m_x, m_e, m_clamp, c_x, c_e, c_m, c_n, in_scale = (f32(v) for v in (guidance, m_x, m_e, m_clamp, c_x, c_e, c_m, c_n, in_scale))
    c_h = [f32(c) for c in c_h]
    R, W, B, C, F, hw = eps.shape
    x, e_all = d(x), d(eps)
    if R == 2:
        eu, ec = e_all[0], e_all[1]
        e_w = eu + g * ec - g * eu
        s_w = eu.abs() + abs(g) * ec.abs() + abs(g) * eu.abs()
    else:
        e_w, s_w = e_all[0], e_all[0].abs()
    stride = F - overlap
    e, s_e = torch.zeros_like(x), torch.zeros_like(x)
    for w in range(W):
        e[:, :, w * stride:w * stride + F] += e_w[w]
        s_e[:, :, w * stride:w * stride + F] += s_w[w]
    cnt = counts(F, overlap, W).double().view(1, 1, -1, 1)
    e, s_e = e / cnt, s_e / cnt
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
    return {"x_out": (xn, s_x, cnt), "m_out": (m, s_m, cnt), "x_in": (in_scale * xn, abs(in_scale) * s_x, cnt)}


def reference_transcription(eps, x, *, overlap, guidance):
    """Lines 687-720 of the reference pipeline, literally, in float64: per window the guided prediction, `mask_full` by `+= 1` on
    slices, then `noise_pred_full += noise_pred / mask`.  Returns (noise_pred_full, mask_full)."""
    R, W, B, C, F, hw = eps.shape
    latents = x.double()
    noise_pred_full = torch.zeros_like(latents)
    mask_full = torch.zeros_like(latents)
    noise_preds = []
    for multidiff_step in range(W):
        start_idx = multidiff_step * (F - overlap)
        mask_full[:, :, start_idx:start_idx + F] += 1
        noise_pred = torch.cat([eps[r, multidiff_step].double() for r in range(R)])
        if R == 2:
            noise_pred_uncond, noise_pred_text = noise_pred.chunk(2)
            noise_pred = noise_pred_uncond + guidance * (noise_pred_text - noise_pred_uncond)
        noise_preds.append(noise_pred)
    for pred_idx, noise_pred in enumerate(noise_preds):
        start_idx = pred_idx * (F - overlap)
        noise_pred_full[:, :, start_idx:start_idx + F] += noise_pred / mask_full[:, :, start_idx:start_idx + F]
    return noise_pred_full, mask_full


# ---- the chain in fp32 (or float64), frame by frame, with the defects of plausible wrong kernels ------------------------------------
DEFECTS = ("window index off by one", "last window dropped", "cnt counts windows past W", "x_in from the old latents",
           "x_in of window w written to w + 1", "uncond half of the neighbouring window", "average before the CFG combine, other window set",
           "in_scale missing on the second rep", "frame read at f_local of the wrong window", "hw runs cross into the next frame",
           "sum not divided")


def applies(defect, case):
    """Whether the defect changes the result of this case at all (a defect of the overlap needs an overlap, ...)."""
    W, ov, cfg, reps, hw = case["W"], case["overlap"], case["cfg"], case["in_reps"], case["hw"]
    return {"window index off by one": W > 1, "last window dropped": W > 1, "cnt counts windows past W": ov > 0,
            "x_in from the old latents": reps > 0, "x_in of window w written to w + 1": reps > 0 and W > 1,
            "uncond half of the neighbouring window": cfg and W > 1,
            "average before the CFG combine, other window set": cfg and W > 1 and ov > 0,
            "in_scale missing on the second rep": reps == 2, "frame read at f_local of the wrong window": W > 1 and ov > 0,
            "hw runs cross into the next frame": hw % 8 != 0 and W > 1 and ov > 0, "sum not divided": W > 1 and ov > 0}[defect]


def chain(eps, x, *, overlap, guidance=1.0, m_x=0.0, m_e=0.0, m_clamp=0.0, c_x=1.0, c_e=0.0, c_m=0.0, c_n=0.0, c_h=(), hist=(),
          noise=None, in_scale=1.0, in_reps=0, in_dtype=torch.float32, dt=torch.float32, defect=None):
    """The kernel's chain in torch ops of dtype `dt`, one rounding per operation, in the kernel's order: per frame the covering
    windows ascending, the division, then the update.  Returns x_out, m_out `[B, C, Ftot, hw]` and x_in `[in_reps, W, B, C, F, hw]`
    (NaN where nothing was written).  `defect`: one of DEFECTS."""
    t = lambda v: torch.tensor(v, dtype=dt)
    R, W, B, C, F, hw = eps.shape
    stride, Ftot = F - overlap, total_frames(F, overlap, W)
    ep, xx = eps.to(dt), x.to(dt)
    g = t(guidance)
    e = torch.zeros_like(xx)
    for f in range(Ftot):
        w_lo, w_hi = covering(f, F, overlap, W)
        cnt = w_hi - w_lo + 1
        if defect == "last window dropped":
            w_hi = min(w_hi, W - 2)
        if defect == "cnt counts windows past W":
            cnt = f // stride - w_lo + 1
        acc = su = sc = None
        for w in range(w_lo, w_hi + 1):
            fl = f - w * stride
            if defect == "frame read at f_local of the wrong window":
                fl = f - w_lo * stride
            wr = min(w + 1, W - 1) if defect == "window index off by one" else w
            eu = ep[0, wr, :, :, fl]
            if R == 2:
                ec = ep[1, wr, :, :, fl]
                if defect == "uncond half of the neighbouring window":
                    eu = ep[0, w + 1 if w + 1 < W else w - 1, :, :, fl]
                e_w = eu + g * (ec - eu)
                if defect == "average before the CFG combine, other window set":
                    wo = min(w + 1, W - 1)
                    su = eu if su is None else su + eu
                    sc = ep[1, wo, :, :, fl] if sc is None else sc + ep[1, wo, :, :, fl]
            else:
                e_w = eu
            acc = e_w if acc is None else acc + e_w
        if su is not None:
            acc = su + g * (sc - su)
        if acc is None:
            acc = torch.zeros_like(xx[:, :, f])
        e[:, :, f] = acc if (cnt == 1 or defect == "sum not divided") else acc / t(float(cnt))
    if defect == "hw runs cross into the next frame":
        e = _crossing_runs(ep, xx, overlap, g)
    m = t(m_x) * xx + t(m_e) * e
    if m_clamp > 0:
        m = torch.minimum(torch.maximum(m, t(-m_clamp)), t(m_clamp))
    acc = t(c_x) * xx + t(c_e) * e
    acc = acc + t(c_m) * m
    for c, h in zip(c_h, hist):
        acc = acc + t(c) * h.to(dt)
    if noise is not None:
        acc = acc + t(c_n) * noise.to(dt)
    out = {"x_out": acc, "m_out": m}
    if in_reps:
        src = xx if defect == "x_in from the old latents" else acc
        xi = windows_of(t(in_scale) * src, F, overlap, W)
        reps = [xi] * in_reps
        if defect == "in_scale missing on the second rep" and in_reps == 2:
            reps = [xi, windows_of(src, F, overlap, W)]
        x_in = torch.stack(reps)
        if defect == "x_in of window w written to w + 1":
            x_in = torch.roll(x_in, 1, dims=1)
        out["x_in"] = x_in.to(in_dtype)
    return out


def _crossing_runs(ep, xx, overlap, g):
    """A kernel that walks the latents in flat runs of 8 and takes the frame, the covering windows and the window addresses of a
    run's FIRST element for all 8: the elements past the end of that frame's hw read on in the window's storage."""
    R, W, B, C, F, hw = ep.shape
    stride, Ftot = F - overlap, total_frames(F, overlap, W)
    flat_e = ep.reshape(R, W, -1)
    i = torch.arange(xx.numel())
    row = (i - i % 8) // hw
    bc, f = row // Ftot, row % Ftot
    lo_hi = torch.tensor([covering(v, F, overlap, W) for v in range(Ftot)])
    w_lo, w_hi = lo_hi[f, 0], lo_hi[f, 1]
    e = torch.zeros(xx.numel(), dtype=xx.dtype)
    for w in range(W):
        at = ((bc * F + f - w * stride) * hw + (i - row * hw)).clamp(0, flat_e.shape[2] - 1)
        e_w = flat_e[0, w, at] + g * (flat_e[1, w, at] - flat_e[0, w, at]) if R == 2 else flat_e[0, w, at]
        e = torch.where((w_lo <= w) & (w <= w_hi), e + e_w, e)
    cnt = (w_hi - w_lo + 1).to(xx.dtype)
    return torch.where(cnt == 1, e, e / cnt).reshape(xx.shape)


def standin_window_step(eps, x, *, overlap, hist=(), noise=None, x_out=None, m_out=None, x_in=None, **kw):
    """`hip_ops.window_step` in plain torch, float64 arithmetic with the coefficients as given (the host tests are about the
    schedulers' float64 numbers and the pipelines' plumbing).  Honours x_out / m_out / x_in like the kernel: every input is read
    before any output is written."""
    flat = lambda t: t.reshape(tuple(t.shape[:-2]) + (-1,))
    out = chain(flat(eps), flat(x), overlap=overlap, hist=[flat(h) for h in hist], noise=None if noise is None else flat(noise),
                in_reps=0 if x_in is None else x_in.shape[0], dt=torch.float64, in_dtype=torch.float64, **kw)
    if x_out is None:
        x_out = torch.empty_like(x)
    x_out.copy_(out["x_out"].reshape(x.shape))
    if m_out is not None:
        m_out.copy_(out["m_out"].reshape(x.shape))
    if x_in is not None:
        x_in.copy_(out["x_in"].reshape(x_in.shape))
    return x_out


# ---- the two instruments ---------------------------------------------------------------------------------------------------------
R_BASE = {"x_out": SC.R_X, "m_out": SC.R_M, "x_in": SC.R_IN}          # plus cnt: see the head of this file


def bound(name, value, mag, cnt, dtype=torch.float32):
    b = (R_BASE[name] + cnt) * U32 * mag
    if dtype == torch.bfloat16:
        b = b + BF16_REL * value.abs()
    return b


def worst_ratio(got, name, value, mag, cnt, dtype=torch.float32):
    """max over elements of |got - value| / bound; NaN (an element never written) counts as infinitely wrong."""
    err = (got.detach().double().cpu() - value).abs()
    err = torch.nan_to_num(err, nan=float("inf"))
    return float((err / bound(name, value, mag, cnt, dtype).clamp_min(1e-300)).max())


def rounded_ratios(outs, ref, case, in_dtype=torch.float32):
    """Instrument 'rounded': {output: worst error / bound}; x_in per rep."""
    F, ov, W = case["F"], case["overlap"], case["W"]
    rat = {k: worst_ratio(outs[k], k, *ref[k]) for k in ("x_out", "m_out") if outs.get(k) is not None}
    if outs.get("x_in") is not None:
        v, mag, cnt = (windows_of(t.expand_as(ref["x_in"][0]), F, ov, W) for t in ref["x_in"])
        for r in range(outs["x_in"].shape[0]):
            rat[f"x_in{r}"] = worst_ratio(outs["x_in"][r], "x_in", v, mag, cnt, in_dtype)
    return rat


def exact_equal(outs, ref, case, in_dtype=torch.float32):
    """Instrument 'exact': every output equals the float64 reference bit for bit (x_in: the reference cast to its dtype, one
    rounding of an exactly representable fp32 value)."""
    F, ov, W = case["F"], case["overlap"], case["W"]
    ok = all(torch.equal(outs[k].detach().double().cpu(), ref[k][0]) for k in ("x_out", "m_out") if outs.get(k) is not None)
    if outs.get("x_in") is not None:
        want = windows_of(ref["x_in"][0], F, ov, W).float().to(in_dtype)
        ok = ok and all(torch.equal(outs["x_in"][r].detach().cpu(), want) for r in range(outs["x_in"].shape[0]))
    return ok


# ---- the cases -------------------------------------------------------------------------------------------------------------------
COEF = dict(guidance=7.5, m_x=1.31, m_e=-0.77, c_x=0.93, c_e=0.21, c_m=-0.35, c_n=0.4, in_scale=0.37)
COEF_EXACT = dict(guidance=2.0, m_x=1.0, m_e=-0.5, c_x=0.5, c_e=0.25, c_m=2.0, c_n=0.5, in_scale=0.5)      # powers of two
C_H, C_H_EXACT = [0.6, -0.45, 0.3], [1.0, -0.5, 2.0]
CLAMP, CLAMP_EXACT = 3.0, 16.0
F_GPU = 4


def _cases():
    """Every (overlap, W, hw) of the issue's table, the other options cycled over them so that each value meets many shapes:
    B, C, eps dtype, x_in dtype and reps, CFG, history length, noise, clamp, x_out aliasing x, where m_out goes, the stride layout."""
    out = []
    shapes = itertools.product((0, 1, 2, 3), (1, 2, 3, 5), (1, 7, 8, 15, 67))
    for i, (ov, W, hw) in enumerate(shapes):
        n_hist = i % 4
        m_modes = [None, "own"] + list(range(n_hist))
        out.append(dict(B=1 + i % 2, C=3 + (i // 2) % 2, F=F_GPU, overlap=ov, W=W, hw=hw, e_bf16=(i // 3) % 2 == 1, in_bf16=(i // 5) % 2 == 1,
                        in_reps=(i + i // 7) % 3, cfg=(i + i // 4) % 3 != 0, n_hist=n_hist, noise=(i // 2 + i // 9) % 2 == 1, clamp=(i // 3 + i // 11) % 2 == 1,
                        alias_x=(i + i // 5) % 2 == 1, m_mode=m_modes[(i // 4) % len(m_modes)], layout=("rw", "wr")[(i + i // 6) % 2]))
    return out


CASES = _cases()


def case_id(c):
    return (f"ov{c['overlap']}-W{c['W']}-hw{c['hw']}-B{c['B']}C{c['C']}-{'bf16' if c['e_bf16'] else 'fp32'}-in{c['in_reps']}{'bf16' if c['in_bf16'] else 'fp32'}"
            f"-{'cfg' if c['cfg'] else 'nocfg'}-h{c['n_hist']}{'-nz' if c['noise'] else ''}{'-cl' if c['clamp'] else ''}{'-ax' if c['alias_x'] else ''}"
            f"-m{c['m_mode']}-{c['layout']}")


def window_buffer(shape, dtype, layout, device="cpu", fill=None):
    """A `[R, W, B, C, F, hw]` view over `[R][W][B]...` storage ("rw": a U-Net batch of all uncond, then all cond windows) or over
    `[W][R][B]...` storage ("wr": one U-Net batch per window)."""
    R, W = shape[:2]
    store = torch.empty((R, W) + tuple(shape[2:]) if layout == "rw" else (W, R) + tuple(shape[2:]), dtype=dtype, device=device)
    if fill is not None:
        store.fill_(fill)
    return store if layout == "rw" else store.transpose(0, 1)


def make_inputs(case, kind):
    """Host inputs of one case.  kind "gauss": standard normal; "exact": integers, every eps a multiple of 12 (the sum of up to 4
    windows divides exactly by 1, 2, 3 and 4; multiples of 12 up to 96 are bf16 values), latents, history and noise small integers."""
    c = case
    g = torch.Generator().manual_seed(1000 + CASES.index(c) if c in CASES else 7)
    R, W, B, C, F, hw = (2 if c["cfg"] else 1), c["W"], c["B"], c["C"], c["F"], c["hw"]
    Ftot = total_frames(F, c["overlap"], W)
    e_dt = torch.bfloat16 if c["e_bf16"] else torch.float32
    if kind == "exact":
        r = lambda shape, lo, hi, mul: (torch.randint(lo, hi + 1, shape, generator=g) * mul).float()
        eps, x = r((R, W, B, C, F, hw), -8, 8, 12), r((B, C, Ftot, hw), -9, 9, 1)
        hist, noise = [r((B, C, Ftot, hw), -9, 9, 1) for _ in range(3)], r((B, C, Ftot, hw), -9, 9, 1)
        coef, c_h, clamp = COEF_EXACT, C_H_EXACT, CLAMP_EXACT
    else:
        r = lambda shape: torch.randn(shape, generator=g)
        eps, x = r((R, W, B, C, F, hw)), r((B, C, Ftot, hw))
        hist, noise = [r((B, C, Ftot, hw)) for _ in range(3)], r((B, C, Ftot, hw))
        coef, c_h, clamp = COEF, C_H, CLAMP
    kw = dict(coef, overlap=c["overlap"], m_clamp=clamp if c["clamp"] else 0.0, c_h=c_h[:c["n_hist"]], hist=hist[:c["n_hist"]],
              noise=noise.to(e_dt) if c["noise"] else None)
    return eps.to(e_dt), x, kw

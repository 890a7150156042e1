"""`fmc_window_step` on the GPU through the raw C ABI: every case of tests/window_common.py under both instruments (exact integer
data against the float64 closed form bit for bit; Gaussian data within the bound whose rounding count is derived at the head of
window_common.py), one window and disjoint windows against `fmc_sampler_step` bit for bit, a shape that sends the grid-stride loop on a second trip,
guarded arenas, the argument errors, and the `hip_ops.window_step` wrapper.

Shapes: F = 4, overlap 0..3 (cnt up to 4), W in {1, 2, 3, 5}, hw in {1, 7, 8, 15, 67} (below, at and above one 8-element run; odd hw
moves every stream's 16-byte alignment from row to row), B in {1, 2}, C in {3, 4}.
"""
import ctypes

import pytest
import torch

from tests import edge_guard_common as EG
from tests import window_common as WC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _coef(kw):
    from synfmc_amd._lib import SamplerCoef
    c_h = list(kw["c_h"]) + [0.0] * (3 - len(kw["c_h"]))
    return SamplerCoef(kw["guidance"], kw["m_x"], kw["m_e"], kw["m_clamp"], kw["c_x"], kw["c_e"], kw["c_m"], kw["c_n"], (ctypes.c_float * 3)(*c_h),
                       kw["in_scale"])


def _raw(K, eps, x, noise, hist, x_out, m_out, x_in, BC, F, stride, W, hw, has_uncond, in_reps, coef, e_sr=None, e_sw=None, i_sr=None, i_sw=None,
         n_hist=None, dtype=None, in_dtype=None):
    from synfmc_amd import _lib
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    h = [p(t) for t in hist] + [None] * (3 - len(hist))
    e_sr, e_sw = (eps.stride(0), eps.stride(1)) if e_sr is None else (e_sr, e_sw)
    if x_in is not None and i_sr is None:
        i_sr, i_sw = x_in.stride(0), x_in.stride(1)
    dtype = K._DT[eps.dtype] if dtype is None else dtype
    in_dtype = (K._DT[x_in.dtype] if x_in is not None else dtype) if in_dtype is None else in_dtype
    return _lib.load().fmc_window_step(p(eps), e_sr, e_sw, p(x), p(noise), h[0], h[1], h[2], p(x_out), p(m_out), p(x_in), i_sr or 0, i_sw or 0,
                                       BC, F, stride, W, hw, int(has_uncond), len(hist) if n_hist is None else n_hist, in_reps, coef, dtype,
                                       in_dtype, K._stream())


def _launch(K, case, kind):
    """One launch of a case.  Returns (outputs on the host, float64 reference, x_in dtype)."""
    c = case
    eps, x, kw = WC.make_inputs(c, kind)
    in_dt = torch.bfloat16 if c["in_bf16"] else torch.float32
    R, W, B, C, F, hw = eps.shape
    d_eps = WC.window_buffer(eps.shape, eps.dtype, c["layout"], "cuda")
    d_eps.copy_(eps)
    d_x = x.cuda()
    d_hist = [h.cuda() for h in kw["hist"]]
    d_noise = None if kw["noise"] is None else kw["noise"].cuda()
    x_out = d_x if c["alias_x"] else torch.full_like(d_x, float("nan"))
    m_out = None if c["m_mode"] is None else (torch.full_like(d_x, float("nan")) if c["m_mode"] == "own" else d_hist[c["m_mode"]])
    x_in = WC.window_buffer((c["in_reps"], W, B, C, F, hw), in_dt, c["layout"], "cuda", fill=float("nan")) if c["in_reps"] else None
    rc = _raw(K, d_eps, d_x, d_noise, d_hist, x_out, m_out, x_in, B * C, F, F - c["overlap"], W, hw, R == 2, c["in_reps"], _coef(kw))
    assert rc == 0, K._lib.load().fmc_last_error()
    torch.cuda.synchronize()
    assert torch.equal(d_eps.cpu(), eps) and (d_noise is None or torch.equal(d_noise.cpu(), kw["noise"]))         # inputs the launch must not write
    for j, h in enumerate(d_hist):
        if c["m_mode"] != j:
            assert torch.equal(h.cpu(), kw["hist"][j])
    outs = {"x_out": x_out.cpu(), "m_out": None if m_out is None else m_out.cpu(), "x_in": None if x_in is None else x_in.cpu()}
    return outs, WC.closed_form(eps, x, **kw), in_dt


@pytest.mark.parametrize("overlap", [0, 1, 2, 3])
def test_exact_integer_data(K, overlap):
    """Integer data, every eps a multiple of 12, powers of two for g and the coefficients: nothing rounds, and every output equals
    the float64 closed form bit for bit."""
    for case in [c for c in WC.CASES if c["overlap"] == overlap]:
        outs, ref, in_dt = _launch(K, case, "exact")
        assert WC.exact_equal(outs, ref, case, in_dt), WC.case_id(case)


@pytest.mark.parametrize("overlap", [0, 1, 2, 3])
def test_gaussian_data_within_the_bound(K, overlap):
    worst = {}
    for case in [c for c in WC.CASES if c["overlap"] == overlap]:
        outs, ref, in_dt = _launch(K, case, "gauss")
        for k, v in WC.rounded_ratios(outs, ref, case, in_dt).items():
            worst[k[:4]] = max(worst.get(k[:4], 0.0), v)
            assert v <= 1.0, (WC.case_id(case), k, v)
    print(f"overlap {overlap}: share of the bound used {({k: round(v, 3) for k, v in worst.items()})}")


def test_one_window_is_sampler_step_bit_for_bit(K):
    from synfmc_amd import _lib
    cases = [c for c in WC.CASES if c["W"] == 1]
    assert len(cases) == 20
    for case in cases:
        outs, _, in_dt = _launch(K, case, "gauss")
        eps, x, kw = WC.make_inputs(case, "gauss")
        n, reps = x.numel(), case["in_reps"]
        d = lambda t: None if t is None else t.cuda()
        hist = [h.cuda() for h in kw["hist"]]
        x_out, m_out = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        x_in = torch.empty(max(reps, 1) * n, dtype=in_dt, device="cuda")
        p = lambda t: None if t is None else t.data_ptr()
        h = [p(t) for t in hist] + [None] * (3 - len(hist))
        nz, d_eps, d_x = d(kw["noise"]), eps.cuda(), x.cuda()
        rc = _lib.load().fmc_sampler_step(p(d_eps), p(d_x), p(nz), h[0], h[1], h[2], p(x_out), p(m_out), p(x_in) if reps else None, n,
                                          int(case["cfg"]), len(hist), reps, _coef(kw), K._DT[eps.dtype], K._DT[in_dt], K._stream())
        assert rc == 0
        torch.cuda.synchronize()
        bits = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)
        assert torch.equal(bits(outs["x_out"].reshape(-1)), bits(x_out.cpu())), WC.case_id(case)
        if outs["m_out"] is not None:
            assert torch.equal(bits(outs["m_out"].reshape(-1)), bits(m_out.cpu())), WC.case_id(case)
        if reps:
            assert torch.equal(bits(outs["x_in"].reshape(-1)), bits(x_in.cpu())), WC.case_id(case)


@pytest.mark.parametrize("layout", ["rw", "wr"])
@pytest.mark.parametrize("e_bf16", [False, True], ids=["fp32", "bf16"])
def test_disjoint_windows_are_sampler_step_bit_for_bit(K, layout, e_bf16):
    """No overlap, three windows, F hw = 4 x 16 (the blocks keep the lanes of the 8-element runs in place): every window's frames,
    x_in and m_out equal `fmc_sampler_step` on that window's own contiguous `[B, C, F, hw]` clip bit for bit."""
    from synfmc_amd import _lib
    case = dict(B=2, C=3, F=4, overlap=0, W=3, hw=16, e_bf16=e_bf16, in_bf16=e_bf16, in_reps=2, cfg=True, n_hist=2, noise=True, clamp=True,
                alias_x=False, m_mode="own", layout=layout)
    outs, _, in_dt = _launch(K, case, "gauss")
    eps, x, kw = WC.make_inputs(case, "gauss")
    bits = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    p = lambda t: t.data_ptr()
    for w in range(3):
        cut = lambda t: t[:, :, 4 * w:4 * w + 4].contiguous().cuda()
        d_eps, d_x, d_nz, hist = eps[:, w].contiguous().cuda(), cut(x), cut(kw["noise"]), [cut(h) for h in kw["hist"]]
        n = d_x.numel()
        x_out, m_out, x_in = torch.empty_like(d_x), torch.empty_like(d_x), torch.empty(2 * n, dtype=in_dt, device="cuda")
        rc = _lib.load().fmc_sampler_step(p(d_eps), p(d_x), p(d_nz), p(hist[0]), p(hist[1]), None, p(x_out), p(m_out), p(x_in), n, 1, 2, 2,
                                          _coef(kw), K._DT[eps.dtype], K._DT[in_dt], K._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(bits(outs["x_out"][:, :, 4 * w:4 * w + 4]), bits(x_out.cpu())), w
        assert torch.equal(bits(outs["m_out"][:, :, 4 * w:4 * w + 4]), bits(m_out.cpu())), w
        assert torch.equal(bits(outs["x_in"][:, w].reshape(-1)), bits(x_in.cpu())), w


@pytest.mark.parametrize("kind", ["exact", "gauss"])
def test_second_trip_of_the_grid_stride_loop(K, kind):
    """4 x 8 rows of 65543 elements: 2 097 376 latent elements, just over `fmc_sampler_step_elems_per_trip()`, and 32 x 8194 work
    items, just over the 1024 x 256 threads of the capped grid."""
    hw = K.sampler_step_elems_per_trip() // 32 + 7
    case = dict(B=1, C=4, F=4, overlap=2, W=3, hw=hw, e_bf16=True, in_bf16=True, in_reps=2, cfg=True, n_hist=2, noise=True, clamp=True,
                alias_x=True, m_mode=1, layout="rw")
    assert 32 * hw > K.sampler_step_elems_per_trip() and 32 * ((hw + 7) // 8 + 1) > 1024 * 256
    outs, ref, in_dt = _launch(K, case, kind)
    if kind == "exact":
        assert WC.exact_equal(outs, ref, case, in_dt)
    else:
        rat = WC.rounded_ratios(outs, ref, case, in_dt)
        print(f"second trip: share of the bound used {rat}")
        assert max(rat.values()) <= 1.0


@pytest.mark.parametrize("e_bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw,overlap,W", [(15, 3, 3), (67, 1, 2)])
def test_guarded_arenas(K, hw, overlap, W, e_bf16):
    """Zeros, NaN and +Inf around every input, sentinels around every output: same bits, nothing outside written, every word of
    x_out, m_out and x_in written."""
    case = dict(B=2, C=3, F=4, overlap=overlap, W=W, hw=hw, e_bf16=e_bf16, in_bf16=e_bf16, in_reps=2, cfg=True, n_hist=3, noise=True, clamp=True,
                alias_x=False, m_mode="own", layout="rw")
    eps, x, kw = WC.make_inputs(case, "gauss")
    dt = eps.dtype
    R, _, B, C, F, _ = eps.shape
    blk, n = B * C * F * hw, x.numel()

    def fn(g):
        d_eps = g.inp(eps.reshape(-1), 1, name="eps")
        d_nz = g.inp(kw["noise"].reshape(-1), 1, name="noise")
        d_x = g.inp(x.reshape(-1), 1, name="x")
        hist = [g.inp(kw["hist"][j].reshape(-1), 1, name=f"hist{j}") for j in range(3)]
        x_out = g.out((n,), torch.float32, 1, name="x_out")
        m_out = g.out((n,), torch.float32, 1, name="m_out")
        x_in = g.out((2 * W * blk,), dt, 1, name="x_in")
        assert _raw(K, d_eps, d_x, d_nz, hist, x_out, m_out, x_in, B * C, F, F - overlap, W, hw, True, 2, _coef(kw), e_sr=W * blk, e_sw=blk,
                    i_sr=W * blk, i_sw=blk, dtype=K._DT[dt], in_dtype=K._DT[dt]) == 0
        return {"x_out": x_out, "m_out": m_out, "x_in": x_in}

    outs = EG.run_surroundings(fn, device="cuda", what=f"window_step hw={hw} ov={overlap} W={W} {dt}", sync=torch.cuda.synchronize)
    host = {"x_out": outs["x_out"].cpu().view(x.shape), "m_out": outs["m_out"].cpu().view(x.shape),
            "x_in": outs["x_in"].cpu().view(2, W, B, C, F, hw)}
    assert max(WC.rounded_ratios(host, WC.closed_form(eps, x, **kw), case, dt).values()) <= 1.0


def test_argument_errors(K):
    from synfmc_amd import _lib
    from synfmc_amd._lib import SamplerCoef
    coef = SamplerCoef(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, (ctypes.c_float * 3)(0, 0, 0), 1.0)
    BC, F, stride, W, hw = 2, 4, 2, 2, 8
    z = lambda n: torch.zeros(n, device="cuda")
    eps, x, out, xin = z(2 * W * BC * F * hw), z(BC * 6 * hw), z(BC * 6 * hw), z(2 * W * BC * F * hw)
    base = dict(eps=eps, x=x, noise=None, hist=[], x_out=out, m_out=None, x_in=None, BC=BC, F=F, stride=stride, W=W, hw=hw, has_uncond=False,
                in_reps=0, coef=coef, e_sr=W * BC * F * hw, e_sw=BC * F * hw, i_sr=W * BC * F * hw, i_sw=BC * F * hw,
                dtype=K._DT[torch.float32], in_dtype=K._DT[torch.float32])
    call = lambda **k: _raw(K, **dict(base, **k))
    assert call() == 0
    assert call(eps=None) == -5 and call(x=None) == -5 and call(x_out=None) == -5
    assert b"NULL" in _lib.load().fmc_last_error()
    assert call(n_hist=2, hist=[x]) == -5 and call(in_reps=1) == -5
    for bad in (dict(stride=0), dict(stride=-1), dict(stride=F + 1), dict(W=0), dict(F=0, stride=0), dict(hw=0), dict(BC=0),
                dict(in_reps=3, x_in=xin), dict(n_hist=4, hist=[x, x, x])):
        assert call(**bad) == -1, bad
    assert call(W=2 ** 30, stride=4) == -1                                      # more rows than one launch indexes
    assert call(dtype=7) == -2 and call(in_reps=1, x_in=xin, in_dtype=7) == -2
    assert call(x=x.data_ptr() + 2) == -3 and call(in_reps=1, x_in=xin.data_ptr() + 2) == -3
    with pytest.raises(ValueError, match="stride=0"):
        _lib.check(call(stride=0), "fmc_window_step")
    torch.cuda.synchronize()


@pytest.mark.parametrize("layout", ["rw", "wr"])
def test_wrapper_takes_both_layouts(K, layout):
    """`hip_ops.window_step` on `[R, W, B, C, F, h, w]` views: the strides come from the views."""
    case = dict(B=2, C=4, F=4, overlap=1, W=3, hw=5 * 7, e_bf16=True, in_bf16=True, in_reps=2, cfg=True, n_hist=1, noise=True, clamp=False,
                alias_x=False, m_mode="own", layout=layout)
    eps, x, kw = WC.make_inputs(case, "gauss")
    sp = lambda t: t.reshape(tuple(t.shape[:-1]) + (5, 7))
    d_eps = WC.window_buffer(sp(eps).shape, eps.dtype, layout, "cuda")
    d_eps.copy_(sp(eps))
    x_in = WC.window_buffer(sp(eps).shape, torch.bfloat16, layout, "cuda", fill=float("nan"))
    m_out = torch.empty_like(sp(x), device="cuda")
    got = K.window_step(d_eps, sp(x).cuda(), overlap=1, hist=[sp(h).cuda() for h in kw["hist"]], noise=sp(kw["noise"]).cuda(), m_out=m_out,
                        x_in=x_in, **{k: v for k, v in kw.items() if k not in ("overlap", "hist", "noise")})
    outs = {"x_out": got.cpu().reshape(x.shape), "m_out": m_out.cpu().reshape(x.shape), "x_in": x_in.cpu().reshape(eps.shape)}
    assert max(WC.rounded_ratios(outs, WC.closed_form(eps, x, **kw), case, torch.bfloat16).values()) <= 1.0
    with pytest.raises(AssertionError, match="cover"):
        K.window_step(d_eps, sp(x).cuda()[:, :, :-1].contiguous(), overlap=1)
    with pytest.raises(ValueError, match="overlap"):
        K.window_step(d_eps, sp(x).cuda(), overlap=4)

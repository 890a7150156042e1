"""The MXFP8 kernels of csrc/gemm_mxfp8.hip through the raw C ABI: `fmc_layernorm_mxfp8_fwd`, `fmc_mxfp8_pack_weight`, `fmc_linear_mxfp8`.

Every case runs inside the arenas of tests/edge_guard_common.py: zeros, the all-ones pattern (a NaN in e4m3, E8M0, bf16 and fp32 alike) and +Inf around every
input, sentinels around every output, the scale arrays included; the outputs must be finite, bit-identical across the three runs and written nowhere
outside (a byte output may legitimately hold the sentinel's value 0x5A, so "written everywhere inside" is asserted for the bf16 output only; inside a
byte output the comparison with the reference covers every element).  What is asserted on the values:

  quantisers   gamma == NULL: the bytes and scales of the reference quantiser (tests/mxfp8_common.py) bit for bit; with LayerNorm: `assert_ln_mx_close`
               against the float64 chain (its bound and the cap on differing bytes are derived in mxfp8_common / profiles/mxfp8_ff.md);
  GEMM, exact  integer operands (each exact in e4m3 under its block scale, block scales 1, 2, 4 mixed so that a scale taken from the wrong block or lane
               shows; every product exact; sum |terms| < 2^24 asserted): the bf16 output equals the float64 product rounded once, bit for bit, with bias
               and residual; the GEGLU form with zero gate weights and gate biases 0 or 16 .. 24, where `fmc_gelu_fast` is exact (0, and g itself):
               bytes and scales equal the reference quantiser of the exact product.  B is random, hence asymmetric.  This is also what catches a
               relapse of the accumulator-read hazard (MX_SETTLE in the kernel);
  GEMM, Gauss  float64 on the dequantised operands: `assert_bf16_close` for the bf16 output, `assert_mx_close` for the MXFP8 output.

Tiles: a workgroup computes TILE_M = 128 token rows x TILE_N = 128 weight rows (asserted against the library).  M = 1, 127 and 129 are one row, one row less
than a tile and one more; 293 = two tiles and 37 rows.  N = 64 / 320 leave half a column tile past the end of the weight; K = 64 is one k-step (less than
the ring's depth), 320 five, 1280 twenty (the ring wraps five times)."""
import pytest
import torch

from tests import edge_guard_common as EG
from tests import mxfp8_common as MX
from tests.conv_fwd_common import assert_bf16_close
from tests.test_gpu_edge_guards import _call, _p, _rnd, _vec_band

pytestmark = pytest.mark.gpu

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
BAND = 160                                   # rows of guard around row-major operands: more than one 128-row tile
M_CASES = [1, MX.TILE_M - 1, MX.TILE_M + 1, 2 * MX.TILE_M + 37]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    lib = hip_ops._lib.load()
    assert (lib.fmc_mxfp8_tile_rows(), lib.fmc_mxfp8_tile_cols()) == (MX.TILE_M, MX.TILE_N)
    return hip_ops


def _run(fn, what):
    return EG.run_surroundings(fn, "cuda", what, torch.cuda.synchronize)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _quant_input(M, C, seed):
    """bf16 rows with blocks of every kind: Gaussian at mixed magnitudes, an amax that is a power of two, values that saturate (scaled amax > 448), zeros."""
    g = _gen(seed)
    x = torch.randn(M, C, generator=g) * torch.exp2(torch.randint(-12, 12, (M, C // 32), generator=g).float()).repeat_interleave(32, 1)
    x[0, :32] = 0.0                                                           # an all-zero block
    x[0, 32:64] = torch.randn(32, generator=g).clamp(-1, 1) * 0.5
    x[0, 40] = 4.0                                                            # amax a power of two
    x[-1, -32:] = torch.randn(32, generator=g).clamp(-1, 1)
    x[-1, -1] = 1.98                                                          # scaled to 506.9: saturates to 448
    x[-1, -2] = -1.8                                                          # scaled to -460.8: saturates too
    return x.to(BF16)


# =====================================================================================================================================
# quantisers
# =====================================================================================================================================
@pytest.mark.parametrize("col_pad", [0, 64])
@pytest.mark.parametrize("C", [64, 320, 1280])
@pytest.mark.parametrize("M", [1, 33])
def test_quantize_rows_equals_the_reference_bit_for_bit(K, M, C, col_pad):
    what = f"quantise rows M {M} C {C} row stride {C + col_pad}"
    h = _quant_input(M, C, 7 * M + C)

    def fn(g):
        hd = g.inp(h, 8, col_pad, "h")
        xq, xs = g.out((M, C), U8, 8, 0, "xq", written=False), g.out((M, C // 32), U8, 64, 0, "xs", written=False)
        _call(K, "fmc_layernorm_mxfp8_fwd", hd.data_ptr(), None, None, xq.data_ptr(), xs.data_ptr(), M, C, C + col_pad, 1e-5, K._stream())
        return {"xq": xq, "xs": xs}
    got = _run(fn, what)
    rq, rs = MX.quantize(h)
    assert torch.equal(got["xs"].cpu(), rs), f"{what}: {int((got['xs'].cpu() != rs).sum())} scale bytes differ from the reference quantiser"
    assert torch.equal(got["xq"].cpu(), rq), f"{what}: {int((got['xq'].cpu() != rq).sum())} element bytes differ from the reference quantiser"
    assert int((MX.decode_e4m3(rq).abs() == 448).sum()) >= 2 and int((rs == 0).sum()) >= 1      # the saturated elements and the zero block are in the data
    wq, ws = K.layernorm_mxfp8(h.cuda(), None, None)                          # the wrapper: the same bytes
    assert torch.equal(wq.cpu(), rq) and torch.equal(ws.cpu(), rs)


@pytest.mark.parametrize("col_pad", [0, 64])
@pytest.mark.parametrize("C", [64, 320, 1280])
@pytest.mark.parametrize("M", [1, 33])
def test_layernorm_mxfp8_against_the_float64_chain(K, M, C, col_pad):
    what = f"layernorm + quantise M {M} C {C} row stride {C + col_pad}"
    h = _rnd((M, C), 11 + M + C, BF16, 1.5, 0.2)
    gamma, beta = _rnd((C,), 2, F32, 0.3, 1.0), _rnd((C,), 3, F32, 0.2)

    def fn(g):
        hd = g.inp(h, 8, col_pad, "h")
        gd, bd = g.inp(gamma, _vec_band(C), 0, "gamma"), g.inp(beta, _vec_band(C), 0, "beta")
        xq, xs = g.out((M, C), U8, 8, 0, "xq", written=False), g.out((M, C // 32), U8, 64, 0, "xs", written=False)
        _call(K, "fmc_layernorm_mxfp8_fwd", hd.data_ptr(), gd.data_ptr(), bd.data_ptr(), xq.data_ptr(), xs.data_ptr(), M, C, C + col_pad, 1e-5, K._stream())
        return {"xq": xq, "xs": xs}
    got = _run(fn, what)
    worst, share = MX.assert_ln_mx_close(got["xq"], got["xs"], h, gamma, beta, 1e-5, what)
    print(f"   {what}: worst err / bound {worst:.3f}, {share:.5f} of the bytes differ from the float64 chain (cap {MX.LN_DIFF_SHARE})")
    wq, ws = K.layernorm_mxfp8(h.cuda(), gamma.cuda(), beta.cuda(), 1e-5)
    assert torch.equal(wq.cpu(), got["xq"].cpu()) and torch.equal(ws.cpu(), got["xs"].cpu())


@pytest.mark.parametrize("geglu", [False, True])
@pytest.mark.parametrize("N,Kd", [(128, 64), (320, 320)])
def test_pack_weight_equals_the_reference_bit_for_bit(K, N, Kd, geglu):
    rows = 2 * N if geglu else N
    what = f"pack weight [{rows}, {Kd}] geglu {geglu}"
    w = _rnd((rows, Kd), 5, BF16, Kd ** -0.5)

    def fn(g):
        wd = g.inp(w, 8, 0, "w")
        wq, ws = g.out((rows, Kd), U8, 8, 0, "wq", written=False), g.out((rows, Kd // 32), U8, 64, 0, "ws", written=False)
        _call(K, "fmc_mxfp8_pack_weight", wd.data_ptr(), wq.data_ptr(), ws.data_ptr(), rows, Kd, N if geglu else 0, K._stream())
        return {"wq": wq, "ws": ws}
    got = _run(fn, what)
    rq, rs = MX.quantize(w[MX.geglu_pack_rows(N)] if geglu else w)
    assert torch.equal(got["wq"].cpu(), rq) and torch.equal(got["ws"].cpu(), rs), what
    pq, ps = K.mxfp8_pack_weight(w.cuda(), geglu=geglu)
    assert torch.equal(pq.cpu(), rq) and torch.equal(ps.cpu(), rs)


# =====================================================================================================================================
# the GEMM
# =====================================================================================================================================
def _launch(K, g, xq, xs, wq, ws, bias, res, M, N, Kd, geglu):
    """One guarded launch: every operand in an arena, outputs (and the scale output) in sentinel arenas."""
    xqd, xsd = g.inp(xq, BAND, 0, "xq"), g.inp(xs, BAND, 0, "xs")
    wqd, wsd = g.inp(wq, BAND, 0, "wq"), g.inp(ws, BAND, 0, "ws")
    bd = None if bias is None else g.inp(bias, _vec_band(bias.numel()), 0, "bias")
    if geglu:
        oq, osc = g.out((M, N), U8, BAND, 0, "oq", written=False), g.out((M, N // 32), U8, BAND, 0, "os", written=False)
        _call(K, "fmc_linear_mxfp8", xqd.data_ptr(), xsd.data_ptr(), wqd.data_ptr(), wsd.data_ptr(), _p(bd), None, oq.data_ptr(), osc.data_ptr(), M, N, Kd, 0, 0, 1,
              K._stream())
        return {"oq": oq, "os": osc}
    rd = None if res is None else g.inp(res, BAND, 8, "residual")
    out = g.out((M, N), BF16, BAND, 8, "out")
    _call(K, "fmc_linear_mxfp8", xqd.data_ptr(), xsd.data_ptr(), wqd.data_ptr(), wsd.data_ptr(), _p(bd), _p(rd), out.data_ptr(), None, M, N, Kd,
          N + 8 if res is not None else 0, N + 8, 0, K._stream())
    return {"out": out}


def _int_operand(rows, Kd, seed):
    """Integers in [-8, 8] times a block factor 1, 2 or 4: exact in e4m3 under the block's scale, the scale bytes of neighbouring blocks differ."""
    g = _gen(seed)
    v = torch.randint(-8, 9, (rows, Kd), generator=g).double()
    f = torch.exp2(torch.randint(0, 3, (rows, Kd // 32), generator=g).double()).repeat_interleave(32, 1)
    q, s = MX.quantize(v * f)
    assert torch.equal(MX.dequantize(q, s), v * f)
    return q, s


@pytest.mark.parametrize("N,Kd", [(64, 64), (320, 320), (64, 1280), (320, 64)])
@pytest.mark.parametrize("M", M_CASES)
def test_linear_mxfp8_exact_integers(K, M, N, Kd):
    what = f"linear_mxfp8 exact M {M} N {N} K {Kd}"
    (xq, xs), (wq, ws) = _int_operand(M, Kd, 1 + M), _int_operand(N, Kd, 2 + N + Kd)
    g = _gen(3)
    bias = torch.randint(-8, 9, (N,), generator=g).to(BF16)
    res = torch.randint(-64, 65, (M, N), generator=g).to(BF16)
    ref, mag = MX.linear_reference(xq, xs, wq, ws, bias, res)
    assert float(mag.max()) < 2 ** 24
    got = _run(lambda gd: _launch(K, gd, xq, xs, wq, ws, bias, res, M, N, Kd, False), what)["out"].cpu()
    want = ref.to(BF16)                                                       # (integers below 2^24: float64 -> bf16 is ONE rounding)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (
        f"{what}: {int((got != want).sum())} / {got.numel()} elements differ from the float64 product rounded once, first at {tuple((got != want).nonzero()[0].tolist())}")
    plain = _run(lambda gd: _launch(K, gd, xq, xs, wq, ws, None, None, M, N, Kd, False), what + " no bias / residual")["out"].cpu()
    assert torch.equal(plain, MX.linear_reference(xq, xs, wq, ws)[0].to(BF16)), what + " no bias / residual"


@pytest.mark.parametrize("inner,Kd", [(64, 64), (64, 320), (1280, 64)])
@pytest.mark.parametrize("M", M_CASES)
def test_geglu_mxfp8_exact_integers(K, M, inner, Kd):
    what = f"geglu_mxfp8 exact M {M} inner {inner} K {Kd}"
    xq, xs = _int_operand(M, Kd, 4 + M)
    vq, vs = _int_operand(inner, Kd, 5 + inner + Kd)
    wq, ws = torch.cat([vq, torch.zeros_like(vq)]), torch.cat([vs, torch.zeros_like(vs)])          # gate rows zero: the gate is its bias
    g = _gen(6)
    gate = torch.randint(15, 25, (inner,), generator=g).double()
    gate[gate == 15] = 0                                                      # 0, or 16 .. 24: fmc_gelu_fast returns 0 resp. g itself
    bias = torch.cat([torch.randint(-8, 9, (inner,), generator=g).double(), gate]).to(BF16)
    y = (MX.dequantize(xq, xs) @ MX.dequantize(vq, vs).T + bias[:inner].double()) * gate
    assert float((MX.dequantize(xq, xs).abs() @ MX.dequantize(vq, vs).abs().T + 8).max() * 24) < 2 ** 24
    assert torch.equal(MX.gelu_fast(gate.float()).double(), gate)             # (the emulation of the function agrees that it is exact there)
    perm = MX.geglu_pack_rows(inner)
    got = _run(lambda gd: _launch(K, gd, xq, xs, wq[perm], ws[perm], bias, None, M, inner, Kd, True), what)
    rq, rs = MX.quantize(y)
    assert torch.equal(got["os"].cpu(), rs), f"{what}: {int((got['os'].cpu() != rs).sum())} / {rs.numel()} scale bytes differ from the reference quantiser of the exact product"
    assert torch.equal(got["oq"].cpu(), rq), f"{what}: {int((got['oq'].cpu() != rq).sum())} / {rq.numel()} bytes differ, first at {tuple((got['oq'].cpu() != rq).nonzero()[0].tolist())}"


def _gauss_operand(rows, Kd, seed, scale):
    return MX.quantize(_rnd((rows, Kd), seed, BF16, scale))


@pytest.mark.parametrize("N,Kd", [(64, 64), (320, 320), (320, 1280), (64, 320)])
@pytest.mark.parametrize("M", M_CASES)
def test_linear_mxfp8_gaussian(K, M, N, Kd):
    what = f"linear_mxfp8 M {M} N {N} K {Kd}"
    (xq, xs), (wq, ws) = _gauss_operand(M, Kd, 21 + M, 1.0), _gauss_operand(N, Kd, 22 + N + Kd, Kd ** -0.5)
    bias, res = _rnd((N,), 23, BF16, 0.3), _rnd((M, N), 24, BF16, 1.0)
    got = _run(lambda gd: _launch(K, gd, xq, xs, wq, ws, bias, res, M, N, Kd, False), what)["out"]
    ref, mag = MX.linear_reference(xq, xs, wq, ws, bias, res)
    print(f"   {what}: worst err / bound {assert_bf16_close(got, ref, mag, what):.3f}")
    wrapped = K.linear_mxfp8(xq.cuda(), xs.cuda(), wq.cuda(), ws.cuda(), bias.cuda(), res.cuda())
    assert torch.equal(wrapped.cpu(), got.cpu()), f"{what}: the wrapper's bits differ from the raw ABI's"


@pytest.mark.parametrize("inner,Kd", [(64, 64), (1280, 320), (64, 1280)])
@pytest.mark.parametrize("M", M_CASES)
def test_geglu_mxfp8_gaussian(K, M, inner, Kd):
    what = f"geglu_mxfp8 M {M} inner {inner} K {Kd}"
    (xq, xs), (wq, ws) = _gauss_operand(M, Kd, 31 + M, 1.0), _gauss_operand(2 * inner, Kd, 32 + inner + Kd, Kd ** -0.5)
    bias = _rnd((2 * inner,), 33, BF16, 0.3)
    perm = MX.geglu_pack_rows(inner)
    got = _run(lambda gd: _launch(K, gd, xq, xs, wq[perm], ws[perm], bias, None, M, inner, Kd, True), what)
    ref, F = MX.geglu_reference(xq, xs, wq, ws, bias, inner)
    print(f"   {what}: worst err / bound {MX.assert_mx_close(got['oq'], got['os'], ref, F, what):.3f}")
    oq, osc = K.linear_mxfp8(xq.cuda(), xs.cuda(), wq[perm].cuda(), ws[perm].cuda(), bias.cuda(), geglu=True)
    assert torch.equal(oq.cpu(), got["oq"].cpu()) and torch.equal(osc.cpu(), got["os"].cpu()), f"{what}: the wrapper's bits differ from the raw ABI's"


# =====================================================================================================================================
# refusals
# =====================================================================================================================================
@pytest.mark.parametrize("case", ["K = 96", "N = 32", "misaligned"])
def test_linear_mxfp8_refuses_and_writes_nothing(K, case):
    M, N, Kd = 33, (32 if case == "N = 32" else 64), (96 if case == "K = 96" else 64)
    lib = K._lib.load()
    assert bool(lib.fmc_linear_mxfp8_supported(M, 64, 64, 0)) and K.mxfp8_supported(M, 64, 64, False)
    if case != "misaligned":
        assert not lib.fmc_linear_mxfp8_supported(M, N, Kd, 0) and not K.mxfp8_supported(M, N, Kd, False)
        assert not lib.fmc_linear_mxfp8_supported(M, N, Kd, 1) and not K.mxfp8_supported(M, N, Kd, True)
    g = EG.Guard("zeros", "cuda")
    xq, xs = g.inp(torch.zeros(M, Kd, dtype=U8), 8, 0, "xq"), g.inp(torch.zeros(M, 4, dtype=U8), 8, 0, "xs")
    wq, ws = g.inp(torch.zeros(N, Kd, dtype=U8), 8, 0, "wq"), g.inp(torch.zeros(N, 4, dtype=U8), 8, 0, "ws")
    out, osc = g.out((M, N), BF16, 8, 0, "out", written=False), g.out((M, 4), U8, 8, 0, "os", written=False)
    off = 1 if case == "misaligned" else 0
    for geglu in (0, 1):
        with pytest.raises(ValueError):
            _call(K, "fmc_linear_mxfp8", xq.data_ptr() + off, xs.data_ptr(), wq.data_ptr(), ws.data_ptr(), None, None, out.data_ptr(), osc.data_ptr(), M,
                  N // 2 if geglu else N, Kd, 0, N, geglu, K._stream())
    torch.cuda.synchronize()
    g.check(case)
    for name, arena, view, _ in g.outputs:                                  # nothing was written inside either
        assert bool((EG._bits(arena) == EG.SENTINEL[arena.dtype][1]).all()), f"{case}: {name} was written"

"""MXFP8 on the CPU (no GPU code runs): the reference quantiser of tests/mxfp8_common.py, the plain-torch emulations of the kernels' rounding chains against
the bounds that tests/test_gpu_mxfp8.py applies (at that file's shapes), wrong stand-ins that those assertions must reject, and the dispatch of
`FeedForward.forward_ln` under `hip_ops.FP8_FF` with tests/fake_kernels.py."""
import pytest
import torch

from tests import edge_guard_common as EG
from tests import fake_kernels
from tests import mxfp8_common as MX
from tests.conv_fwd_common import assert_bf16_close

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
M_CASES = [1, MX.TILE_M - 1, MX.TILE_M + 1, 2 * MX.TILE_M + 37]


def _rnd(shape, seed, dtype, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift).to(dtype)


# =====================================================================================================================================
# 1. the reference quantiser
# =====================================================================================================================================
def test_e4m3_codec_round_trips_every_finite_byte_and_agrees_with_torch():
    b = torch.arange(256, dtype=U8)
    b = b[(b & 0x7F) != 0x7F]
    v = MX.decode_e4m3(b)
    assert torch.equal(MX.encode_e4m3(v), b) and float(v.abs().max()) == 448.0
    assert torch.equal(v.float(), b.view(torch.float8_e4m3fn).float())
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)).double() * 100
    mine = MX.encode_e4m3(MX.round_e4m3(x))
    assert torch.equal(mine, x.clamp(-448, 448).float().to(torch.float8_e4m3fn).view(U8))     # (clamp first: torch's cast does not saturate)


def test_quantiser_is_exact_on_integers_under_mixed_block_scales():
    g = torch.Generator().manual_seed(1)
    v = torch.randint(-8, 9, (37, 320), generator=g).double() * torch.exp2(torch.randint(0, 3, (37, 10), generator=g).double()).repeat_interleave(32, 1)
    q, s = MX.quantize(v)
    assert torch.equal(MX.dequantize(q, s), v)
    assert len(set(s.flatten().tolist())) >= 3


def test_quantiser_is_idempotent():
    x = _rnd((33, 320), 2, BF16, 3.0)
    q, s = MX.quantize(x)
    q2, s2 = MX.quantize(MX.dequantize(q, s))
    assert torch.equal(q, q2) and torch.equal(s, s2)


def test_quantiser_saturates_power_of_two_and_zero_blocks():
    x = torch.zeros(1, 96, dtype=torch.float64)
    x[0, 0], x[0, 1], x[0, 2] = 1.98, -1.8, 1.0             # scaled by 2^8: 506.9 and -460.8 saturate, 256 stays
    x[0, 32], x[0, 33] = 4.0, 3.9                            # amax a power of two: e = 2 - 8, scaled amax exactly 256
    q, s = MX.quantize(x)
    d = MX.dequantize(q, s)
    assert s.tolist() == [[127 - 8, 127 + 2 - 8, 0]]
    assert d[0, :3].tolist() == [448 / 256, -448 / 256, 1.0]
    assert float(d[0, 32]) == 4.0 and abs(float(d[0, 33]) - 3.9) <= 0.5 * 16 / 64 and torch.equal(q[0, 64:], torch.zeros(32, dtype=U8))
    tiny = torch.full((1, 32), 2.0 ** -130, dtype=torch.float64)          # below the E8M0 range: byte 0, elements flush
    assert MX.quantize(tiny)[1].tolist() == [[0]]


# =====================================================================================================================================
# 2. the emulations meet the bounds of the GPU tests, at their shapes
# =====================================================================================================================================
def _gauss(rows, Kd, seed, scale):
    return MX.quantize(_rnd((rows, Kd), seed, BF16, scale))


@pytest.mark.parametrize("N,Kd", [(64, 64), (320, 320), (320, 1280), (64, 320)])
@pytest.mark.parametrize("M", M_CASES)
def test_linear_emulation_meets_the_bf16_bound(M, N, Kd):
    (xq, xs), (wq, ws) = _gauss(M, Kd, 21 + M, 1.0), _gauss(N, Kd, 22 + N + Kd, Kd ** -0.5)
    bias, res = _rnd((N,), 23, BF16, 0.3), _rnd((M, N), 24, BF16, 1.0)
    ref, mag = MX.linear_reference(xq, xs, wq, ws, bias, res)
    assert assert_bf16_close(MX.emulate_linear(xq, xs, wq, ws, bias, res), ref, mag) <= 1.0


def _geglu_case(M, inner, Kd):
    (xq, xs), (wq, ws) = _gauss(M, Kd, 31 + M, 1.0), _gauss(2 * inner, Kd, 32 + inner + Kd, Kd ** -0.5)
    bias = _rnd((2 * inner,), 33, BF16, 0.3)
    return xq, xs, wq, ws, bias, MX.geglu_reference(xq, xs, wq, ws, bias, inner)


@pytest.mark.parametrize("inner,Kd", [(64, 64), (1280, 320), (64, 1280)])
@pytest.mark.parametrize("M", M_CASES)
def test_geglu_emulation_meets_the_mxfp8_bound(M, inner, Kd):
    xq, xs, wq, ws, bias, (ref, F) = _geglu_case(M, inner, Kd)
    oq, osc = MX.emulate_geglu(xq, xs, wq, ws, bias, inner)
    assert MX.assert_mx_close(oq, osc, ref, F) <= 1.0


@pytest.mark.parametrize("C", [64, 320, 1280])
@pytest.mark.parametrize("M", [1, 33])
def test_layernorm_emulation_meets_the_bound_and_the_cap(M, C):
    h = _rnd((M, C), 11 + M + C, BF16, 1.5, 0.2)
    gamma, beta = _rnd((C,), 2, F32, 0.3, 1.0), _rnd((C,), 3, F32, 0.2)
    q, s = MX.emulate_layernorm_mxfp8(h, gamma, beta, 1e-5)
    worst, share = MX.assert_ln_mx_close(q, s, h, gamma, beta, 1e-5)
    assert worst <= 1.0 and share <= MX.LN_DIFF_SHARE / 2               # the emulation alone stays well inside the cap


def test_geglu_pack_rows_is_the_value_gate_interleave():
    p = MX.geglu_pack_rows(128)
    assert sorted(p.tolist()) == list(range(256))
    assert p[:32].tolist() == list(range(32)) and p[32:64].tolist() == list(range(128, 160)) and p[64:96].tolist() == list(range(32, 64))


# =====================================================================================================================================
# 3. wrong stand-ins are rejected by the assertions of the GPU tests
# =====================================================================================================================================
def _int_operand(rows, Kd, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-8, 9, (rows, Kd), generator=g).double() * torch.exp2(torch.randint(0, 3, (rows, Kd // 32), generator=g).double()).repeat_interleave(32, 1)
    return MX.quantize(v)


def _exact_fails(got, xq, xs, wq, ws):
    want = MX.linear_reference(xq, xs, wq, ws)[0].to(BF16)
    return not torch.equal(got.to(BF16), want)


def test_right_standins_pass():
    (xq, xs), (wq, ws) = _int_operand(33, 320, 1), _int_operand(64, 320, 2)
    assert not _exact_fails(MX.emulate_linear(xq, xs, wq, ws), xq, xs, wq, ws)


def test_scale_per_16_elements_is_caught_by_the_quantiser_comparison():
    x = _rnd((33, 320), 3, BF16, 2.0)
    q, s = MX.quantize(x)
    q16, s16 = MX.quantize(x, block=16)
    assert not torch.equal(q, q16)


@pytest.mark.parametrize("kind", ["truncation", "no saturation"])
def test_wrong_rounding_is_caught_by_the_quantiser_comparison(kind):
    x = _rnd((33, 320), 4, BF16, 2.0)
    x[0, 0] = 1.98 * 2.0 ** torch.floor(torch.log2(x[0, :32].float().abs().max())).item()       # 1.98 x the block's binade: scaled to 506.9, saturates
    q, s = MX.quantize(x)
    qw, sw = MX.quantize(x, mode="floor") if kind == "truncation" else MX.quantize(x, saturate=False)
    assert torch.equal(s, sw) and not torch.equal(q, qw)


def test_value_and_gate_swapped_is_caught():
    xq, xs, wq, ws, bias, (ref, F) = _geglu_case(33, 64, 64)
    oq, osc = MX.emulate_geglu(xq, xs, wq, ws, bias, 64, swap=True)
    with pytest.raises(AssertionError):
        MX.assert_mx_close(oq, osc, ref, F)


def test_scale_of_the_neighbouring_k_block_is_caught_by_the_exact_test():
    (xq, xs), (wq, ws) = _int_operand(33, 320, 1), _int_operand(64, 320, 2)
    assert _exact_fails(MX.emulate_linear(xq, xs.roll(1, -1), wq, ws), xq, xs, wq, ws)
    assert _exact_fails(MX.emulate_linear(xq, xs, wq, ws.roll(1, -1)), xq, xs, wq, ws)


def test_permuted_k_order_inside_a_lane_is_caught_by_the_exact_test():
    (xq, xs), (wq, ws) = _int_operand(33, 320, 1), _int_operand(64, 320, 2)
    perm = torch.arange(320).reshape(10, 32)[:, torch.cat([torch.arange(16, 32), torch.arange(16)])].reshape(-1)       # the halves of every block swapped, A only
    assert _exact_fails(MX.emulate_linear(xq[:, perm], xs, wq, ws), xq, xs, wq, ws)


def test_a_whole_block_per_lane_is_caught_by_the_exact_test():
    """The lane map a first design assumed (lane half h holds k = 32 h .. 32 h + 31): the instruction then takes the 16-byte chunks 1 and 2 of every 64-deep
    k-step for each other's scale block, in both operands -- every dot product is the same sum, under the wrong scales."""
    (xq, xs), (wq, ws) = _int_operand(33, 320, 1), _int_operand(64, 320, 2)
    perm = torch.arange(320).reshape(5, 4, 16)[:, [0, 2, 1, 3]].reshape(-1)
    assert not _exact_fails(MX.emulate_linear(xq[:, perm], xs, wq[:, perm], ws), xq[:, perm], xs, wq[:, perm], ws)   # (a relabelled k is still a right product)
    got = (MX.dequantize(xq[:, perm], xs).float() @ MX.dequantize(wq[:, perm], ws).float().T).bfloat16()
    assert _exact_fails(got, xq, xs, wq, ws)


def test_a_row_past_m_stored_is_seen_by_the_sentinels():
    M, N = 33, 64
    g = EG.Guard("zeros")
    out = g.out((M, N), BF16, 160, 8, "out")
    out.copy_(torch.zeros(M, N, dtype=BF16))
    g.check("right")
    g.outputs[0][1][(out.data_ptr() - g.outputs[0][1].data_ptr()) // 2 + M * (N + 8)] = 1.0                         # row M, column 0
    with pytest.raises(EG.OutsideTouched):
        g.check("row past M")
    s = EG.Guard("zeros")                                                   # the scale array likewise
    osc = s.out((M, 2), U8, 160, 0, "os")
    osc.fill_(127)
    s.outputs[0][1][(osc.data_ptr() - s.outputs[0][1].data_ptr()) + M * 2] = 127
    with pytest.raises(EG.OutsideTouched):
        s.check("scale row past M")


def test_output_scale_over_16_columns_is_caught():
    xq, xs, wq, ws, bias, (ref, F) = _geglu_case(129, 64, 64)
    oq, osc = MX.emulate_geglu(xq, xs, wq, ws, bias, 64, block=16)
    with pytest.raises(AssertionError):
        MX.assert_mx_close(oq, osc, ref, F)


# =====================================================================================================================================
# 4. dispatch
# =====================================================================================================================================
@pytest.fixture()
def K():
    from synfmc_amd import hip_ops
    return hip_ops


def _install(monkeypatch, K):
    fake_kernels.install(monkeypatch)
    monkeypatch.setattr(K, "_on_gpu", lambda t: True)
    monkeypatch.setattr(K, "_ff_on_gpu", lambda t: True)
    monkeypatch.setattr(K, "_cus", lambda device: 8)

    def pack(w, geglu=False):
        return torch.zeros(w.shape, dtype=U8), torch.zeros(w.shape[0], w.shape[1] // 32, dtype=U8)

    def ln(h, gamma, beta, eps=1e-5):
        C = h.shape[-1]
        K._log_call("mxfp8", ("ln", h.numel() // C, C), 0.0)
        return torch.zeros(h.numel() // C, C, dtype=U8), torch.zeros(h.numel() // C, C // 32, dtype=U8)

    def lin(xq, xs, wq, ws, bias=None, residual=None, geglu=False):
        M, N = xq.shape[0], wq.shape[0] // 2 if geglu else wq.shape[0]
        K._log_call("mxfp8", ("geglu" if geglu else "linear", M, N, xq.shape[1]), 0.0)
        return (torch.zeros(M, N, dtype=U8), torch.zeros(M, N // 32, dtype=U8)) if geglu else torch.zeros(M, N, dtype=BF16)
    for name, fn in (("mxfp8_pack_weight", pack), ("layernorm_mxfp8", ln), ("linear_mxfp8", lin)):
        monkeypatch.setattr(K, name, fn)
    monkeypatch.setattr(K, "call_log", [])


def _mx_calls(K):
    log = [c for c in K.call_log if c[0] == "mxfp8"]
    del K.call_log[:]
    return log


@pytest.mark.parametrize("C", [320, 640])
def test_forward_ln_dispatch_under_fp8_ff(monkeypatch, K, C):
    from synfmc_amd.models import layers as L
    _install(monkeypatch, K)
    torch.manual_seed(0)
    ff = L.FeedForward(C).eval().requires_grad_(False).to(BF16)
    norm = L.LayerNorm(C).eval().requires_grad_(False).to(BF16)
    M = 330
    h = torch.randn(M, C).to(BF16)
    assert K.FP8_FF is False and C in K.MXFP8_FF_SLOWER                    # (measured slower at the bench clip: not routed by default, profiles/mxfp8_ff.md)
    with torch.no_grad():
        monkeypatch.setattr(K, "FP8_FF", True)
        ff.forward_ln(h, norm, h)
        assert _mx_calls(K) == []
        monkeypatch.setattr(K, "FP8_FF", False)
    monkeypatch.setattr(K, "MXFP8_FF_SLOWER", ())                          # every other condition of the route, at this width
    with torch.no_grad():
        ff.forward_ln(h, norm, h)
        assert _mx_calls(K) == []                                           # switch off: no launch of the family
        monkeypatch.setattr(K, "FP8_FF", True)
        y = ff.forward_ln(h, norm, h)
        assert [c[1][0] for c in _mx_calls(K)] == ["ln", "geglu", "linear"]    # three per feed-forward
        assert y.shape == h.shape and y.dtype == BF16 and getattr(y, "_fmc_tail", None) is None
        y = ff.forward_ln(h.view(2, M // 2, C), norm, h.view(2, M // 2, C), tail=(torch.zeros(C, C, dtype=BF16), None, h, 0))
        assert len(_mx_calls(K)) == 3 and y.shape == (2, M // 2, C) and getattr(y, "_fmc_tail", None) is None      # the tail fold stays a bf16 route
        for tag in ("_fmc_pending_add", "_fmc_ln", "_fmc_pending_ln"):      # a pending tag: somebody else's h
            h2 = h.clone()
            setattr(h2, tag, (torch.zeros(M, 2), None, True))
            ff.forward_ln(h2, norm, h2)
            assert _mx_calls(K) == [], tag
        ff32, norm32 = L.FeedForward(C).eval().requires_grad_(False), L.LayerNorm(C).eval().requires_grad_(False)
        assert not ff32.mxfp8_route(h.float(), h.float()) and not ff32.mxfp8_route(h, h)                           # fp32 storage
        monkeypatch.setattr(K, "MXFP8_FF_SLOWER", (C,))                      # a width that is not routed
        ff.forward_ln(h, norm, h)
        assert _mx_calls(K) == []
    with torch.enable_grad():                                              # under a gradient
        monkeypatch.setattr(K, "MXFP8_FF_SLOWER", ())
        ff.forward_ln(h, norm, h)
        assert _mx_calls(K) == []


def test_ff_mxfp8_ok_follows_the_shape_rule(monkeypatch, K):
    monkeypatch.setattr(K, "_on_gpu", lambda t: True)
    h = torch.zeros(7, 320, dtype=BF16)
    w1, w2 = torch.zeros(2560, 320, dtype=BF16), torch.zeros(320, 1280, dtype=BF16)
    with torch.no_grad():
        assert not K.ff_mxfp8_ok(h, w1, w2, h)                             # a width measured slower
        monkeypatch.setattr(K, "MXFP8_FF_SLOWER", ())
        assert K.ff_mxfp8_ok(h, w1, w2, h) and K.ff_mxfp8_ok(h, w1, w2, None)
        assert not K.ff_mxfp8_ok(h, w1, w2, torch.zeros(7, 320))           # an fp32 residual
        assert not K.ff_mxfp8_ok(h[:, :160], w1[:, :160], w2, None)        # not contiguous, and K % 64 != 0
        assert not K.ff_mxfp8_ok(h, w1.float(), w2, h)
    assert K.mxfp8_supported(1, 64, 64, True) and not K.mxfp8_supported(1, 64, 96, False) and not K.mxfp8_supported(1, 32, 64, False) \
        and not K.mxfp8_supported(0, 64, 64, False) and not K.mxfp8_supported(1 << 25, 64, 64, False)

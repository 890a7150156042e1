"""Exact integer runs of the fused transformer blocks: every output element of the temporal attention block (`fmc_temporal_block_bf16`, C = 320 and 640,
whole and partial tiles), of the text cross-attention blocks (`fmc_xattn_block320_bf16`, `fmc_xattn_block640_bf16` and their partial forms) and of the
LayerNorm + GEGLU kernels (`fmc_geglu320_ln_bf16`, `fmc_geglu640_ln_bf16`, `fmc_geglu_pipe_ln_bf16` variants 0 and 1 and its partial form) against a
float64 expectation with ZERO tolerance.

tests/fused_block_common.py builds inputs on which LayerNorm, softmax and GELU have exactly representable results (asserted on the reference by
`assert_exact_conditions`; profiles/fused_block_bounds.md has the derivations), so a dropped, doubled or mis-addressed term -- a padded text key that
leaks, a head's 8-channel tail weighted wrongly, the neighbouring frame's positional encoding, another head's fragments, another pixel's v -- moves an
output by at least 1/4.  tests/test_fused_block_reference_host.py shows on the CPU that each of those is caught in every case it applies to.

Every case is launched twice: through the `hip_ops` wrapper, and through the C ABI on output buffers pre-filled with NaN; both must give the same bits.
The row statistics for the next LayerNorm are held, element by element, to bounds counted from the source (`STATS_MEAN_CHAIN`, `STATS_RSTD_CHAIN`)
against float64 statistics of the kernel's own output, in the exact cases and on the Gaussian inputs of the existing tests."""
import pytest
import torch

from tests import ff_partial_common as FFC
from tests import fused_block_common as FB
from tests.test_gpu_kernels import rnd

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _cus(K):
    return K._cus(torch.device("cuda", torch.cuda.current_device()))


def _nan(shape, dtype=BF16):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _bf(t):
    return None if t is None else t.to(BF16).cuda().contiguous()


def _f32(t):
    return t.to(F32).cuda().contiguous()


def _same(a, b, what):
    """Bit identity of two launches (NaN included: the second buffer started as NaN, a word nobody wrote stays NaN and differs from the first)."""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    ai, bi = (t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32) for t in (a, b))
    assert torch.equal(ai, bi), f"{what}: {int((ai != bi).sum())} words differ between the two launches"


# =====================================================================================================================================
# temporal block
# =====================================================================================================================================
def _temporal(K, c):
    FB.assert_exact_conditions(c)
    dd = FB.inputs(c)
    C, B, hw, what = c.C, c.B, c.hw, FB.case_id(c)
    h = _bf(FB.expand_pixels(dd["h"], hw, 2))
    gamma, bpe, bout = _f32(dd["gamma"]), _f32(dd["bpe"]), _bf(dd["b_out"])
    pack_w = K._w_tilemajor if C == 320 else K.pack_w_frag80
    wq = (K.pack_temporal_qkv if C == 320 else K.pack_temporal_qkv80)(_bf(dd["w_qkv"]))
    wo = pack_w(_bf(dd["w_out"])).contiguous()
    wm = pack_w(_bf(dd["w_merge"])).contiguous() if c.merge else None
    pt = _bf(FB.expand_pixels(dd["pose"], hw, 2)) if c.merge else None
    kw = dict(w_merge_tm=wm, pose_term=pt, merge_scale=dd["merge_scale"]) if c.merge else {}
    got = K.temporal_block(h, gamma, bpe, FB.LN_EPS, wq, wo, bout, FB.SCALE, stats_eps=FB.LN_EPS if c.stats else None, partial_tiles=c.partial, **kw)
    out, stats = got if c.stats else (got, None)
    FB.check_exact(out, FB.expected_full(c), what)
    # the second launch: the C ABI on NaN-filled buffers
    out2 = _nan(h.shape)
    stats2 = _nan((h.numel() // C, 2), F32) if c.stats else None
    name = "fmc_temporal_block_partial_bf16" if c.partial else "fmc_temporal_block_bf16"
    K._lib.check(getattr(K._lib.load(), name)(h.data_ptr(), out2.data_ptr(), gamma.data_ptr(), bpe.data_ptr(), FB.LN_EPS, K._p(wm), K._p(pt),
                                              float(dd["merge_scale"]), wq.data_ptr(), wo.data_ptr(), bout.data_ptr(), K._p(stats2),
                                              FB.LN_EPS if c.stats else 0.0, B, 16, hw, C, 8, FB.SCALE, K._stream()), name)
    _same(out2, out, what)
    if c.stats:
        _same(stats2, stats, what + " statistics")
        FB.check_stats(stats, out, what)


def _tid(c):
    return FB.case_id(c)


@pytest.mark.parametrize("c", [c for c in FB.TEMPORAL if not c.persistent], ids=_tid)
def test_temporal_block_exact(K, c):
    _temporal(K, c)


@pytest.mark.parametrize("c", [c for c in FB.TEMPORAL if c.persistent], ids=_tid)
def test_temporal_block_exact_persistent_loop(K, c):
    """One clip of `2 * CUs + 3` tiles: every workgroup runs two tiles, three of them a third.  The expectation is the periodic one of
    PERIOD pixels, expanded (the block is local to a pixel)."""
    c = c._replace(hw=FB.persistent_hw(c, _cus(K)))
    assert c.hw // (10 if c.C == 320 else 5) == 2 * _cus(K) + 3
    _temporal(K, c)


# =====================================================================================================================================
# text cross-attention block
# =====================================================================================================================================
def _text(K, c):
    FB.assert_exact_conditions(c)
    dd = FB.inputs(c)
    C, hw, what = c.C, c.hw, FB.case_id(c)
    N = c.B * c.ipt
    h = _bf(FB.expand_pixels(dd["h"], hw, 1))
    gamma, bout, kv = _f32(dd["gamma"]), _bf(dd["b_out"]), _bf(dd["kv"])
    btab = _f32(dd["beta"][None].expand(16, C))
    if C == 320:
        wq, wo = K.pack_xattn_q40(_bf(dd["w_q"])), K._w_tilemajor(_bf(dd["w_out"])).contiguous()
    else:
        wq, wo = K.pack_w_frag80(_bf(dd["w_q"])), K.pack_w_frag80(_bf(dd["w_out"]))
    frag = K.xattn_pack_kv(kv)
    got = K.xattn_block(h, gamma, btab, FB.LN_EPS, wq, kv, wo, bout, FB.SCALE, c.ipt, stats_eps=FB.LN_EPS if c.stats else None, partial_tiles=c.partial)
    out, stats = got if c.stats else (got, None)
    FB.check_exact(out, FB.expected_full(c), what)
    out2 = _nan(h.shape)
    stats2 = _nan((N * hw, 2), F32) if c.stats else None
    L = K._lib.load()
    if C == 320:
        name = "fmc_xattn_block320_partial_bf16" if c.partial else "fmc_xattn_block320_bf16"
        K._lib.check(getattr(L, name)(h.data_ptr(), out2.data_ptr(), gamma.data_ptr(), btab.data_ptr(), FB.LN_EPS, wq.data_ptr(), frag.data_ptr(), wo.data_ptr(),
                                      bout.data_ptr(), K._p(stats2), FB.LN_EPS if c.stats else 0.0, N, hw, c.S, c.ipt, FB.SCALE, K._stream()), name)
    else:
        name = "fmc_xattn_block640_partial_bf16" if c.partial else "fmc_xattn_block640_bf16"
        K._lib.check(getattr(L, name)(h.data_ptr(), out2.data_ptr(), gamma.data_ptr(), btab.data_ptr(), FB.LN_EPS, wq.data_ptr(), frag.data_ptr(), wo.data_ptr(),
                                      bout.data_ptr(), N, hw, c.S, c.ipt, FB.SCALE, K._stream()), name)
    _same(out2, out, what)
    if c.stats:
        _same(stats2, stats, what + " statistics")
        FB.check_stats(stats, out, what)


@pytest.mark.parametrize("c", FB.TEXT, ids=_tid)
def test_xattn_block_exact(K, c):
    _text(K, c)


# =====================================================================================================================================
# LayerNorm + GEGLU
# =====================================================================================================================================
def _unblock(K, t, M, cff):
    """Tile-major `[ceil(M / 160)][cff / 32][160][32]` storage -> the valid rows `[M, cff]`."""
    store = torch.empty(0, dtype=BF16, device="cuda").set_(t.untyped_storage(), t.storage_offset(), (K.ff_blocked_numel(M, cff),))
    return FFC.from_blocked(store, M, cff)


def _geglu(K, c):
    FB.assert_exact_conditions(c)
    dd = FB.inputs(c)
    C, M, cff, what = c.C, c.M, c.cff, FB.case_id(c)
    h, gamma, beta, bias = _bf(dd["h"]), _f32(dd["gamma"]), _f32(dd["beta"]), _bf(dd["bias"])
    ref = FB.expectation(c)[0].to(BF16)
    L = K._lib.load()
    if c.kernel == "direct":
        wp = K.pack_geglu_frag80(_bf(dd["w"]))
        run = lambda blocked: K.geglu_ln_direct(h, gamma, beta, FB.LN_EPS, wp, bias, cff, blocked=blocked)
        name = "fmc_geglu640_ln_bf16" if C == 640 else "fmc_geglu320_ln_bf16"
        raw = lambda o, blocked: getattr(L, name)(h.data_ptr(), o.data_ptr(), gamma.data_ptr(), beta.data_ptr(), FB.LN_EPS, wp.data_ptr(), K._p(bias), M, cff,
                                                  int(blocked), K._stream())
    else:
        wp = K.pack_geglu_frag(_bf(dd["w"]), 16 if c.variant == 1 else 32)
        run = lambda blocked: K.geglu_ln_pipe(h, gamma, beta, FB.LN_EPS, wp, bias, cff, blocked=blocked, variant=c.variant, partial_tiles=c.partial)
        name = "fmc_geglu_pipe_ln_partial_bf16" if c.partial else "fmc_geglu_pipe_ln_bf16"
        raw = lambda o, blocked: getattr(L, name)(h.data_ptr(), o.data_ptr(), gamma.data_ptr(), beta.data_ptr(), FB.LN_EPS, wp.data_ptr(), K._p(bias), M, cff, C,
                                                  int(blocked), c.variant, K._stream())
    for blocked in ((False, True) if (M % 160 == 0 or c.partial) else (False,)):
        w2 = f"{what} {'tile-major' if blocked else 'row-major'}"
        out = run(blocked)
        rows = _unblock(K, out, M, cff) if blocked else out
        FB.check_exact(rows, ref, w2)
        out2 = _nan((K.ff_blocked_numel(M, cff),)) if blocked else _nan((M, cff))
        K._lib.check(raw(out2, blocked), name)
        _same(FFC.from_blocked(out2, M, cff) if blocked else out2, rows, w2)


@pytest.mark.parametrize("c", FB.GEGLU, ids=_tid)
def test_geglu_ln_exact(K, c):
    _geglu(K, c)


# =====================================================================================================================================
# row statistics on the Gaussian inputs of the existing tests (test_temporal_block_fused, test_xattn_block_fused_320: copied, those stay)
# =====================================================================================================================================
@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("B,hw", [(1, 10), (3, 70)])
def test_temporal_block_statistics_element_by_element(K, merge, B, hw):
    C, Fr = 320, 16
    ho, hd = rnd((B, Fr, hw, C), 1, BF16, scale=1.5, shift=0.2)
    go, _ = rnd((C,), 2, F32, scale=0.3, shift=1.0)
    bo, _ = rnd((C,), 3, F32, scale=0.2)
    peo, _ = rnd((32, C), 4, F32, scale=0.7)
    wqo, wqd = rnd((3 * C, C), 5, BF16, scale=C ** -0.5 * 1.5)
    woo, wod = rnd((C, C), 6, BF16, scale=C ** -0.5)
    boo, bod = rnd((C,), 7, BF16, scale=0.3)
    wmo, wmd = rnd((C, C), 8, BF16, scale=C ** -0.5)
    bmo, bmd = rnd((C,), 9, BF16, scale=0.3)
    poo, pod = rnd((B, Fr, hw, C), 10, BF16)
    s = 0.7
    bpe = (bo[None] + peo[:Fr]).cuda().contiguous()
    pt = K.linear_bf16(pod.view(-1, C), wmd, bmd, None, s).view(B, Fr, hw, C) if merge else None
    kw = dict(w_merge_tm=K._w_tilemajor(wmd), pose_term=pt, merge_scale=s) if merge else {}
    out, stats = K.temporal_block(hd, go.cuda(), bpe, 1e-5, K.pack_temporal_qkv(wqd), K._w_tilemajor(wod), bod, 40 ** -0.5, stats_eps=1e-5, **kw)
    FB.check_stats(stats, out, f"temporal_block statistics merge {merge} B {B} hw {hw}")


@pytest.mark.parametrize("B,Fr,hw,S", [(1, 1, 160, 77), (3, 2, 320, 80), (2, 3, 160, 5)])
def test_xattn_block_statistics_element_by_element(K, B, Fr, hw, S):
    C, d = 320, 40
    N = B * Fr
    ho, hd = rnd((N, hw, C), 1, BF16, scale=1.5, shift=0.2)
    go, _ = rnd((C,), 2, F32, scale=0.3, shift=1.0)
    bo, _ = rnd((C,), 3, F32, scale=0.2)
    wqo, wqd = rnd((C, C), 5, BF16, scale=C ** -0.5 * 1.5)
    woo, wod = rnd((C, C), 6, BF16, scale=C ** -0.5)
    boo, bod = rnd((C,), 7, BF16, scale=0.3)
    kvo, kvd = rnd((B, S, 2 * C), 8, BF16, scale=1.2)
    btab = bo[None].expand(16, C).contiguous().cuda()
    out, stats = K.xattn_block(hd, go.cuda(), btab, 1e-5, K.pack_xattn_q40(wqd), kvd, K._w_tilemajor(wod), bod, d ** -0.5, Fr, stats_eps=1e-5)
    FB.check_stats(stats, out, f"xattn_block statistics B {B} Fr {Fr} hw {hw} S {S}")

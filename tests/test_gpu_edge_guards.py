"""Every forward kernel with an edge, at the smallest shapes that reach it, with poison around its inputs and sentinels around its outputs.

An output comparison cannot see a read outside the extents while the memory there is finite, nor a write outside them at all.  Here every
operand lives in an arena of the test's own (tests/edge_guard_common.py) and every case runs three times -- zeros, quiet NaN and +Inf in
every element around the inputs -- through the raw C ABI, so that the outputs live in sentinel-filled arenas too.  Asserted per case:

  1. every output is finite and BIT-IDENTICAL across the three runs (`torch.equal`; no tolerance): `0 * NaN`, a pad score in a row maximum,
     a pad row in a statistic all move a bit;
  2. the run meets the reference and the gate the kernel's own test uses (imported from test_gpu_kernels.py / restated constants of
     test_gpu_conv_halo.py, no new tolerance);
  3. every word outside an output view keeps the sentinel and every word inside was written (`assert_contained`), side outputs included:
     LSE, statistics, partials, workspaces (a workspace the ABI sizes "at least" may be used in part).

The guard bands are in ROWS of the guarded tensor and at least the largest tile of the kernel, in rows (the `*_BAND` constants below, from the
sources): a reach of one tile past any edge lands in memory this file allocated.  One run is recorded in profiles/edge_guards.md."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import edge_guard_common as EG
from tests.test_gpu_kernels import TOL, assert_bf16_close, assert_f32_close, oracle_attention, rel_inf

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [BF16, F32]
TAG = {BF16: "bf16", F32: "fp32"}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _call(K, name, *args):
    K._lib.check(getattr(K._lib.load(), name)(*args), name)


def _p(t):
    return None if t is None else t.data_ptr()


def _run(fn, what):
    """The case under zeros, NaN and +Inf: containment of every output of every run, then finite and bit-identical."""
    seen = {}

    def wrapped(g):
        outs = fn(g)
        seen["outputs"] = [name for name, *_ in g.outputs]
        seen["bands"] = g.bands
        return outs
    out = EG.run_surroundings(wrapped, "cuda", what, torch.cuda.synchronize)
    print(f"edge-guard {what}: zeros / nan / inf bit-identical; guarded outputs: {', '.join(seen['outputs'])}")
    return out


def _rnd(shape, seed, dtype, scale=1.0, shift=0.0):
    """Seeded values of `dtype` on the CPU (`.float()` of it is exact: the reference's input)."""
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift).to(dtype)


def _vec_band(n, reach=512):
    """Band, in rows of `n` elements, of a 1-D operand (bias, gamma): at least `reach` elements."""
    return -(-reach // n) + 1


# =====================================================================================================================================
# Spatial attention, fmc_spatial_attn_fwd (csrc/spatial_attn.hip)
#   query rows per workgroup: 128 / 256 (tiled, 1 / 2 blocks per wave), 256 (sa40d), 160 (sa_small160), 320 (sa_big80 w10), 32 (xattn40)
#   keys staged at a time:    64 (tiled, sa40d: and its 4-buffer ring reaches 3 tiles = 192 keys ahead), 96 / 160 (sa_small160), 96 (xattn40)
# =====================================================================================================================================
SA_BAND_Q = 320                      # rows of q / o around them
SA_BAND_KV = 256                     # rows of k | v
SA_BAND_LSE = 320                    # floats of lse, rounded up to whole rows of Sq

# name -> (dtypes, B, Bkv, H, D, Sq, Skv): k | v are the column blocks of one fused [Bkv, Skv, 2C] projection, q | k | v of one [B, S, 3C] when
# Sq == Skv; `_sep`: q, k and v are three tensors of their own (`spatial_attention(q, k, v)`), so K's last head ends at the guard as well.  Every
# row has 8 spare (poisoned) columns: a 16-column block past D = 40 or 8 of the last head reaches them in every row
SA_CASES = {
    "tiled_d40_130x77": (DTYPES, 2, 2, 2, 40, 130, 77),              # short-KV path with prefetch (bf16), two key tiles, the second 13 keys
    "tiled_d40_300x200": (DTYPES, 2, 2, 2, 40, 300, 200),            # two query blocks per wave; partial 64-key tile and partial 32-key block
    "tiled_d64_257x257": (DTYPES, 2, 2, 2, 64, 257, 257),            # one query block per wave; one row and one key over
    "tiled_d8_96x33": (DTYPES, 2, 2, 2, 8, 96, 33),                  # one key tile, 33 of 64
    "tiled_d160_130x200": (DTYPES, 1, 1, 2, 160, 130, 200),          # ten k-steps, rolled staging
    "xattn40_64x77_div2": ([BF16], 4, 2, 8, 40, 64, 77),             # xattn40_kernel, kv_batch_div 2
    "xattn40_32x1": ([BF16], 2, 2, 8, 40, 32, 1),                    # ... one key
    "small160_33x77": ([BF16], 2, 2, 2, 160, 33, 77),                # sa_small160_kernel<3>
    "small160_170x100": ([BF16], 2, 2, 2, 160, 170, 100),            # sa_small160_kernel<5>, ten rows over 160
    "big80_170x288": ([BF16], 1, 1, 2, 80, 170, 288),                # sa_big80_kernel_w10
    "sa40d_256x128_bh2": ([BF16], 1, 1, 2, 40, 256, 128),            # 2 tiles: the prologue's requests for tiles 2, 3 are out of range
    "sa40d_256x128_bh8": ([BF16], 2, 2, 4, 40, 256, 128),
    "sa40d_256x192_bh2": ([BF16], 1, 1, 2, 40, 256, 192),            # 3 tiles: one out-of-range request
    "sa40d_256x192_bh8": ([BF16], 2, 1, 4, 40, 256, 192),            # ... both batch entries on one K / V
    "sa40d_512x320_bh2": ([BF16], 1, 1, 2, 40, 512, 320),            # 5 tiles: the 4-buffer ring wraps
    "sa40d_512x320_bh8": ([BF16], 2, 2, 4, 40, 512, 320),
    "tiled_d40_130x77_sep": (DTYPES, 2, 2, 2, 40, 130, 77),
    "tiled_d40_300x200_sep": (DTYPES, 2, 2, 2, 40, 300, 200),
    "tiled_d8_96x33_sep": (DTYPES, 2, 2, 2, 8, 96, 33),
    "xattn40_64x77_div2_sep": ([BF16], 4, 2, 8, 40, 64, 77),
    "small160_33x77_sep": ([BF16], 2, 2, 2, 160, 33, 77),
    "big80_170x288_sep": ([BF16], 1, 1, 2, 80, 170, 288),
    "sa40d_256x128_bh2_sep": ([BF16], 1, 1, 2, 40, 256, 128),
    "sa40d_256x192_bh8_sep": ([BF16], 2, 1, 4, 40, 256, 192),
}
SA_PARAMS = [pytest.param(n, d, id=f"{n}-{TAG[d]}") for n, c in SA_CASES.items() for d in c[0]]


@functools.lru_cache(maxsize=None)
def _sa_data(name, dtype):
    _, B, Bkv, H, D, Sq, Skv = SA_CASES[name]
    C, seed = H * D, 7000 + 10 * sorted(SA_CASES).index(name)
    if name.endswith("_sep"):
        fused = (_rnd((B, Sq, C), seed, dtype), _rnd((Bkv, Skv, C), seed + 1, dtype), _rnd((Bkv, Skv, C), seed + 2, dtype))
        q, k, v = fused
    elif Sq == Skv and B == Bkv:
        qkv = _rnd((B, Sq, 3 * C), seed, dtype)
        q, k, v, fused = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], (qkv,)
    else:
        qd, kv = _rnd((B, Sq, C), seed, dtype), _rnd((Bkv, Skv, 2 * C), seed + 1, dtype)
        q, k, v, fused = qd, kv[..., :C], kv[..., C:], (qd, kv)
    rep = B // Bkv
    qo, ko, vo = q.float(), k.float().repeat_interleave(rep, 0), v.float().repeat_interleave(rep, 0)
    ref = oracle_attention(qo, ko, vo, H)
    qh = qo.reshape(B, Sq, H, D).permute(0, 2, 1, 3)
    kh = ko.reshape(B, Skv, H, D).permute(0, 2, 1, 3)
    lse = torch.logsumexp(qh @ kh.transpose(-1, -2) * D ** -0.5, dim=-1)
    return fused, ref, lse


@pytest.mark.parametrize("name,dtype", SA_PARAMS)
def test_spatial_attention_forward(K, name, dtype):
    _, B, Bkv, H, D, Sq, Skv = SA_CASES[name]
    C = H * D
    fused, ref, lse_ref = _sa_data(name, dtype)

    def fn(g):
        if len(fused) == 3:
            q, k, v = g.inp(fused[0], SA_BAND_Q, 8, "q"), g.inp(fused[1], SA_BAND_KV, 8, "k"), g.inp(fused[2], SA_BAND_KV, 8, "v")
            assert k.stride() == v.stride()
        elif len(fused) == 1:
            t = g.inp(fused[0], SA_BAND_Q, 8, "qkv")
            q, k, v = t[..., :C], t[..., C:2 * C], t[..., 2 * C:]
        else:
            q = g.inp(fused[0], SA_BAND_Q, 8, "q")
            t = g.inp(fused[1], SA_BAND_KV, 8, "kv")
            k, v = t[..., :C], t[..., C:]
        o = g.out((B, Sq, C), dtype, SA_BAND_Q, 8, "o")
        lse = g.out((B, H, Sq), F32, -(-SA_BAND_LSE // Sq) + 1, 0, "lse")
        for t in (q, k, v, o):
            assert t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0
        _call(K, "fmc_spatial_attn_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, Sq, Skv, D, q.stride(0),
              q.stride(1), k.stride(0), k.stride(1), o.stride(0), o.stride(1), B // Bkv, D ** -0.5, K._dt(q), K._stream())
        return {"o": o, "lse": lse}

    out = _run(fn, f"spatial_attn {name} {TAG[dtype]}")
    err, lerr = rel_inf(out["o"].float(), ref), float((out["lse"].cpu() - lse_ref).abs().max())
    print(f"   rel-inf {err:.3e} (gate {TOL[dtype]:.0e}), lse {lerr:.3e}")
    assert err < TOL[dtype]
    assert lerr < (1e-4 if dtype == F32 else 2e-2)


# =====================================================================================================================================
# fmc_attention_fwd (csrc/attn_generic.hip): 64 query rows per workgroup, 32 keys per stage; the key mask is guarded too
# =====================================================================================================================================
AG_BAND = 64
# (B, H, Sq, Skv, D, causal, keep): q | k | v are slices of ONE fused projection, as test_attention_generic_against_exact_softmax issues them
AG_CASES = [(2, 1, 300, 300, 512, False, False), (2, 12, 77, 77, 64, True, True), (2, 2, 70, 130, 32, False, True)]


@pytest.mark.parametrize("dtype,tol", [(F32, 2e-5), (BF16, 1.5e-2)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,H,Sq,Skv,D,causal,keep", AG_CASES)
def test_attention_generic_forward(K, dtype, tol, B, H, Sq, Skv, D, causal, keep):
    C, S = H * D, max(Sq, Skv)
    gen = torch.Generator().manual_seed(4100 + Sq + D)
    qkv = (torch.randn(B, S, 3 * C, generator=gen) * 1.5).to(dtype)
    kk = None
    if keep:
        kk = torch.rand(B, Skv, generator=gen) > 0.3
        kk[:, 0] = True

    def fn(g):
        if Sq == Skv:
            tq = tk = g.inp(qkv, AG_BAND, 8, "qkv")
        else:                                                                 # each side's fused rows end at its own guard
            tq, tk = g.inp(qkv[:, :Sq].contiguous(), AG_BAND, 8, "qkv (q rows)"), g.inp(qkv[:, :Skv].contiguous(), AG_BAND, 8, "qkv (k | v rows)")
        q, k, v = tq[..., :C], tk[..., C:2 * C], tk[..., 2 * C:]
        km = None if kk is None else g.inp(kk.to(torch.uint8), 2, 0, "key_keep")
        o = g.out((B, Sq, C), dtype, AG_BAND, 8, "o")
        _call(K, "fmc_attention_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), _p(km), B, H, Sq, Skv, D, q.stride(0), q.stride(1),
              k.stride(0), k.stride(1), o.stride(0), o.stride(1), D ** -0.5, int(causal), K._dt(q), K._stream())
        return {"o": o}

    got = _run(fn, f"attention {(B, H, Sq, Skv, D, causal, keep)} {TAG[dtype]}")["o"]
    q64, k64, v64 = (t.double().view(B, -1, H, D).transpose(1, 2) for t in (qkv[:, :Sq, :C], qkv[:, :Skv, C:2 * C], qkv[:, :Skv, 2 * C:]))
    s = q64 @ k64.transpose(-1, -2) * D ** -0.5
    mask = torch.ones(Sq, Skv, dtype=torch.bool)
    if causal:
        mask = mask.tril()
    mask = mask[None, None].expand(B, 1, Sq, Skv)
    if kk is not None:
        mask = mask & kk[:, None, None, :]
    want = (s.masked_fill(~mask, float("-inf")).softmax(-1) @ v64).transpose(1, 2).reshape(B, Sq, C)
    err = rel_inf(got, want)
    print(f"   rel-inf {err:.3e} (gate {tol:.1e})")
    assert err < tol
    bound = (2.0 ** -7 if dtype == BF16 else 1e-5) * v64.abs().amax(dim=(1, 2, 3)).view(B, 1, 1) * 1.5
    assert bool(((got.double().cpu() - want).abs() <= bound).all())


# =====================================================================================================================================
# Fused text cross-attention blocks (csrc/temporal_block.hip / temporal_block640.hip) with their pack routines
#   row tiles: 160 (C = 320, persistent) / 80 (C = 640); keys: S <= 80 packed into fragments of 80 (96 at C = 320) key slots
# =====================================================================================================================================
XB_BAND_ROWS = 160
XB_BAND_KV = 96
# (C, B, Fr, hw, S): one tile and three tiles of rows, Fr of 1 and 3, S = 77 and S = 5
XB_CASES = [(320, 1, 1, 160, 77), (320, 1, 3, 160, 5), (320, 2, 3, 160, 77),
            (640, 1, 1, 80, 77), (640, 1, 3, 80, 5), (640, 2, 3, 80, 77)]


@pytest.mark.parametrize("C,B,Fr,hw,S", XB_CASES)
def test_xattn_block_forward(K, C, B, Fr, hw, S):
    H, d, N = 8, C // 8, B * Fr
    h = _rnd((N * hw, C), 1, BF16, 1.5, 0.2)
    gamma, beta = _rnd((C,), 2, F32, 0.3, 1.0), _rnd((C,), 3, F32, 0.2)
    wq, wo, bo = _rnd((C, C), 5, BF16, C ** -0.5 * 1.5), _rnd((C, C), 6, BF16, C ** -0.5), _rnd((C,), 7, BF16, 0.3)
    kv = _rnd((B, S, 2 * C), 8, BF16, 1.2)
    btab = beta[None].expand(16, C).contiguous()
    wq_p = (K.pack_xattn_q40 if C == 320 else K.pack_w_frag80)(wq.cuda())
    wo_p = (K._w_tilemajor if C == 320 else K.pack_w_frag80)(wo.cuda())
    frag_len = 7680 if C == 320 else 12800

    def fn(g):
        kvd = g.inp(kv, XB_BAND_KV, 0, "kv")
        frag = g.out((B * 8, frag_len), BF16, 1, 0, "kvfrag")
        _call(K, "fmc_xattn_pack_kv40" if C == 320 else "fmc_xattn_pack_kv", kvd.data_ptr(), frag.data_ptr(), B, S, kvd.stride(0), K._stream())
        fragd = g.inp(frag.clone(), 1, 0, "kvfrag (as the block's operand)")
        hd = g.inp(h, XB_BAND_ROWS, 0, "h")
        gd, bd, wqd, wod, bod = (g.inp(t, _vec_band(t.shape[-1]), 0, n) for t, n in
                                 ((gamma, "ln_gamma"), (btab, "ln_btab"), (wq_p.cpu().view(-1, C), "w_q"), (wo_p.cpu().reshape(-1, C), "w_out"), (bo, "b_out")))
        out = g.out((N * hw, C), BF16, XB_BAND_ROWS, 0, "out")
        res = {"out": out, "kvfrag": frag}
        if C == 320:
            stats = g.out((N * hw, 2), F32, XB_BAND_ROWS, 0, "ln_stats")
            _call(K, "fmc_xattn_block320_bf16", hd.data_ptr(), out.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1e-5, wqd.data_ptr(), fragd.data_ptr(),
                  wod.data_ptr(), bod.data_ptr(), stats.data_ptr(), 1e-5, N, hw, S, Fr, d ** -0.5, K._stream())
            res["ln_stats"] = stats
        else:
            _call(K, "fmc_xattn_block640_bf16", hd.data_ptr(), out.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1e-5, wqd.data_ptr(), fragd.data_ptr(),
                  wod.data_ptr(), bod.data_ptr(), N, hw, S, Fr, d ** -0.5, K._stream())
        return res

    got = _run(fn, f"xattn_block{C} B {B} Fr {Fr} hw {hw} S {S}")
    ho, kvo = h.float().view(N, hw, C), kv.float()

    def reference(round_bf16):
        r = (lambda t: t.bfloat16().float()) if round_bf16 else (lambda t: t)
        x = r(F.layer_norm(ho, (C,), gamma, beta, 1e-5))
        q = r(F.linear(x, wq.float())).reshape(B, Fr * hw, H, d).permute(0, 2, 1, 3)
        k = kvo[..., :C].reshape(B, S, H, d).permute(0, 2, 1, 3)
        v = kvo[..., C:].reshape(B, S, H, d).permute(0, 2, 1, 3)
        p = r(torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1))
        o = r(p @ v).permute(0, 2, 1, 3).reshape(N, hw, C)
        return F.linear(o, wo.float(), bo.float()) + ho
    ref_r, ref_f = reference(True), reference(False)
    out = got["out"].float().cpu().view(N, hw, C)
    assert rel_inf(out, ref_f) < 2e-2
    err = (out - ref_r).abs()
    bound = 2.0 ** -8 * ref_r.abs() + 1.5 * 2.0 ** -8 * float(ref_r.abs().max())           # (test_xattn_block_fused_320 / _640)
    assert not bool((err > bound).any()), f"{int((err > bound).sum())} / {err.numel()} beyond the bound"
    if C == 320:
        mu, rstd = out.mean(-1).view(-1), (out.var(-1, unbiased=False) + 1e-5).rsqrt().view(-1)
        assert rel_inf(got["ln_stats"][:, 0], mu) < 1e-4 and rel_inf(got["ln_stats"][:, 1], rstd) < 1e-4


# =====================================================================================================================================
# Norms (csrc/norm_kernels.hip).  Rows in flight per workgroup: GN_U = 4 rows per thread, block / (C / 8) threads across a row, at most
# 1024 / 8 * 4 = 512 rows (C = 64); LayerNorm / GEGLU: a few rows per wave.
# =====================================================================================================================================
NORM_BAND = 512
GN_CASES = [(2, 33, 64, 0), (2, 7, 2560, 0), (2, 2499, 320, 0), (1, 256, 128, 0), (2, 40, 640, 320), (2, 2499, 640, 320)]    # (N, HW, C, C1 of a two-source input)


def _gn_ref(x, gamma, beta, act, G=32, eps=1e-5):
    ref = F.group_norm(x.float().permute(0, 2, 1), G, gamma, beta, eps)
    return (F.silu(ref) if act else ref).permute(0, 2, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("N,HW,C,C1", GN_CASES)
def test_groupnorm_silu_forward(K, dtype, N, HW, C, C1):
    G, eps, act = 32, 1e-5, True
    x = _rnd((N, HW, C), 1, dtype, 1.5, 0.7)
    gamma, beta = _rnd((C,), 2, F32), _rnd((C,), 3, F32)
    ws_bytes = K._lib.load().fmc_groupnorm_workspace_bytes(N, C, G)

    def fn(g):
        if C1:
            xa, xb = g.inp(x[..., :C1].contiguous(), NORM_BAND, 0, "x"), g.inp(x[..., C1:].contiguous(), NORM_BAND, 0, "x2")
        else:
            xa, xb = g.inp(x, NORM_BAND, 0, "x"), None
        gd, bd = g.inp(gamma, _vec_band(C), 0, "gamma"), g.inp(beta, _vec_band(C), 0, "beta")
        y = g.out((N, HW, C), dtype, NORM_BAND, 0, "y")
        stats = g.out((N, G * 2), F32, 8, 0, "stats")
        ws = g.out((ws_bytes // 4 // (G * 2), G * 2), F32, 64, 0, "workspace", written=False)
        _call(K, "fmc_groupnorm_silu_fwd", xa.data_ptr(), y.data_ptr(), gd.data_ptr(), bd.data_ptr(), stats.data_ptr(), ws.data_ptr(), N, HW, C, G, eps,
              int(act), K._dt(xa), _p(xb), C1, K._stream())
        return {"y": y, "stats": stats}

    got = _run(fn, f"groupnorm_silu_fwd {(N, HW, C, C1)} {TAG[dtype]}")
    err = rel_inf(got["y"].float(), _gn_ref(x, gamma, beta, act))
    gate = TOL[dtype] * (5 if dtype == F32 and C1 else 1)                       # (test_groupnorm_silu / test_groupnorm_two_source_concat)
    print(f"   rel-inf {err:.3e} (gate {gate:.0e})")
    assert err < gate
    xg = x.double().view(N, HW, G, C // G)
    assert rel_inf(got["stats"].view(N, G, 2)[..., 0], xg.mean((1, 3))) < 1e-4


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("N,HW,C,C1", [(2, 2499, 320, 0), (2, 33, 64, 0), (2, 170, 640, 320)])
def test_groupnorm_partials_apply_coef(K, dtype, N, HW, C, C1):
    """`fmc_groupnorm_partials` -> `fmc_groupnorm_apply_fwd` and -> `fmc_groupnorm_coef`, every link guarded."""
    G, eps = 32, 1e-5
    L = K._lib.load()
    x = _rnd((N, HW, C), 4, dtype, 1.5, 0.7)
    gamma, beta = _rnd((C,), 5, F32, 0.3, 1.0), _rnd((C,), 6, F32, 0.2)
    splits = L.fmc_groupnorm_partial_splits(HW, C)
    assert 1 <= splits <= 64

    def fn(g):
        if C1:
            xa, xb = g.inp(x[..., :C1].contiguous(), NORM_BAND, 0, "x"), g.inp(x[..., C1:].contiguous(), NORM_BAND, 0, "x2")
        else:
            xa, xb = g.inp(x, NORM_BAND, 0, "x"), None
        part = g.out((N * splits, G * 2), F32, 64, 0, "partials")
        _call(K, "fmc_groupnorm_partials", xa.data_ptr(), _p(xb), C1, part.data_ptr(), N, HW, C, G, K._dt(xa), K._stream())
        pin = g.inp(part.clone(), 64, 0, "partials (as an operand)")
        gd, bd = g.inp(gamma, _vec_band(C), 0, "gamma"), g.inp(beta, _vec_band(C), 0, "beta")
        coef = g.out((N * C, 2), F32, 512, 0, "coef")
        cstats = g.out((N, G * 2), F32, 8, 0, "coef stats")
        _call(K, "fmc_groupnorm_coef", pin.data_ptr(), splits, gd.data_ptr(), bd.data_ptr(), coef.data_ptr(), cstats.data_ptr(), N, HW, C, G, eps, K._stream())
        res = {"partials": part, "coef": coef, "coef_stats": cstats}
        if not C1:                                                           # (the apply pass takes one source)
            y = g.out((N, HW, C), dtype, NORM_BAND, 0, "y")
            stats = g.out((N, G * 2), F32, 8, 0, "stats")
            _call(K, "fmc_groupnorm_apply_fwd", xa.data_ptr(), y.data_ptr(), gd.data_ptr(), bd.data_ptr(), stats.data_ptr(), pin.data_ptr(), splits, N, HW, C,
                  G, eps, 1, K._dt(xa), K._stream())
            res.update(y=y, stats=stats)
        return res

    got = _run(fn, f"groupnorm partials / coef / apply {(N, HW, C, C1)} {TAG[dtype]}")
    xg = x.double().view(N, HW, G, C // G)
    part = got["partials"].view(N, splits, G, 2).double().sum(1).cpu()
    assert rel_inf(part[..., 0], xg.sum((1, 3))) < 1e-4 and rel_inf(part[..., 1], (xg * xg).sum((1, 3))) < 1e-4     # (test_gpu_conv_halo.py: partial sums)
    coef = got["coef"].view(N, C, 2).cpu()
    z_dev = x.float() * coef[:, None, :, 0] + coef[:, None, :, 1]
    assert rel_inf(z_dev, _gn_ref(x, gamma, beta, False)) < 1e-5                 # (test_conv3x3_halo_groupnorm_prologue_and_statistics_epilogue)
    assert rel_inf(got["coef_stats"].view(N, G, 2)[..., 0], xg.mean((1, 3))) < 1e-5
    if not C1:
        assert rel_inf(got["y"].float(), _gn_ref(x, gamma, beta, True)) < TOL[dtype]
        assert torch.equal(got["stats"], got["coef_stats"]) or rel_inf(got["stats"], got["coef_stats"]) < 1e-5


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("C,use_pe,add", [(64, False, False), (64, True, False), (320, False, False), (320, True, False), (320, False, True), (320, True, True)])
def test_layernorm_forward(K, dtype, C, use_pe, add):
    M, Fr, P = 160, 16, 10                                                    # rows [(b f), hw]: frame = (row // 10) % 16
    x, r = _rnd((M, C), 6, dtype, 2.0, 0.5), _rnd((M, C), 9, dtype)
    gamma, beta, pe = _rnd((C,), 7, F32), _rnd((C,), 8, F32), _rnd((Fr, C), 10, F32)

    def fn(g):
        xd = g.inp(x, NORM_BAND, 0, "x")
        gd, bd = g.inp(gamma, _vec_band(C), 0, "gamma"), g.inp(beta, _vec_band(C), 0, "beta")
        ped = g.inp(pe, 32, 0, "pe") if use_pe else None
        y = g.out((M, C), dtype, NORM_BAND, 0, "y")
        pe_args = (P, Fr) if use_pe else (1, 1)
        if add:
            rd = g.inp(r, NORM_BAND, 0, "addend")
            s = g.out((M, C), dtype, NORM_BAND, 0, "sum_out")
            _call(K, "fmc_layernorm_add_fwd", xd.data_ptr(), rd.data_ptr(), s.data_ptr(), y.data_ptr(), gd.data_ptr(), bd.data_ptr(), _p(ped), M, C, 1e-5,
                  *pe_args, K._dt(xd), K._stream())
            return {"y": y, "sum_out": s}
        _call(K, "fmc_layernorm_fwd", xd.data_ptr(), y.data_ptr(), gd.data_ptr(), bd.data_ptr(), _p(ped), M, C, 1e-5, *pe_args, K._dt(xd), K._stream())
        return {"y": y}

    got = _run(fn, f"layernorm{'_add' if add else ''}_fwd C {C} pe {use_pe} {TAG[dtype]}")
    hsum = torch.add(r, x) if add else x                                       # rounded to the storage type, like the kernel's sum_out
    if add:
        assert torch.equal(got["sum_out"].cpu(), hsum)                         # (test_layernorm_with_the_residual_add_in_front)
    ref = F.layer_norm(hsum.float(), (C,), gamma, beta, 1e-5)
    if use_pe:
        ref = ref + pe[(torch.arange(M) // P) % Fr]
    assert rel_inf(got["y"].float(), ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
def test_geglu_forward(K, dtype):
    M, Cff = 150, 2560
    x = _rnd((M, 2 * Cff), 8, dtype, 2.0)

    def fn(g):
        xd = g.inp(x, 64, 0, "x")
        y = g.out((M, Cff), dtype, 64, 0, "y")
        _call(K, "fmc_geglu_fwd", xd.data_ptr(), y.data_ptr(), M, Cff, K._dt(xd), K._stream())
        return {"y": y}

    got = _run(fn, f"geglu_fwd {TAG[dtype]}")
    a, gt = x.float().chunk(2, dim=-1)
    assert rel_inf(got["y"].float(), a * F.gelu(gt)) < TOL[dtype]


# =====================================================================================================================================
# Element-wise conditioning kernels (csrc/cond_kernels.hip): grid-stride loops over 8-element chunks / single elements, 256 threads
# =====================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
def test_mask_modulate_forward(K, dtype):
    N, h, w, C, Hin, Win = 3, 7, 11, 24, 64, 96                                 # 77 pixels x 3 chunks: no multiple of the 256-thread block
    x = _rnd((N, h * w, C), 31, dtype)
    mask = torch.rand(N, Hin, Win, generator=torch.Generator().manual_seed(30))
    mask = mask * (mask > 0.4)

    def fn(g):
        xd, md = g.inp(x, 512, 0, "x"), g.inp(mask, 64, 0, "mask_in")
        y, mo = g.out((N, h * w, C), dtype, 512, 0, "y"), g.out((N, h * w), F32, 8, 0, "mask_out")
        _call(K, "fmc_mask_modulate_fwd", xd.data_ptr(), md.data_ptr(), y.data_ptr(), mo.data_ptr(), N, h, w, C, Hin, Win, K._dt(xd), K._stream())
        return {"y": y, "mask_out": mo}

    got = _run(fn, f"mask_modulate_fwd {TAG[dtype]}")
    m_ref = F.interpolate(mask[:, None], size=(h, w), mode="nearest")
    assert torch.equal(got["mask_out"].cpu().view(N, h, w), m_ref[:, 0])
    assert rel_inf(got["y"].float(), x.float() * m_ref.reshape(N, h * w, 1)) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
def test_feature_add_forward(K, dtype):
    n, skip = 8 * 1001, 8 * 333                                                # (the ABI takes multiples of 8; 1001 chunks: no multiple of the block)
    hv, tv = _rnd((n,), 40, dtype), _rnd((n - skip,), 41, dtype)

    def fn(g):
        hd, td = g.inp(hv, 1, 0, "h"), g.inp(tv, 1, 0, "t")
        out = g.out((n,), dtype, 1, 0, "out")
        _call(K, "fmc_feature_add_fwd", hd.data_ptr(), td.data_ptr(), out.data_ptr(), n, skip, K._dt(hd), K._stream())
        return {"out": out}

    got = _run(fn, f"feature_add_fwd {TAG[dtype]}")["out"]
    ref = hv.float().clone()
    ref[skip:] += tv.float()
    assert rel_inf(got.float(), ref) < TOL[dtype]
    assert torch.equal(got[:skip].cpu(), hv[:skip])


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
def test_cfg_ddim_step_forward(K, dtype):
    n, gd, a_t, a_p = 4 * 1000 + 3, 8.0, 0.35, 0.52                              # n % 4 == 3: no vector width divides it
    eps, x = _rnd((2, n), 51, dtype), _rnd((n,), 50, F32)

    def fn(g):
        ed, xd = g.inp(eps.view(-1), 1, 0, "eps_uc"), g.inp(x, 1, 0, "x")
        out = g.out((n,), F32, 1, 0, "x_out")
        _call(K, "fmc_cfg_ddim_step", ed.data_ptr(), xd.data_ptr(), out.data_ptr(), n, 1, gd, a_t, a_p, K._dt(ed), K._stream())
        return {"x_out": out}

    got = _run(fn, f"cfg_ddim_step {TAG[dtype]}")["x_out"]
    e = eps[0].double() + gd * (eps[1].double() - eps[0].double())
    x0 = (x.double() - math.sqrt(1 - a_t) * e) / math.sqrt(a_t)
    assert rel_inf(got, math.sqrt(a_p) * x0 + math.sqrt(1 - a_p) * e) < 1e-5     # (test_cfg_ddim_step)


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_plucker_forward(K, dtype, layout):
    from oracle import conditioning as OC
    B, Fr, H, W = 1, 3, 24, 40                                                  # 960 pixels x 6: no multiple of the block; layout 2 wants H, W % 8 == 0
    gen = torch.Generator().manual_seed(77)
    Kin = torch.tensor([30.0, 35.0, 20.0, 12.0]).repeat(B, Fr, 1) + torch.randn(B, Fr, 4, generator=gen)          # (fx, fy, cx, cy) in pixels
    c2w = torch.eye(4)[None, None, :3].repeat(B, Fr, 1, 1) + 0.1 * torch.randn(B, Fr, 3, 4, generator=gen)
    shape = {0: (B, Fr, H, W, 6), 1: (B, 6, Fr, H, W), 2: (B * Fr, H // 8, W // 8, 384)}[layout]

    def fn(g):
        kd, cd = g.inp(Kin.reshape(B * Fr, 4), 8, 0, "K"), g.inp(c2w.reshape(B * Fr, 12), 8, 0, "c2w")
        out = g.out((math.prod(shape[:-1]), shape[-1]), dtype, 512, 0, "out")
        _call(K, "fmc_plucker_fwd", kd.data_ptr(), cd.data_ptr(), out.data_ptr(), B, Fr, H, W, 3, layout, K._dt(out), K._stream())
        return {"out": out}

    got = _run(fn, f"plucker_fwd layout {layout} {TAG[dtype]}")["out"].float().cpu().view(shape)
    c2w4 = torch.cat([c2w, torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(B, Fr, 1, 4)], 2)
    ref = OC.ray_condition(Kin.double(), c2w4.double(), H, W)                    # [B, F, H, W, 6]
    if layout == 1:
        ref = ref.permute(0, 4, 1, 2, 3)
    elif layout == 2:
        ref = F.pixel_unshuffle(ref.permute(0, 1, 4, 2, 3).reshape(-1, 6, H, W), 8).permute(0, 2, 3, 1)
    err = rel_inf(got, ref)
    print(f"   rel-inf {err:.3e}")
    assert err < (2e-6 if dtype == F32 else 5e-3)                               # (test_plucker_against_golden_and_oracle)


# =====================================================================================================================================
# GEMM front end (csrc/gemm_conv.hip, gemm4.hip): tiles of up to 256 x 320; the 8-phase arms request operand half-tiles 4 / 5 ahead
# =====================================================================================================================================
GEMM_BAND = 320                      # rows of A, residuals and out (a 256-row tile + the deepest prefetch of 64-row pieces)
GEMM_BAND_W = 320                    # rows of W (a 320-column tile)
WS_ROW = 1024                        # workspaces are guarded as rows of 1024 floats, 256 of them = one 256 x 256 fp32 tile each side
WS_BAND = 256


def _gemm_data(M, N, Kd, seed, k2=0):
    x, w = _rnd((M, Kd), seed, BF16), _rnd((N, Kd + k2), seed + 1, BF16, (Kd + k2) ** -0.5)
    b, r, r2 = _rnd((N,), seed + 2, BF16), _rnd((M, N), seed + 3, BF16), _rnd((M, N), seed + 4, BF16)
    x2 = _rnd((M, k2), seed + 5, BF16) if k2 else None
    return x, w, b, r, r2, x2


def _gemm_ref(x, w, b, r, r2, alpha, x2=None):
    xa = x if x2 is None else torch.cat([x, x2], -1)
    ref = xa.double() @ w.double().t()
    mag = xa.abs().double() @ w.abs().double().t()
    if b is not None:
        ref, mag = ref + b.double(), mag + b.abs().double()
    ref, mag = alpha * ref, abs(alpha) * mag
    for t in (r, r2):
        if t is not None:
            ref, mag = ref + t.double(), mag + t.abs().double()
    return ref, mag


def _ws(g, nbytes, flags=False):
    """A guarded workspace of at least `nbytes`; `flags`: the first 4096 bytes zero (stream-K)."""
    rows = -(-nbytes // (4 * WS_ROW))
    ws = g.out((rows, WS_ROW), F32, WS_BAND, 0, "workspace", written=False)
    if flags:
        ws.view(-1)[:1024].zero_()
    return ws, rows * WS_ROW * 4


def _tilemajor(w):
    """`[N, K]` -> `[N / 320][K / 32][320][32]` (`hip_ops._w_tilemajor`: what C-ABI tile 18 reads), as `[N, K]` rows for the guard."""
    N, Kd = w.shape
    return w.reshape(N // 320, 320, Kd // 32, 32).permute(0, 2, 1, 3).contiguous().view(N, Kd)


def _linear(K, g, x, w, b, r, r2, alpha, tile, split_k=1, x2=None, ws_bytes=0):
    """`fmc_linear_bf16` with A (and the second source) a column slice of a wider poisoned matrix, residuals and out with ldres / ldo > N;
    tile 18 gets the weight tile-major, as the product's default 160 x 320 arm does."""
    M, Kd = x.shape
    N = w.shape[0]
    if tile == 18:
        w = _tilemajor(w)
    xd = g.inp(x, GEMM_BAND, 64, "x")
    x2d = g.inp(x2, GEMM_BAND, 64, "x2") if x2 is not None else None
    wd = g.inp(w, GEMM_BAND_W, 0, "w")
    bd = g.inp(b, _vec_band(N), 0, "bias") if b is not None else None
    rd = g.inp(r, GEMM_BAND, 8, "residual") if r is not None else None
    r2d = g.inp(r2, GEMM_BAND, 8, "residual2") if r2 is not None else None
    out = g.out((M, N), BF16, GEMM_BAND, 8, "out")
    ws, nbytes = (None, 0)
    if split_k > 1:
        ws = g.out((split_k * M, N), F32, GEMM_BAND, 0, "split-K workspace")
        nbytes = split_k * M * N * 4
    elif split_k < 0:
        ws, nbytes = _ws(g, ws_bytes, flags=True)
    _call(K, "fmc_linear_bf16", xd.data_ptr(), wd.data_ptr(), _p(bd), _p(rd), out.data_ptr(), M, N, w.shape[1], xd.stride(0), rd.stride(0) if r is not None else 0,
          out.stride(0), alpha, 0, tile, split_k, _p(ws), nbytes, _p(x2d), x2d.stride(0) if x2 is not None else 0, Kd if x2 is not None else 0, _p(r2d),
          K._stream())
    res = {"out": out}
    if split_k < 0:
        res["flags"] = ws.view(-1)[:1024]
        torch.cuda.synchronize()
        used = int((ws.view(-1)[1024:].view(torch.int32) != EG.SENTINEL[F32][1]).sum())
        assert used > 0, "stream-K: no partial slot was written -- the launch fell back to the plain grid"
    return res


def _check_linear(got, ref, mag, elementwise, what):
    err = rel_inf(got.float(), ref)
    print(f"   {what}: rel-inf {err:.3e} (gate 1e-2)" + (", element-wise bf16 bound" if elementwise else ""))
    assert err < 1e-2
    if elementwise:
        assert_bf16_close(got, ref, mag, what)


# (C-ABI tile, M, N, K): M one over a multiple of the tile's rows, the raggedest N the arm takes (N % 8 == 0; N % 320 == 0 for tile 16)
PLAIN_TILES = [(t, 257, 328, 320) for t in range(1, 13)]                         # test_gemm_tile_geometries_agree: 128 / 256-row tiles, 128 / 256 / 320 columns
SMALL_M_TILES = [(t, 65, 136, 64) for t in (19, 20, 21, 22)]                     # test_gemm_small_m_tiles (arms 600 .. 603): 64 / 128-row tiles
PHASE8_TILES = [(t, 257, 264, 64) for t in (13, 14)] + [(13, 257, 264, 320)]     # test_gemm_8phase_arms: one k-tile (every prefetch out of range), and five
T160_TILES = [(t, 161, 320, 64) for t in (16, 18)] + [(t, 161, 640, 320) for t in (16, 18)]     # test_gemm_160x320_arm, test_tile_major_weights_are_bit_identical: plain form


@pytest.mark.parametrize("tile,M,N,Kd", PLAIN_TILES + SMALL_M_TILES + PHASE8_TILES + T160_TILES)
def test_linear_bf16_plain_grid(K, tile, M, N, Kd):
    x, w, b, r, r2, _ = _gemm_data(M, N, Kd, 60 + tile)
    ref, mag = _gemm_ref(x, w, b, r, None, 0.5)
    got = _run(lambda g: _linear(K, g, x, w, b, r, None, 0.5, tile), f"linear_bf16 tile {tile} {(M, N, Kd)} bias + residual")["out"]
    _check_linear(got, ref, mag, tile not in (19, 20, 21, 22), f"tile {tile}")
    ref2, mag2 = _gemm_ref(x, w, None, r, r2, 1.0)
    got2 = _run(lambda g: _linear(K, g, x, w, None, r, r2, 1.0, tile), f"linear_bf16 tile {tile} {(M, N, Kd)} two residuals")["out"]
    _check_linear(got2, ref2, mag2, False, f"tile {tile}, two residuals")


@pytest.mark.parametrize("tile", [1, 3, 5, 11, 13])
def test_linear_bf16_two_source(K, tile):
    M, N, K1, K2 = 257, 328, 128, 64                                             # (test_linear_two_source_concat's tiles; 13 falls back to 3)
    x, w, b, _, _, x2 = _gemm_data(M, N, K1, 94, K2)
    ref, mag = _gemm_ref(x, w, b, None, None, 1.0, x2)
    got = _run(lambda g: _linear(K, g, x, w, b, None, None, 1.0, tile, x2=x2), f"linear_bf16 tile {tile} two-source A")["out"]
    _check_linear(got, ref, mag, False, f"two-source, tile {tile}")


@pytest.mark.parametrize("tile", [16, 18])
def test_linear_bf16_160x320_persistent_form(K, tile):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, N, Kd = 160 * (cus + 1), 320, 64                                          # one tile more than CUs: gemm160p_kernel, the last workgroup's second tile
    x, w, b, r, _, _ = _gemm_data(M, N, Kd, 710)
    ref, mag = _gemm_ref(x, w, b, r, None, 0.5)
    got = _run(lambda g: _linear(K, g, x, w, b, r, None, 0.5, tile), f"linear_bf16 tile {tile} persistent {(M, N, Kd)}")["out"]
    _check_linear(got, ref, mag, True, "160 x 320 persistent")


def test_linear_bf16_k320_weight_stationary(K):
    """C-ABI tile 15 (test_gemm_k320_weight_stationary_arm): 64-row A tiles by LDS-DMA two tiles ahead, so the last workgroups request tiles
    past M; one tile more than CUs, x and the residual column slices of wider poisoned matrices."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, N, Kd = 64 * (cus + 1), 320, 320
    x, w, b, r, _, _ = _gemm_data(M, N, Kd, 145)
    ref = 0.5 * F.linear(x.float(), w.float(), b.float()) + r.float()
    got = _run(lambda g: _linear(K, g, x, w, b, r, None, 0.5, 15), f"linear_bf16 tile 15 {(M, N, Kd)}")["out"]
    err = rel_inf(got.float(), ref)
    print(f"   tile 15: rel-inf {err:.3e} (gate 1e-2)")
    assert err < 1e-2


@pytest.mark.parametrize("tile,split_k,M,N,Kd", [(1, 2, 129, 200, 192), (2, 4, 257, 200, 320), (9, 2, 257, 200, 192), (16, 2, 161, 320, 192),
                                                  (18, 2, 161, 320, 192)])
def test_linear_bf16_split_k(K, tile, split_k, M, N, Kd):
    """Split-K (test_gemm_split_k: tiles 1, 2, 9; test_gemm_160x320_split_k): k-tiles that do not divide by the split, the fp32 partials in a
    guarded workspace of exactly split_k * M * N floats."""
    x, w, b, r, _, _ = _gemm_data(M, N, Kd, 50 + tile)
    ref, mag = _gemm_ref(x, w, b, r, None, 0.5)
    got = _run(lambda g: _linear(K, g, x, w, b, r, None, 0.5, tile, split_k), f"linear_bf16 tile {tile} split-K {split_k} {(M, N, Kd)}")["out"]
    _check_linear(got, ref, mag, tile in (16, 18), f"split-K, tile {tile}")


@pytest.mark.parametrize("tile", [1, 13])
def test_linear_bf16_stream_k(K, tile):
    """Stream-K (test_gemm_stream_k, test_gemm_8phase_arms: 128 + tile): the smallest problem the arm does not hand back to the plain grid,
    flags and partial slots in a guarded workspace of the size the header states; the flags come back zero."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if tile == 1:                                                               # ring kernel: g = 2 workgroups per CU, needs tiles * K / 64 >= 4 g
        M, N = 1025, 1032
        Kd = 64 * -(-4 * 2 * cus // (9 * 9))
        ws_bytes = 4096 + 2 * cus * 128 * 128 * 4
    else:                                                                       # 8-phase: g = CUs, needs tiles * K / 64 >= 2 g; <= ceil(tiles / g) + 2 slots per CU
        M, N = 1025, 1032
        Kd = 64 * -(-2 * cus // 25)
        ws_bytes = 4096 + cus * 3 * 256 * 256 * 4
    x, w, b, r, _, _ = _gemm_data(M, N, Kd, 45)
    ref = F.linear(x.float(), w.float(), b.float()) + r.float()
    got = _run(lambda g: _linear(K, g, x, w, b, r, None, 1.0, tile, -1, ws_bytes=ws_bytes), f"linear_bf16 tile {tile} stream-K {(M, N, Kd)}")
    err = rel_inf(got["out"].float(), ref)
    print(f"   stream-K tile {tile}: rel-inf {err:.3e} (gate 1e-2)")
    assert err < 1e-2
    assert int(got["flags"].view(torch.int32).abs().sum()) == 0


@pytest.mark.parametrize("split_k", [-18, -19, -3])
def test_linear_bf16_8phase_k_lockstep_split(K, split_k):
    """The K-lockstep split of the 8-phase kernel (test_gemm_8phase_k_lockstep_split; `split_k` = -(16 + S), or -3: S from the cost model): S chunks per
    tile, `tiles * S` fp32 slots of 256 x 256 in accumulator layout in a guarded workspace, `sk_finish_kernel` with the epilogue.  One row and eight
    columns over a tile in M and N; five k-tiles in S = 2 / 3 chunks (the last one shorter), twelve for the model's own choice."""
    M, N = 257, 264
    Kd = 768 if split_k == -3 else 320
    tiles, S_max = 2 * 2, 16
    x, w, b, r, _, _ = _gemm_data(M, N, Kd, 860)
    ref, mag = _gemm_ref(x, w, b, r, None, 0.5)
    got = _run(lambda g: _linear(K, g, x, w, b, r, None, 0.5, 13, split_k, ws_bytes=4096 + tiles * S_max * 256 * 256 * 4),
               f"linear_bf16 tile 13 k-lockstep split_k {split_k} {(M, N, Kd)}")
    _check_linear(got["out"], ref, mag, False, f"k-lockstep {split_k}")
    assert int(got["flags"].view(torch.int32).abs().sum()) == 0


def test_linear_bf16_8phase_hybrid_stream_k(K):
    """The hybrid form of the 8-phase kernel (test_gemm_8phase_arms: 256 + 13, `split_k` = -2): the whole rounds of tiles on the plain grid, the last
    partial round (64 tiles here) through the two stream-K launches.  The smallest problem the arm does not hand back: more tiles than CUs and
    rem * K / 64 >= 2 CUs; M one row, N eight columns over a tile."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g8, tiles_n, rem = cus & ~7, 16, 64
    tiles_m = (g8 + rem) // tiles_n
    assert tiles_m * tiles_n == g8 + rem
    M, N, Kd = 256 * (tiles_m - 1) + 1, 256 * (tiles_n - 1) + 8, 64 * -(-2 * g8 // rem)
    x, w, b, r, _, _ = _gemm_data(M, N, Kd, 870)
    ref = F.linear(x.float(), w.float(), b.float()) + r.float()
    got = _run(lambda g: _linear(K, g, x, w, b, r, None, 1.0, 13, -2, ws_bytes=4096 + g8 * 3 * 256 * 256 * 4), f"linear_bf16 tile 13 hybrid stream-K {(M, N, Kd)}")
    err = rel_inf(got["out"].float(), ref)
    print(f"   hybrid stream-K: rel-inf {err:.3e} (gate 1e-2)")
    assert err < 1e-2
    assert int(got["flags"].view(torch.int32).abs().sum()) == 0


@pytest.mark.parametrize("M,N,Kd,extras", [(161, 200, 128, 3), (321, 168, 64, 0)])
def test_linear4_bf16_forward(K, M, N, Kd, extras):
    """`fmc_linear4_bf16`: 160 x 160 tiles, one row over, ragged N, the shortest reduction (test_linear4_small_m_projection's small shapes)."""
    x, w, b, r, r2, _ = _gemm_data(M, N, Kd, 971)
    b, r, r2 = (b if extras >= 1 else None), (r if extras >= 2 else None), (r2 if extras >= 3 else None)
    alpha = 0.7 if extras >= 2 else 1.0
    ref, mag = _gemm_ref(x, w, b, r, r2, alpha)

    def fn(g):
        xd, wd = g.inp(x, GEMM_BAND, 64, "x"), g.inp(w, GEMM_BAND_W, 0, "w")
        bd = g.inp(b, _vec_band(N), 0, "bias") if b is not None else None
        rd = g.inp(r, GEMM_BAND, 8, "residual") if r is not None else None
        r2d = g.inp(r2, GEMM_BAND, 8, "residual2") if r2 is not None else None
        out = g.out((M, N), BF16, GEMM_BAND, 8, "out")
        assert K._lib.load().fmc_linear4_supported(M, N, Kd, xd.stride(0))
        _call(K, "fmc_linear4_bf16", xd.data_ptr(), wd.data_ptr(), _p(bd), _p(rd), _p(r2d), out.data_ptr(), M, N, Kd, xd.stride(0),
              rd.stride(0) if r is not None else 0, out.stride(0), alpha, K._stream())
        return {"out": out}

    got = _run(fn, f"linear4_bf16 {(M, N, Kd)} extras {extras}")["out"]
    assert_bf16_close(got, ref, mag, f"linear4 {(M, N, Kd)}")


@pytest.mark.parametrize("tile,split_k", [(1, 1), (13, 1), (16, 1), (2, 2)])
def test_linear_x3_f32_forward(K, tile, split_k):
    """`fmc_linear_x3_f32` (test_linear_f32_split3): the split-bf16 x3 operands guarded (A with ldx > 3 K), fp32 bias / residuals / out."""
    M, N, Kd = 129, 320 if tile == 16 else 72, 64
    gen = torch.Generator().manual_seed(900)
    x, w = torch.randn(M, Kd, generator=gen), torch.randn(N, Kd, generator=gen) * Kd ** -0.5
    b, r, r2 = torch.randn(N, generator=gen), torch.randn(M, N, generator=gen), torch.randn(M, N, generator=gen)
    x3, w3 = K.split_bf16x3(x.cuda(), 0).cpu(), K.split_bf16x3(w.cuda(), 1).cpu()

    def fn(g):
        xd, wd = g.inp(x3, GEMM_BAND, 64, "x3"), g.inp(w3, GEMM_BAND_W, 0, "w3")
        bd, rd, r2d = g.inp(b, _vec_band(N), 0, "bias"), g.inp(r, GEMM_BAND, 8, "residual"), g.inp(r2, GEMM_BAND, 8, "residual2")
        out = g.out((M, N), F32, GEMM_BAND, 8, "out")
        ws, nbytes = (g.out((split_k * M, N), F32, GEMM_BAND, 0, "split-K workspace"), split_k * M * N * 4) if split_k > 1 else (None, 0)
        _call(K, "fmc_linear_x3_f32", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rd.data_ptr(), out.data_ptr(), M, N, 3 * Kd, xd.stride(0), rd.stride(0),
              out.stride(0), 0.7, 0, tile, split_k, _p(ws), nbytes, r2d.data_ptr(), K._stream())
        return {"out": out}

    got = _run(fn, f"linear_x3_f32 tile {tile} split {split_k}")["out"]
    ref = 0.7 * (x.double() @ w.double().t() + b.double()) + r.double() + r2.double()
    mag = 0.7 * (x.abs().double() @ w.abs().double().t() + b.abs()) + r.abs() + r2.abs()
    assert_f32_close(got, ref, mag, f"linear_x3_f32 tile {tile}")


# =====================================================================================================================================
# Convolutions.  Rows are PIXELS (channels-last): a ring / 8-phase tile is up to 256 pixels and reads one image row + 1 pixel either side;
# a halo tile is 10 x 32 (+ halo) or 320 pixels of whole row blocks; the filter is read by up to 320 output channels x 9 taps.
# =====================================================================================================================================
CONV_BAND = 448                      # pixels around x, residual and out
CONV_BAND_W = 320 * 9                # rows of [Cout * 9, Cin] around the filter and its packed copies


def _conv_data(n, hs, ws, cin, cout, seed, c2=0, h=None, w=None, temb_rows=None):
    h, w = (hs, ws) if h is None else (h, w)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, hs, ws, cin - c2, generator=gen).bfloat16()
    x2 = torch.randn(n, hs, ws, c2, generator=gen).bfloat16() if c2 else None
    wt = (torch.randn(cout, cin, 3, 3, generator=gen) * (9 * cin) ** -0.5).bfloat16().contiguous(memory_format=torch.channels_last)
    bias = torch.randn(cout, generator=gen).bfloat16()
    temb = torch.randn(n if temb_rows is None else temb_rows, cout, generator=gen).bfloat16()
    res = torch.randn(n, h, w, cout, generator=gen).bfloat16()
    return x, x2, wt, bias, temb, res


def _conv_ref(x, x2, wt, bias=None, temb=None, res=None, temb_div=1, mode=0, coef=None, act=True):
    """tests/test_gpu_conv_halo.py `_ref`, plus stride 2 (mode 2); mode 1 = nearest 2x upsample in front."""
    xin = x.float() if x2 is None else torch.cat([x.float(), x2.float()], -1)
    if coef is not None:
        z = xin * coef[:, None, None, :, 0] + coef[:, None, None, :, 1]
        xin = (F.silu(z) if act else z).bfloat16().float()
    xin = xin.permute(0, 3, 1, 2)
    if mode == 1:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    y = F.conv2d(xin, wt.float(), None if bias is None else bias.float(), stride=2 if mode == 2 else 1, padding=1)
    if temb is not None:
        y = y + temb.float().repeat_interleave(temb_div, 0)[:, :, None, None]
    if res is not None:
        y = y + res.float().permute(0, 3, 1, 2)
    return y.permute(0, 2, 3, 1)


def _pixels(t):
    return t.reshape(-1, t.shape[-1])


def _filter_rows(wt):
    """The channels-last filter as its physical `[Cout * 9, Cin]` rows."""
    cout, cin = wt.shape[:2]
    return wt.permute(0, 2, 3, 1).reshape(cout * 9, cin)


def _conv_operands(g, x, x2, bias, temb, res):
    xd = g.inp(_pixels(x), CONV_BAND, 0, "x")
    x2d = g.inp(_pixels(x2), CONV_BAND, 0, "x2") if x2 is not None else None
    bd = g.inp(bias, _vec_band(bias.shape[0]), 0, "bias") if bias is not None else None
    td = g.inp(temb, 64, 8, "temb") if temb is not None else None                  # rows of a wider projection: temb_row_stride > Cout
    rd = g.inp(_pixels(res), CONV_BAND, 0, "residual") if res is not None else None
    return xd, x2d, bd, td, rd


# (n, source H, source W, Cin, Cout, mode, tile, extras): test_conv3x3_bf16_fused_epilogue / _stride2 / _fused_upsample and their tiles
CONV_CASES = ([(3, 9, 7, 640, 320, 0, 0, False), (3, 9, 7, 640, 320, 0, 16, True), (3, 9, 7, 640, 320, 0, 18, True)]      # (18: the filter tile-major, `_w_tilemajor_conv`)
              + [(3, 20, 28, 128, 320, 2, t, False) for t in (0, 2, 5, 11)]
              + [(3, 10, 14, 128, 320, 1, t, False) for t in (0, 1, 3, 11)]
              + [(18, 10, 14, 128, 320, 1, 128 + 2, False)])      # stream-K on tile 2 (256 x 128): 40 x 3 tiles x 18 k-tiles >= 4 x 512 workgroups, so the launch is cut


@pytest.mark.parametrize("n,hs,ws,cin,cout,mode,tile,extras", CONV_CASES)
def test_conv3x3_bf16_forward(K, n, hs, ws, cin, cout, mode, tile, extras):
    h, w = {0: (hs, ws), 1: (2 * hs, 2 * ws), 2: (hs // 2, ws // 2)}[mode]
    x, _, wt, bias, temb, res = _conv_data(n, hs, ws, cin, cout, 70 + tile + mode, h=h, w=w)
    temb, res = (temb, res) if extras else (None, None)
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def fn(g):
        xd, _, bd, td, rd = _conv_operands(g, x, None, bias, temb, res)
        wrows = _filter_rows(wt)
        if tile == 18:
            wrows = wrows.reshape(cout // 320, 320, 9, cin // 64, 2, 32).permute(0, 3, 2, 4, 1, 5).contiguous().view(cout * 9, cin)
        wd = g.inp(wrows, CONV_BAND_W, 0, "w")
        out = g.out((n * h * w, cout), BF16, CONV_BAND, 0, "out")
        ws, nbytes = _ws(g, 4096 + 2 * cus * 256 * 128 * 4, flags=True) if tile >= 128 else (None, 0)
        _call(K, "fmc_conv3x3_bf16", xd.data_ptr(), wd.data_ptr(), _p(bd), _p(td), _p(rd), out.data_ptr(), n, h, w, cin, cout, td.stride(0) if extras else 0, 1,
              mode, tile & 127, -1 if tile >= 128 else 1, _p(ws), nbytes, K._stream())
        if tile >= 128:
            torch.cuda.synchronize()
            used = int((ws.view(-1)[1024:].view(torch.int32) != EG.SENTINEL[F32][1]).sum())
            assert used > 0, "stream-K: no partial slot was written -- the launch fell back to the plain grid"
            return {"out": out, "flags": ws.view(-1)[:1024]}
        return {"out": out}

    res3 = _run(fn, f"conv3x3_bf16 {(n, hs, ws, cin, cout)} mode {mode} tile {tile}")
    if tile >= 128:
        assert int(res3["flags"].view(torch.int32).abs().sum()) == 0
    got = res3["out"].view(n, h, w, cout)
    err = rel_inf(got.float(), _conv_ref(x, None, wt, bias, temb, res, 1, mode))
    print(f"   rel-inf {err:.3e} (gate 1e-2)")
    assert err < 1e-2


def test_conv3x3_bf16_split_k_workspace(K):
    """test_gemm_split_k's conv: 5 x 8 images, ragged Cout, the partials in a guarded workspace."""
    n, h, w, cin, cout, tile, split_k = 2, 5, 8, 256, 136, 1, 2
    x, _, wt, _, temb, res = _conv_data(n, h, w, cin, cout, 54)

    def fn(g):
        xd, _, _, td, rd = _conv_operands(g, x, None, None, temb, res)
        wd = g.inp(_filter_rows(wt), CONV_BAND_W, 0, "w")
        out = g.out((n * h * w, cout), BF16, CONV_BAND, 0, "out")
        ws = g.out((split_k * n * h * w, cout), F32, CONV_BAND, 0, "split-K workspace")
        _call(K, "fmc_conv3x3_bf16", xd.data_ptr(), wd.data_ptr(), None, td.data_ptr(), rd.data_ptr(), out.data_ptr(), n, h, w, cin, cout, td.stride(0), 1, 0,
              tile, split_k, ws.data_ptr(), split_k * n * h * w * cout * 4, K._stream())
        return {"out": out}

    got = _run(fn, "conv3x3_bf16 split-K 2")["out"].view(n, h, w, cout)
    assert rel_inf(got.float(), _conv_ref(x, None, wt, None, temb, res)) < 1e-2


def test_conv3x3_x3_f32_forward(K):
    n, h, w, cin, cout = 2, 9, 7, 64, 72
    gen = torch.Generator().manual_seed(901)
    x, wt = torch.randn(n, cin, h, w, generator=gen), torch.randn(cout, cin, 3, 3, generator=gen) * (9 * cin) ** -0.5
    b, t, r = torch.randn(cout, generator=gen), torch.randn(1, cout, generator=gen), torch.randn(n, cout, h, w, generator=gen)
    x3 = K.split_bf16x3(x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous().cuda(), 0).cpu()
    w3 = K.split_bf16x3(wt.permute(0, 2, 3, 1).reshape(cout * 9, cin).contiguous().cuda(), 1).cpu()

    def fn(g):
        xd, wd = g.inp(x3, CONV_BAND, 0, "x3"), g.inp(w3, CONV_BAND_W, 0, "w3")
        bd, td = g.inp(b, _vec_band(cout), 0, "bias"), g.inp(t, 64, 8, "temb")
        rd = g.inp(r.permute(0, 2, 3, 1).reshape(-1, cout), CONV_BAND, 0, "residual")
        out = g.out((n * h * w, cout), F32, CONV_BAND, 0, "out")
        _call(K, "fmc_conv3x3_x3_f32", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), td.data_ptr(), rd.data_ptr(), out.data_ptr(), n, h, w, 3 * cin, cout,
              td.stride(0), 2, 0, 0, 1, None, 0, K._stream())
        return {"out": out}

    got = _run(fn, "conv3x3_x3_f32")["out"].view(n, h, w, cout).permute(0, 3, 1, 2)
    tt = t.repeat_interleave(2, dim=0)[:, :, None, None].double()
    ref = F.conv2d(x.double(), wt.double(), None, 1, 1) + b.double()[None, :, None, None] + tt + r.double()
    mag = F.conv2d(x.abs().double(), wt.abs().double(), None, 1, 1) + b.abs()[None, :, None, None] + tt.abs() + r.abs()
    assert_f32_close(got, ref, mag, "conv3x3_x3_f32")                            # (test_conv3x3_f32_split3)


def test_conv3x3_bf16_gn_forward(K):
    """`fmc_conv3x3_bf16_gn` (tile 16, row-major filter): 160 pixels per image = one statistics tile each, the partials guarded."""
    n, h, w, cin, cout = 3, 10, 16, 64, 320
    x, _, wt, bias, temb, res = _conv_data(n, h, w, cin, cout, 951)

    def fn(g):
        xd, _, bd, td, rd = _conv_operands(g, x, None, bias, temb, res)
        wd = g.inp(_filter_rows(wt), CONV_BAND_W, 0, "w")
        out = g.out((n * h * w, cout), BF16, CONV_BAND, 0, "out")
        part = g.out((n * (h * w // 160), 64), F32, 8, 0, "gn_partials")
        _call(K, "fmc_conv3x3_bf16_gn", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), td.data_ptr(), rd.data_ptr(), out.data_ptr(), n, h, w, cin, cout, td.stride(0),
              1, 0, part.data_ptr(), 0, K._stream())
        return {"out": out, "gn_partials": part}

    got = _run(fn, "conv3x3_bf16_gn")
    out = got["out"].view(n, h, w, cout)
    assert rel_inf(out.float(), _conv_ref(x, None, wt, bias, temb, res)) < 1e-2
    o = out.float().cpu().reshape(n, h * w, 32, cout // 32)
    part = got["gn_partials"].view(n, -1, 32, 2).sum(1)
    assert rel_inf(part[..., 0], o.sum((1, 3))) < 1e-4 and rel_inf(part[..., 1], (o * o).sum((1, 3))) < 1e-5    # (test_groupnorm_statistics_from_the_producing_epilogue)


def _packed(K, g, fn_name, wt, factor, *args):
    """The filter through a pack routine into a guarded buffer (checked on the pack kernel's output side), then as a poisoned operand."""
    cout, cin = wt.shape[:2]
    wd = g.inp(_filter_rows(wt), CONV_BAND_W, 0, "w")
    dst = g.out((cout * factor, cin), BF16, CONV_BAND_W, 0, f"packed filter ({fn_name})")
    _call(K, fn_name, wd.data_ptr(), dst.data_ptr(), cin, cout, *args, K._stream())
    return g.inp(dst.clone(), CONV_BAND_W, 0, "packed filter (as an operand)")


def _check_partials(got, out, n, cout):
    o = out.float().cpu().reshape(n, -1, 32, cout // 32)
    s_ref = torch.stack([o.sum((1, 3)), (o * o).sum((1, 3))], -1)
    assert rel_inf(got.view(n, -1, 32, 2).sum(1), s_ref) < 1e-4               # (test_gpu_conv_halo.py)


# (n, H, W, Cin, Cout, c2, upsample, extras, gn): test_conv3x3_halo_matches_fp32_conv's edges; gn = the GroupNorm operand path + statistics epilogue
HALO_CASES = [(1, 7, 32, 64, 160, 0, False, False, False), (2, 24, 32, 192, 160, 0, False, True, False), (2, 20, 32, 320, 320, 128, False, True, False),
              (2, 20, 64, 128, 160, 0, True, True, False), (2, 20, 32, 128, 320, 0, False, False, True)]


@pytest.mark.parametrize("n,h,w,cin,cout,c2,ups,extras,gn", HALO_CASES)
def test_conv3x3_halo_forward(K, n, h, w, cin, cout, c2, ups, extras, gn):
    L = K._lib.load()
    hs, ws = (h // 2, w // 2) if ups else (h, w)
    assert L.fmc_conv3x3_halo_supported(n, h, w, cin, cin - c2, cout, int(ups))
    div = 2 if extras else 1
    x, x2, wt, bias, temb, res = _conv_data(n, hs, ws, cin, cout, h + cin, c2, h, w, temb_rows=n // div)
    if not extras:
        bias = temb = res = None
    coef = None
    if gn:
        x = (x.float() * 1.7 + 0.3).bfloat16()
        gamma, beta = _rnd((cin,), 5, F32, 0.3, 1.0), _rnd((cin,), 6, F32, 0.2)
        xs = x.float().reshape(n, 2, h * w // 2, 32, cin // 32)
        part = torch.stack([xs.sum((2, 4)), (xs * xs).sum((2, 4))], -1).contiguous()
        coef = K.groupnorm_coef(part.cuda(), gamma.cuda(), beta.cuda(), h * w, cin, 32, 1e-5).cpu()
    tiles = L.fmc_conv3x3_halo_tiles_per_image(h, w)

    def fn(g):
        xd, x2d, bd, td, rd = _conv_operands(g, x, x2, bias, temb, res)
        wp = _packed(K, g, "fmc_conv3x3_halo_pack_weight", wt, 9)
        cd = g.inp(coef.view(n * cin, 2), 512, 0, "gn_coef") if gn else None
        out = g.out((n * h * w, cout), BF16, CONV_BAND, 0, "out")
        part = g.out((n * tiles, 64), F32, max(tiles, 4), 0, "gn_partials") if gn else None
        _call(K, "fmc_conv3x3_halo_bf16", xd.data_ptr(), _p(x2d), cin - c2, wp.data_ptr(), _p(bd), _p(td), _p(rd), out.data_ptr(), n, h, w, cin, cout,
              td.stride(0) if extras else 0, div, int(ups), _p(cd), 1, _p(part), K._stream())
        return {"out": out, "gn_partials": part} if gn else {"out": out}

    got = _run(fn, f"conv3x3_halo {(n, h, w, cin, cout)} c2 {c2} ups {ups} extras {extras} gn {gn}")
    out = got["out"].view(n, h, w, cout)
    err = rel_inf(out, _conv_ref(x, x2, wt, bias, temb, res, div, int(ups), coef, act=True))
    print(f"   rel-inf {err:.3e} (gate {'8e-3' if gn else '6e-3'})")
    assert err < (8e-3 if gn else 6e-3)
    if gn:
        _check_partials(got["gn_partials"], out, n, cout)


# (n, H, W, Cin, Cout, c2, extras, split_k, wide): test_conv3x3_halo4_matches_fp32_conv's edges
HALO4_CASES = [(11, 5, 8, 64, 80, 0, False, 1, False), (5, 10, 16, 192, 160, 0, True, 1, False), (3, 16, 16, 64, 80, 0, True, 1, False),
               (6, 10, 16, 256, 160, 128, True, 1, False), (5, 10, 16, 192, 160, 0, True, 2, False), (2, 20, 32, 128, 160, 0, True, 1, True)]


@pytest.mark.parametrize("n,h,w,cin,cout,c2,extras,split_k,wide", HALO4_CASES)
def test_conv3x3_halo4_forward(K, n, h, w, cin, cout, c2, extras, split_k, wide):
    L = K._lib.load()
    assert L.fmc_conv3x3_halo4_supported(n, h, w, cin, cin - c2, cout, 0, int(wide))
    div = 2 if extras and n % 2 == 0 else 1
    x, x2, wt, bias, temb, res = _conv_data(n, h, w, cin, cout, h + cin + n, c2, temb_rows=n // div)
    if not extras:
        bias = temb = res = None
    emit = split_k == 1 and cout % 64 == 0 and (160 if wide else 80) % (cout // 32) == 0
    blocks = L.fmc_conv3x3_halo4_row_blocks_per_image(h, w)

    def fn(g):
        xd, x2d, bd, td, rd = _conv_operands(g, x, x2, bias, temb, res)
        wp = _packed(K, g, "fmc_conv3x3_halo4_pack_weight", wt, 9, int(wide))
        out = g.out((n * h * w, cout), BF16, CONV_BAND, 0, "out")
        part = g.out((n * blocks, 64), F32, max(blocks, 4), 0, "gn_partials") if emit else None
        ws = g.out((split_k * n * h * w, cout), F32, CONV_BAND, 0, "split-K workspace") if split_k > 1 else None
        _call(K, "fmc_conv3x3_halo4_bf16", xd.data_ptr(), _p(x2d), cin - c2, wp.data_ptr(), _p(bd), _p(td), _p(rd), out.data_ptr(), n, h, w, cin, cout,
              td.stride(0) if extras else 0, div, 0, _p(part), split_k, _p(ws), split_k * n * h * w * cout * 4 if split_k > 1 else 0, int(wide), K._stream())
        return {"out": out, "gn_partials": part} if emit else {"out": out}

    got = _run(fn, f"conv3x3_halo4 {(n, h, w, cin, cout)} c2 {c2} extras {extras} split {split_k} wide {wide}")
    out = got["out"].view(n, h, w, cout)
    err = rel_inf(out, _conv_ref(x, x2, wt, bias, temb, res, div))
    print(f"   rel-inf {err:.3e} (gate 6e-3)")
    assert err < 6e-3
    if emit:
        _check_partials(got["gn_partials"], out, n, cout)


# (arm, n, source H, source W, Cin, Cout): the smallest sources of tests/test_conv_upsample_fold.py's EDGE_SHAPES
FOLD_CASES = [("halo", 2, 7, 64, 64, 320), ("halo4", 11, 5, 8, 64, 80), ("halo4w", 2, 10, 32, 128, 160)]


@pytest.mark.parametrize("arm,n,hs,ws,cin,cout", FOLD_CASES)
def test_conv3x3_fold_forward(K, arm, n, hs, ws, cin, cout):
    L = K._lib.load()
    wide = arm == "halo4w"
    if arm == "halo":
        assert L.fmc_conv3x3_halo_fold_supported(n, hs, ws, cin, cout)
        splits = 4 * L.fmc_conv3x3_halo_tiles_per_image(hs, ws)
    else:
        assert L.fmc_conv3x3_halo4_fold_supported(n, hs, ws, cin, cout, int(wide))
        splits = 4 * L.fmc_conv3x3_halo4_row_blocks_per_image(hs, ws)
    bn = 80 if arm == "halo4" else 160
    emit = cout % 64 == 0 and bn % (cout // 32) == 0
    x, _, wt, bias, _, _ = _conv_data(n, hs, ws, cin, cout, hs + cin + n)

    def fn(g):
        xd, _, bd, _, _ = _conv_operands(g, x, None, bias, None, None)
        wp = _packed(K, g, "fmc_conv3x3_upfold_pack_weight", wt, 16, bn)
        out = g.out((n * 4 * hs * ws, cout), BF16, 4 * CONV_BAND, 0, "out")
        part = g.out((n * splits, 64), F32, max(splits, 4), 0, "gn_partials") if emit else None
        if arm == "halo":
            _call(K, "fmc_conv3x3_halo_fold_bf16", xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), out.data_ptr(), n, hs, ws, cin, cout, _p(part), K._stream())
        else:
            _call(K, "fmc_conv3x3_halo4_fold_bf16", xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), out.data_ptr(), n, hs, ws, cin, cout, _p(part), int(wide),
                  K._stream())
        return {"out": out, "gn_partials": part} if emit else {"out": out}

    got = _run(fn, f"conv3x3 fold {arm} {(n, hs, ws, cin, cout)}")
    out = got["out"].view(n, 2 * hs, 2 * ws, cout)
    err = rel_inf(out, _conv_ref(x, None, wt, bias, mode=1))
    print(f"   rel-inf {err:.3e} (gate 6e-3)")
    assert err < 6e-3
    if emit:
        _check_partials(got["gn_partials"], out, n, cout)

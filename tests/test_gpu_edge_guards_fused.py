"""The fused forward kernels at the far ends of their operands: the GEGLU epilogue of the GEMMs, the tile-16-only entry points (`fmc_linear_bf16_gn` /
`_ln` / `_lnc` / `_ffblk` / `_fftail` / `_imgw`, `fmc_groupnorm_fold_linear`), the fused temporal blocks, the direct LayerNorm + GEGLU kernels, the
convolution loaders of the hybrid and K-lockstep forms, and the fp8 q | k | v projection.

The conventions of tests/test_gpu_edge_guards.py: raw C ABI, every operand (packed weights included) in an arena of the test's own
(tests/edge_guard_common.py), every case under zeros, quiet NaN and +Inf around the inputs.  These kernels refuse ragged M, so the edge here is the END
of each operand: a persistent loop that asks for "the next tile" once too often, a buffer descriptor a row too long, a second-segment loader past
`k_split`, a side output (ln_out, ln_stats, gn_partials, amax, a tile-major block) one block too far.  Asserted per case:

  1. every output and side output is finite and BIT-IDENTICAL across the three runs (`torch.equal`);
  2. the zeros run meets the reference and the gate of the kernel's own test in tests/test_gpu_kernels.py (restated next to each case; no new
     tolerance); where that gate is bit-identity with another launch, the other launch runs on plain tensors;
  3. every word outside an output view keeps the sentinel and every word inside was written; `amax_bits`, which the ABI accumulates into, starts at
     zero and only its outside is checked; the poison around every input is still in place.

Persistent forms run with one tile MORE than `hip_ops._cus()` compute units (one workgroup runs a second tile, the one-ahead prefetch of every other
workgroup has no target); forms that take "at least as many tiles as CUs" also run with exactly that many.  Bands in ROWS of the guarded tensor, next
to the case tables with the source line they come from.  One run is recorded in profiles/edge_guards.md."""
import functools

import pytest
import torch
import torch.nn.functional as F

from synfmc_amd.models.layers import interleave_geglu
from tests import edge_guard_common as EG
from tests.test_gpu_edge_guards import (CONV_BAND, CONV_BAND_W, GEMM_BAND, GEMM_BAND_W, _call, _conv_data, _conv_ref, _filter_rows, _gemm_data, _p, _pixels,
                                        _rnd, _run, _tilemajor, _vec_band, _ws)
from tests.test_gpu_kernels import assert_bf16_close, rel_inf

pytestmark = pytest.mark.gpu

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8

# Tile 16 / 17 / 18 (gemm_conv.hip: gemm160p_kernel): 160-row (17: 256-row) x 320-column tiles; the persistent form requests the NEXT tile's operands
# under the epilogue, so a workgroup's reach past its last tile is one whole tile: 320 rows of A cover both tile heights, and one `[160][32]`-blocked
# tile column of a tile-major intermediate is 160 x 32 = 5120 elements, less than 320 rows of any width used here (>= 128).
P_BAND = 320                          # rows of A, residuals, out, ln_out, tile-major intermediates (gemm_conv.hip, `linear_impl`: tile 16's persistent form only)
P_BAND_W = 320                        # rows of W and of its tile-major copy: one 320-column block (hip_ops._w_tilemajor)
STAT_BAND = 320                       # rows of ln_stats [M][2]: one tile of rows each side
PART_BAND = 8                         # rows of 64 floats around gn_partials: >= the tiles of one image in these cases, as the existing file's rule


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _cus(K):
    return K._cus(torch.device("cuda", torch.cuda.current_device()))


def _dev(t):
    return None if t is None else t.cuda()


def _blocked(t):
    """`[M, C]` -> tile-major `[M / 160][C / 32][160][32]`, as `[M, C]` rows for the guard."""
    M, C = t.shape
    return t.view(M // 160, 160, C // 32, 32).permute(0, 2, 1, 3).contiguous().view(M, C)


def _unblocked(t):
    M, C = t.shape
    return t.reshape(M // 160, C // 32, 160, 32).permute(0, 2, 1, 3).reshape(M, C)


def _geglu_ref(x, w, b):
    """fp64 GEGLU of `[value rows | gate rows]` weights with the `mag` of test_gemm_256x320_persistent_geglu."""
    y = x.double() @ w.double().t()
    m = x.abs().double() @ w.abs().double().t()
    if b is not None:
        y, m = y + b.double(), m + b.abs().double()
    (a, g), (ma, mg) = y.chunk(2, dim=-1), m.chunk(2, dim=-1)
    return a * F.gelu(g), F.gelu(g).abs() * ma + 1.13 * a.abs() * mg + 1e-3


# =====================================================================================================================================
# fmc_linear_bf16, epilogue = 1 (GEGLU): every tile geometry that takes it
# =====================================================================================================================================
def _linear_geglu(K, g, x, w, b, tile, split_k=1, ws_bytes=0):
    """`w`, `b` in [value | gate] order; interleaved here as the arm wants (blocks of 32; 8 for tiles 16 / 17 / 18; 18 also tile-major)."""
    M, Kd = x.shape
    N = w.shape[0]
    wi, bi = interleave_geglu(w, b, 8 if tile in (16, 17, 18) else 32)
    if tile == 18:
        wi = _tilemajor(wi)
    xd = g.inp(x, GEMM_BAND, 64, "x")
    wd = g.inp(wi, GEMM_BAND_W, 0, "w")
    bd = g.inp(bi, _vec_band(N), 0, "bias") if b is not None else None
    out = g.out((M, N // 2), BF16, GEMM_BAND, 8, "out")
    ws, nbytes = _ws(g, ws_bytes, flags=True) if split_k < 0 else (None, 0)
    _call(K, "fmc_linear_bf16", xd.data_ptr(), wd.data_ptr(), _p(bd), None, out.data_ptr(), M, N, Kd, xd.stride(0), 0, out.stride(0), 1.0, 1, tile, split_k,
          _p(ws), nbytes, None, 0, 0, None, K._stream())
    res = {"out": out}
    if split_k < 0:
        res["flags"] = ws.view(-1)[:1024]
        torch.cuda.synchronize()
        used = int((ws.view(-1)[1024:].view(torch.int32) != EG.SENTINEL[F32][1]).sum())
        assert used > 0, "no partial slot was written -- the launch fell back to the plain grid"
    return res


def _check_geglu(got, x, w, b, elementwise, what):
    ref, mag = _geglu_ref(x, w, b)
    err = rel_inf(got.float(), ref)
    print(f"   {what}: rel-inf {err:.3e} (gate 1e-2)" + (", element-wise bf16 bound" if elementwise else ""))
    assert err < 1e-2                                                            # (test_gemm_tile_geometries_agree, test_gemm_8phase_arms)
    if elementwise:
        assert_bf16_close(got, ref, mag, what)                                   # (test_gemm_160x320_arm, test_gemm_256x320_persistent_geglu)


# (tile, M, N, K): ragged M and N = 7 x 64 (a multiple of 64, of no tile width: 128 / 256 / 320) where the arm takes them; tile 16 / 18: N % 320 == 0
GEGLU_TILES = ([(t, 257, 448, 320) for t in range(1, 13)] + [(t, 257, 448, 64) for t in (13, 14)] + [(13, 257, 448, 320)]
               + [(t, 161, 640, 64) for t in (16, 18)])


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("tile,M,N,Kd", GEGLU_TILES)
def test_linear_bf16_geglu_plain_grid(K, tile, M, N, Kd, bias):
    x, w, b, _, _, _ = _gemm_data(M, N, Kd, 300 + tile)
    b = b if bias else None
    got = _run(lambda g: _linear_geglu(K, g, x, w, b, tile), f"linear_bf16 GEGLU tile {tile} {(M, N, Kd)} {'bias' if bias else 'no bias'}")["out"]
    _check_geglu(got, x, w, b, tile in (16, 18), f"GEGLU tile {tile}")


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("tile", [16, 17, 18])
def test_linear_bf16_geglu_persistent_form(K, tile, bias):
    """CUs + 1 tiles of 160 x 320 (17: 256 x 320, M % 256 == 0).  Tiles 17 and 18 give the bits of tile 16 on plain tensors."""
    rows = 256 if tile == 17 else 160
    M, N, Kd = rows * (_cus(K) + 1), 320, 64
    x, w, b, _, _, _ = _gemm_data(M, N, Kd, 320)
    b = b if bias else None
    got = _run(lambda g: _linear_geglu(K, g, x, w, b, tile), f"linear_bf16 GEGLU tile {tile} persistent {(M, N, Kd)} {'bias' if bias else 'no bias'}")["out"]
    _check_geglu(got, x, w, b, True, f"GEGLU tile {tile} persistent")
    if tile != 16:
        wi, bi = interleave_geglu(w.cuda(), _dev(b), 8)
        assert torch.equal(got, K.linear_bf16(x.cuda(), wi, bi, geglu=True, tile=K.ARM_160)), f"tile {tile} differs from tile 16 on plain tensors"


def test_linear_bf16_geglu_stream_k(K):
    """Stream-K of the ring kernel with the GEGLU epilogue (test_gemm_stream_k's GEGLU leg), the smallest problem the arm does not hand back."""
    cus = _cus(K)
    M, N = 1025, 1088                                                            # 9 x 9 tiles of 128 x 128; N = 17 x 64
    Kd = 64 * -(-4 * 2 * cus // (9 * 9))
    x, w, b, _, _, _ = _gemm_data(M, N, Kd, 345)
    got = _run(lambda g: _linear_geglu(K, g, x, w, b, 1, -1, 4096 + 2 * cus * 128 * 128 * 4), f"linear_bf16 GEGLU tile 1 stream-K {(M, N, Kd)}")
    _check_geglu(got["out"], x, w, b, False, "GEGLU stream-K tile 1")
    assert int(got["flags"].view(torch.int32).abs().sum()) == 0


def test_linear_bf16_geglu_k_lockstep(K):
    """K-lockstep split of the 8-phase kernel with the GEGLU epilogue: its own finishing launch (test_gemm_8phase_k_lockstep_split's GEGLU leg)."""
    M, N, Kd = 257, 320, 320
    x, w, b, _, _, _ = _gemm_data(M, N, Kd, 861)
    got = _run(lambda g: _linear_geglu(K, g, x, w, b, 13, -18, 4096 + 2 * 2 * 16 * 256 * 256 * 4), f"linear_bf16 GEGLU tile 13 k-lockstep -18 {(M, N, Kd)}")
    _check_geglu(got["out"], x, w, b, False, "GEGLU k-lockstep -18")
    assert int(got["flags"].view(torch.int32).abs().sum()) == 0


# =====================================================================================================================================
# The tile-16-only entry points.  Operand names and checks (gemm_conv.hip, `linear_impl`).
# =====================================================================================================================================
def _w16(g, w, tm, name="w"):
    return g.inp(_tilemajor(w) if tm else w, P_BAND_W, 0, name)


def _plain16(K, x, w, b, r, alpha, r2=None):
    """Tile 16 on plain tensors: the launch the fused entry points must agree with bit for bit."""
    return K.linear_bf16(x.cuda(), w.cuda(), _dev(b), _dev(r), alpha, tile=K.ARM_160, residual2=_dev(r2))


def _check_gn_partials(part, out, what):
    """(sum, sum of squares) per (160-row tile, group of N / 32 channels) of the ROUNDED outputs: 1e-4 (test_ff_tail_*, test_groupnorm_statistics_*)."""
    M, N = out.shape
    v = out.float().view(M // 160, 160, 32, N // 32)
    part = part.view(M // 160, 32, 2)
    e0, e1 = rel_inf(part[..., 0], v.sum(dim=(1, 3))), rel_inf(part[..., 1], (v * v).sum(dim=(1, 3)))
    print(f"   {what}: gn_partials rel-inf sum {e0:.2e} squares {e1:.2e} (gate 1e-4)")
    assert e0 < 1e-4 and e1 < 1e-4


@pytest.mark.parametrize("tm", [0, 1], ids=["rowmajor-w", "tilemajor-w"])
@pytest.mark.parametrize("form", ["plain-grid", "persistent"])
def test_linear_bf16_gn(K, form, tm):
    """`fmc_linear_bf16_gn`: plain grid (4 tiles) and persistent form (CUs + 1 tiles); images of one 160-row tile, so gn_partials has a row per tile."""
    M, N, Kd = (320, 640, 64) if form == "plain-grid" else (160 * (_cus(K) + 1), 320, 64)
    x, w, b, r, r2, _ = _gemm_data(M, N, Kd, 410)

    def fn(g):
        xd, wd, bd = g.inp(x, P_BAND, 64, "x"), _w16(g, w, tm), g.inp(b, _vec_band(N), 0, "bias")
        rd, r2d = g.inp(r, P_BAND, 8, "residual"), g.inp(r2, P_BAND, 8, "residual2")
        out = g.out((M, N), BF16, P_BAND, 8, "out")
        part = g.out((M // 160, 64), F32, PART_BAND, 0, "gn_partials")
        _call(K, "fmc_linear_bf16_gn", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rd.data_ptr(), out.data_ptr(), M, N, Kd, xd.stride(0), rd.stride(0),
              out.stride(0), 0.5, r2d.data_ptr(), part.data_ptr(), 160, tm, K._stream())
        return {"out": out, "gn_partials": part}

    what = f"linear_bf16_gn {form} {(M, N, Kd)} w_tilemajor {tm}"
    got = _run(fn, what)
    assert torch.equal(got["out"], _plain16(K, x, w, b, r, 0.5, r2)), "out differs from the plain tile-16 launch"
    _check_gn_partials(got["gn_partials"], got["out"], what)


LN_FRAMES, LN_INNER = 3, 160           # a positional-encoding row per 160-row tile, three of them in turn: tiles 2, 5, 8, ... read the table's last row


@pytest.mark.parametrize("residuals", [1, 2])
@pytest.mark.parametrize("mode", ["ln_out+pe", "ln_stats"])
def test_linear_bf16_ln(K, mode, residuals):
    """`fmc_linear_bf16_ln`, CUs + 1 tiles: out = the plain tile-16 launch's bits; ln_out against the fp64 LayerNorm (+ pe row) of the rounded out,
    ln_stats against its fp64 mean / rstd (test_linear_with_the_consumers_layernorm_in_its_epilogue, test_layernorm_applied_in_the_consuming_gemm)."""
    M, N, Kd = 160 * (_cus(K) + 1), 320, 64
    x, w, b, r, r2, _ = _gemm_data(M, N, Kd, 420)
    r2 = r2 if residuals == 2 else None
    gamma, beta, pe = _rnd((N,), 421, F32, 0.3, 1.0), _rnd((N,), 422, F32, 0.2), _rnd((LN_FRAMES, N), 423, F32)
    with_out = mode == "ln_out+pe"

    def fn(g):
        xd, wd, bd, rd = g.inp(x, P_BAND, 64, "x"), _w16(g, w, 1), g.inp(b, _vec_band(N), 0, "bias"), g.inp(r, P_BAND, 8, "residual")
        r2d = g.inp(r2, P_BAND, 8, "residual2") if r2 is not None else None
        gd, btd = g.inp(gamma, _vec_band(N), 0, "ln_gamma"), g.inp(beta, _vec_band(N), 0, "ln_beta")
        ped = g.inp(pe, _vec_band(N), 0, "ln_pe") if with_out else None
        out = g.out((M, N), BF16, P_BAND, 8, "out")
        ln_out = g.out((M, N), BF16, P_BAND, 0, "ln_out") if with_out else None
        stats = None if with_out else g.out((M, 2), F32, STAT_BAND, 0, "ln_stats")
        _call(K, "fmc_linear_bf16_ln", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rd.data_ptr(), out.data_ptr(), M, N, Kd, xd.stride(0), rd.stride(0),
              out.stride(0), 0.5, _p(r2d), _p(ln_out), gd.data_ptr(), btd.data_ptr(), 1e-5, _p(ped), LN_INNER if with_out else 1, LN_FRAMES if with_out else 1,
              _p(stats), 1, K._stream())
        return {"out": out, "ln_out": ln_out} if with_out else {"out": out, "ln_stats": stats}

    what = f"linear_bf16_ln {mode} residuals {residuals} {(M, N, Kd)}"
    got = _run(fn, what)
    assert torch.equal(got["out"], _plain16(K, x, w, b, r, 0.5, r2)), "out differs from the plain tile-16 launch"
    o64 = got["out"].double().cpu()
    mu, var = o64.mean(-1, keepdim=True), o64.var(-1, unbiased=False, keepdim=True)
    if with_out:
        rows = (torch.arange(M) // LN_INNER) % LN_FRAMES
        ref = (o64 - mu) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double() + pe.double()[rows]
        mag = (o64 - mu).abs() / torch.sqrt(var + 1e-5) * gamma.double().abs() + beta.double().abs() + pe.double()[rows].abs()
        assert_bf16_close(got["ln_out"], ref, 8.0 * mag + 1.0, what)
    else:
        st = got["ln_stats"].double().cpu()
        e_mu, e_rstd = float((st[:, 0] - mu[:, 0]).abs().max()), float((st[:, 1] * torch.sqrt(var[:, 0] + 1e-5) - 1.0).abs().max())
        print(f"   {what}: |mean err| {e_mu:.2e} (gate {1e-5 * (1.0 + float(mu.abs().max())):.1e}), rstd rel err {e_rstd:.2e} (gate 1e-4)")
        assert e_mu < 1e-5 * (1.0 + float(mu.abs().max())) and e_rstd < 1e-4


def _lnc_operands(x, w, b, gamma, beta, block=None):
    """What `hip_ops._ln_folded_weight` builds: (W diag(gamma) in bf16, its row sums, W beta + b), and (mean, rstd) of the rows of x in fp32."""
    if block is not None:
        w, b = interleave_geglu(w, b, block)
    wg = (w.float() * gamma[None, :]).to(BF16).contiguous()
    x64 = x.double()
    stats = torch.stack([x64.mean(-1), (x64.var(-1, unbiased=False) + 1e-5).rsqrt()], -1).float().contiguous()
    return wg, wg.float().sum(dim=1).contiguous(), (w.float() @ beta + b.float()).contiguous(), stats


def _lnc_reference(x, w, b, gamma, beta, geglu):
    """fp64 LayerNorm + projection of the same bf16 rows with the bound of test_layernorm_applied_in_the_consuming_gemm."""
    x64 = x.double()
    ln = (x64 - x64.mean(-1, keepdim=True)) / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + 1e-5) * gamma.double() + beta.double()
    y, m = ln @ w.double().t() + b.double(), ln.abs() @ w.abs().double().t() + b.abs().double()
    if not geglu:
        return y, 2.0 ** -7 * m + 2.0 ** -8 * y.abs() + 1e-3
    (a, gt), (ma, mg) = y.chunk(2, dim=-1), m.chunk(2, dim=-1)
    ref = a * F.gelu(gt)
    return ref, 2.0 ** -7 * (F.gelu(gt).abs() * ma + 1.13 * a.abs() * mg) + 2.0 ** -8 * ref.abs() + 2e-3


@pytest.mark.parametrize("geglu", [False, True], ids=["plain", "geglu"])
def test_linear_bf16_lnc(K, geglu):
    """`fmc_linear_bf16_lnc`: N = 320 and CUs + 1 tiles; GEGLU: N = 640 (two column tiles per row tile) and CUs + 2, the next count above CUs."""
    cus = _cus(K)
    M, N, Kd = (160 * (cus // 2 + 1), 640, 64) if geglu else (160 * (cus + 1), 320, 64)
    x, w, b, _, _, _ = _gemm_data(M, N, Kd, 430)
    x = (x.float() + 0.5).to(BF16)                                               # (a row mean to cancel in acc - mean c)
    gamma, beta = _rnd((Kd,), 431, F32, 0.3, 1.0), _rnd((Kd,), 432, F32, 0.2)
    wg, c, lb, stats = _lnc_operands(x, w, b, gamma, beta, 8 if geglu else None)
    n_out = N // 2 if geglu else N

    def fn(g):
        xd, wd = g.inp(x, P_BAND, 64, "x"), _w16(g, wg, 1, "w_gamma")
        sd, cd, lbd = g.inp(stats, STAT_BAND, 0, "ln_stats"), g.inp(c, _vec_band(N), 0, "ln_c"), g.inp(lb, _vec_band(N), 0, "ln_bias")
        out = g.out((M, n_out), BF16, P_BAND, 8, "out")
        _call(K, "fmc_linear_bf16_lnc", xd.data_ptr(), wd.data_ptr(), out.data_ptr(), M, N, Kd, xd.stride(0), out.stride(0), int(geglu), sd.data_ptr(),
              cd.data_ptr(), lbd.data_ptr(), 1, K._stream())
        return {"out": out}

    what = f"linear_bf16_lnc {'GEGLU' if geglu else 'plain'} {(M, N, Kd)}"
    got = _run(fn, what)["out"]
    ref, bound = _lnc_reference(x, w, b, gamma, beta, geglu)
    worst = float(((got.double().cpu() - ref).abs() / bound).max())
    print(f"   {what}: worst error in units of its bound {worst:.3f}")
    assert worst < 1.0


@pytest.mark.parametrize("ln", [False, True], ids=["bias", "layernorm"])
def test_linear_bf16_ffblk_out_blocked(K, ln):
    """The GEGLU projection writing its gated output tile-major (`out_blocked`), plain and with its input's LayerNorm applied (`ln_stats` / `ln_c` /
    `ln_bias`): the tile-major tensor is the row-major launch's on plain tensors, permuted (test_feed_forward_with_a_tile_major_intermediate)."""
    cus = _cus(K)
    M, N, Kd = 160 * (cus // 2 + 1), 640, 64                                     # CUs + 2 tiles of 160 x 320
    x, w, b, _, _, _ = _gemm_data(M, N, Kd, 440)
    gamma, beta = _rnd((Kd,), 441, F32, 0.3, 1.0), _rnd((Kd,), 442, F32, 0.2)
    wi, bi = interleave_geglu(w, b, 8)
    wg, c, lb, stats = _lnc_operands(x, w, b, gamma, beta, 8)

    def fn(g):
        xd = g.inp(x, P_BAND, 0, "x")
        out = g.out((M, N // 2), BF16, P_BAND, 0, "out (tile-major)")
        if ln:
            wd, sd = _w16(g, wg, 1, "w_gamma"), g.inp(stats, STAT_BAND, 0, "ln_stats")
            cd, lbd = g.inp(c, _vec_band(N), 0, "ln_c"), g.inp(lb, _vec_band(N), 0, "ln_bias")
            extra = (None, None, out.data_ptr(), M, N, Kd, 0, 1.0, 1, 0, 1, sd.data_ptr(), cd.data_ptr(), lbd.data_ptr(), 1)
        else:
            wd, bd = _w16(g, wi, 1), g.inp(bi, _vec_band(N), 0, "bias")
            extra = (bd.data_ptr(), None, out.data_ptr(), M, N, Kd, 0, 1.0, 1, 0, 1, None, None, None, 1)
        _call(K, "fmc_linear_bf16_ffblk", xd.data_ptr(), wd.data_ptr(), *extra, K._stream())
        return {"out": out}

    got = _unblocked(_run(fn, f"linear_bf16_ffblk out_blocked {'+ LayerNorm' if ln else 'bias'} {(M, N, Kd)}")["out"])
    if ln:                                                                       # the row-major `fmc_linear_bf16_lnc` on plain tensors
        xd, wt, sd, cd, lbd = x.cuda(), _tilemajor(wg).cuda(), stats.cuda(), c.cuda(), lb.cuda()
        want = torch.empty(M, N // 2, dtype=BF16, device="cuda")
        _call(K, "fmc_linear_bf16_lnc", xd.data_ptr(), wt.data_ptr(), want.data_ptr(), M, N, Kd, Kd, N // 2, 1, sd.data_ptr(), cd.data_ptr(), lbd.data_ptr(), 1,
              K._stream())
    else:
        want = K.linear_bf16(x.cuda(), wi.cuda(), bi.cuda(), geglu=True, tile=K.ARM_160)
    assert torch.equal(got, want), "the tile-major intermediate is not the row-major one permuted"


@pytest.mark.parametrize("res", [True, False], ids=["residual", "noresidual"])
def test_linear_bf16_ffblk_x_blocked(K, res):
    """The second GEMM of the feed-forward reading its A operand tile-major (`x_blocked`), CUs + 1 tiles: the bits of the row-major launch."""
    M, N, Kd = 160 * (_cus(K) + 1), 320, 128
    x, w, b, r, _, _ = _gemm_data(M, N, Kd, 450)
    r = r if res else None

    def fn(g):
        xd, wd, bd = g.inp(_blocked(x), P_BAND, 0, "x (tile-major)"), _w16(g, w, 1), g.inp(b, _vec_band(N), 0, "bias")
        rd = g.inp(r, P_BAND, 8, "residual") if res else None
        out = g.out((M, N), BF16, P_BAND, 0, "out")
        _call(K, "fmc_linear_bf16_ffblk", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), _p(rd), out.data_ptr(), M, N, Kd, rd.stride(0) if res else 0, 1.0, 0, 1, 0,
              None, None, None, 1, K._stream())
        return {"out": out}

    got = _run(fn, f"linear_bf16_ffblk x_blocked {'residual' if res else 'no residual'} {(M, N, Kd)}")["out"]
    assert torch.equal(got, _plain16(K, x, w, b, r, 1.0)), "differs from the row-major launch on plain tensors"


@pytest.mark.parametrize("gn", [True, False], ids=["gn_partials", "nopartials"])
@pytest.mark.parametrize("extra_tiles", [0, 1], ids=["tiles=CUs", "tiles=CUs+1"])
def test_linear_bf16_fftail(K, extra_tiles, gn):
    """`fmc_linear_bf16_fftail`: the reduction's first segment (k_split = 128 of K = 192: a multiple of 64 and 32, not K / 2) from the tile-major g, the
    second from row-major x2 with ldx2 = 64 + 64 spare columns.  Element-wise against the folded product in fp64
    (test_ff_tail_folded_output_projection_and_proj_out)."""
    M, N, Kd, ks = 160 * (_cus(K) + extra_tiles), 320, 192, 128
    gx, w, b, r, _, h = _gemm_data(M, N, ks, 460, Kd - ks)

    def fn(g):
        gd, hd = g.inp(_blocked(gx), P_BAND, 0, "x (tile-major)"), g.inp(h, P_BAND, 64, "x2")
        wd, bd, rd = _w16(g, w, 1), g.inp(b, _vec_band(N), 0, "bias"), g.inp(r, P_BAND, 8, "residual")
        out = g.out((M, N), BF16, P_BAND, 0, "out")
        part = g.out((M // 160, 64), F32, PART_BAND, 0, "gn_partials") if gn else None
        _call(K, "fmc_linear_bf16_fftail", gd.data_ptr(), hd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rd.data_ptr(), out.data_ptr(), M, N, Kd, ks, hd.stride(0),
              rd.stride(0), _p(part), 160 if gn else 0, 1, K._stream())
        return {"out": out, "gn_partials": part} if gn else {"out": out}

    what = f"linear_bf16_fftail tiles CUs + {extra_tiles} {'gn_partials' if gn else 'no partials'} {(M, N, Kd)}"
    got = _run(fn, what)
    a64 = torch.cat([gx, h], dim=1).double()
    folded = a64 @ w.double().t() + b.double() + r.double()
    mag = a64.abs() @ w.double().abs().t() + b.double().abs() + r.double().abs()
    assert_bf16_close(got["out"], folded, mag, what)
    if gn:
        _check_gn_partials(got["gn_partials"], got["out"], what)


@pytest.mark.parametrize("with_ln", [True, False], ids=["ln_stats", "nostats"])
@pytest.mark.parametrize("splits", [1, 4])
@pytest.mark.parametrize("extra_tiles", [0, 1], ids=["tiles=CUs", "tiles=CUs+4"])
def test_groupnorm_fold_linear_and_imgw(K, extra_tiles, splits, with_ln):
    """`fmc_groupnorm_fold_linear` -> `fmc_linear_bf16_imgw`, four images (the middle ones' weight blocks have finite neighbours, the last has none) of
    CUs / 4 tiles each (tiles == CUs) and of one more each (CUs + 4: a prime CUs + 1 has no such factorisation).  The fold's outputs land in guarded
    outputs and are then the projection's guarded inputs.  Gates of test_linear_gnfold_groupnorm_folded_into_per_image_weights."""
    n_img, C, N, G = 4, 64, 320, 32
    hw = 160 * (_cus(K) // n_img + extra_tiles)
    M = n_img * hw
    gen = torch.Generator().manual_seed(470)
    base = torch.randn(n_img, hw, C, generator=gen) * (0.5 + torch.rand(n_img, 1, C, generator=gen))
    shift = (torch.rand(n_img, 1, G, generator=gen) * 12.0 - 6.0).repeat_interleave(C // G, dim=2)
    x = (base + shift).to(BF16)
    xo = x.float()
    gam, bet = _rnd((C,), 471, F32, 0.3, 1.0), _rnd((C,), 472, F32, 0.3)
    w, b = _rnd((N, C), 473, BF16, C ** -0.5), _rnd((N,), 474, BF16, 0.2)
    v = xo.view(n_img, splits, hw // splits, G, C // G)
    part = torch.stack([v.sum(dim=(2, 4)), (v * v).sum(dim=(2, 4))], dim=-1).contiguous()                 # [n_img, splits, 32, 2]

    def fn(g):
        pd = g.inp(part.view(n_img * splits, G * 2), PART_BAND, 0, "partials")
        gd, btd = g.inp(gam, _vec_band(C), 0, "gamma"), g.inp(bet, _vec_band(C), 0, "beta")
        wd, bd = g.inp(w, P_BAND_W, 0, "w"), g.inp(b, _vec_band(N), 0, "bias")
        w_img = g.out((n_img * N, C), BF16, P_BAND_W, 0, "w_img")
        b_img = g.out((n_img, N), F32, 2, 0, "bias_img")
        _call(K, "fmc_groupnorm_fold_linear", pd.data_ptr(), splits, gd.data_ptr(), btd.data_ptr(), wd.data_ptr(), bd.data_ptr(), w_img.data_ptr(), b_img.data_ptr(),
              n_img, hw, C, G, N, 1e-6, 1, K._stream())
        torch.cuda.synchronize()
        wi, bi = g.inp(w_img.cpu(), P_BAND_W, 0, "w_img (as the projection's operand)"), g.inp(b_img.cpu(), 2, 0, "bias_img (as the projection's operand)")
        xd = g.inp(x.view(M, C), P_BAND, 64, "x")
        out = g.out((M, N), BF16, P_BAND, 8, "out")
        stats = g.out((M, 2), F32, STAT_BAND, 0, "ln_stats") if with_ln else None
        _call(K, "fmc_linear_bf16_imgw", xd.data_ptr(), wi.data_ptr(), bi.data_ptr(), out.data_ptr(), M, N, C, xd.stride(0), out.stride(0), hw, _p(stats),
              1e-5 if with_ln else 0.0, 1, K._stream())
        res = {"w_img": w_img, "bias_img": b_img, "out": out}
        if with_ln:
            res["ln_stats"] = stats
        return res

    what = f"groupnorm_fold_linear + linear_bf16_imgw images {n_img} hw {hw} splits {splits} {'ln_stats' if with_ln else 'no stats'}"
    got = _run(fn, what)
    out = got["out"].view(n_img, hw, N)
    want = F.linear(F.group_norm(xo.transpose(1, 2), G, gam, bet, 1e-6).transpose(1, 2), w.float(), b.float())
    err = rel_inf(out, want)
    print(f"   {what}: rel-inf {err:.3e} (gate 1.2e-2)")
    assert err < 1.2e-2
    s = part.double().sum(dim=1)
    cnt = hw * (C // G)
    mean = s[..., 0] / cnt
    rstd = 1.0 / torch.sqrt((s[..., 1] / cnt - mean * mean).clamp_min(0) + 1e-6)
    a = rstd.float().repeat_interleave(C // G, dim=1) * gam[None, :]
    wq = (w.float()[None] * a[:, None, :]).to(BF16).double()
    xc = xo.double() - mean.repeat_interleave(C // G, dim=1)[:, None, :]
    folded = torch.einsum("imc,inc->imn", xc, wq) + (w.double() @ bet.double() + b.double())[None, None, :]
    mag = torch.einsum("imc,inc->imn", xc.abs(), wq.abs()) + (w.double().abs() @ bet.double().abs() + b.double().abs())[None, None, :]
    assert_bf16_close(out, folded, mag * 4, what)
    if with_ln:
        rws = out.float().cpu().view(-1, N)
        assert rel_inf(got["ln_stats"][:, 0], rws.mean(dim=1)) < 1e-3 and rel_inf(got["ln_stats"][:, 1], (rws.var(dim=1, unbiased=False) + 1e-5).rsqrt()) < 1e-3


# =====================================================================================================================================
# fmc_temporal_block_bf16 (temporal_block.hip: C = 320, 160-row tiles = 10 pixels x 16 frames, persistent over min(tiles, CUs) workgroups,
# temporal_block.hip:800-805; temporal_block640.hip: C = 640, 80-row tiles = 5 pixels x 16 frames, one workgroup per tile, :839-842)
# =====================================================================================================================================
TB_BAND = 320                          # rows of h / pose_term / out around them: two 160-row tiles (four 80-row ones)
TB_BAND_W = 320                        # rows of C elements around each packed weight: >= one head's fragment block (C = 320: 40960 elements = 128 rows,
                                       # pack_temporal_qkv; C = 640: 153600 = 240 rows, pack_temporal_qkv80; a wave's 51200 = 80 rows, pack_w_frag80)


def _tb_shapes(K, C):
    px = 10 if C == 320 else 5
    return [(1, px), (3, 7 * px), (1, px * (_cus(K) + 1))]                        # one tile; 21 tiles (an odd count below the CUs); CUs + 1 tiles


@functools.lru_cache(maxsize=None)
def _tb_case(C, B, hw, merge):
    """Inputs (CPU), packed weights, and the two references of test_temporal_block_fused / _640 computed in fp32 on the device (the same restatement;
    the large cases are 20 000 - 41 000 rows)."""
    from synfmc_amd import hip_ops as K
    H, Fr, d, s = 8, 16, C // 8, 0.7
    h = _rnd((B, Fr, hw, C), 1, BF16, 1.5, 0.2)
    gamma, beta, pe = _rnd((C,), 2, F32, 0.3, 1.0), _rnd((C,), 3, F32, 0.2), _rnd((32, C), 4, F32, 0.7)
    wq, wo, bo = _rnd((3 * C, C), 5, BF16, C ** -0.5 * 1.5), _rnd((C, C), 6, BF16, C ** -0.5), _rnd((C,), 7, BF16, 0.3)
    wm, bm, pose = _rnd((C, C), 8, BF16, C ** -0.5), _rnd((C,), 9, BF16, 0.3), _rnd((B, Fr, hw, C), 10, BF16)
    bpe = (beta[None] + pe[:Fr]).contiguous()
    f = lambda t: t.float().cuda()
    pt = (s * (F.linear(f(pose), f(wm)) + f(bm))).bfloat16() if merge else None                 # the pose term the kernel reads, rounded once

    def reference(round_bf16):
        r = (lambda t: t.bfloat16().float()) if round_bf16 else (lambda t: t)
        x = r(F.layer_norm(f(h), (C,), f(gamma), f(beta), 1e-5) + f(pe)[None, :Fr, None, :])
        m = r(s * F.linear(x, f(wm)) + pt.float() + x) if merge else x
        qkv = r(F.linear(m, f(wq)))
        q, k, v = (t.reshape(B, Fr, hw, H, d).permute(0, 2, 3, 1, 4) for t in qkv.chunk(3, dim=-1))
        p = r(torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1))
        o = r(p @ v).permute(0, 3, 1, 2, 4).reshape(B, Fr, hw, C)
        return (F.linear(o, f(wo), f(bo)) + f(h)).cpu()
    if C == 320:
        packed = (K.pack_temporal_qkv(wq), _tilemajor(wo), _tilemajor(wm))
    else:
        packed = (K.pack_temporal_qkv80(wq), K.pack_w_frag80(wo), K.pack_w_frag80(wm))
    return h, gamma, bpe, bo, (pt.cpu() if merge else None), packed, reference(True), reference(False), s


def _temporal_block(K, C, shape_index, merge, stats):
    B, hw = _tb_shapes(K, C)[shape_index]
    h, gamma, bpe, bo, pt, (wq_p, wo_p, wm_p), ref_r, ref_f, s = _tb_case(C, B, hw, merge)
    rows, d = B * 16 * hw, C // 8

    def fn(g):
        hd = g.inp(h.view(rows, C), TB_BAND, 0, "h")
        gd, bpd, bod = g.inp(gamma, _vec_band(C), 0, "ln_gamma"), g.inp(bpe, 2, 0, "ln_bpe"), g.inp(bo, _vec_band(C), 0, "b_out")
        wqd, wod = g.inp(wq_p.view(-1, C), TB_BAND_W, 0, "w_qkv_packed"), g.inp(wo_p.reshape(-1, C), TB_BAND_W, 0, "w_out")
        wmd = g.inp(wm_p.reshape(-1, C), TB_BAND_W, 0, "w_merge") if merge else None
        ptd = g.inp(pt.view(rows, C), TB_BAND, 0, "pose_term") if merge else None
        out = g.out((rows, C), BF16, TB_BAND, 0, "out")
        st = g.out((rows, 2), F32, TB_BAND, 0, "ln_stats") if stats else None
        _call(K, "fmc_temporal_block_bf16", hd.data_ptr(), out.data_ptr(), gd.data_ptr(), bpd.data_ptr(), 1e-5, _p(wmd), _p(ptd), s, wqd.data_ptr(), wod.data_ptr(),
              bod.data_ptr(), _p(st), 1e-5 if stats else 0.0, B, 16, hw, C, 8, d ** -0.5, K._stream())
        return {"out": out, "ln_stats": st} if stats else {"out": out}

    what = f"temporal_block C {C} B {B} hw {hw} merge {merge} ln_stats {stats}"
    got = _run(fn, what)
    out = got["out"].float().cpu().view(B, 16, hw, C)
    e_f = rel_inf(out, ref_f)
    err = (out - ref_r).abs()
    bound = 2.0 ** -8 * ref_r.abs() + 1.5 * 2.0 ** -8 * float(ref_r.abs().max())             # (test_temporal_block_fused / _640)
    print(f"   {what}: rel-inf {e_f:.3e} (gate 2e-2), worst error in units of the fused blocks' bound {float((err / bound).max()):.3f}")
    assert e_f < 2e-2
    assert not bool((err > bound).any()), f"{int((err > bound).sum())} / {err.numel()} beyond the bound"
    if stats:
        o = got["out"].float()
        mu, rstd = o.mean(-1).view(-1), (o.var(-1, unbiased=False) + 1e-5).rsqrt().view(-1)
        assert rel_inf(got["ln_stats"][:, 0], mu) < 1e-4 and rel_inf(got["ln_stats"][:, 1], rstd) < 1e-4


@pytest.mark.parametrize("stats", [True, False], ids=["ln_stats", "nostats"])
@pytest.mark.parametrize("merge", [True, False], ids=["merge", "nomerge"])
@pytest.mark.parametrize("shape_index", [0, 1, 2], ids=["one-tile", "21-tiles", "CUs+1-tiles"])
def test_temporal_block_320(K, shape_index, merge, stats):
    _temporal_block(K, 320, shape_index, merge, stats)


@pytest.mark.parametrize("merge", [True, False], ids=["merge", "nomerge"])
@pytest.mark.parametrize("shape_index", [0, 1, 2], ids=["one-tile", "21-tiles", "CUs+1-tiles"])
def test_temporal_block_640(K, shape_index, merge):
    _temporal_block(K, 640, shape_index, merge, False)


# =====================================================================================================================================
# fmc_geglu640_ln_bf16 / fmc_geglu320_ln_bf16 (temporal_block640.hip:889-929) and fmc_geglu_pipe_ln_bf16 (geglu_pipe.hip:346-372): one workgroup per
# 80-row (or 160-row) tile, grid = M / 80 or M / 160; one or two workgroups fit a CU, so 2 (CUs + 1) tiles of 80 rows are more than a full round.
# =====================================================================================================================================
GL_BAND = 320                          # rows of h and out: two 160-row tiles; also >= one `[160][32]` block of the tile-major output
GL_BAND_W = 320                        # rows of C elements around the packed weight: >= one chunk's fragment stream (80 x C or 2 x 32 x C elements)

# (kernel, C, smallest cff, a cff with an odd chunk count): chunks of 320 (direct 640), 160 (direct 320), 128 (pipe)
GL_KERNELS = {"geglu640": (640, 320, 960), "geglu320": (320, 160, 480), "pipe0-320": (320, 128, 384), "pipe0-640": (640, 128, 384), "pipe1-320": (320, 128, 384)}


# (rows, which cff, tile-major out, bias): one tile row-major; one tile more than a full round, row-major on the smallest cff and tile-major on the odd
# chunk count; 160 rows (the smallest tile-major output) without bias
GL_FORMS = {"one-tile": (None, 0, False, True), "round+1": ("big", 0, False, False), "round+1-tilemajor": ("big", 1, True, True),
            "160-rows-tilemajor": (160, 1, True, False)}


@functools.lru_cache(maxsize=None)
def _gl_case(C, M, cff):
    h, gamma, beta = _rnd((M, C), 1, BF16, 1.5, 0.2), _rnd((C,), 2, F32, 0.3, 1.0), _rnd((C,), 3, F32, 0.2)
    w, b = _rnd((2 * cff, C), 4, BF16, C ** -0.5), _rnd((2 * cff,), 5, BF16, 0.3)
    f = lambda t: t.float().cuda()

    def reference(round_bf16, bias):
        n = F.layer_norm(f(h), (C,), f(gamma), f(beta), 1e-5)
        y = F.linear(n.bfloat16().float() if round_bf16 else n, f(w), f(b) if bias else None)
        return (y[:, :cff] * F.gelu(y[:, cff:])).cpu()
    refs = {bias: (reference(True, bias), reference(False, bias)) for bias in (True, False)}
    return h, gamma, beta, w, b, refs


@pytest.mark.parametrize("form", list(GL_FORMS))
@pytest.mark.parametrize("name", list(GL_KERNELS))
def test_geglu_ln_direct_and_pipe(K, name, form):
    M, which, blocked, bias = GL_FORMS[form]
    M = 160 * (_cus(K) + 1) if M == "big" else (160 if name == "pipe1-320" else 80) if M is None else M
    C, cff = GL_KERNELS[name][0], GL_KERNELS[name][1 + which]
    h, gamma, beta, w, b, refs = _gl_case(C, M, cff)
    ref_r, ref_f = refs[bias]
    variant = 1 if name == "pipe1-320" else 0
    wp = K.pack_geglu_frag(w, 16 if variant else 32) if name.startswith("pipe") else K.pack_geglu_frag80(w)

    def fn(g):
        hd, gd, btd = g.inp(h, GL_BAND, 0, "h"), g.inp(gamma, _vec_band(C), 0, "ln_gamma"), g.inp(beta, _vec_band(C), 0, "ln_beta")
        wd = g.inp(wp.view(-1, C), GL_BAND_W, 0, "w_packed")
        bd = g.inp(b, _vec_band(2 * cff), 0, "bias") if bias else None
        out = g.out((M, cff), BF16, GL_BAND, 0, "out (tile-major)" if blocked else "out")
        if name.startswith("pipe"):
            assert K._lib.load().fmc_geglu_pipe_supported(M, cff, C, variant)
            _call(K, "fmc_geglu_pipe_ln_bf16", hd.data_ptr(), out.data_ptr(), gd.data_ptr(), btd.data_ptr(), 1e-5, wd.data_ptr(), _p(bd), M, cff, C, int(blocked),
                  variant, K._stream())
        else:
            _call(K, f"fmc_{name}_ln_bf16", hd.data_ptr(), out.data_ptr(), gd.data_ptr(), btd.data_ptr(), 1e-5, wd.data_ptr(), _p(bd), M, cff, int(blocked),
                  K._stream())
        return {"out": out}

    what = f"{name} M {M} cff {cff} {'tile-major' if blocked else 'row-major'} {'bias' if bias else 'no bias'}"
    got = _run(fn, what)["out"]
    got = (_unblocked(got) if blocked else got).float().cpu()
    e_f = rel_inf(got, ref_f)
    err = (got - ref_r).abs()
    bound = 2.0 ** -8 * ref_r.abs() + 0.02                                       # (test_geglu_ln_direct, test_geglu_ln_pipe)
    print(f"   {what}: rel-inf {e_f:.3e} (gate 2e-2), worst error in units of 2^-8 |ref| + 0.02: {float((err / bound).max()):.3f}")
    assert e_f < 2e-2
    assert not bool((err > bound).any()), f"{int((err > bound).sum())} / {err.numel()} beyond the bound"


# =====================================================================================================================================
# fmc_conv3x3_bf16 on the hybrid (split_k = -2) and K-lockstep (-18, -3) forms of the 8-phase kernel (tiles 13 / 14: 256 pixels x 256 channels,
# gemm_conv.hip:2498-2576): the convolution loaders with a last tile that hangs over the last image row
# =====================================================================================================================================
def _conv8_shape(K, split_k, upsample):
    """(h, w, cin, cout, workspace bytes).  Hybrid: more tiles than CUs with a partial last round of 64 (`rem * K / 64 >= 2 CUs`, gemm_conv.hip:2513-2518):
    one image 62 pixels wide, so no tile boundary falls on a row end.  K-lockstep: 2 x 2 tiles, nine k-tiles in two chunks."""
    if split_k == -2:
        g8, rem = _cus(K), 64
        tiles_m = (g8 + rem) // 2
        w = 62
        h = (256 * tiles_m - 1) // w
        h -= h & 1 if upsample else 0
        assert 256 * (tiles_m - 1) < h * w < 256 * tiles_m
        return h, w, 64, 320, 4096 + g8 * 3 * 256 * 256 * 4
    return (10, 26, 64, 264, 4096 + 4 * 16 * 256 * 256 * 4) if upsample else (9, 29, 64, 264, 4096 + 4 * 16 * 256 * 256 * 4)


@functools.lru_cache(maxsize=None)
def _conv8_case(h, w, cin, cout, upsample):
    hs, ws = (h // 2, w // 2) if upsample else (h, w)
    x, _, wt, bias, _, res = _conv_data(1, hs, ws, cin, cout, 880 + upsample, h=h, w=w)
    return x, wt, bias, res, _conv_ref(x, None, wt, bias, None, res, 1, int(upsample))


@pytest.mark.parametrize("upsample", [False, True], ids=["stride1", "upsample"])
@pytest.mark.parametrize("split_k", [-2, -18, -3])
@pytest.mark.parametrize("tile", [13, 14])
def test_conv3x3_bf16_8phase_hybrid_and_k_lockstep(K, tile, split_k, upsample):
    h, w, cin, cout, ws_bytes = _conv8_shape(K, split_k, upsample)
    x, wt, bias, res, ref = _conv8_case(h, w, cin, cout, upsample)

    def fn(g):
        xd, bd, rd = g.inp(_pixels(x), CONV_BAND, 0, "x"), g.inp(bias, _vec_band(cout), 0, "bias"), g.inp(_pixels(res), CONV_BAND, 0, "residual")
        wd = g.inp(_filter_rows(wt), CONV_BAND_W, 0, "w")
        out = g.out((h * w, cout), BF16, CONV_BAND, 0, "out")
        ws, nbytes = _ws(g, ws_bytes, flags=True)
        _call(K, "fmc_conv3x3_bf16", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, rd.data_ptr(), out.data_ptr(), 1, h, w, cin, cout, 0, 1, int(upsample), tile,
              split_k, ws.data_ptr(), nbytes, K._stream())
        torch.cuda.synchronize()
        used = int((ws.view(-1)[1024:].view(torch.int32) != EG.SENTINEL[F32][1]).sum())
        assert used > 0, "no partial slot was written -- the launch fell back to the plain grid"
        return {"out": out, "flags": ws.view(-1)[:1024]}

    what = f"conv3x3_bf16 tile {tile} split_k {split_k} {'upsample' if upsample else 'stride 1'} {(h, w, cin, cout)}"
    got = _run(fn, what)
    assert int(got["flags"].view(torch.int32).abs().sum()) == 0
    err = rel_inf(got["out"].view(1, h, w, cout).float(), ref)
    print(f"   {what}: rel-inf {err:.3e} (gate 1e-2)")
    assert err < 1e-2                                                            # (test_gemm_8phase_arms / test_gemm_8phase_k_lockstep_split's conv legs)


# =====================================================================================================================================
# fmc_linear_fp8_qkv (gemm_conv.hip: the 8-phase 256 x 256 kernel with an e4m3 epilogue) and fmc_fp8_scales_roll
# =====================================================================================================================================
FP8_TOP = 16.0                         # |acc * inv_scale| <= 16 = byte 0x58: no output byte can equal the sentinel 0x5A (= 20.0), so "every byte written" holds


@pytest.mark.parametrize("with_amax", [True, False], ids=["amax", "noamax"])
@pytest.mark.parametrize("M,C,Kd", [(257, 64, 128), (257, 320, 320)])
def test_linear_fp8_qkv(K, M, C, Kd, with_amax):
    """Ragged M; out_fp8 bytes in a byte-sentinel arena, `amax_bits` (atomicMax of non-negative float bit patterns: order-free, bit-compared) starting at
    zero in an arena of its own, and NULL as a second run.  Gates of test_linear_fp8_qkv_epilogue."""
    x = _rnd((M, Kd), 70, BF16)
    w = torch.randn(3 * C, Kd, generator=torch.Generator().manual_seed(71)) * Kd ** -0.5
    w[C:2 * C] *= 3.0
    w = w.to(BF16)
    ref = F.linear(x.float(), w.float())
    blocks = [ref[:, i * C:(i + 1) * C] for i in range(3)]
    scale = torch.tensor([float(b.abs().max()) / FP8_TOP for b in blocks])
    inv = (1.0 / scale).float()

    def fn(g):
        xd, wd, ivd = g.inp(x, GEMM_BAND, 64, "x"), g.inp(w, GEMM_BAND_W, 0, "w"), g.inp(inv, 8, 0, "inv_scales")
        out = g.out((M, 3 * C), U8, GEMM_BAND, 0, "out_fp8")
        amax = g.out((3,), F32, 8, 0, "amax_bits", init=0.0) if with_amax else None
        _call(K, "fmc_linear_fp8_qkv", xd.data_ptr(), wd.data_ptr(), out.data_ptr(), M, 3 * C, Kd, xd.stride(0), ivd.data_ptr(), _p(amax), K._stream())
        return {"out_fp8": out, "amax_bits": amax} if with_amax else {"out_fp8": out}

    what = f"linear_fp8_qkv {(M, C, Kd)} {'amax' if with_amax else 'amax NULL'}"
    got = _run(fn, what)
    out = got["out_fp8"].view(torch.float8_e4m3fn).float().cpu()
    for i, b in enumerate(blocks):
        s = float(scale[i])
        if with_amax:
            assert abs(float(got["amax_bits"][i]) - float(b.abs().max())) < 2e-3 * float(b.abs().max())
        have = out[:, i * C:(i + 1) * C] * s
        want = (b / s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float() * s
        exact = (have == want).float().mean().item()
        print(f"   {what} block {i}: {exact:.4f} of the bytes exact (gate 0.98)")
        assert exact > 0.98
        assert bool(((have - want).abs() <= 0.13 * torch.maximum(have.abs(), want.abs()).clamp_min(s * 2 ** -6)).all())


def test_fp8_scales_roll(K):
    """Three 3-word arrays, each in an arena of its own: amax is read and reset, scale and inv_scale are written."""
    amax0, margin = torch.tensor([3.5, 0.0, 917.25]), 1.25

    def fn(g):
        amax = g.out((3,), F32, 8, 0, "amax", init=amax0)
        scale, inv = g.out((3,), F32, 8, 0, "scale"), g.out((3,), F32, 8, 0, "inv_scale")
        _call(K, "fmc_fp8_scales_roll", amax.data_ptr(), scale.data_ptr(), inv.data_ptr(), margin, K._stream())
        return {"amax": amax, "scale": scale, "inv_scale": inv}

    got = _run(fn, "fp8_scales_roll")
    want = torch.clamp(margin * amax0.double() / 448.0, min=1e-12)
    assert bool((got["amax"] == 0).all())
    assert bool(((got["scale"].double().cpu() - want).abs() <= 1e-5 * want).all())          # (test_linear_fp8_qkv_epilogue: 1e-5 relative)
    assert bool(((got["inv_scale"].double().cpu() * want - 1.0).abs() <= 1e-5).all())

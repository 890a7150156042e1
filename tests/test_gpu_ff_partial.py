"""The feed-forward chain at row counts that do not fill whole tiles: `fmc_geglu_pipe_ln_partial_bf16` (csrc/geglu_pipe.hip, PARTIAL_) and
`fmc_linear_bf16_ffblk_partial` / `fmc_linear_bf16_fftail_partial` (csrc/gemm_conv.hip, gemm160p_kernel<..., PARTIAL>), their `hip_ops` wrappers, and the
route `FeedForward.forward_ln` takes with `hip_ops.PARTIAL_TILES` on.

M is one flat row count, so exactly one tile per launch is ragged.  Asserted per kernel-level case, through the raw C ABI inside the arenas of
tests/edge_guard_common.py / tests/ff_partial_common.py:

  1. bit identity: the valid rows equal the whole-tile entry point's output on the same tokens padded to whole tiles with arbitrary finite rows;
  2. zeros, quiet NaN and +Inf around every input AND in the pad rows of the tile-major operand; outputs inside sentinel-filled arenas (the pad rows of
     a tile-major output count as outside): finite, bit-identical across the three fills, every word inside written, every sentinel outside intact;
  3. accuracy with the whole-tile tests' gates: `test_geglu_ln_pipe`'s `2^-8 |ref| + 0.02` against the rounding-point reference (and 2e-2 max norm
     against fp32) for the pipe kernel, `assert_bf16_close` against the folded product in float64 for the GEMMs;
  4. a whole-tile M through the new entry points gives the old entry points' bits, and the old entry points keep refusing a ragged M.

Shapes: the smallest that reach each edge (tests/ff_partial_common.py has the tables; tests/test_ff_partial_host.py shows from the restated tile order
that the three tile totals of the GEMM cases put the ragged tile at a workgroup's only tile, beside a workgroup with a second tile, and at a
workgroup's second tile behind an epilogue, and that wrong stand-ins fail these assertions)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import edge_guard_common as EG  # noqa: F401
from tests import ff_partial_common as FFC
from tests.conv_fwd_common import assert_bf16_close
from tests.test_gpu_edge_guards import _call, _p, _rnd, _tilemajor, _vec_band
from tests.test_gpu_kernels import rel_inf

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
BAND = 200                                   # rows of guard around row-major operands: more than one 160-row tile


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _cus(K):
    return K._cus(torch.device("cuda", torch.cuda.current_device()))


def _run(fn, what):
    return FFC.run_surroundings(fn, "cuda", what, torch.cuda.synchronize)


# =====================================================================================================================================
# LayerNorm + GEGLU projection, fmc_geglu_pipe_ln_partial_bf16
# =====================================================================================================================================
def _pipe(K, variant, C, cff, M):
    rows = 160 if variant == 1 else 80
    what = f"geglu_pipe partial variant {variant} C {C} cff {cff} M {M} ({FFC.tiles(M, rows)} tiles of {rows}, {FFC.last_tile_rows(M, rows)} rows in the last)"
    Mp = FFC.tiles(M) * 160                                                  # (whole 160-row tiles: what the tile-major form of either variant wants)
    hp = _rnd((Mp, C), 1, BF16, 1.5, 0.2)                                    # rows [M, Mp): the arbitrary finite rows of the padded launch
    h = hp[:M].contiguous()
    gamma, beta = _rnd((C,), 2, F32, 0.3, 1.0), _rnd((C,), 3, F32, 0.2)
    w, bias = _rnd((2 * cff, C), 4, BF16, C ** -0.5), _rnd((2 * cff,), 5, BF16, 0.3)
    wp = K.pack_geglu_frag(w.cuda(), 16 if variant == 1 else 32).cpu()
    assert bool(K._lib.load().fmc_geglu_pipe_partial_supported(M, cff, C, variant)) and K.geglu_pipe_partial_supported(M, cff, C, variant)

    # ---- 2: the raw ABI, everything guarded, row-major and tile-major -------------------------------------------------------------------------
    def fn(g):
        hd = g.inp(h, BAND, 0, "h")
        gd, bd = g.inp(gamma, _vec_band(C), 0, "ln_gamma"), g.inp(beta, _vec_band(C), 0, "ln_beta")
        wd, bid = g.inp(wp.view(-1, C), 64, 0, "w_packed"), g.inp(bias, _vec_band(2 * cff), 0, "bias")
        out = g.out((M, cff), BF16, BAND, 0, "out")
        ob = g.blocked_out(M, cff, BF16, name="out_blocked")
        for o, blocked in ((out, 0), (ob, 1)):
            _call(K, "fmc_geglu_pipe_ln_partial_bf16", hd.data_ptr(), o.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1e-5, wd.data_ptr(), bid.data_ptr(), M, cff, C,
                  blocked, variant, K._stream())
        return {"out": out, "out_blocked": FFC.from_blocked(ob, M, cff)}
    got = _run(fn, what)
    out = got["out"]
    assert torch.equal(got["out_blocked"], out), f"{what}: the tile-major form differs from the row-major one"

    # ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
    def reference(round_bf16):
        r = (lambda t: t.bfloat16().float()) if round_bf16 else (lambda t: t)
        y = F.linear(r(F.layer_norm(h.float(), (C,), gamma, beta, 1e-5)), w.float(), bias.float())
        return y[:, :cff] * F.gelu(y[:, cff:])
    ref_r, ref_f = reference(True), reference(False)
    err = (out.float().cpu() - ref_r).abs()
    bound = 2.0 ** -8 * ref_r.abs() + 0.02
    print(f"   {what}: rel-inf {rel_inf(out.float(), ref_f):.3e} (gate 2e-2), worst error / bound {float((err / bound).max()):.3f}")
    assert rel_inf(out.float(), ref_f) < 2e-2, what
    assert not bool((err > bound).any()), f"{what}: {int((err > bound).sum())} / {err.numel()} beyond the bound"

    # ---- 1, 4: the wrappers, the whole-tile entry point on padded tokens ------------------------------------------------------------------------
    gd, bd, wd, bid = gamma.cuda(), beta.cuda(), wp.cuda(), bias.cuda()
    run = lambda hh, **kw: K.geglu_ln_pipe(hh, gd, bd, 1e-5, wd, bid, cff, variant=variant, **kw)
    FFC.assert_valid_rows_equal(run(h.cuda(), partial_tiles=True), out, f"{what}: wrapper vs raw ABI")
    blk = run(h.cuda(), blocked=True, partial_tiles=True)
    assert blk.shape == (M, cff) and blk.untyped_storage().nbytes() == K.ff_blocked_numel(M, cff) * 2
    store = torch.empty(0, dtype=BF16, device="cuda").set_(blk.untyped_storage(), 0, (K.ff_blocked_numel(M, cff),))
    FFC.assert_valid_rows_equal(FFC.from_blocked(store, M, cff), out, f"{what}: tile-major wrapper")
    whole = run(hp.cuda())
    FFC.assert_valid_rows_equal(out, whole[:M], what)
    whole_b = run(hp.cuda(), blocked=True).view(-1)
    FFC.assert_valid_rows_equal(FFC.from_blocked(whole_b, M, cff), out, f"{what}: tile-major")
    assert torch.equal(run(hp.cuda(), partial_tiles=True), whole), f"{what}: a whole-tile M through the partial entry point"
    assert torch.equal(run(hp.cuda(), blocked=True, partial_tiles=True).view(-1), whole_b), f"{what}: a whole-tile M through the partial entry point, tile-major"
    if M % rows:
        with pytest.raises(ValueError):
            run(h.cuda())


@pytest.mark.parametrize("M", [1] + [160 + r for r in FFC.PIPE80_REMAINDERS])
@pytest.mark.parametrize("cff", FFC.PIPE_CFF)
@pytest.mark.parametrize("C", [320, 640])
def test_geglu_pipe_partial_80_row_tiles(K, C, cff, M):
    _pipe(K, 0, C, cff, M)


@pytest.mark.parametrize("M", [1] + [160 + r for r in FFC.PIPE160_REMAINDERS])
@pytest.mark.parametrize("cff", FFC.PIPE_CFF)
def test_geglu_pipe_partial_160_row_tiles(K, cff, M):
    _pipe(K, 1, 320, cff, M)


# =====================================================================================================================================
# the consumers of the tile-major intermediate, fmc_linear_bf16_ffblk_partial / fmc_linear_bf16_fftail_partial
# =====================================================================================================================================
GN, GK, GK2 = 320, 128, 64                   # N, columns of the tile-major segment, columns of the row-major second segment (the tail: K = 192)
WIDE = (FFC.WIDE_N, 512, 128)                # the same three for the wide shape (K = 640 either way; the plain form reads all 640 columns tile-major)


@functools.lru_cache(maxsize=2)
def _gemm_base(tiles_max, N=GN, KA=GK, K2=GK2):
    """Operands for the largest case of a shape, once: every case takes the leading rows (and the plain form the leading or all columns of the weight)."""
    Mmax = tiles_max * 160
    a, a2 = _rnd((Mmax, KA + (K2 if N != GN else 0)), 11, BF16, 0.7), _rnd((Mmax, K2), 12, BF16, 1.2, 0.1)
    res = _rnd((Mmax, N), 13, BF16, 1.0, -0.2)
    w, bias = _rnd((N, KA + K2), 14, BF16, (KA + K2) ** -0.5), _rnd((N,), 15, BF16, 0.2)
    return {k: v.cuda() for k, v in dict(a=a, a2=a2, res=res, w=w, bias=bias).items()}


def _whole_blocked(x):
    """`[Mp, K]` (Mp % 160 == 0) -> the whole-tile kernels' tile-major tensor, shaped `[Mp, K]`."""
    Mp, Kd = x.shape
    return x.view(Mp // 160, 160, Kd // 32, 32).permute(0, 2, 1, 3).contiguous().view(Mp, Kd)


def _gemm(K, tiles_m, rem, residual, tail, b, N=GN, KA=GK, K2=GK2, where=""):
    """One case of either form: `tiles_m` row tiles, `rem` valid rows in the last.  `KA` columns tile-major, `K2` more from the row-major x2 (tail only)."""
    M, Mp = (tiles_m - 1) * 160 + rem, tiles_m * 160
    what = f"{'fftail' if tail else 'ffblk'}_partial N {N} K {KA + (K2 if tail else 0)}, {tiles_m} row tiles, {rem} rows in the last{where}, residual {residual}"
    Kd = KA + K2 if tail else KA
    w = b["w"][:, :Kd].contiguous()
    a, a2, res = b["a"][:M, :KA].contiguous(), b["a2"][:M], (b["res"][:M] if residual else None)
    wt = _tilemajor(w.cpu())
    ldres = N if residual else 0

    # ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------
    def fn(g):
        ad = g.blocked_inp(a, name="x_blocked")
        a2d = g.inp(a2, BAND, 0, "x2") if tail else None
        wd, bd = g.inp(wt, 64, 0, "w"), g.inp(b["bias"], _vec_band(N), 0, "bias")
        rd = g.inp(res, BAND, 0, "residual") if residual else None
        out = g.out((M, N), BF16, BAND, 0, "out")
        if tail:
            _call(K, "fmc_linear_bf16_fftail_partial", ad.data_ptr(), a2d.data_ptr(), wd.data_ptr(), bd.data_ptr(), _p(rd), out.data_ptr(), M, N, Kd, KA, K2,
                  ldres, None, 0, 1, K._stream())
        else:
            _call(K, "fmc_linear_bf16_ffblk_partial", ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), _p(rd), out.data_ptr(), M, N, Kd, ldres, 1.0, 1, K._stream())
        return {"out": out}
    out = _run(fn, what)["out"]

    # ---- 3: the folded product in float64 (one rounding of an fp32 accumulator) -------------------------------------------------------------------
    a64 = (torch.cat([a, a2], 1) if tail else a).double()
    ref = a64 @ w.double().t() + b["bias"].double()
    mag = a64.abs() @ w.double().abs().t() + b["bias"].double().abs()
    if residual:
        ref, mag = ref + res.double(), mag + res.double().abs()
    worst = assert_bf16_close(out, ref, mag, what)
    print(f"   {what}: worst error / bf16 bound {worst:.3f}")

    # ---- 1: the whole-tile entry point, raw, on the tokens padded to whole tiles (the next rows of the base: arbitrary, finite) ---------------------
    ab, resp = _whole_blocked(b["a"][:Mp, :KA].contiguous()), (b["res"][:Mp] if residual else None)
    wtd, whole = wt.cuda(), torch.empty(Mp, N, dtype=BF16, device="cuda")
    if tail:
        _call(K, "fmc_linear_bf16_fftail", ab.data_ptr(), b["a2"][:Mp].data_ptr(), wtd.data_ptr(), b["bias"].data_ptr(), _p(resp), whole.data_ptr(), Mp, N, Kd, KA, K2,
              ldres, None, 0, 1, K._stream())
    else:
        _call(K, "fmc_linear_bf16_ffblk", ab.data_ptr(), wtd.data_ptr(), b["bias"].data_ptr(), _p(resp), whole.data_ptr(), Mp, N, Kd, ldres, 1.0, 0, 1, 0, None, None,
              None, 1, K._stream())
    FFC.assert_valid_rows_equal(out, whole[:M], what)
    return out


def _narrow(K, extra, rem, residual, tail):
    cus = _cus(K)
    wg, at, n, _ = FFC.placement(cus + extra, cus)
    _gemm(K, cus + extra, rem, residual, tail, _gemm_base(cus + 8), where=f" (CUs + {extra} tiles: workgroup {wg}, its tile {at + 1} of {n})")


@pytest.mark.parametrize("residual", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("rem", FFC.GEMM_REMAINDERS)
@pytest.mark.parametrize("extra", FFC.GEMM_EXTRA_TILES)
def test_linear_from_blocked_partial(K, extra, rem, residual):
    _narrow(K, extra, rem, residual, tail=False)


@pytest.mark.parametrize("residual", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("rem", FFC.GEMM_REMAINDERS)
@pytest.mark.parametrize("extra", FFC.GEMM_EXTRA_TILES)
def test_ff_tail_partial(K, extra, rem, residual):
    """(Without a residual: the C ABI takes NULL on both sides; the `hip_ops` wrapper never passes one.)"""
    _narrow(K, extra, rem, residual, tail=True)


@pytest.mark.parametrize("tail", [False, True], ids=["ffblk", "fftail"])
@pytest.mark.parametrize("rem", [1, 81])
def test_ragged_tile_first_in_a_workgroup_with_a_second_tile_after_it(K, rem, tail):
    """N = 2560 (8 column tiles), K = 640: the grouped tile order puts one tile of the ragged row tile at the head of a workgroup that runs another tile
    behind it, so that tile's first phase -- `vmcnt(S_EPI + NE)` -- counts the ragged tile's redirected (rem = 81) or dead-pass (rem = 1) stores.  Placement
    from the restated order (tests/test_ff_partial_host.py proves it for 104, 256 and 304 CUs)."""
    cus = _cus(K)
    N, KA, K2 = WIDE
    tiles_m = FFC.wide_tiles_m(cus)
    assert tiles_m is not None, f"no such placement at N = {N} for {cus} CUs"
    where = FFC.ragged_placements(tiles_m, N // 320, FFC.g160p_group_m(tiles_m, N // 320, N, KA + K2), cus)
    first = [(tn, wg) for tn, wg, at, n in where if at == 0 and n >= 2]
    assert first
    b = _gemm_base(tiles_m, N, KA, K2)
    _gemm(K, tiles_m, rem, True, tail, b, N=N, KA=KA if tail else KA + K2, K2=K2, where=f" (column tile {first[0][0]} opens workgroup {first[0][1]})")


@pytest.mark.parametrize("extra", FFC.GEMM_EXTRA_TILES)
def test_whole_tile_m_through_the_partial_gemm_entry_points(K, extra):
    cus = _cus(K)
    b = _gemm_base(cus + 8)
    M = (cus + extra) * 160
    ab, a2, res, w = _whole_blocked(b["a"][:M]), b["a2"][:M], b["res"][:M], b["w"]
    w1 = w[:, :GK].contiguous()
    with torch.no_grad():
        assert torch.equal(K.linear_from_blocked(ab, w1, b["bias"], res, partial_tiles=True), K.linear_from_blocked(ab, w1, b["bias"], res))
        assert torch.equal(K.linear_from_blocked(ab, w1, b["bias"], None, alpha=0.5, partial_tiles=True), K.linear_from_blocked(ab, w1, b["bias"], None, alpha=0.5))
        assert torch.equal(K.ff_tail(ab, a2, w, b["bias"], res, partial_tiles=True), K.ff_tail(ab, a2, w, b["bias"], res))


def test_the_entry_points_refuse_what_they_do_not_take(K):
    cus = _cus(K)
    b = _gemm_base(cus + 8)
    M = cus * 160 + 7
    x = torch.empty(K.ff_blocked_numel(M, GK), dtype=BF16, device="cuda")[:M * GK].view(M, GK)
    w1 = b["w"][:, :GK].contiguous()
    with torch.no_grad():
        with pytest.raises(ValueError):                                     # the whole-tile entry points keep refusing a ragged M
            K.linear_from_blocked(x, w1, b["bias"], None)
        with pytest.raises(ValueError):
            K.ff_tail(x, b["a2"][:M], b["w"], b["bias"], b["res"][:M])
        small = torch.empty(K.ff_blocked_numel(167, GK), dtype=BF16, device="cuda")[:167 * GK].view(167, GK)
        with pytest.raises(ValueError):                                     # fewer tiles than CUs
            K.linear_from_blocked(small, w1, b["bias"], None, partial_tiles=True)
        with pytest.raises(AssertionError):                                 # a copy of the intermediate has lost its last tile
            K.linear_from_blocked(x.clone(), w1, b["bias"], None, partial_tiles=True)
    lib = K._lib.load()
    part = torch.zeros(64, dtype=F32, device="cuda")
    rc = lib.fmc_linear_bf16_fftail_partial(x.data_ptr(), b["a2"].data_ptr(), b["w"].data_ptr(), None, None, b["res"].data_ptr(), M, GN, GK + GK2, GK, GK2, 0,
                                            part.data_ptr(), 160, 0, K._stream())
    assert rc != 0                                                          # GroupNorm partial sums: refused
    for args in ((0, 128, 320, 0), (5, 100, 320, 0), (5, 128, 640, 1), (5, 128, 256, 0)):
        assert not lib.fmc_geglu_pipe_partial_supported(*args) and not K.geglu_pipe_partial_supported(*args)
    for Mx in (1, 79, 161, 49152, 12288):
        for C, var in ((320, 0), (320, 1), (640, 0)):
            assert bool(lib.fmc_geglu_pipe_partial_supported(Mx, 1280, C, var)) == K.geglu_pipe_partial_supported(Mx, 1280, C, var) is True


# =====================================================================================================================================
# chain level: pipe (tile-major, partial) -> linear_from_blocked / ff_tail (partial), against the same chain on padded tokens
# =====================================================================================================================================
@pytest.mark.parametrize("rem", [79, 81])
def test_chain_partial_against_the_chain_on_padded_tokens(K, rem):
    cus = _cus(K)
    C, cff = 320, 256
    M, Mp = cus * 160 + rem, (cus + 1) * 160                                # CUs + 1 tiles
    hp = _rnd((Mp, C), 21, BF16, 1.5, 0.2).cuda()
    xp = _rnd((Mp, C), 22, BF16, 1.0, -0.2).cuda()
    h, x = hp[:M].contiguous(), xp[:M].contiguous()
    gamma, beta = _rnd((C,), 23, F32, 0.3, 1.0).cuda(), _rnd((C,), 24, F32, 0.2).cuda()
    w1, b1 = _rnd((2 * cff, C), 25, BF16, C ** -0.5).cuda(), _rnd((2 * cff,), 26, BF16, 0.3).cuda()
    w2, b2 = _rnd((C, cff), 27, BF16, cff ** -0.5).cuda(), _rnd((C,), 28, BF16, 0.2).cuda()
    wpj, bpj = _rnd((C, C), 29, BF16, C ** -0.5).cuda(), _rnd((C,), 30, BF16, 0.2).cuda()
    frag = K.pack_geglu_frag(w1, 16)
    wc, bc = K.fold_ff_tail(w2, b2, wpj, bpj)
    with torch.no_grad():
        assert K.geglu_ln_partial_ok(h, w1) and K.geglu_direct_blocked_partial_ok(h, w2, h) and K.ff_tail_partial_ok(h, w2, wpj, x)
        assert not K.geglu_ln_direct_ok(h, w1) and not K.geglu_direct_blocked_ok(h, w2, h) and not K.ff_tail_ok(h, w2, wpj, x)
        mid = K.geglu_ln_pipe(h, gamma, beta, 1e-5, frag, b1, cff, blocked=True, variant=1, partial_tiles=True)
        y = K.linear_from_blocked(mid, w2, b2, h, partial_tiles=True)
        z = K.ff_tail(mid, h, wc, bc, x, partial_tiles=True)
        mid_w = K.geglu_ln_pipe(hp, gamma, beta, 1e-5, frag, b1, cff, blocked=True, variant=1)
        y_w = K.linear_from_blocked(mid_w, w2, b2, hp)
        z_w = K.ff_tail(mid_w, hp, wc, bc, xp)
    FFC.assert_valid_rows_equal(y, y_w[:M], f"chain -> linear_from_blocked, {rem} rows in the last tile")
    FFC.assert_valid_rows_equal(z, z_w[:M], f"chain -> ff_tail, {rem} rows in the last tile")
    assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(z.float()).all())
    n = F.layer_norm(h.float(), (C,), gamma, beta, 1e-5)
    t = F.linear(n, w1.float(), b1.float())
    ref = F.linear(t[:, :cff] * F.gelu(t[:, cff:]), w2.float(), b2.float()) + h.float()
    assert rel_inf(y, ref) < 2e-2


# =====================================================================================================================================
# model level: the full-width U-Net + CMC + OMC at 16x192x448 -- level 0: 24 x 56 = 1344 pixels, 21504 rows per clip (134.4 tiles), 43008 at CFG batch 2
# (268.8 tiles: more than the CUs, the smallest latent size in whole multiples of 8 that is); level 1: 336 pixels.  Every feed-forward site of the
# two levels is ragged (rows % 80 != 0).
# =====================================================================================================================================
MH, MW = 192, 448


def _counts(log):
    fam = {}
    for family, shape, _ in log:
        key = family
        if family == "own_linear" and len(shape) > 3 and isinstance(shape[3], str) and shape[3].endswith("-partial"):
            key = shape[3]
        elif family == "geglu_direct" and "partial" in shape:
            key = "geglu_direct partial"
        fam[key] = fam.get(key, 0) + 1
    return fam


@pytest.fixture(scope="module")
def model_ragged(K):
    """The case of tests/test_gpu_partial_tiles.py's `model64` at the size above.  The fp32 oracle of this size is beyond a CPU fixture's budget (the
    64x128 one takes 22 s at a tenth of the tokens), so the oracle modules run their plain-torch fp32 arithmetic on the device.  `format_err` is, as there, the rounded oracle against the fp32 oracle: what the bf16 FORMAT costs on this case."""
    from einops import rearrange

    from oracle import conditioning as OC
    from tests import common_models as CM
    torch.set_num_threads(16)
    ou, oe, oa, clip = CM.full_width_case(43, 143, MH, MW)
    t = torch.tensor([801])
    with torch.no_grad():
        pose_emb = rearrange(OC.to_plucker_embedding(clip["c2w"], clip["K"], (MH, MW)), "b f c h w -> b c f h w")

        def run():
            pf = [rearrange(x, "(b f) c h w -> b c f h w", b=1) for x in oe(pose_emb.cuda())]
            tr = OC.get_traj_features(clip["infos"], clip["masks"], lambda feats, msk: oa(feats.cuda(), msk.cuda()))
            return ou(clip["latents"].cuda(), t.cuda(), clip["text"].cuda(), pose_embedding_features=pf, traj_features=tr).sample.float().cpu()
        for mod in (ou, oe, oa):
            mod.cuda()
        ref = run()
        with CM.bf16_rounding(ou, oe, oa):
            ref16 = run()
    pu, pe, pa = CM.build_product(ou, oe, oa, CM.FULL_WIDTHS, CM.FULL_CROSS_DIM, dtype=BF16)
    del ou, oe, oa
    torch.cuda.empty_cache()
    format_err = rel_inf(ref16, ref)
    print(f"   16x{MH}x{MW}: bf16 format alone (rounded oracle vs fp32 oracle) {format_err:.3e}")
    assert 2e-3 < format_err < 4e-2                                         # (the sanity window of test_full_width_bf16_parity_and_format_share)
    return dict(pu=pu, pe=pe, pa=pa, clip=clip, t=t, ref=ref, format_err=format_err)


def test_full_width_unet_ff_partial_switch_eager(K, model_ragged):
    """Eager forward, switch off against on: with it on the feed-forwards of level 0 launch the pipe kernel (`geglu_direct` in `hip_ops.call_log`) and
    fewer launches go to the vendor arm; the two bf16 paths stay within twice the case's format error (the gate of test_gpu_partial_tiles.py)."""
    from einops import rearrange

    from synfmc_amd.data.dataset import to_plucker_embedding
    from synfmc_amd.models.pose_obj_adaptor import CamObjPoseAdaptor
    from synfmc_amd.util import get_traj_features_v2
    m, clip = model_ragged, model_ragged["clip"]
    assert not K.PARTIAL_TILES
    with torch.no_grad():
        emb = to_plucker_embedding(clip["c2w"].cuda(), clip["K"].cuda(), (MH, MW))
        pose_emb = rearrange(emb, "b f c h w -> b c f h w").to(BF16)
        tf = get_traj_features_v2(clip["infos"], clip["masks"], m["pa"], False, 0.0, [False], "cuda", BF16)
        wrapper = CamObjPoseAdaptor(m["pu"], m["pe"])
        args = (clip["latents"].cuda().to(BF16), m["t"].cuda(), clip["text"].cuda().to(BF16), pose_emb)
        outs, counts = {}, {}
        for on in (False, True):
            K.PARTIAL_TILES = on
            try:
                wrapper(*args, tf)                                           # (autotuned arms, cached pose terms and packs settle)
                K.call_log = []
                outs[on] = wrapper(*args, tf).float().cpu()
            finally:
                K.PARTIAL_TILES = False
                log, K.call_log = K.call_log, None
            counts[on] = _counts(log)
    gap = rel_inf(outs[True], outs[False])
    print(f"   eager 16x{MH}x{MW}: launches off {counts[False]}, on {counts[True]}; on vs off {gap:.3e} (gate {2.0 * m['format_err']:.3e}), on vs fp32 oracle "
          f"{rel_inf(outs[True], m['ref']):.3e}, off vs fp32 oracle {rel_inf(outs[False], m['ref']):.3e}")
    assert counts[False].get("geglu_direct", 0) == 0 and counts[False].get("geglu_direct partial", 0) == 0
    assert counts[True].get("geglu_direct partial", 0) > 0 and counts[True].get("geglu_direct", 0) == 0
    assert counts[True].get("vendor", 0) < counts[False].get("vendor", 0)
    assert gap < 2.0 * m["format_err"]
    assert rel_inf(outs[True], m["ref"]) < 2.5 * m["format_err"] and rel_inf(outs[True], m["ref"]) < 4e-2


def test_full_width_pipeline_ff_partial_graph_gives_its_own_bits_again(K, model_ragged, monkeypatch):
    """`CameraObjCtrlPipeline`, captured graph, CFG batch 2 (269 tiles at level 0: the folded tail `ff_tail(..., partial_tiles=True)` is in the graph),
    two steps, switch on: the replay gives the capturing call's bits again."""
    from synfmc_amd.models.pose_adaptor import features_to_video
    from synfmc_amd.pipelines.pipeline_animation_cm_om import CameraObjCtrlPipeline
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.util import stack_object_inputs
    monkeypatch.setattr(K, "DETERMINISTIC", True)      # (as test_pipeline_graph_reuse_across_clips: no vendor convolution arm, whose atomics differ run to run)
    m, clip = model_ragged, model_ragged["clip"]
    uncond = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(99))
    sk = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    pipe = CameraObjCtrlPipeline(None, None, None, m["pu"], DDIMScheduler(**sk), m["pe"])
    with torch.no_grad():
        poses, masks = stack_object_inputs(clip["infos"], clip["masks"], "cuda")
        feats, mk = K.omc_rasterize(poses, masks, "unshuffle8", BF16)
        kw = dict(prompt=None, video_length=16, height=MH, width=MW, num_inference_steps=2, guidance_scale=2.0,
                  prompt_embeds=torch.cat([uncond, clip["text"]]).to("cuda", BF16), latents=clip["latents"].cuda(), output_type="latent",
                  pose_embedding=K.plucker(clip["K"].cuda(), clip["c2w"].cuda(), MH, MW, "unshuffle8", BF16), pose_embedding_unshuffled=True,
                  traj_features=features_to_video(m["pa"](feats, mk), 1))
        K.PARTIAL_TILES = True
        try:
            K.call_log = []
            a = torch.as_tensor(pipe(**kw).videos).float().cpu()            # captures
            log, K.call_log = K.call_log, None
            b = torch.as_tensor(pipe(**kw).videos).float().cpu()            # replays
        finally:
            K.PARTIAL_TILES, K.call_log = False, None
    counts = _counts(log)
    print(f"   graph 16x{MH}x{MW}, CFG batch 2, 2 steps: launches at capture {counts}")
    assert _cus(K) < 269 and counts.get("ff-tail-partial", 0) > 0 and counts.get("geglu_direct partial", 0) > 0
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)

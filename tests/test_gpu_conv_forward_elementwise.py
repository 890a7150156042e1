"""Every 3x3 convolution forward launch, element by element (tests/conv_fwd_common.py has the references, generators and bounds;
profiles/conv_forward_bounds.md the derivations and the measured shares):

* exact runs -- integer data on which every partial sum is exact in fp32 and bf16: the output and every `gn_partials` entry equal the float64
  reference bit for bit, whatever the accumulation order, split, wave count or tile order;
* rounding runs -- Gaussian data: every element within `2^-8 |ref| + 1e-5 sum|terms|` (`assert_bf16_close`; `assert_f32_close` for the fp32-storage
  kernel) of the float64 result on the same operands, the GroupNorm + SiLU operand path with its counted rounding ties; every `gn_partials` entry
  within `STATS_REL * sum|addends|` of the float64 sums of the kernel's own output over the tile's pixels.

Kernels: fmc_conv3x3_halo_bf16 (GroupNorm operand path, statistics epilogue), fmc_conv3x3_halo_sc_bf16, fmc_conv3x3_halo4_bf16 (4-wave, wide,
split-K), the two *_fold_bf16 launches, fmc_conv3x3_bf16 (plain, stride 2, upsample, split-K, stream-K, `_gn`) and fmc_conv3x3_x3_f32, through
the `hip_ops` wrappers.  Each case prints the share of its bound that the kernel used."""
import pytest
import torch

from tests import conv_fwd_common as C

pytestmark = pytest.mark.gpu

INSTRUMENTS = ["exact", "rounding"]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _cu(d):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items()}


def _id(s):
    if isinstance(s, C.Spec):
        return "-".join(str(int(v) if isinstance(v, bool) else v) or "none" for v in s[1:])
    return str(s)


def _check(instrument, s, r, out, what, parts=None, layout=None):
    """One launch's output (and statistics) against the case's reference under the instrument; prints the share of the bound it used."""
    torch.cuda.synchronize()
    assert out.shape == r["ref"].shape, (what, out.shape, r["ref"].shape)
    if instrument == "exact":
        C.check_exact(out, r["ref"], what)
        if parts is not None:
            C.check_stats_exact(parts, r["ref"], layout, what)
        print(f"   {what}: exact")
        return
    if s.kind == "f32":
        used = C.assert_f32_close(out, r["ref"], r["mag"], what)
    else:
        used = C.assert_bf16_close(out, r["ref"], r["mag"], what, extra=r["extra"])
    line = f"   {what}: err / bound {used:.3f}, rel-inf {C.rel_inf(out, r['ref']):.3e}"
    if r["extra"] is not None:
        line += f", ambiguous operands {100 * r['amb_share']:.3f} %"
    if parts is not None:
        line += f", statistics err / bound {C.check_stats_rounding(parts, out.cpu(), layout, what):.3f}"
    print(line)


# ---- conv_halo_kernel ----------------------------------------------------------------------------------------------------------------------------
def _halo(K, s, g, instrument, emit):
    shortcut = (g["xs"], g["xs2"], g["wsc"], g["bsc"]) if s.cs1 else None
    bias = g["bias"]
    got = K.conv3x3_halo(g["x"], g["w"], bias, g["temb"], g["res"], temb_div=s.tdiv, upsample=s.ups, x2_nhwc=g["x2"], gn_coef=g["coef"],
                         gn_act=s.gn == 1 and instrument == "rounding", emit_gn=emit, shortcut=shortcut)
    return got if emit else (got, None)


@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("s", C.HALO + C.HALO_SC, ids=_id)
def test_conv3x3_halo_every_element(K, s, instrument):
    """`fmc_conv3x3_halo_bf16` / `_sc_bf16`: plain, epilogue addends (temb rows per clip), two sources, nearest 2x, the GroupNorm operand path (indexing
    of `gn_coef` by image and channel across both sources, zero padding of the NORMALISED tensor), the 1x1 shortcut segment; with and without the
    statistics epilogue where Cout allows it (per 10 x 32 tile, a tile over the last image row counting only the rows that exist)."""
    assert K.conv3x3_halo_supported(s.n, s.h, s.w, s.cin, s.cin - s.c2, s.cout, s.ups)
    assert not s.cs1 or K.conv3x3_halo_sc_supported(s.n, s.h, s.w, s.cin, s.cout, s.cs1 + s.cs2, s.cs1)
    d, r = C.case(s, instrument)
    g = _cu(d)
    what = f"conv3x3_halo {_id(s)}"
    out, _ = _halo(K, s, g, instrument, False)
    _check(instrument, s, r, out, what)
    if s.cout % 64 == 0 and 160 % (s.cout // 32) == 0:
        out_e, parts = _halo(K, s, g, instrument, True)
        assert parts.shape == (s.n, C.slot_map("halo", s.h, s.w)[1], 32, 2)
        _check(instrument, s, r, out_e, what + " emit_gn", parts, "halo")
        assert torch.equal(out_e, out)


# ---- conv_halo4_kernel ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("s", C.HALO4, ids=_id)
def test_conv3x3_halo4_every_element(K, s, instrument):
    """`fmc_conv3x3_halo4_bf16`: the 4-wave form, split-K 2 and Cin / 64 and the wrapper's own choice, the 8-wave form where it is supported; statistics
    per row block of 10 x 16 or 5 x 8 pixels where Cout allows them."""
    assert K.conv3x3_halo4_supported(s.n, s.h, s.w, s.cin, s.cin - s.c2, s.cout, s.ups)
    d, r = C.case(s, instrument)
    g = _cu(d)
    run = lambda **kw: K.conv3x3_halo4(g["x"], g["w"], g["bias"], g["temb"], g["res"], temb_div=s.tdiv, upsample=s.ups, x2_nhwc=g["x2"], **kw)
    what = f"conv3x3_halo4 {_id(s)}"
    forms = [("4 waves", dict(split_k=1, wide=False), 80)]
    if K.conv3x3_halo4_supported(s.n, s.h, s.w, s.cin, s.cin - s.c2, s.cout, s.ups, wide=True):
        forms.append(("8 waves", dict(split_k=1, wide=True), 160))
    for name, kw, bn in forms:
        _check(instrument, s, r, run(**kw), f"{what} {name}")
        if s.cout % 64 == 0 and bn % (s.cout // 32) == 0:
            out_e, parts = run(emit_gn=True, **kw)
            assert parts.shape == (s.n, C.slot_map("halo4", s.h, s.w)[1], 32, 2)
            _check(instrument, s, r, out_e, f"{what} {name} emit_gn", parts, "halo4")
    if s.cin >= 128:
        for sk in sorted({2, s.cin // 64}):
            _check(instrument, s, r, run(split_k=sk), f"{what} split_k {sk}")
    _check(instrument, s, r, run(), f"{what} split_k of the wrapper's choice")


# ---- the folded upsample launches ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("n,hs,ws,cin,cout,arm", C.FOLD)
def test_folded_upsample_launch_every_element(K, n, hs, ws, cin, cout, arm, with_bias, instrument):
    """`fmc_conv3x3_halo_fold_bf16` / `fmc_conv3x3_halo4_fold_bf16` (4 and 8 waves).  Exact runs: the fold of integers is exact, so the launch equals the
    9-tap reference bit for bit.  Rounding runs: the reference is the fold in float64 rounded to bf16 once, the bound unchanged.  Statistics per (source
    tile or row block, phase)."""
    s = C.fold_spec(n, hs, ws, cin, cout, with_bias)
    d, r = C.case(s, instrument, True)
    g = _cu(d)
    bn = 80 if arm == "halo4" else 160
    layout = "halo_fold" if arm == "halo" else "halo4_fold"
    what = f"conv3x3_upfold {arm} n={n} {hs}x{ws} {cin}->{cout} bias={with_bias}"
    _check(instrument, s, r, K.conv3x3_upfold(g["x"], g["w"], g["bias"], arm=arm), what)
    if cout % 64 == 0 and bn % (cout // 32) == 0:
        out_e, parts = K.conv3x3_upfold(g["x"], g["w"], g["bias"], emit_gn=True, arm=arm)
        assert parts.shape == (n, C.slot_map(layout, 2 * hs, 2 * ws)[1], 32, 2)
        _check(instrument, s, r, out_e, what + " emit_gn", parts, layout)


# ---- the ring kernel -------------------------------------------------------------------------------------------------------------------------------------
def _ring(K, s, g, **kw):
    return K.conv3x3_bf16(g["x"], g["w"], g["bias"], g["temb"], g["res"], temb_div=s.tdiv, upsample=s.ups, stride2=s.s2, **kw)


@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("s", C.RING_EPILOGUE, ids=_id)
def test_conv3x3_ring_epilogues_every_element(K, s, instrument):
    """`fmc_conv3x3_bf16` on the plain grid: bias, temb per image and per clip, residual, all three; ragged Cout and pixel count."""
    d, r = C.case(s, instrument)
    g = _cu(d)
    for tile in C.RING_EPILOGUE_TILES:
        _check(instrument, s, r, _ring(K, s, g, tile=tile), f"conv3x3_bf16 {_id(s)} tile {tile}")


@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("s,tiles", [(C.RING_STRIDE2, C.RING_STRIDE2_TILES), (C.RING_UPSAMPLE, C.RING_UPSAMPLE_TILES)], ids=["stride2", "upsample"])
def test_conv3x3_ring_resampling_every_element(K, s, tiles, instrument):
    """`fmc_conv3x3_bf16` with stride 2 and with the nearest 2x upsample in its addressing (tile 130: the stream-K form)."""
    d, r = C.case(s, instrument)
    g = _cu(d)
    for tile in tiles:
        _check(instrument, s, r, _ring(K, s, g, tile=tile), f"conv3x3_bf16 {_id(s)} tile {tile}")


@pytest.mark.parametrize("instrument", INSTRUMENTS)
def test_conv3x3_ring_split_k_every_element(K, instrument):
    """`fmc_conv3x3_bf16` split-K 2 / 4 / 8 (fp32 partials, fixed-order reduce) on three tile geometries, temb + residual in the finishing pass."""
    s = C.RING_SPLIT
    d, r = C.case(s, instrument)
    g = _cu(d)
    for tile in C.RING_SPLIT_TILES:
        for sk in C.RING_SPLITS:
            _check(instrument, s, r, _ring(K, s, g, tile=tile, split_k=sk), f"conv3x3_bf16 {_id(s)} tile {tile} split_k {sk}")


@pytest.mark.parametrize("instrument", INSTRUMENTS)
def test_conv3x3_ring_gn_every_element(K, instrument):
    """`fmc_conv3x3_bf16_gn` (tile 16 with the statistics epilogue): two 160-pixel statistics tiles per image."""
    s = C.RING_GN
    d, r = C.case(s, instrument)
    g = _cu(d)
    out, (parts, cout) = K.conv3x3_gn(g["x"], g["w"], g["bias"], g["temb"], g["res"], s.tdiv, False, False)
    assert cout == s.cout and parts.shape == (s.n, s.h * s.w // 160, 32, 2)
    _check(instrument, s, r, out, f"conv3x3_gn {_id(s)}", parts, "ring")


@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("s", C.F32, ids=_id)
def test_conv3x3_f32_every_element(K, s, instrument):
    """`fmc_conv3x3_x3_f32` (split-bf16 x3): integers live in the high part, so the exact runs must be exact; Gaussian data within `assert_f32_close`."""
    d, r = C.case(s, instrument)
    g = _cu(d)
    for tile in C.F32_TILES:
        out = K.conv3x3_f32(g["x"], g["w"], g["bias"], g["temb"], g["res"], tile=tile, temb_div=s.tdiv, upsample=s.ups, stride2=s.s2)
        _check(instrument, s, r, out, f"conv3x3_f32 {_id(s)} tile {tile}")

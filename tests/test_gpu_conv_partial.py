"""The halo convolutions at ANY image width (`fmc_conv3x3_halo*_partial_*`: partly filled column tiles; include/fmc_hip.h), through the `hip_ops`
wrappers with `partial_tiles=True`.  tests/conv_partial_common.py has the cases, the ragged slot map and the padding helper; tests/conv_fwd_common.py
the references and both instruments; tests/test_conv_partial_host.py the CPU side (tile arithmetic, the cases' conditions, the wrong stand-ins).

Per case, wherever it applies:
1. both instruments -- exact (integer data: output and every `gn_partials` entry bit for bit; the run that sees a column wrap, because the word behind
   `(y, W - 1)` is `(y + 1, 0)`, valid data) and rounding (`assert_bf16_close` element by element, statistics within `STATS_REL * sum|addends|`);
2. bit identity with the whole-tile kernel on the same data zero-padded in width (GroupNorm mode 0), valid columns, `torch.equal`;
3. a whole-tile shape through the partial entry: the existing entry's bits, output and statistics;
4. poisoned surroundings through the raw C ABI in `edge_guard_common` arenas: finite, bit-identical under zeros / NaN / +Inf, every word inside
   written, every sentinel intact (a pad-column store behind the last image's last row lands past the end: only the sentinels see it);
5. three repeated launches are bit-equal;
6. module and model level: `hip_ops.PARTIAL_TILES` on routes ragged widths to the partial launches (`call_log`), off changes nothing."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import conv_fwd_common as C
from tests import conv_partial_common as P
from tests import edge_guard_common as EG  # noqa: F401
from tests.test_gpu_edge_guards import (CONV_BAND, _call, _check_partials, _conv_data, _conv_operands, _conv_ref, _p, _packed, _run)

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
INSTRUMENTS = ["exact", "rounding"]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _cu(d):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items()}


def _check(instrument, s, r, out, what, parts=None, layout=None, tw=None):
    """One launch's output (and statistics) against the case's reference under the instrument; prints each figure before it asserts."""
    torch.cuda.synchronize()
    assert out.shape == r["ref"].shape, (what, out.shape, r["ref"].shape)
    if instrument == "exact":
        C.check_exact(out, r["ref"], what)
        if parts is not None:
            P.check_stats_exact(parts, r["ref"], layout, tw, what)
        print(f"   {what}: exact")
        return
    print(f"   {what}: rel-inf {C.rel_inf(out, r['ref']):.3e}", end="")
    used = C.assert_bf16_close(out, r["ref"], r["mag"], what, extra=r["extra"])
    line = f", err / bound {used:.3f}"
    if r["extra"] is not None:
        line += f", ambiguous operands {100 * r['amb_share']:.3f} %"
    if parts is not None:
        line += f", statistics err / bound {P.check_stats_rounding(parts, out.cpu(), layout, tw, what):.3f}"
    print(line)


def _repeatable(run, what):
    a = run()
    torch.cuda.synchronize()
    for _ in range(2):
        b = run()
        torch.cuda.synchronize()
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert torch.equal(x, y), f"{what}: repeated launches differ"


# ---- conv_halo_kernel<.., PARTIAL> -------------------------------------------------------------------------------------------------------------------
def _halo(K, s, g, instrument, emit, partial=True):
    shortcut = (g["xs"], g["xs2"], g["wsc"], g["bsc"]) if s.cs1 else None
    got = K.conv3x3_halo(g["x"], g["w"], g["bias"], g["temb"], g["res"], temb_div=s.tdiv, upsample=s.ups, x2_nhwc=g["x2"], gn_coef=g["coef"],
                         gn_act=s.gn == 1 and instrument == "rounding", emit_gn=emit, shortcut=shortcut, partial_tiles=partial)
    return got if emit else (got, None)


@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("s", P.HALO + P.HALO_SC, ids=P.sid)
def test_conv3x3_halo_partial_every_element(K, s, instrument):
    """`fmc_conv3x3_halo_partial_bf16` / `_sc_partial_bf16` at widths the whole-tile entries refuse: both instruments, with and without the statistics
    epilogue (per 10 x 32 tile through the ragged slot map), three launches bit-equal, and -- GroupNorm mode 0 -- the valid columns bit-identical to the
    whole-tile kernel's on the same data zero-padded to the next multiple of 32."""
    assert K.conv3x3_halo_partial_supported(s.n, s.h, s.w, s.cin, s.cin - s.c2, s.cout, s.ups)
    assert not K.conv3x3_halo_supported(s.n, s.h, s.w, s.cin, s.cin - s.c2, s.cout, s.ups)
    if s.cs1:
        assert K.conv3x3_halo_sc_partial_supported(s.n, s.h, s.w, s.cin, s.cout, s.cs1 + s.cs2, s.cs1)
        assert not K.conv3x3_halo_sc_supported(s.n, s.h, s.w, s.cin, s.cout, s.cs1 + s.cs2, s.cs1)
    d, r = C.case(s, instrument)
    g = _cu(d)
    what = f"conv3x3_halo partial {P.sid(s)}"
    out, _ = _halo(K, s, g, instrument, False)
    _check(instrument, s, r, out, what)
    emit = s.cout % 64 == 0 and 160 % (s.cout // 32) == 0
    if emit:
        out_e, parts = _halo(K, s, g, instrument, True)
        assert parts.shape == (s.n, P.slot_map("halo", s.h, s.w)[1], 32, 2)
        _check(instrument, s, r, out_e, what + " emit_gn", parts, "halo")
        assert torch.equal(out_e, out)
    _repeatable(lambda: tuple(t for t in _halo(K, s, g, instrument, emit) if t is not None), what)
    if not s.gn:
        sp, dp = P.pad_case(s, d, P.halo_pad_width(s.w))
        assert K.conv3x3_halo_supported(sp.n, sp.h, sp.w, sp.cin, sp.cin - sp.c2, sp.cout, sp.ups)
        whole, _ = _halo(K, sp, _cu(dp), instrument, False, partial=False)
        assert torch.equal(whole[:, :, :s.w], out), f"{what}: differs from the whole-tile kernel on the zero-padded image"


@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("n,hs,ws,cin,cout", P.HALO_FOLD)
def test_conv3x3_halo_fold_partial_every_element(K, n, hs, ws, cin, cout, instrument):
    """`fmc_conv3x3_halo_fold_partial_bf16`: the pixel-shuffled store of a ragged SOURCE tile, statistics per (source tile, phase)."""
    L = K._lib.load()
    assert L.fmc_conv3x3_halo_fold_partial_supported(n, hs, ws, cin, cout) and not L.fmc_conv3x3_halo_fold_supported(n, hs, ws, cin, cout)
    s = C.fold_spec(n, hs, ws, cin, cout, True)
    d, r = C.case(s, instrument, True)
    g = _cu(d)
    what = f"conv3x3_upfold halo partial n={n} {hs}x{ws} {cin}->{cout}"
    out = K.conv3x3_upfold(g["x"], g["w"], g["bias"], arm="halo", partial_tiles=True)
    _check(instrument, s, r, out, what)
    out_e, parts = K.conv3x3_upfold(g["x"], g["w"], g["bias"], emit_gn=True, arm="halo_partial")
    assert parts.shape == (n, P.slot_map("halo_fold", 2 * hs, 2 * ws)[1], 32, 2)
    _check(instrument, s, r, out_e, what + " emit_gn", parts, "halo_fold")
    assert torch.equal(out_e, out)
    _repeatable(lambda: K.conv3x3_upfold(g["x"], g["w"], g["bias"], emit_gn=True, arm="halo_partial"), what)
    sp, dp = P.pad_case(s, d, 2 * P.halo_pad_width(ws))
    whole = K.conv3x3_upfold(dp["x"].cuda(), g["w"], g["bias"], arm="halo")
    assert torch.equal(whole[:, :, :2 * ws], out), f"{what}: differs from the whole-tile kernel on the zero-padded source"


# ---- conv_halo4_kernel<.., PARTIAL> ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("s,tws,splits,wide", P.HALO4, ids=lambda v: P.sid(v) if isinstance(v, C.Spec) else str(v))
def test_conv3x3_halo4_partial_every_element(K, s, tws, splits, wide, instrument):
    """`fmc_conv3x3_halo4_partial_bf16` at widths that are no multiple of 8, at each row-block geometry of the case: one pass, split over the reduction
    (the fp32 partials of pad columns are not written: see the poisoned runs), the wrapper's own geometry and split, statistics per row block where Cout
    allows; bit identity with the whole-tile kernel at the same geometry on the zero-padded image."""
    assert K.conv3x3_halo4_partial_supported(s.n, s.h, s.w, s.cin, s.cin - s.c2, s.cout, s.ups, wide)
    assert not K.conv3x3_halo4_supported(s.n, s.h, s.w, s.cin, s.cin - s.c2, s.cout, s.ups, wide)
    d, r = C.case(s, instrument)
    g = _cu(d)
    run = lambda gg=g, **kw: K.conv3x3_halo4(gg["x"], gg["w"], gg["bias"], gg["temb"], gg["res"], temb_div=s.tdiv, upsample=s.ups, x2_nhwc=gg["x2"],
                                             wide=wide, **kw)
    bn = 160 if wide else 80
    for tw in tws:
        what = f"conv3x3_halo4 partial {P.sid(s)} tw {tw}{' wide' if wide else ''}"
        out = run(split_k=1, partial_tiles=True, tw=tw)
        _check(instrument, s, r, out, what)
        if s.cout % 64 == 0 and bn % (s.cout // 32) == 0:
            out_e, parts = run(split_k=1, emit_gn=True, partial_tiles=True, tw=tw)
            assert parts.shape == (s.n, P.halo4_row_blocks_per_image(s.h, s.w, tw), 32, 2)
            _check(instrument, s, r, out_e, what + " emit_gn", parts, "halo4", tw)
            assert torch.equal(out_e, out)
            _repeatable(lambda: run(split_k=1, emit_gn=True, partial_tiles=True, tw=tw), what)
        else:
            _repeatable(lambda: run(split_k=1, partial_tiles=True, tw=tw), what)
        sp, dp = P.pad_case(s, d, P.halo4_pad_width(s.w, tw))
        assert K.conv3x3_halo4_supported(sp.n, sp.h, sp.w, sp.cin, sp.cin - sp.c2, sp.cout, sp.ups, wide)
        gp = _cu(dp)
        assert torch.equal(run(gp, split_k=1)[:, :, :s.w], out), f"{what}: differs from the whole-tile kernel on the zero-padded image"
        for sk in splits:
            out_s = run(split_k=sk, partial_tiles=True, tw=tw)
            _check(instrument, s, r, out_s, f"{what} split_k {sk}")
            assert torch.equal(run(gp, split_k=sk)[:, :, :s.w], out_s), f"{what} split_k {sk}: differs from the whole-tile kernel"
            _repeatable(lambda: run(split_k=sk, partial_tiles=True, tw=tw), f"{what} split_k {sk}")
    _check(instrument, s, r, run(partial_tiles=True), f"conv3x3_halo4 partial {P.sid(s)} geometry and split of the wrapper's choice")


@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("tw,wide", P.HALO4_FOLD_GEOMETRIES)
@pytest.mark.parametrize("n,hs,ws,cin,cout", P.HALO4_FOLD)
def test_conv3x3_halo4_fold_partial_every_element(K, n, hs, ws, cin, cout, tw, wide, instrument):
    """`fmc_conv3x3_halo4_fold_partial_bf16` at the three geometries: 5 x 8 and 10 x 16 source row blocks on 4 waves, 10 x 16 on 8."""
    L = K._lib.load()
    assert L.fmc_conv3x3_halo4_fold_partial_supported(n, hs, ws, cin, cout, int(wide)) and not L.fmc_conv3x3_halo4_fold_supported(n, hs, ws, cin, cout, int(wide))
    s = C.fold_spec(n, hs, ws, cin, cout, True)
    d, r = C.case(s, instrument, True)
    g = _cu(d)
    arm = "halo4w" if wide else "halo4"
    what = f"conv3x3_upfold {arm} partial n={n} {hs}x{ws} {cin}->{cout} tw {tw}"
    out = K.conv3x3_upfold(g["x"], g["w"], g["bias"], arm=arm, partial_tiles=True, tw=tw)
    _check(instrument, s, r, out, what)
    _repeatable(lambda: K.conv3x3_upfold(g["x"], g["w"], g["bias"], arm=arm, partial_tiles=True, tw=tw), what)
    sp, dp = P.pad_case(s, d, 2 * P.halo4_pad_width(ws, tw))
    whole = K.conv3x3_upfold(dp["x"].cuda(), g["w"], g["bias"], arm=arm)
    assert torch.equal(whole[:, :, :2 * ws], out), f"{what}: differs from the whole-tile kernel on the zero-padded source"


def test_conv3x3_halo4_fold_partial_statistics(K):
    """The fold's statistics per (source row block, phase) at Cout = 320, both instruments, both 4-wave geometries."""
    n, hs, ws, cin, cout = P.HALO4_FOLD_STATS
    s = C.fold_spec(n, hs, ws, cin, cout, True)
    for instrument in INSTRUMENTS:
        d, r = C.case(s, instrument, True)
        g = _cu(d)
        for tw in (8, 16):
            out, parts = K.conv3x3_upfold(g["x"], g["w"], g["bias"], emit_gn=True, arm="halo4", partial_tiles=True, tw=tw)
            assert parts.shape == (n, 4 * P.halo4_row_blocks_per_image(hs, ws, tw), 32, 2)
            _check(instrument, s, r, out, f"conv3x3_upfold halo4 partial statistics tw {tw}", parts, "halo4_fold", tw)


# ---- 3. a whole-tile shape through the partial entry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("instrument", INSTRUMENTS)
def test_whole_tile_shapes_through_the_partial_entries_give_the_existing_bits(K, instrument):
    for s in P.WHOLE_HALO:
        d, r = C.case(s, instrument)
        g = _cu(d)
        a, pa = _halo(K, s, g, instrument, True, partial=True)
        b, pb = _halo(K, s, g, instrument, True, partial=False)
        _check(instrument, s, r, a, f"conv3x3_halo partial entry, whole tiles {P.sid(s)}", pa, "halo")
        assert torch.equal(a, b) and torch.equal(pa, pb)
    for s, tw in P.WHOLE_HALO4:
        d, r = C.case(s, instrument)
        g = _cu(d)
        run = lambda **kw: K.conv3x3_halo4(g["x"], g["w"], g["bias"], g["temb"], g["res"], temb_div=s.tdiv, **kw)
        a, pa = run(emit_gn=True, partial_tiles=True)                        # (the default geometry is the whole-tile entry's)
        b, pb = run(emit_gn=True)
        _check(instrument, s, r, a, f"conv3x3_halo4 partial entry, whole tiles {P.sid(s)}", pa, "halo4", tw)
        assert pa.shape == pb.shape and torch.equal(a, b) and torch.equal(pa, pb)
        if s.cin >= 128:
            assert torch.equal(run(split_k=2, partial_tiles=True, tw=tw), run(split_k=2))
    n, hs, ws, cin, cout = P.WHOLE_FOLD
    s = C.fold_spec(n, hs, ws, cin, cout, True)
    d, r = C.case(s, instrument, True)
    g = _cu(d)
    for arm in ("halo", "halo4", "halo4w"):
        a, pa = K.conv3x3_upfold(g["x"], g["w"], g["bias"], emit_gn=True, arm=arm, partial_tiles=True)
        b, pb = K.conv3x3_upfold(g["x"], g["w"], g["bias"], emit_gn=True, arm=arm)
        _check(instrument, s, r, a, f"conv3x3_upfold {arm} partial entry, whole tiles", pa, "halo_fold" if arm == "halo" else "halo4_fold", 16)
        assert pa.shape == pb.shape and torch.equal(a, b) and torch.equal(pa, pb), arm


def test_the_whole_tile_entries_keep_refusing_ragged_widths(K):
    L = K._lib.load()
    x = torch.zeros(2 * 8 * 12 * 64, dtype=BF16, device="cuda")
    w = torch.zeros(160 * 9 * 64, dtype=BF16, device="cuda")
    out = torch.zeros(2 * 8 * 12 * 160, dtype=BF16, device="cuda")
    rc = L.fmc_conv3x3_halo_bf16(x.data_ptr(), None, 64, w.data_ptr(), None, None, None, out.data_ptr(), 2, 8, 12, 64, 160, 0, 1, 0, None, 0, None, K._stream())
    assert rc != 0 and b"needs W % 32 == 0" in L.fmc_last_error()          # (its message as it was)
    rc = L.fmc_conv3x3_halo4_bf16(x.data_ptr(), None, 64, w.data_ptr(), None, None, None, out.data_ptr(), 2, 8, 12, 64, 160, 0, 1, 0, None, 1, None, 0, 0, K._stream())
    assert rc != 0 and b"needs W % 8 == 0" in L.fmc_last_error()
    rc = L.fmc_conv3x3_halo4_partial_bf16(x.data_ptr(), None, 64, w.data_ptr(), None, None, None, out.data_ptr(), 2, 8, 12, 64, 160, 0, 1, 0, None, 1, None, 0, 0, 12,
                                          K._stream())
    assert rc != 0                                                           # tw: 8 or 16
    rc = L.fmc_conv3x3_halo4_partial_bf16(x.data_ptr(), None, 64, w.data_ptr(), None, None, None, out.data_ptr(), 2, 8, 12, 64, 160, 0, 1, 0, None, 1, None, 0, 1, 8,
                                          K._stream())
    assert rc != 0                                                           # the wide form has 16-pixel row blocks only
    torch.cuda.synchronize()
    assert int(out.view(torch.int16).abs().sum()) == 0                       # nothing was launched


# ---- 4. poisoned surroundings, raw C ABI ---------------------------------------------------------------------------------------------------------------------
# (n, H, W, Cin, Cout, c2, upsample, extras, gn): the last image's last row ends in a ragged tile in every case
GUARD_HALO = [(3, 11, 48, 128, 160, 0, False, True, False), (2, 12, 31, 128, 320, 0, False, False, True), (1, 5, 40, 192, 160, 64, False, True, False),
              (2, 12, 44, 64, 160, 0, True, True, False), (2, 13, 1, 64, 160, 0, False, False, False)]


@pytest.mark.parametrize("n,h,w,cin,cout,c2,ups,extras,gn", GUARD_HALO)
def test_conv3x3_halo_partial_poisoned_surroundings(K, n, h, w, cin, cout, c2, ups, extras, gn):
    L = K._lib.load()
    hs, ws = (h // 2, w // 2) if ups else (h, w)
    assert L.fmc_conv3x3_halo_partial_supported(n, h, w, cin, cin - c2, cout, int(ups))
    div = n if extras and n > 1 else 1
    x, x2, wt, bias, temb, res = _conv_data(n, hs, ws, cin, cout, h + cin, c2, h, w, temb_rows=n // div)
    if not extras:
        bias = temb = res = None
    coef = None
    if gn:
        x = (x.float() * 1.7 + 0.3).bfloat16()
        gen = torch.Generator().manual_seed(5)
        coef = torch.stack([torch.randn(n, cin, generator=gen) * 0.3 + 1.0, torch.randn(n, cin, generator=gen) * 0.2], -1).contiguous()
    tiles = L.fmc_conv3x3_halo_partial_tiles_per_image(h, w)
    emit = cout % 64 == 0

    def fn(g):
        xd, x2d, bd, td, rd = _conv_operands(g, x, x2, bias, temb, res)
        wp = _packed(K, g, "fmc_conv3x3_halo_pack_weight", wt, 9)
        cd = g.inp(coef.view(n * cin, 2), 512, 0, "gn_coef") if gn else None
        out = g.out((n * h * w, cout), BF16, CONV_BAND, 0, "out")
        part = g.out((n * tiles, 64), F32, max(tiles, 4), 0, "gn_partials") if emit else None
        _call(K, "fmc_conv3x3_halo_partial_bf16", xd.data_ptr(), _p(x2d), cin - c2, wp.data_ptr(), _p(bd), _p(td), _p(rd), out.data_ptr(), n, h, w, cin, cout,
              td.stride(0) if extras else 0, div, int(ups), _p(cd), 1, _p(part), K._stream())
        return {"out": out, "gn_partials": part} if emit else {"out": out}

    got = _run(fn, f"conv3x3_halo partial {(n, h, w, cin, cout)} c2 {c2} ups {ups} extras {extras} gn {gn}")
    out = got["out"].view(n, h, w, cout)
    err = C.rel_inf(out, _conv_ref(x, x2, wt, bias, temb, res, div, int(ups), coef, act=True))
    print(f"   rel-inf {err:.3e} (gate {'8e-3' if gn else '6e-3'})")
    assert err < (8e-3 if gn else 6e-3)
    if emit:
        _check_partials(got["gn_partials"], out, n, cout)


def test_conv3x3_halo_sc_partial_poisoned_surroundings(K):
    n, h, w, cin, cout, cs1, cs2 = 2, 11, 48, 64, 320, 64, 64
    x, _, wt, bias, _, _ = _conv_data(n, h, w, cin, cout, 321)
    gen = torch.Generator().manual_seed(322)
    xs, xs2 = torch.randn(n, h, w, cs1, generator=gen).bfloat16(), torch.randn(n, h, w, cs2, generator=gen).bfloat16()
    wsc, bsc = (torch.randn(cout, cs1 + cs2, generator=gen) * (cs1 + cs2) ** -0.5).bfloat16(), torch.randn(cout, generator=gen).bfloat16()
    tiles = K._lib.load().fmc_conv3x3_halo_partial_tiles_per_image(h, w)

    def fn(g):
        xd, _, bd, _, _ = _conv_operands(g, x, None, bias, None, None)
        xsd, xs2d = g.inp(xs.reshape(-1, cs1), CONV_BAND, 0, "xs"), g.inp(xs2.reshape(-1, cs2), CONV_BAND, 0, "xs2")
        bscd = g.inp(bsc, 8, 0, "shortcut bias")
        wp = g.inp(K._w_halo_sc_packed(wt.cuda(), wsc.cuda()).cpu().view(-1, cin), 320 * 9, 0, "packed filter")
        out = g.out((n * h * w, cout), BF16, CONV_BAND, 0, "out")
        part = g.out((n * tiles, 64), F32, max(tiles, 4), 0, "gn_partials")
        _call(K, "fmc_conv3x3_halo_sc_partial_bf16", xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), bscd.data_ptr(), out.data_ptr(), xsd.data_ptr(), xs2d.data_ptr(),
              cs1, cs1 + cs2, n, h, w, cin, cout, cout, n, part.data_ptr(), K._stream())
        return {"out": out, "gn_partials": part}

    got = _run(fn, f"conv3x3_halo_sc partial {(n, h, w, cin, cout)} shortcut {cs1}+{cs2}")
    out = got["out"].view(n, h, w, cout)
    ref = _conv_ref(x, None, wt, bias) + torch.cat([xs, xs2], -1).float() @ wsc.float().t() + bsc.float()
    err = C.rel_inf(out, ref)
    print(f"   rel-inf {err:.3e} (gate 6e-3)")
    assert err < 6e-3
    _check_partials(got["gn_partials"], out, n, cout)


# (n, H, W, Cin, Cout, extras, split_k, wide, tw)
GUARD_HALO4 = [(5, 4, 6, 128, 80, True, 1, False, 8), (3, 8, 12, 192, 160, True, 2, False, 16), (3, 8, 12, 192, 160, True, 3, False, 8),
               (3, 11, 20, 64, 320, False, 1, False, 8), (3, 11, 20, 64, 320, True, 1, False, 16), (2, 7, 28, 64, 160, True, 1, True, 16),
               (9, 5, 7, 64, 80, False, 1, False, 8)]


@pytest.mark.parametrize("n,h,w,cin,cout,extras,split_k,wide,tw", GUARD_HALO4)
def test_conv3x3_halo4_partial_poisoned_surroundings(K, n, h, w, cin, cout, extras, split_k, wide, tw):
    L = K._lib.load()
    assert L.fmc_conv3x3_halo4_partial_supported(n, h, w, cin, cin, cout, 0, int(wide))
    div = n if extras and n == 3 else 1
    x, _, wt, bias, temb, res = _conv_data(n, h, w, cin, cout, h + cin + n, temb_rows=n // div)
    if not extras:
        bias = temb = res = None
    emit = split_k == 1 and cout % 64 == 0 and (160 if wide else 80) % (cout // 32) == 0
    blocks = L.fmc_conv3x3_halo4_partial_row_blocks_per_image(h, w, tw)

    def fn(g):
        xd, _, bd, td, rd = _conv_operands(g, x, None, bias, temb, res)
        wp = _packed(K, g, "fmc_conv3x3_halo4_pack_weight", wt, 9, int(wide))
        out = g.out((n * h * w, cout), BF16, CONV_BAND, 0, "out")
        part = g.out((n * blocks, 64), F32, max(blocks, 4), 0, "gn_partials") if emit else None
        ws = g.out((split_k * n * h * w, cout), F32, CONV_BAND, 0, "split-K workspace") if split_k > 1 else None
        _call(K, "fmc_conv3x3_halo4_partial_bf16", xd.data_ptr(), None, cin, wp.data_ptr(), _p(bd), _p(td), _p(rd), out.data_ptr(), n, h, w, cin, cout,
              td.stride(0) if extras else 0, div, 0, _p(part), split_k, _p(ws), split_k * n * h * w * cout * 4 if split_k > 1 else 0, int(wide), tw, K._stream())
        return {"out": out, "gn_partials": part} if emit else {"out": out}

    got = _run(fn, f"conv3x3_halo4 partial {(n, h, w, cin, cout)} extras {extras} split {split_k} wide {wide} tw {tw}")
    out = got["out"].view(n, h, w, cout)
    err = C.rel_inf(out, _conv_ref(x, None, wt, bias, temb, res, div))
    print(f"   rel-inf {err:.3e} (gate 6e-3)")
    assert err < 6e-3
    if emit:
        _check_partials(got["gn_partials"], out, n, cout)


# (arm, n, source H, source W, Cin, Cout, tw)
GUARD_FOLD = [("halo", 2, 5, 20, 64, 320, 32), ("halo4", 3, 8, 12, 128, 160, 8), ("halo4", 3, 8, 12, 128, 160, 16), ("halo4w", 3, 8, 12, 128, 320, 16)]


@pytest.mark.parametrize("arm,n,hs,ws,cin,cout,tw", GUARD_FOLD)
def test_conv3x3_fold_partial_poisoned_surroundings(K, arm, n, hs, ws, cin, cout, tw):
    L = K._lib.load()
    wide = arm == "halo4w"
    splits = 4 * (L.fmc_conv3x3_halo_partial_tiles_per_image(hs, ws) if arm == "halo" else L.fmc_conv3x3_halo4_partial_row_blocks_per_image(hs, ws, tw))
    bn = 80 if arm == "halo4" else 160
    emit = cout % 64 == 0 and bn % (cout // 32) == 0
    x, _, wt, bias, _, _ = _conv_data(n, hs, ws, cin, cout, hs + cin + n)

    def fn(g):
        xd, _, bd, _, _ = _conv_operands(g, x, None, bias, None, None)
        wp = _packed(K, g, "fmc_conv3x3_upfold_pack_weight", wt, 16, bn)
        out = g.out((n * 4 * hs * ws, cout), BF16, 4 * CONV_BAND, 0, "out")
        part = g.out((n * splits, 64), F32, max(splits, 4), 0, "gn_partials") if emit else None
        if arm == "halo":
            _call(K, "fmc_conv3x3_halo_fold_partial_bf16", xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), out.data_ptr(), n, hs, ws, cin, cout, _p(part), K._stream())
        else:
            _call(K, "fmc_conv3x3_halo4_fold_partial_bf16", xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), out.data_ptr(), n, hs, ws, cin, cout, _p(part), int(wide), tw,
                  K._stream())
        return {"out": out, "gn_partials": part} if emit else {"out": out}

    got = _run(fn, f"conv3x3 fold partial {arm} {(n, hs, ws, cin, cout)} tw {tw}")
    out = got["out"].view(n, 2 * hs, 2 * ws, cout)
    err = C.rel_inf(out, _conv_ref(x, None, wt, bias, mode=1))
    print(f"   rel-inf {err:.3e} (gate 6e-3)")
    assert err < 6e-3
    if emit:
        _check_partials(got["gn_partials"], out, n, cout)


# ---- 6. module and model level ---------------------------------------------------------------------------------------------------------------------------------
def _is_partial(shape):
    return any(e == "partial" or (isinstance(e, tuple) and e and e[0] == "partial") for e in shape)


def test_frozen_conv3x3_forward_and_backward_at_8x12(K, monkeypatch):
    """Stage-2 / stage-3 training at the reference's own resolution: forward and backward-data of a frozen 3x3 convolution on 8 x 12 images take the
    partial launch with the switch on; Y and dX element by element against float64."""
    monkeypatch.setattr(K, "CONV_HALO_MIN_TILES", 1)
    monkeypatch.setattr(K, "PARTIAL_TILES", True)
    monkeypatch.setattr(K, "PARTIAL_CONV_ROUTED", K.PARTIAL_CONV_ROUTED | {"halo4"})
    n, h, w, c = 3, 8, 12, 320
    gen = torch.Generator().manual_seed(812)
    x = torch.randn(n, c, h, w, generator=gen).bfloat16().contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(c, c, 3, 3, generator=gen) * (9 * c) ** -0.5).bfloat16().contiguous(memory_format=torch.channels_last)
    bias = torch.randn(c, generator=gen).bfloat16()
    dy = torch.randn(n, c, h, w, generator=gen).bfloat16().contiguous(memory_format=torch.channels_last)
    xd = x.cuda().requires_grad_(True)
    K.call_log = []
    try:
        y = K.conv3x3_frozen(xd, wt.cuda(), bias.cuda())
        y.backward(dy.cuda())
        torch.cuda.synchronize()
    finally:
        log, K.call_log = K.call_log, None
    assert [f for f, *_ in log] == ["conv_halo4", "conv_halo4"] and all(_is_partial(s) for _, s, _ in log), log
    ref_y = F.conv2d(x.double(), wt.double(), bias.double(), 1, 1)
    mag_y = F.conv2d(x.double().abs(), wt.double().abs(), bias.double().abs(), 1, 1)
    ref_dx = F.conv_transpose2d(dy.double(), wt.double(), None, 1, 1)
    mag_dx = F.conv_transpose2d(dy.double().abs(), wt.double().abs(), None, 1, 1)
    print(f"   frozen conv 8x12: Y rel-inf {C.rel_inf(y, ref_y):.3e}, dX rel-inf {C.rel_inf(xd.grad, ref_dx):.3e}")
    uy = C.assert_bf16_close(y, ref_y, mag_y, "frozen conv3x3 8x12 forward")
    ux = C.assert_bf16_close(xd.grad, ref_dx, mag_dx, "frozen conv3x3 8x12 dX")
    print(f"   err / bound: Y {uy:.3f}, dX {ux:.3f}")


def test_full_width_unet_conv_partial_switch(K, monkeypatch, golden_dir):
    """The full-width U-Net + CMC + OMC of tests/test_gpu_full_width.py (16 x 128 x 192: latent 16 x 24, inner levels 8 x 12, 4 x 6 and 2 x 3 -- the
    256 x 384 clip's levels 1 .. 3 at half size), bf16, `CONV_HALO_MIN_TILES` lowered for the 16-image input.  Switch on: the 3x3 convolutions of the
    ragged levels run as partial launches and the output meets that test's gate against the reference golden.  Switch off: no partial launch, no halo
    launch at a width that is no multiple of 8.  (The small-width stack of tests/common_models.py cannot show this: its channel counts, 64 .. 256, are
    no multiple of the halo kernels' 80-channel tiles.)"""
    import numpy as np
    from einops import rearrange

    from synfmc_amd.data.dataset import to_plucker_embedding
    from synfmc_amd.models.pose_obj_adaptor import CamObjPoseAdaptor
    from synfmc_amd.util import get_traj_features_v2
    from tests import common_models as CM
    H, W = 128, 192
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    g = np.load(os.path.join(golden_dir, "g5_unet_full_width.npz"))
    ou, oe, oa, clip = CM.full_width_case(int(g["seed"]), int(g["clip_seed"]), H, W)
    pu, pe, pa = CM.build_product(ou, oe, oa, CM.FULL_WIDTHS, CM.FULL_CROSS_DIM, dtype=BF16)
    del ou, oe, oa
    gold = torch.from_numpy(g["out"])
    monkeypatch.setattr(K, "CONV_HALO_MIN_TILES", 1)
    monkeypatch.setattr(K, "DETERMINISTIC", True)
    assert not K.PARTIAL_TILES
    with torch.no_grad():
        emb = to_plucker_embedding(clip["c2w"].cuda(), clip["K"].cuda(), (H, W))
        pose_emb = rearrange(emb, "b f c h w -> b c f h w").to(BF16)
        tf = get_traj_features_v2(clip["infos"], clip["masks"], pa, False, 0.0, [False], "cuda", BF16)
        wrapper = CamObjPoseAdaptor(pu, pe)
        args = (clip["latents"].cuda().to(BF16), torch.tensor([801]).cuda(), clip["text"].cuda().to(BF16), pose_emb)
        outs, logs = {}, {}
        for on in (False, True):
            K.PARTIAL_TILES = on
            try:
                wrapper(*args, tf)                                           # (autotuned arms, cached pose terms and packs settle)
                K.call_log = []
                outs[on] = wrapper(*args, tf).float().cpu()
            finally:
                K.PARTIAL_TILES = False
                logs[on], K.call_log = K.call_log, None
    halo = {on: [(f, s) for f, s, _ in logs[on] if f in ("conv_halo", "conv_halo4")] for on in logs}
    ragged = lambda s: s[2] % 8 != 0 and not (len(s) > 5 and s[5] is True and (s[2] // 2) % 8 == 0)      # (n, h, w, ...): the launch's own width
    n_partial = {on: sum(_is_partial(s) for _, s in halo[on]) for on in halo}
    e_on, e_off = C.rel_inf(outs[True], gold), C.rel_inf(outs[False], gold)
    print(f"   16x{H}x{W}: halo launches off {len(halo[False])} (partial {n_partial[False]}), on {len(halo[True])} (partial {n_partial[True]}); "
          f"vs golden: on {e_on:.3e}, off {e_off:.3e}; on vs off {C.rel_inf(outs[True], outs[False]):.3e}")
    assert n_partial[False] == 0 and not any(ragged(s) for _, s in halo[False]), "switch off: a halo launch at a ragged width"
    assert len(logs[False]) >= len(logs[True])
    assert n_partial[True] > 0 and {s[2] for _, s in halo[True] if _is_partial(s)} >= {24, 12, 6}         # (level 0 on 10 x 32 tiles, levels 1 and 2 on row blocks)
    assert all(_is_partial(s) for _, s in halo[True] if ragged(s))
    assert len(halo[True]) > len(halo[False])                                # launches that were the ring kernel's or the vendor arm's
    assert e_on < 4e-2 and e_off < 4e-2                                      # (test_full_width_bf16_parity_and_format_share: e_gold < 4e-2)

"""CPU side of tests/test_gpu_conv_partial.py (the halo convolutions at any image width; tests/conv_partial_common.py):

1. the tile arithmetic restated in the test module -- ceiling tile counts, `partial_tw`, the ragged slot maps -- against brute force over H, W in 1 .. 50
   and against the library's own count functions (host code: they need no GPU);
2. the references of every GPU case meet the exact instrument's conditions and the ambiguity cap;
3. the dispatch with `hip_ops.PARTIAL_TILES` off and on, on recording stand-ins for the launch wrappers;
4. the wrong plain-torch stand-ins, each rejected by the assertion meant for it."""
import pytest
import torch

from tests import conv_fwd_common as C
from tests import conv_partial_common as P
from tests import edge_guard_common as EG
from tests import halo_host_surface_common as S
from tests.conv_dispatch_standins import Launches as _Launches

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def K():
    from synfmc_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def L(K):
    return K._lib.load()


# ---- 1. tile arithmetic ----------------------------------------------------------------------------------------------------------------------------------
def _brute_tiles(h, w, th, tw):
    """Tiles of th x tw pixels that hold at least one pixel of an h x w image, and the pixels they cover, by enumeration."""
    tiles = {(y // th, x // tw) for y in range(h) for x in range(w)}
    return len(tiles), len(tiles) * th * tw


def test_tile_counts_against_brute_force_and_the_library(L):
    for h in range(1, 51):
        for w in range(1, 51):
            n_halo, _ = _brute_tiles(h, w, 10, 32)
            assert P.halo_tiles_per_image(h, w) == n_halo == L.fmc_conv3x3_halo_partial_tiles_per_image(h, w)
            if w % 32 == 0:
                assert n_halo == L.fmc_conv3x3_halo_tiles_per_image(h, w)
            pads = {}
            for tw in (8, 16):
                blocks, pads[tw] = _brute_tiles(h, w, P.halo4_th(tw), tw)
                assert P.halo4_row_blocks_per_image(h, w, tw) == blocks == L.fmc_conv3x3_halo4_partial_row_blocks_per_image(h, w, tw)
                assert P.halo4_padded_pixels(h, w, tw) == pads[tw]
                for n, cout, wide in ((1, 80, 0), (5, 320, 0), (9, 160, 0), (3, 320, 1)):
                    if wide and tw == 8:
                        continue
                    per_tile = 8 if tw == 8 else 2
                    want = -(-n * blocks // per_tile) * (cout // (160 if wide else 80))
                    assert P.halo4_tiles(n, h, w, cout, wide, tw) == want == L.fmc_conv3x3_halo4_partial_tiles(n, h, w, cout, wide, tw)
            if w % 8 == 0:
                want_tw = 16 if w % 16 == 0 else 8
                assert L.fmc_conv3x3_halo4_row_blocks_per_image(h, w) == P.halo4_row_blocks_per_image(h, w, want_tw)
                assert L.fmc_conv3x3_halo4_tiles(5, h, w, 320, 0) == P.halo4_tiles(5, h, w, 320, False, want_tw)
            else:
                want_tw = 8 if pads[8] < pads[16] else 16                   # fewer pad pixels over the image, ties to 16
            assert P.partial_tw(h, w) == want_tw == L.fmc_conv3x3_halo4_partial_tw(h, w, 0)
            assert P.partial_tw(h, w, True) == 16 == L.fmc_conv3x3_halo4_partial_tw(h, w, 1)
    assert [P.partial_tw(h, w) for h, w in ((4, 6), (8, 12), (16, 24), (11, 20), (7, 28), (5, 7), (6, 17))] == [8, 16, 8, 8, 16, 8, 8]


@pytest.mark.parametrize("layout,th,tw", [("halo", 10, 32), ("halo4", 10, 16), ("halo4", 5, 8)])
def test_slot_maps_against_brute_force(layout, th, tw):
    for h in range(1, 51, 3):
        for w in range(1, 51):
            slot, per = P.slot_map(layout, h, w, None if layout == "halo" else tw)
            tx = -(-w // tw)
            assert per == _brute_tiles(h, w, th, tw)[0] and slot.shape == (h, w)
            want = torch.tensor([[(y // th) * tx + x // tw for x in range(w)] for y in range(h)])
            assert torch.equal(slot, want)
            assert int(slot.max()) == per - 1 and len(slot.unique()) == per          # every slot holds a pixel: no slot of pad columns alone
            if (layout == "halo" and w % 32 == 0) or (layout == "halo4" and w % 8 == 0 and (16 if w % 16 == 0 else 8) == tw):
                old, old_per = C.slot_map(layout, h, w)
                assert old_per == per and torch.equal(old, slot)
    for h, w in ((6, 10), (10, 34), (22, 50)):                                       # the fold: four slots per SOURCE tile
        slot, per = P.slot_map(layout + "_fold", 2 * h, 2 * w, None if layout == "halo" else tw)
        base, bper = P.slot_map(layout, h, w, None if layout == "halo" else tw)
        assert per == 4 * bper
        for y in range(2 * h):
            for x in range(2 * w):
                assert int(slot[y, x]) == 4 * int(base[y // 2, x // 2]) + 2 * (y % 2) + (x % 2)


def test_pad_widths():
    assert [P.halo_pad_width(w) for w in (1, 31, 32, 33, 48)] == [32, 32, 32, 64, 64]
    assert P.halo4_pad_width(12, 8) == 24 and P.halo4_pad_width(28, 8) == 40 and P.halo4_pad_width(12, 16) == 16 and P.halo4_pad_width(6, 8) == 8
    assert P.halo4_pad_width(17, 8) == 24 and P.halo4_pad_width(17, 16) == 32 and P.halo4_pad_width(7, 16) == 16 and P.halo4_pad_width(20, 8) == 24


def test_predicates_drop_the_width_rule_alone(K, L):
    for w in range(1, 70):
        assert K.conv3x3_halo_partial_supported(2, 11, w, 128, 128, 160, False)
        assert K.conv3x3_halo_supported(2, 11, w, 128, 128, 160, False) == (w % 32 == 0)
        assert K.conv3x3_halo_sc_partial_supported(2, 11, w, 64, 160, 128, 64)
        assert K.conv3x3_halo_sc_supported(2, 11, w, 64, 160, 128, 64) == (w % 32 == 0)
        assert K.conv3x3_halo4_partial_supported(2, 11, w, 128, 128, 80, False)
        assert K.conv3x3_halo4_supported(2, 11, w, 128, 128, 80, False) == (w % 8 == 0)
        assert K.conv3x3_halo4_partial_supported(2, 11, w, 128, 128, 160, False, wide=True)
        assert K.conv3x3_halo4_supported(2, 11, w, 128, 128, 160, False, wide=True) == (w % 16 == 0)
        assert L.fmc_conv3x3_halo_fold_partial_supported(2, 11, w, 64, 160) and L.fmc_conv3x3_halo4_fold_partial_supported(2, 11, w, 64, 80, 0)
        assert bool(L.fmc_conv3x3_halo_fold_supported(2, 11, w, 64, 160)) == (w % 32 == 0)
        assert bool(L.fmc_conv3x3_halo4_fold_supported(2, 11, w, 64, 80, 0)) == (w % 8 == 0)
    # every other condition stays
    assert not K.conv3x3_halo_partial_supported(2, 11, 48, 96, 96, 160, False) and not K.conv3x3_halo_partial_supported(2, 11, 48, 128, 128, 80, False)
    assert not K.conv3x3_halo_partial_supported(2, 11, 0, 128, 128, 160, False) and not K.conv3x3_halo_partial_supported(0, 11, 48, 128, 128, 160, False)
    assert not K.conv3x3_halo_partial_supported(2, 11, 47, 128, 128, 160, True)                  # upsample: an even output size
    assert not K.conv3x3_halo_partial_supported(2, 11, 48, 128, 96, 160, False)                  # the first source's channels % 64
    assert not K.conv3x3_halo4_partial_supported(2, 11, 12, 128, 128, 120, False) and not K.conv3x3_halo4_partial_supported(2, 11, 12, 128, 128, 80, False, wide=True)
    assert not K.conv3x3_halo_sc_partial_supported(2, 11, 48, 64, 160, 96, 96)
    assert not K.conv3x3_halo_partial_supported(1 << 12, 1 << 9, 1 << 9 | 1, 64, 64, 160, False)  # an operand of 2 GiB


# ---- 2. the GPU cases' references ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,folded", P.all_specs(), ids=lambda v: P.sid(v) if isinstance(v, C.Spec) else str(v))
def test_case_references_meet_the_instruments_conditions(s, folded):
    """`conv_fwd_common.case` asserts `assert_exact_conditions` (sum|terms| < 256, integer outputs, sums of squares < 2^24) and the ambiguity cap."""
    d, r = C.case(s, "exact", folded)
    C.assert_exact_conditions(r, s)
    peak = float(r["mag"].max())
    d2, r2 = C.case(s, "rounding", folded)
    assert r2["amb_share"] <= C.AMBIGUOUS_CAP
    print(f"   {P.sid(s)}: exact sum|terms| peaks at {peak:.0f} (< 256), ambiguous operands {100 * r2['amb_share']:.3f} %")


# ---- 3. dispatch ---------------------------------------------------------------------------------------------------------------------------------------------
def _conv_args(n, h, w, cin, cout):
    x = torch.zeros(n, h, w, cin, dtype=BF16).permute(0, 3, 1, 2)
    wt = torch.zeros(cout, cin, 3, 3, dtype=BF16).contiguous(memory_format=torch.channels_last)
    return x, wt


ALL_KINDS = frozenset(("halo", "halo_sc", "halo4", "upfold_halo", "upfold_halo4"))


def test_conv3x3_dispatch_switch_off_and_on(monkeypatch, K):
    calls = _Launches(monkeypatch, K)
    assert K.PARTIAL_TILES is False                                         # default off
    assert K.PARTIAL_CONV_ROUTED == ALL_KINDS - {"upfold_halo"}              # (the fold on conv_halo4's row blocks measured faster wherever both run)
    run = lambda n, h, w, cin, cout, **kw: K.conv3x3(*_conv_args(n, h, w, cin, cout), None, **kw)
    with torch.no_grad():
        # switch off: a ragged width goes where it went -- conv_halo4's whole row blocks (W % 8 == 0) or the ring kernel / vendor arm
        monkeypatch.setattr(K, "PARTIAL_CONV_ROUTED", ALL_KINDS)
        for w, want in ((48, [("halo4", False, None)]), (24, [("halo4", False, None)]), (12, [("ring",)]), (6, [("ring",)]), (7, [("ring",)]),
                        (32, [("halo", False)]), (16, [("halo4", False, None)])):
            run(4, 8, w, 320, 320)
            assert calls.take() == want, w
        run(4, 4, 6, 320, 320, upsample=True)
        assert calls.take() == [("ring",)]
        # switch on, every kind routed: the partial launches; whole-tile shapes keep their launches
        monkeypatch.setattr(K, "PARTIAL_TILES", True)
        for w, want in ((48, [("halo", True)]), (24, [("halo", True)]), (12, [("halo", True)]), (32, [("halo", False)]), (64, [("halo", False)])):
            run(4, 8, w, 320, 320)
            assert calls.take() == want, w
        run(4, 8, 12, 320, 240)                                              # Cout % 160: conv_halo refuses, conv_halo4's row blocks take it
        assert calls.take() == [("halo4", True, 16)]
        run(4, 4, 6, 320, 240)
        assert calls.take() == [("halo4", True, 8)]
        run(4, 4, 6, 320, 320, upsample=True)                                # source 4 x 6 -> the fold on 10 x 32 source tiles
        assert calls.take() == [("upfold", "halo_partial")]
        run(4, 4, 6, 320, 240, upsample=True)
        assert calls.take() == [("upfold", "halo4_partial")]
        run(4, 8, 16, 320, 240, upsample=True)                               # source width 16: the whole-tile fold, as without the switch
        assert calls.take() == [("upfold", "halo4")]
        run(4, 8, 12, 320, 200)                                              # Cout % 80: no halo kernel
        assert calls.take() == [("ring",)]
        run(4, 16, 12, 320, 320, stride=(2, 2))                              # stride 2: out of scope
        assert calls.take() == [("ring",)]
        # only the routed kinds
        monkeypatch.setattr(K, "PARTIAL_CONV_ROUTED", frozenset(("halo4", "upfold_halo4")))
        for w, want in ((48, [("halo4", False, None)]), (24, [("halo4", False, None)]), (12, [("halo4", True, 16)]), (6, [("halo4", True, 8)])):
            run(4, 8 if w > 6 else 4, w, 320, 320)
            assert calls.take() == want, w
        run(4, 4, 6, 320, 320, upsample=True)
        assert calls.take() == [("upfold", "halo4_partial")]
        monkeypatch.setattr(K, "PARTIAL_CONV_ROUTED", frozenset())
        run(4, 8, 12, 320, 320)
        run(4, 4, 6, 320, 320, upsample=True)
        assert calls.take() == [("ring",), ("ring",)]
        # the launch count threshold counts the ceiling tile counts
        monkeypatch.setattr(K, "PARTIAL_CONV_ROUTED", ALL_KINDS)
        monkeypatch.setattr(K, "CONV_HALO_MIN_TILES", 9)
        run(4, 8, 48, 320, 320)                                              # 4 images x 2 column tiles x 2 channel tiles = 16 workgroups
        assert calls.take() == [("halo", True)]
        monkeypatch.setattr(K, "CONV_HALO_MIN_TILES", 17)
        run(4, 8, 48, 320, 320)
        assert calls.take() == [("halo4", False, None)]
    # a gradient: the forward of a frozen convolution and its backward-data take the same dispatch (statistics are not emitted)
    monkeypatch.setattr(K, "CONV_HALO_MIN_TILES", 1)
    monkeypatch.setattr(K, "PARTIAL_CONV_ROUTED", frozenset(("halo4",)))
    x, wt = _conv_args(4, 8, 12, 320, 320)
    K.conv3x3_frozen(x.requires_grad_(True), wt, None).sum().backward()
    assert calls.take() == [("halo4", True, 16), ("halo4", True, 16)]


def test_shortcut_fold_dispatch(monkeypatch, K):
    calls = _Launches(monkeypatch, K)
    partial = lambda *a: getattr(K._shortcut_route(*a), "partial", False)    # the shortcut route asked for "partial" (no route: no)
    args = (4, 8, 48, 320, 320, 640, 320)
    assert not partial(*args)                                                # switch off
    monkeypatch.setattr(K, "PARTIAL_TILES", True)
    monkeypatch.setattr(K, "PARTIAL_CONV_ROUTED", frozenset(("halo_sc",)))
    assert partial(*args) and not partial(4, 8, 64, 320, 320, 640, 320)      # a whole-tile width keeps its launch
    assert not partial(4, 8, 48, 320, 240, 640, 320)
    # (storage-less operands that say they are on the GPU: `conv3x3` asks the same route as `shortcut_fold_ok`, which looks at them)
    x, wt = S.image(4, 8, 48, 320, nchw=True, cuda=True), S.filter_cl(320, 320)
    xs = S.image(4, 8, 48, 320, nchw=True, cuda=True)
    with torch.no_grad():
        assert K.shortcut_fold_ok(x, wt, xs, xs)
        K.conv3x3(x, wt, None, shortcut=(xs, xs, S.image(320, 640), None))
        assert calls.take() == [("halo_sc", True)]
        x, xs = S.image(4, 8, 64, 320, nchw=True, cuda=True), S.image(4, 8, 64, 320, nchw=True, cuda=True)
        assert K.shortcut_fold_ok(x, wt, xs, xs)
        K.conv3x3(x, wt, None, shortcut=(xs, xs, S.image(320, 640), None))
        assert calls.take() == [("halo_sc", False)]
    monkeypatch.setattr(K, "PARTIAL_CONV_ROUTED", frozenset(("halo",)))
    assert not partial(*args)
    x, xs = S.image(4, 8, 48, 320, nchw=True, cuda=True), S.image(4, 8, 48, 320, nchw=True, cuda=True)
    with torch.no_grad():
        assert not K.shortcut_fold_ok(x, wt, xs, xs)


def test_routing_rule_restates_the_measured_table(K):
    """`hip_ops.partial_conv_routed` on rows of profiles/partial_tiles.md section 17 (n, H, W, Cin, Cout of the launch; the fold: its source)."""
    assert K.PARTIAL_CONV_RULES is True
    routed = [("halo", 16, 32, 48, 320, 320), ("halo", 32, 32, 48, 320, 320), ("halo", 16, 32, 48, 832, 320), ("halo", 32, 16, 24, 1920, 640),
              ("halo", 32, 16, 24, 1280, 1280), ("halo", 16, 32, 48, 320, 640), ("halo_sc", 32, 32, 48, 320, 320), ("halo_sc", 32, 16, 24, 640, 640),
              ("halo4", 32, 4, 6, 1280, 1280), ("halo4", 16, 8, 12, 1280, 1280), ("halo4", 32, 8, 12, 640, 1280), ("halo4", 16, 8, 12, 640, 1280),
              ("upfold_halo4", 32, 4, 6, 1280, 1280), ("upfold_halo4", 32, 8, 12, 1280, 1280)]
    kept = [("halo", 32, 32, 48, 640, 320), ("halo", 32, 32, 48, 960, 320), ("halo", 32, 32, 48, 640, 640), ("halo", 32, 16, 24, 1920, 1280),
            ("halo", 32, 16, 24, 2560, 1280), ("halo", 32, 8, 12, 640, 1280), ("halo", 32, 8, 12, 1280, 1280), ("halo", 32, 4, 6, 1280, 1280),
            ("halo_sc", 32, 8, 12, 1280, 1280), ("halo_sc", 32, 4, 6, 1280, 1280), ("halo_sc", 32, 16, 24, 1280, 1280),
            ("halo4", 32, 4, 6, 2560, 1280), ("halo4", 32, 8, 12, 1280, 1280), ("halo4", 32, 8, 12, 1920, 1280), ("halo4", 32, 8, 12, 2560, 1280),
            ("upfold_halo", 32, 4, 6, 1280, 1280), ("upfold_halo", 32, 8, 12, 1280, 1280)]
    for row in routed:
        assert K.partial_conv_routed(*row), row
    for row in kept:
        assert not K.partial_conv_routed(*row), row


def test_split_counts_the_partial_tiles(K):
    # 32 images of 4 x 6 at tw = 8: 32 row blocks = 4 pixel tiles x 16 channel tiles = 64 workgroups on 256 CUs -> split 4 of 20 chunks
    assert K.conv3x3_halo4_split(32, 4, 6, 1280, 1280, tw=8) == K.conv3x3_halo4_split(32, 5, 8, 1280, 1280) == 4
    # 8 x 12 at tw = 16: one row block per image, 16 x 16 = 256 workgroups -> no split, as 10 x 16
    assert K.conv3x3_halo4_split(32, 8, 12, 1280, 1280, tw=16) == K.conv3x3_halo4_split(32, 10, 16, 1280, 1280) == 1


# ---- 4. the wrong stand-ins --------------------------------------------------------------------------------------------------------------------------------
SPEC_R = C.spec("bf16", 2, 3, 11, 64, 64, extras="br")                       # tw = 8: the second column tile holds three columns


@pytest.fixture(scope="module")
def small_case():
    d = C.int_inputs(SPEC_R, 77)
    r = C.reference(SPEC_R, d, act=False)
    C.assert_exact_conditions(r, SPEC_R)
    return d, r


def _judge(s, r, got, tw):
    """What the GPU test asserts of a launch's arenas, in its order."""
    EG.assert_contained(got["out_arena"], got["out"], "out")
    if got["ws_arena"] is not None:
        EG.assert_contained(got["ws_arena"], got["ws"], "split-K workspace")
    C.check_exact(got["out"].reshape(r["ref"].shape), r["ref"], "out")
    if got["parts"] is not None:
        P.check_stats_exact(got["parts"], r["ref"], "halo4", tw, "stand-in")


@pytest.mark.parametrize("tw", [8, 16])
@pytest.mark.parametrize("splits", [1, 2])
def test_the_documented_launch_passes(small_case, tw, splits):
    d, r = small_case
    s = SPEC_R if splits == 1 else SPEC_R._replace(cin=128)
    if splits > 1:
        d = C.int_inputs(s, 78)
        r = C.reference(s, d, act=False)
    _judge(s, r, P.standin(s, d, tw, None, splits), tw)


def test_pad_column_read_as_the_next_rows_first_pixel_is_caught(small_case):
    d, r = small_case
    got = P.standin(SPEC_R, d, 8, "wrap_read")
    EG.assert_contained(got["out_arena"], got["out"], "out")                 # nothing is written outside, no poison moves ...
    with pytest.raises(AssertionError, match="differ from the exact result"):
        C.check_exact(got["out"].reshape(r["ref"].shape), r["ref"], "out")
    bad = (got["out"].reshape(r["ref"].shape).double() != r["ref"]).nonzero()
    assert set(bad[:, 2].tolist()) == {SPEC_R.w - 1}                         # ... only the last column's outputs change
    err = C.rel_inf(got["out"].reshape(r["ref"].shape), r["ref"])
    print(f"   a wrapped pad column moves the max-norm by {err:.3e}")


def test_pad_columns_in_a_statistics_slot_are_caught(small_case):
    d, r = small_case
    got = P.standin(SPEC_R, d, 8, "stats_pad")
    C.check_exact(got["out"].reshape(r["ref"].shape), r["ref"], "out")       # the output is right
    with pytest.raises(AssertionError, match="gn_partials"):
        P.check_stats_exact(got["parts"], r["ref"], "halo4", 8, "stand-in")


def test_a_stored_pad_column_is_caught_twice(small_case):
    d, r = small_case
    got = P.standin(SPEC_R, d, 8, "store_pad")
    with pytest.raises(EG.OutsideTouched):                                   # behind the last image's last row: only the sentinels see it
        EG.assert_contained(got["out_arena"], got["out"], "out")
    with pytest.raises(AssertionError, match="differ from the exact result"):     # over the next row's first pixels: only the values see it
        C.check_exact(got["out"].reshape(r["ref"].shape), r["ref"], "out")
    bad = (got["out"].reshape(r["ref"].shape).double() != r["ref"]).nonzero()
    assert set(bad[:, 2].tolist()) <= set(range(16 - SPEC_R.w))              # the first 16 - 11 columns of the rows behind


def test_floored_tile_count_is_caught(small_case):
    d, _ = small_case
    got = P.standin(SPEC_R, d, 8, "floor_tiles")
    with pytest.raises(EG.InsideUnwritten):
        EG.assert_contained(got["out_arena"], got["out"], "out")


def test_clamped_residual_on_a_valid_column_is_caught(small_case):
    d, r = small_case
    got = P.standin(SPEC_R, d, 8, "clamped_residual")
    EG.assert_contained(got["out_arena"], got["out"], "out")
    with pytest.raises(AssertionError, match="differ from the exact result"):
        C.check_exact(got["out"].reshape(r["ref"].shape), r["ref"], "out")
    bad = (got["out"].reshape(r["ref"].shape).double() != r["ref"]).nonzero()
    assert set(bad[:, 2].tolist()) <= {9, 10}                                # the partly filled tile's columns behind its first


def test_split_k_partial_of_a_pad_column_is_caught():
    s = SPEC_R._replace(cin=128)
    d = C.int_inputs(s, 78)
    r = C.reference(s, d, act=False)
    got = P.standin(s, d, 8, "splitk_pad", splits=2)
    with pytest.raises(EG.OutsideTouched):
        EG.assert_contained(got["ws_arena"], got["ws"], "split-K workspace")
    with pytest.raises(AssertionError, match="differ from the exact result"):
        C.check_exact(got["out"].reshape(r["ref"].shape), r["ref"], "out")

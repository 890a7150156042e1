"""Shared by tests/test_gpu_conv_partial.py (GPU) and tests/test_conv_partial_host.py (CPU): the halo convolutions at ANY image width
(`fmc_conv3x3_halo*_partial_*`, include/fmc_hip.h) -- the case tables, the slot map of a ragged width, the zero padding that turns a case into one the
whole-tile entry points take, and the wrong stand-ins the assertions have to reject.  References, generators and bounds are tests/conv_fwd_common.py's.

What a ragged width adds to the element-wise instruments of conv_fwd_common: in NHWC the word behind `(y, W - 1)` is `(y + 1, 0)` -- valid, finite data.
A pad column that is READ as that word, or STORED over it, moves no poison and stays below any max-norm gate; the exact runs see it (an output changes
by >= 1), and so every case here runs under both instruments."""
import torch
import torch.nn.functional as F

from tests import conv_fwd_common as C
from tests import edge_guard_common as EG

F64 = torch.float64


def cdiv(a, b):
    return -(-a // b)


# ---- tile arithmetic, restated from include/fmc_hip.h ---------------------------------------------------------------------------------------------------
def halo4_th(tw):
    return 5 if tw == 8 else 10


def halo_tiles_per_image(h, w):
    return cdiv(h, 10) * cdiv(w, 32)


def halo4_row_blocks_per_image(h, w, tw):
    return cdiv(h, halo4_th(tw)) * cdiv(w, tw)


def halo4_tiles(n, h, w, cout, wide, tw):
    nb = 8 if tw == 8 else 2
    return cdiv(n * halo4_row_blocks_per_image(h, w, tw), nb) * (cout // (160 if wide else 80))


def halo4_padded_pixels(h, w, tw):
    th = halo4_th(tw)
    return cdiv(h, th) * th * cdiv(w, tw) * tw


def partial_tw(h, w, wide=False):
    """`fmc_conv3x3_halo4_partial_tw`: the whole-tile entry's geometry where W % 8 == 0, else the one with fewer pad pixels over the image, ties to 16."""
    if wide:
        return 16
    if w % 8 == 0:
        return 16 if w % 16 == 0 else 8
    return 8 if halo4_padded_pixels(h, w, 8) < halo4_padded_pixels(h, w, 16) else 16


def slot_map(layout, h, w, tw=None):
    """`conv_fwd_common.slot_map` for any width: -> (slot of every output pixel `[h, w]`, slots per image), the column-tile count a ceiling.
    "halo": 10 x 32-pixel tiles; "halo4": row blocks of 10 x 16 (`tw` = 16) or 5 x 8 (`tw` = 8) pixels; "*_fold": the SOURCE image's tiles, four slots
    each (slot 4 t + 2 py + px sums the outputs (2 i + py, 2 j + px))."""
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    if layout.endswith("_fold"):
        base, per = slot_map(layout[:-5], h // 2, w // 2, tw)
        return base[y // 2, x // 2] * 4 + (y % 2) * 2 + (x % 2), 4 * per
    if layout == "halo":
        th, tw = 10, 32
    else:
        assert layout == "halo4" and tw in (8, 16)
        th = halo4_th(tw)
    tx = cdiv(w, tw)
    return (y // th) * tx + x // tw, cdiv(h, th) * tx


def tile_stats(out, layout, tw=None):
    """`conv_fwd_common.tile_stats` through the ragged slot map: (partials `[n, slots, 32, 2]` in float64, the same sums over absolute values)."""
    n, h, w, cout = out.shape
    slot, per = slot_map(layout, h, w, tw)
    o = out.double().reshape(n, h * w, 32, cout // 32)
    both = torch.stack([o.sum(-1), (o * o).sum(-1), o.abs().sum(-1)], -1)
    acc = torch.zeros(n, per, 32, 3, dtype=F64).index_add_(1, slot.reshape(-1), both)
    return acc[..., :2].contiguous(), acc[..., [2, 1]].contiguous()


def check_stats_exact(parts, out_ref, layout, tw=None, what=""):
    want, _ = tile_stats(out_ref, layout, tw)
    assert float(want[..., 1].max()) < 2.0 ** 24
    assert parts.numel() == want.numel(), (what, tuple(parts.shape), tuple(want.shape))
    C.check_exact(parts.reshape(want.shape), want, what + " gn_partials")


def check_stats_rounding(parts, got_out, layout, tw=None, what=""):
    """|partial - float64 sum of the kernel's OWN rounded output over the slot's valid pixels| <= STATS_REL * sum|addends| (conv_fwd_common: the chain
    of dependent fp32 additions is no longer for a partly filled tile, which sums fewer rows).  Returns the largest err / bound."""
    want, mag = tile_stats(got_out, layout, tw)
    assert parts.numel() == want.numel(), (what, tuple(parts.shape), tuple(want.shape))
    err = (parts.detach().double().cpu().reshape(want.shape) - want).abs()
    bound = C.STATS_REL * mag
    bad = err > bound
    assert not bool(bad.any()), (f"{what} gn_partials: {int(bad.sum())} / {bad.numel()} entries beyond {C.STATS_REL:.2e} * sum|addends|, first at "
                                 f"(image, slot, group, which) {tuple(bad.nonzero()[0].tolist())}")
    return float((err / bound.clamp_min(1e-300)).max())


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------
S = C.spec
# conv_halo_kernel<.., PARTIAL> (10 x 32 tiles), (n, H, W, Cin, Cout): the real level-0 width with a ragged row AND column tile; one valid column in the
# second tile (two channel tiles, statistics at 10 channels per group); a one-column image; the GroupNorm operand path; two sources; the 9-tap upsample
HALO = [
    S("bf16", 3, 11, 48, 128, 160, extras="btr", tdiv=3),
    S("bf16", 2, 3, 33, 64, 320, extras="b"),
    S("bf16", 2, 13, 1, 64, 160),
    S("bf16", 2, 12, 31, 128, 320, extras="t", gn=1),
    S("bf16", 2, 12, 31, 128, 320, extras="t", gn=2),
    S("bf16", 1, 5, 40, 192, 160, c2=64),
    S("bf16", 2, 12, 44, 64, 160, ups=True, extras="b"),
]
HALO_SC = [S("bf16", 2, 11, 48, 64, 160, extras="b", cs1=64, cs2=64)]
# (n, source H, source W, Cin, Cout) -> fmc_conv3x3_halo_fold_partial_bf16, Cout = 320: with statistics
HALO_FOLD = [(2, 5, 20, 64, 320), (1, 6, 48, 64, 320)]
# conv_halo4_kernel<.., PARTIAL>: (spec, row-block widths, split_k values beyond 1, wide).  Level 3 / mid (five one-block images in an eight-block tile:
# the last tile ragged in blocks and in columns); level 2 at both geometries and split over the reduction; statistics; W = 28 in the wide form and on 4 waves (at tw = 8 the whole-tile comparison pads to 40); W = 7; W = 17 (one
# column past a 16 tile and past two 8 tiles)
HALO4 = [
    (S("bf16", 5, 4, 6, 128, 80, extras="btr"), (8,), (), False),
    (S("bf16", 3, 8, 12, 192, 160, extras="tr", tdiv=3), (8, 16), (2, 3), False),
    (S("bf16", 3, 11, 20, 64, 320), (8, 16), (), False),
    (S("bf16", 2, 7, 28, 64, 160), (16,), (), True),
    (S("bf16", 2, 7, 28, 64, 160), (8, 16), (), False),
    (S("bf16", 9, 5, 7, 64, 80), (8, 16), (), False),
    (S("bf16", 2, 6, 17, 64, 320, extras="b"), (8, 16), (), False),
]
# (n, source H, source W, Cin, Cout) -> fmc_conv3x3_halo4_fold_partial_bf16 at (tw, wide) = (8, 0), (16, 0), (16, 1)
HALO4_FOLD = [(3, 8, 12, 128, 160)]
HALO4_FOLD_GEOMETRIES = [(8, False), (16, False), (16, True)]
HALO4_FOLD_STATS = (2, 7, 12, 64, 320)                                       # Cout = 320: the fold's statistics per (source row block, phase)
# whole-tile shapes through the partial entry points: the existing entry's bits, output and statistics
WHOLE_HALO = [S("bf16", 2, 13, 32, 64, 320, extras="btr", tdiv=2)]
WHOLE_HALO4 = [(S("bf16", 3, 11, 16, 64, 320, extras="btr", tdiv=3), 16), (S("bf16", 5, 6, 8, 128, 320, extras="btr"), 8)]
WHOLE_FOLD = (2, 7, 32, 64, 320)                                             # a source every fold arm takes


def sid(s):
    return "-".join(str(int(v) if isinstance(v, bool) else v) or "none" for v in s[1:]) if isinstance(s, C.Spec) else str(s)


def all_specs():
    """(spec, folded) of every GPU case, for the CPU test of the exact instrument's conditions and the ambiguity cap."""
    out = [(s, False) for s in HALO + HALO_SC + [c[0] for c in HALO4] + WHOLE_HALO + [c[0] for c in WHOLE_HALO4]]
    out += [(C.fold_spec(n, hs, ws, cin, cout, True), True) for n, hs, ws, cin, cout in HALO_FOLD + HALO4_FOLD + [HALO4_FOLD_STATS, WHOLE_FOLD]]
    return out


# ---- the whole-tile comparison: the same data zero-padded in width ---------------------------------------------------------------------------------------
def halo_pad_width(w):
    return cdiv(w, 32) * 32


def halo4_pad_width(w, tw):
    """The narrowest width >= w the whole-tile entry takes AND cuts into row blocks `tw` wide (it picks 16 where W % 16 == 0, else 8): W = 12 at tw = 8
    pads to 24, W = 28 at tw = 8 to 40."""
    wp = cdiv(w, tw) * tw
    while (16 if wp % 16 == 0 else 8) != tw:
        wp += tw
    return wp


def pad_case(s, d, wp, seed=5):
    """The case `(s, d)` at output width `wp >= s.w`: activations (both sources, the shortcut's) zero-padded on the right -- a zero column IS the
    convolution's own padding, so the valid columns keep their values bit for bit -- and the residual padded with arbitrary finite values, which only pad
    outputs see.  GroupNorm mode 0 only: a zero-padded GroupNorm operand is not zero.  Returns (padded spec, padded inputs)."""
    assert not s.gn and not s.s2 and wp >= s.w and (not s.ups or wp % 2 == 0)
    extra = wp - s.w
    src_extra = extra // 2 if s.ups else extra
    zpad = lambda t: None if t is None else F.pad(t, (0, 0, 0, src_extra)).contiguous()
    p = dict(d)
    for k in ("x", "x2"):
        p[k] = zpad(d[k])
    if s.cs1:
        p["xs"], p["xs2"] = zpad(d["xs"]), zpad(d["xs2"])
    if d["res"] is not None:
        g = torch.Generator().manual_seed(seed)
        junk = torch.randint(-3, 4, (s.n, s.h, extra, s.cout), generator=g).to(d["res"].dtype)
        p["res"] = torch.cat([d["res"], junk], 2).contiguous()
    return s._replace(w=wp), p


# ---- plain-torch stand-ins: the launch as documented, and the ways a ragged width can go wrong -----------------------------------------------------------
FAULTS = ("wrap_read", "stats_pad", "store_pad", "floor_tiles", "clamped_residual", "splitk_pad")


def _conv_terms(s, x, d):
    """float64 convolution (+ bias + temb, no residual) of an operand `x [n, hs, ws, cin]` at the case's other inputs -> `[n, h, ws', cout]`."""
    y = F.conv2d(C._resample(s, x), d["w"].double(), None, 1, 1)
    if d["bias"] is not None:
        y = y + d["bias"].double()[None, :, None, None]
    if d["temb"] is not None:
        y = y + d["temb"].double().repeat_interleave(d["tdiv"], 0)[:, :, None, None]
    return y.permute(0, 2, 3, 1)


def standin(s, d, tw, fault=None, splits=1, band=64):
    """One launch on column tiles `tw` wide in plain torch, the output (and the split-K workspace) in `edge_guard_common` arenas as the GPU tests hold
    them -> dict(out_arena, out, parts, ws_arena, ws).  Exact-instrument data only (everything is an integer; the arithmetic is float64).
    `fault` None is the kernel as documented.  The faults, each the absence of one `if constexpr (PARTIAL)` of the kernels:
      wrap_read         a pad column's input is the next word in memory -- the next row's first pixel -- instead of zero;
      stats_pad         the statistics slots sum the pad columns of their tile too;
      store_pad         pad columns are stored: over the next row's first pixels, and past the end of the tensor behind the last row;
      floor_tiles       tiles_x = W / tw: the last, partly filled column tile never runs;
      clamped_residual  the residual of every row of a partly filled tile is the clamped pixel's (the tile's first), valid columns included;
      splitk_pad        the fp32 partials of pad columns are written to the split-K workspace."""
    assert fault in (None,) + FAULTS and not s.ups and not s.gn and not s.cs1 and not s.c2
    n, h, w, cout = s.n, s.h, s.w, s.cout
    wp = cdiv(w, tw) * tw
    x = d["x"].double()
    xpad = F.pad(x, (0, 0, 0, wp - w))
    if fault == "wrap_read":
        flat = torch.cat([x.reshape(-1, s.cin), torch.zeros(wp, s.cin, dtype=F64)])
        for j in range(wp - w):
            idx = (torch.arange(n * h) * w + w + j)
            xpad[:, :, w + j] = flat[idx].reshape(n, h, s.cin)
    chunks = torch.arange(s.cin) // 64 * splits // (s.cin // 64)              # which split a channel's chunk belongs to
    acc = torch.stack([_conv_terms(s._replace(extras=""), xpad * (chunks == k), dict(d, bias=None, temb=None)) for k in range(splits)])   # [splits, n, h, wp, cout]
    side = _conv_terms(s, torch.zeros_like(xpad), d)                          # bias + temb
    res = torch.zeros(n, h, wp, cout, dtype=F64)
    if d["res"] is not None:
        res[:, :, :w] = d["res"].double()
        if fault == "clamped_residual" and w % tw:
            x0 = w // tw * tw
            res[:, :, x0:] = d["res"].double()[:, :, x0:x0 + 1]              # (every row of the tile reads its tile's first pixel)
    full = acc.sum(0) + side + res                                            # [n, h, wp, cout]: the pad columns carry bias and neighbour taps
    cols = w // tw * tw if fault == "floor_tiles" else w
    pix = (torch.arange(n * h)[:, None] * w + torch.arange(wp)[None, :])      # flat pixel a (row, tile column) stores to
    out_arena, out = EG.guarded_output((n * h * w, cout), torch.bfloat16, band, band)
    ws_arena = ws = None
    if splits > 1:
        ws_arena, ws = EG.guarded_output((splits * n * h * w, cout), torch.float32, band, band)
        flat_ws = ws_arena[ws.storage_offset():].view(-1, cout)       # (pixel rows from the view's start on, the band behind it included)
        for k in range(splits):
            rows = acc[k].reshape(n * h, wp, cout)
            ws[k * n * h * w:(k + 1) * n * h * w] = rows[:, :w].reshape(-1, cout).float()
            if fault == "splitk_pad":                                         # (behind the valid ones: over the next row, the next split, the end)
                flat_ws[(k * n * h * w + pix[:, w:]).reshape(-1)] = rows[:, w:].reshape(-1, cout).float()
        full = torch.zeros(n, h, wp, cout, dtype=F64)
        full[:, :, :w] = (ws.double().reshape(splits, n, h, w, cout).sum(0) + side[:, :, :w] + res[:, :, :w])       # the finishing pass, per pixel
    rows = full.reshape(n * h, wp, cout).bfloat16()
    flat_out = out_arena[out.storage_offset():].view(-1, cout)
    flat_out[pix[:, :cols].reshape(-1)] = rows[:, :cols].reshape(-1, cout)
    if fault == "store_pad":                                                  # (behind the valid stores: the next row's first pixels are lost)
        flat_out[pix[:, w:].reshape(-1)] = rows[:, w:].reshape(-1, cout)
    parts = None
    if cout % 64 == 0 and splits == 1:
        layout = "halo" if tw == 32 else "halo4"
        if fault == "stats_pad":
            slot, per = slot_map(layout, h, wp, None if tw == 32 else tw)
            o = rows.double().reshape(n, h * wp, 32, cout // 32)
            both = torch.stack([o.sum(-1), (o * o).sum(-1)], -1)
            parts = torch.zeros(n, per, 32, 2, dtype=F64).index_add_(1, slot.reshape(-1), both).float()
        else:
            parts = tile_stats(rows[:, :w].reshape(n, h, w, cout), layout, None if tw == 32 else tw)[0].float()
    return dict(out_arena=out_arena, out=out, parts=parts, ws_arena=ws_arena, ws=ws)

"""Host side of the partial-tile forms of the fused attention blocks (no GPU).

1. The tile and segment arithmetic (`hip_ops.temporal_tile / temporal_tile_count / xattn_tile / xattn_tile_count`, the Python mirror of
   `tile_row0` / `tile_valid` in csrc/temporal_block.hip) against brute force: every valid row is covered exactly once, no tile holds rows of two
   texts, pad counts are right.
2. The dispatch, on `tests/fake_kernels.py` and recording stand-ins for the two fused wrappers: with `hip_ops.PARTIAL_TILES` off (the default) ragged
   sizes keep the un-fused chain and the whole-tile predicates are what they were; with it on they take the new entry point; a gradient, F != 16, fp32,
   fp8 projections and a pose feature of another shape fall back as before.
3. Wrong stand-ins in plain torch, stored through the same tile plan into the arenas of tests/edge_guard_common.py: each mistake the GPU file
   (tests/test_gpu_partial_tiles.py) is there for is caught by the assertion that is said to catch it -- and the right stand-in passes all of them."""
import pytest
import torch

from tests import edge_guard_common as EG
from tests import fake_kernels


@pytest.fixture()
def K():
    from synfmc_amd import hip_ops
    return hip_ops


# =====================================================================================================================================
# 1. tile and segment arithmetic
# =====================================================================================================================================
@pytest.mark.parametrize("C", [320, 640])
def test_temporal_tiles_cover_every_pixel_once(K, C):
    px = 10 if C == 320 else 5
    for hw in range(1, 401):
        for B in (1, 3):
            n = K.temporal_tile_count(B, hw, C)
            assert n == B * ((hw + px - 1) // px)
            seen = [[0] * hw for _ in range(B)]
            pads = 0
            for t in range(n):
                clip, p0, nv = K.temporal_tile(t, hw, C)
                assert 0 <= clip < B and 1 <= nv <= px and p0 % px == 0 and p0 + nv <= hw
                assert nv == px or p0 + nv == hw                          # only the last tile of a clip is partly filled
                pads += px - nv
                for p in range(p0, p0 + nv):
                    seen[clip][p] += 1
            assert all(c == 1 for row in seen for c in row), (hw, B)
            assert pads == B * (-hw % px)
            if hw % px == 0:                                              # whole tiles: the whole-tile kernel's plan (tile t -> clip t / (hw / px), pixel ...)
                assert all(K.temporal_tile(t, hw, C) == (t // (hw // px), (t % (hw // px)) * px, px) for t in range(n))


@pytest.mark.parametrize("C", [320, 640])
def test_xattn_tiles_cover_every_row_once_and_never_span_two_texts(K, C):
    T = 160 if C == 320 else 80
    for seg in range(1, 701):
        B = 3
        n = B * ((seg + T - 1) // T)
        seen = [0] * (B * seg)
        pads = 0
        for t in range(n):
            text, r0, nv = K.xattn_tile(t, seg, C)
            assert 0 <= text < B and 1 <= nv <= T
            assert text * seg <= r0 and r0 + nv <= (text + 1) * seg       # every valid row of the tile belongs to `text`
            assert (r0 - text * seg) % T == 0
            pads += T - nv
            for r in range(r0, r0 + nv):
                seen[r] += 1
        assert all(c == 1 for c in seen), seg
        assert pads == B * (-seg % T)
    # the count the wrappers log = the grid: images / images_per_text segments of images_per_text * hw rows
    for n_images, ipt, hw in ((32, 16, 1536), (32, 16, 384), (6, 3, 100), (6, 2, 161), (2, 1, 24)):
        seg = ipt * hw
        assert K.xattn_tile_count(n_images, hw, ipt, C) == (n_images // ipt) * ((seg + T - 1) // T)
    # whole tiles: the whole-tile kernel's plan, tile t = rows [T t, T t + T)
    assert all(K.xattn_tile(t, 4 * T, C) == (t // 4, t * T, T) for t in range(12))


# =====================================================================================================================================
# 2. dispatch
# =====================================================================================================================================
class _Recorder:
    """Stand-in for a fused wrapper: records the call, returns the residual stream unchanged (+ zero statistics when asked)."""

    def __init__(self):
        self.calls = []

    def __call__(self, h, *a, **k):
        self.calls.append(bool(k.get("partial_tiles")))
        if k.get("stats_eps") is not None:
            return h.clone(), torch.zeros(h.numel() // h.shape[-1], 2)
        return h.clone()


def _temporal_block(C, pose_proc=False):
    from synfmc_amd.models import motion_module as MM
    from synfmc_amd.models.attention_processor import AttnProcessor, PoseAdaptorAttnProcessor
    torch.manual_seed(0)
    blk = MM.TemporalTransformerBlock(dim=C, num_attention_heads=8, attention_head_dim=C // 8, attention_block_types=("Temporal_Self", "Temporal_Self"),
                                      temporal_position_encoding=True, temporal_position_encoding_max_len=32)
    blk.attention_blocks[0].set_processor(PoseAdaptorAttnProcessor(hidden_size=C, pose_feature_dim=C, query_condition=True, key_value_condition=True, scale=0.8)
                                          if pose_proc else AttnProcessor())
    blk.attention_blocks[1].set_processor(AttnProcessor())
    return blk.eval().requires_grad_(False)


@pytest.mark.parametrize("C,P", [(320, 39), (640, 34)])
def test_temporal_dispatch_switch(monkeypatch, K, C, P):
    from synfmc_amd.models import motion_module as MM
    fake_kernels.install(monkeypatch)
    monkeypatch.setattr(K, "_on_gpu", lambda t: True)                      # (every OTHER condition of the new predicates on CPU tensors)
    rec = _Recorder()
    monkeypatch.setattr(K, "temporal_block", rec)
    blk = _temporal_block(C).to(torch.bfloat16)
    x = torch.randn(2, 16, P, C).to(torch.bfloat16)
    assert K.PARTIAL_TILES is False                                        # default off
    with torch.no_grad():
        # the whole-tile predicates are what they were: a CPU tensor, a ragged P
        assert not K.temporal_block_supported(x, 8) and not blk.fused_blocks_ok(x, None, {})
        assert K.temporal_block_partial_supported(x, 8) and blk.fused_blocks_partial_ok(x, None, {})
        off = blk(x)                                                       # default off: the un-fused chain
        assert rec.calls == [] and off.shape == x.shape
        monkeypatch.setattr(K, "PARTIAL_TILES", True)
        on = blk(x)
        assert rec.calls == [True, True] and on.shape == x.shape           # both attention blocks, through the partial entry point
        rec.calls.clear()
        # fall-backs, switch on
        assert not blk.fused_blocks_partial_ok(x[:, :15].contiguous(), None, {})                       # F != 16
        assert not blk.fused_blocks_partial_ok(x.float(), None, {})                                    # fp32
        assert not blk.fused_blocks_partial_ok(x, torch.ones(1), {})                                   # a mask
        assert not K.temporal_block_partial_supported(x.transpose(1, 2), 8)                            # not contiguous
        assert not K.temporal_block_partial_supported(x, 4)                                            # heads
        blk.attention_blocks[1].__dict__["_fp8_scales"] = object()                                     # fp8 projections
        assert not blk.fused_blocks_partial_ok(x, None, {})
        del blk.attention_blocks[1].__dict__["_fp8_scales"]
        assert blk.fused_blocks_partial_ok(x, None, {})
        monkeypatch.setattr(MM, "TEMPORAL_FUSED", False)
        assert not blk.fused_blocks_partial_ok(x, None, {})
        monkeypatch.setattr(MM, "TEMPORAL_FUSED", True)
    with torch.enable_grad():                                              # a gradient: the predicate refuses, and `forward` does not ask it
        assert not K.temporal_block_partial_supported(x, 8)
        blk(x)
        assert rec.calls == []


def test_temporal_dispatch_pose_feature_of_another_shape_falls_back(monkeypatch, K):
    fake_kernels.install(monkeypatch)
    monkeypatch.setattr(K, "_on_gpu", lambda t: True)
    monkeypatch.setattr(K, "PARTIAL_TILES", True)
    C, P = 320, 39
    blk = _temporal_block(C, pose_proc=True).to(torch.bfloat16)
    x = torch.randn(2, 16, P, C).to(torch.bfloat16)
    with torch.no_grad():
        assert blk.fused_blocks_partial_ok(x, None, {"pose_feature": torch.randn(2, 16, P, C).to(torch.bfloat16)})
        assert blk.fused_blocks_partial_ok(x, None, {"pose_feature": torch.randn(2, C, 16, 3, 13).to(torch.bfloat16)})     # [b, c, f, h, w], h w = P
        assert not blk.fused_blocks_partial_ok(x, None, {"pose_feature": torch.randn(2, 16, P + 1, C).to(torch.bfloat16)})
        assert not blk.fused_blocks_partial_ok(x, None, {"pose_feature": torch.randn(2, C, 16, 3, 12).to(torch.bfloat16)})
        assert not blk.fused_blocks_partial_ok(x, None, {"pose_feature": torch.randn(2, 16, P, C)})                        # fp32 pose feature
        assert not blk.fused_blocks_partial_ok(x, None, {})                                                                # none at all
        assert not blk.fused_blocks_ok(x, None, {"pose_feature": torch.randn(2, 16, P, C).to(torch.bfloat16)})             # whole tiles: P is ragged


@pytest.mark.parametrize("C,hw", [(320, 39), (640, 34)])
def test_xattn_dispatch_switch(monkeypatch, K, C, hw):
    from synfmc_amd.models import layers as L
    fake_kernels.install(monkeypatch)
    monkeypatch.setattr(K, "_on_gpu", lambda t: True)
    rec = _Recorder()
    monkeypatch.setattr(K, "xattn_block", rec)
    monkeypatch.setattr(K, "xattn_pack_kv", lambda kv: torch.zeros(1, dtype=kv.dtype))
    torch.manual_seed(0)
    blk = L.BasicTransformerBlock(C, 8, C // 8, cross_attention_dim=64).eval().requires_grad_(False).to(torch.bfloat16)
    x = torch.randn(6, hw, C).to(torch.bfloat16)
    text = torch.randn(2, 7, 64).to(torch.bfloat16)
    assert K.PARTIAL_TILES is False
    with torch.no_grad():
        assert not K.xattn_block_supported(x, 7, 8) and K.xattn_block_partial_supported(x, 7, 8)
        blk(x, encoder_hidden_states=text)
        assert rec.calls == []                                             # default off: the un-fused chain
        monkeypatch.setattr(K, "PARTIAL_TILES", True)
        blk(x, encoder_hidden_states=text)
        assert rec.calls == [True]
        rec.calls.clear()
        assert not K.xattn_block_partial_supported(x, 81, 8) and not K.xattn_block_partial_supported(x.float(), 7, 8)
        assert not K.xattn_block_partial_supported(x, 7, 4)
        with pytest.raises(NotImplementedError):                           # a text mask never reaches the fused block (the un-fused chain refuses it)
            blk(x, encoder_hidden_states=text, encoder_attention_mask=torch.zeros(2, 7))
        assert rec.calls == []
    with torch.enable_grad():
        blk(x, encoder_hidden_states=text)
        assert rec.calls == []


# =====================================================================================================================================
# 3. what the GPU file's assertions catch: stand-ins in plain torch, stored through the tile plan with raw addresses
# =====================================================================================================================================
CW = 4                                   # channels of the stand-ins (the plan does not depend on them)
BAND = 40                                # rows of guard each side: more than one tile of any form reaches


def _ints(shape, seed):
    """Small integers as fp32: sums over any slice are exact, so `torch.equal` compares the plan and not a reduction order."""
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(seed)).float()


def _temporal_result(h):
    """What the block stands for here: a row's result depends on the 16 frames of its own pixel."""
    return h * 2.0 + h.sum(dim=1, keepdim=True)


def _row_stats(v):
    """Stand-in for (mean, rstd) of the output rows: two exact row reductions."""
    return torch.stack([v.sum(-1), v.max(-1).values], -1)


def _temporal_standin(K, h, C, g, bug=None):
    """`[B, 16, hw, CW]` tokens through the tile plan of the temporal form.  Stores go to raw addresses of the flat arenas, as the kernel's do."""
    B, Fr, hw, _ = h.shape
    px = 10 if C == 320 else 5
    out, st = g.out((B * Fr * hw, CW), torch.float32, BAND, 0, "out"), g.out((B * Fr * hw, 2), torch.float32, BAND, 0, "ln_stats")
    (_, a_out, _, _), (_, a_st, _, _) = g.outputs
    o0, s0 = (out.data_ptr() - a_out.data_ptr()) // 4, (st.data_ptr() - a_st.data_ptr()) // 4
    for t in range(K.temporal_tile_count(B, hw, C)):
        clip, p0, nv = K.temporal_tile(t, hw, C)
        if bug == "drop_last_partial" and nv < px:
            continue
        for j in range(px):
            src_clip, src_p = clip, p0 + min(j, nv - 1)                   # the clamp: a pad pixel reads the tile's last valid one
            if bug == "valid_from_wrong_clip" and nv < px:                # a pad clamp applied to the valid rows as well, in the wrong clip
                src_clip, src_p = (clip + 1) % B, p0 + nv - 1
            val = _temporal_result(h[src_clip:src_clip + 1, :, src_p:src_p + 1])[0, :, 0]             # [16, CW]
            if j >= nv and bug not in ("store_pad", "stats_pad"):
                continue
            for f in range(Fr):
                row = (clip * Fr + f) * hw + p0 + j                       # raw address: a pad pixel of frame f IS pixel p0 + j - hw of frame f + 1
                if j < nv or bug == "store_pad":
                    a_out[o0 + row * CW:o0 + (row + 1) * CW] = val[f]
                if j < nv or bug == "stats_pad":
                    a_st[s0 + row * 2:s0 + row * 2 + 2] = _row_stats(val[f])
    return out, st


def _temporal_check(K, B, hw, C, bug):
    h = _ints((B, 16, hw, CW), 1)
    ref = _temporal_result(h).reshape(-1, CW)
    ref_st = _row_stats(ref)
    g = EG.Guard("zeros")
    out, st = _temporal_standin(K, h, C, g, bug)
    return {"out_equal": torch.equal(out, ref), "stats_equal": torch.equal(st, ref_st), "guard": g}


@pytest.mark.parametrize("C,B,hw", [(320, 1, 1), (320, 2, 11), (320, 3, 19), (640, 2, 6), (640, 3, 9)])
def test_right_temporal_standin_passes(K, C, B, hw):
    r = _temporal_check(K, B, hw, C, None)
    assert r["out_equal"] and r["stats_equal"]
    r["guard"].check("right stand-in")


def test_pad_rows_stored_into_the_next_frame_show_in_the_comparison_and_past_the_end_in_the_sentinels(K):
    r = _temporal_check(K, 2, 11, 320, "store_pad")
    assert not r["out_equal"]                                             # (frame f + 1, pixels 0..8) overwritten: assertions 1 / 2
    with pytest.raises(EG.OutsideTouched):                                # the last frame of the last clip: past the end, assertion 4 only
        r["guard"].check("store_pad")


def test_statistics_written_for_pad_rows_are_caught(K):
    r = _temporal_check(K, 2, 11, 320, "stats_pad")
    assert r["out_equal"] and not r["stats_equal"]
    with pytest.raises(EG.OutsideTouched):
        r["guard"].check("stats_pad")


def test_dropped_last_partial_tile_is_caught(K):
    r = _temporal_check(K, 2, 11, 320, "drop_last_partial")
    assert not r["out_equal"]
    with pytest.raises(EG.InsideUnwritten):
        r["guard"].check("drop_last_partial")


def test_pad_rows_from_the_wrong_clip_stored_as_valid_are_caught(K):
    r = _temporal_check(K, 2, 11, 320, "valid_from_wrong_clip")
    assert not r["out_equal"]                                             # every word written, nothing outside: only the comparison sees it
    r["guard"].check("valid_from_wrong_clip")


def _xattn_standin(K, h, text_vals, ipt, C, g, bug=None):
    """`[N, hw, CW]` tokens, a value per text: a row's result depends on the row and on ITS text."""
    N, hw, _ = h.shape
    T, seg, rows = (160 if C == 320 else 80), ipt * hw, N * hw
    out = g.out((rows, CW), torch.float32, 2 * T, 0, "out")
    _, a_out, _, _ = g.outputs[-1]
    o0 = (out.data_ptr() - a_out.data_ptr()) // 4
    flat = h.reshape(rows, CW)
    for t in range(K.xattn_tile_count(N, hw, ipt, C)):
        text, r0, nv = K.xattn_tile(t, seg, C)
        if bug == "neighbour_text":                                       # the whole-tile kernel's index: tile * ROWS / hw / images_per_text
            text = (t * T // hw) // ipt
        for j in range(T):
            if j >= nv and bug != "store_pad":
                continue
            val = flat[r0 + min(j, nv - 1)] * 2.0 + (text_vals[text] if text < len(text_vals) else 999.0)   # (past the last text: whatever lies there)
            a_out[o0 + (r0 + j) * CW:o0 + (r0 + j + 1) * CW] = val
    return out


def _xattn_check(K, B, ipt, hw, C, bug):
    h = _ints((B * ipt, hw, CW), 3)
    text_vals = torch.arange(1, B + 1, dtype=torch.float32) * 10.0
    ref = h.reshape(B, ipt * hw, CW) * 2.0 + text_vals[:, None, None]
    g = EG.Guard("zeros")
    out = _xattn_standin(K, h, text_vals, ipt, C, g, bug)
    return torch.equal(out, ref.reshape(-1, CW)), g


@pytest.mark.parametrize("C,B,ipt,hw", [(320, 2, 1, 24), (320, 2, 3, 100), (320, 3, 2, 161), (640, 2, 3, 50), (640, 3, 2, 81)])
def test_right_xattn_standin_passes_and_the_neighbouring_text_is_caught(K, C, B, ipt, hw):
    ok, g = _xattn_check(K, B, ipt, hw, C, None)
    assert ok
    g.check("right stand-in")
    T, seg = (160 if C == 320 else 80), ipt * hw
    differs = any((t * T // hw) // ipt != K.xattn_tile(t, seg, C)[0] for t in range(K.xattn_tile_count(B * ipt, hw, ipt, C)))
    assert differs or (C, B, ipt, hw) in ((320, 2, 3, 100), (640, 2, 3, 50))   # (at these two sizes the whole-tile index happens to be right)
    ok, g = _xattn_check(K, B, ipt, hw, C, "neighbour_text")
    assert ok == (not differs)                                            # texts differ per batch entry: the comparison sees every wrong one
    g.check("neighbour_text")


def test_xattn_pad_rows_stored_are_only_seen_by_the_sentinels(K):
    """In row order a stored pad row of text b lands on the first rows of text b + 1, which that text's own tile writes afterwards: the comparison
    passes.  The pad rows of the LAST text land past the end -- why assertion 4 stands next to assertions 1 and 2."""
    ok, g = _xattn_check(K, 2, 3, 100, 320, "store_pad")
    assert ok
    with pytest.raises(EG.OutsideTouched):
        g.check("store_pad")

"""Host side of the feed-forward chain with a partly filled last tile (no GPU).

1. The tile arithmetic (`hip_ops.ff_tile_count`, `ff_blocked_numel`; the layout and last-tile helpers of tests/ff_partial_common.py) against brute force,
   and the restatement of the persistent GEMM's tile order kept in tests/ff_partial_common.py (`g160p_tile_of` = `tile_of` + `lin_to_tile` of
   csrc/gemm_conv.hip) as a permutation with the XCD ranges it promises.
2. Case selection: from that restatement, the three tile totals of tests/test_gpu_ff_partial.py put the ragged tile where the GPU file says --
   a workgroup's only tile, a tile beside a workgroup that runs a second one, a workgroup's second tile (behind an epilogue: the `after_epi` wait);
   and the wide shape (N = 2560) puts a ragged tile at the head of a workgroup that runs another tile behind it.
3. Dispatch of `FeedForward.forward_ln` and of the two row-statistics decisions, on recording stand-ins: switch off = the old calls, switch on = the
   new ones, whole-tile sizes never reach the new entry points.
4. Wrong stand-ins in plain torch, run through the assertions of tests/ff_partial_common.py (the ones the GPU file uses): pad rows stored, a residual
   row read past M, the last valid row dropped, a pad row's value landing in a valid row, a tile-major range computed from M / 160 instead of the
   ceiling -- each is caught by the assertion said to catch it, and the right stand-in passes all of them."""
import pytest
import torch

from tests import edge_guard_common as EG
from tests import fake_kernels
from tests import ff_partial_common as FFC
from tests.fused_host_surface_common import claims_gpu


@pytest.fixture()
def K():
    from synfmc_amd import hip_ops
    return hip_ops


# =====================================================================================================================================
# 1. tile arithmetic
# =====================================================================================================================================
@pytest.mark.parametrize("rows", [80, 160])
def test_tile_count_and_last_tile_rows_against_brute_force(K, rows):
    for M in range(1, 1000):
        seen = {}
        for m in range(M):
            seen.setdefault(m // rows, []).append(m)
        assert K.ff_tile_count(M, rows) == len(seen) == FFC.tiles(M, rows)
        assert FFC.last_tile_rows(M, rows) == len(seen[max(seen)])
        assert all(len(v) == rows for t, v in seen.items() if t != max(seen))      # exactly one tile is ragged: M is one flat row count


@pytest.mark.parametrize("M,Kd", [(1, 32), (159, 64), (160, 64), (161, 32), (417, 96), (800, 128)])
def test_tile_major_size_and_offsets_against_the_layout(K, M, Kd):
    idx = FFC.blocked_index(M, Kd)
    assert K.ff_blocked_numel(M, Kd) == FFC.tiles(M) * 160 * Kd
    assert int(idx.max()) < K.ff_blocked_numel(M, Kd) and idx.unique().numel() == M * Kd
    # the layout is the whole-tile kernels': [M / 160][K / 32][160][32] of the padded rows
    Mp = FFC.tiles(M) * 160
    x = torch.arange(Mp * Kd, dtype=torch.float32).view(Mp, Kd)
    blk = x.view(Mp // 160, 160, Kd // 32, 32).permute(0, 2, 1, 3).contiguous().view(-1)
    assert torch.equal(blk[idx.reshape(-1)].view(M, Kd), x[:M])
    assert torch.equal(FFC.from_blocked(FFC.to_blocked(x[:M], -1.0), M, Kd), x[:M])
    assert int((FFC.to_blocked(x[:M], -1.0) == -1.0).sum()) == (Mp - M) * Kd


@pytest.mark.parametrize("tiles_m,tiles_n,gm", [(8, 1, 1), (257, 1, 1), (264, 1, 1), (77, 2, 1), (77, 2, 4), (308, 4, 6), (13, 3, 5)])
def test_persistent_tile_order_is_a_permutation_with_contiguous_xcd_ranges(K, tiles_m, tiles_n, gm):
    total = tiles_m * tiles_n
    order = [FFC.g160p_tile_of(i, tiles_m, tiles_n, gm) for i in range(total)]
    assert sorted(order) == [(m, n) for m in range(tiles_m) for n in range(tiles_n)]
    # linear order (lin_to_tile): groups of gm m-tiles, n-outer / m-inner inside a group
    lin = []
    for first in range(0, tiles_m, gm):
        g = min(gm, tiles_m - first)
        lin += [(first + i, n) for n in range(tiles_n) for i in range(g)]
    pos = {t: i for i, t in enumerate(lin)}
    q, r = divmod(total, 8)
    start = 0
    for x in range(8):                                    # XCD x = ids x, x + 8, ...: a contiguous range of the linear order, in order
        mine = [pos[order[i]] for i in range(x, total, 8)]
        n = q + (1 if x < r else 0)
        assert mine == list(range(start, start + n))
        start += n


def test_group_m_restatement():
    # (xcd_group_m: 1 while the weight fits 2.5 MiB; else round(sqrt(2 c)), c = min(32, tiles / 8), kept only if it beats row-major's n-span)
    assert FFC.g160p_group_m(308, 1, 320, 1280) == 1        # 800 KiB weight
    assert FFC.g160p_group_m(264, 1, 320, 128) == 1
    assert FFC.g160p_group_m(512, 8, 2560, 640) == 8        # c = 32: round(sqrt(64)) = 8, 16 > 12
    assert FFC.g160p_group_m(512, 4, 1280, 1280) == 1       # 8 > 12 fails: row-major


# =====================================================================================================================================
# 2. case selection of the GPU file
# =====================================================================================================================================
@pytest.mark.parametrize("cus", [8, 64, 104, 256, 304])
def test_the_three_tile_totals_put_the_ragged_tile_where_the_gpu_file_says(K, cus):
    assert FFC.GEMM_EXTRA_TILES == (0, 1, 8)
    # N = 320, K = 128 | 192: one n-tile, a weight far below 2.5 MiB -> group_m = 1
    assert FFC.g160p_group_m(cus, 1, 320, 128) == 1 and FFC.g160p_group_m(cus + 8, 1, 320, 192) == 1
    wg, at, n, most = FFC.placement(cus, cus)
    assert (at, n, most) == (0, 1, 1)                                     # a workgroup's only tile; nobody runs a second one
    wg, at, n, most = FFC.placement(cus + 1, cus)
    assert (at, n, most) == (0, 1, 2)                                     # still an only tile, beside a workgroup that runs a second one
    wg, at, n, most = FFC.placement(cus + 8, cus)
    assert (at, n, most) == (1, 2, 2)                                     # a workgroup's second tile: requested under, and run behind, an epilogue


@pytest.mark.parametrize("cus", [104, 256, 304])
def test_the_wide_shape_puts_a_ragged_tile_first_in_a_workgroup_with_a_second_tile(cus):
    """With one column tile the last row tile is always the LAST tile of its workgroup (the end of XCD 7's range).  A grouped order over 8 column tiles
    moves it: at N = 2560, K = 640 one tile of the ragged row tile opens a workgroup that then runs another tile."""
    assert all(FFC.placement(cus + e, cus)[1] + 1 == FFC.placement(cus + e, cus)[2] for e in FFC.GEMM_EXTRA_TILES)
    tiles_m = FFC.wide_tiles_m(cus)
    assert tiles_m is not None and tiles_m * 8 >= cus
    gm = FFC.g160p_group_m(tiles_m, 8, FFC.WIDE_N, FFC.WIDE_K)
    assert gm > 1
    where = FFC.ragged_placements(tiles_m, 8, gm, cus)
    assert [tn for tn, *_ in where] == list(range(8))
    assert any(at == 0 and n == 2 for _, _, at, n in where)
    if cus == 256:
        assert tiles_m == 37 and gm == 8 and where[0] == (0, 15, 0, 2) and where[7] == (7, 39, 1, 2)


def test_remainder_tables_reach_every_edge():
    for rem in FFC.PIPE80_REMAINDERS:
        assert 1 <= rem < 80
    assert {r % 16 for r in FFC.PIPE80_REMAINDERS} >= {15, 0, 1}            # around the 16-row MFMA block
    assert {79, 80, 81} <= set(FFC.PIPE160_REMAINDERS) and {79, 80, 81} <= set(FFC.GEMM_REMAINDERS)   # around the 80-row wave row / epilogue pass
    assert any(r <= 80 for r in FFC.GEMM_REMAINDERS) and any(r > 80 for r in FFC.GEMM_REMAINDERS)     # a dead second pass, and a ragged one
    assert [c // 128 for c in FFC.PIPE_CFF] == [1, 2, 3]


# =====================================================================================================================================
# 3. dispatch
# =====================================================================================================================================
class _Calls:
    def __init__(self, monkeypatch, K, cus):
        self.log = []
        monkeypatch.setattr(K, "_on_gpu", lambda t: True)                  # (every OTHER condition of the predicates on CPU tensors)
        monkeypatch.setattr(K, "_ff_on_gpu", lambda t: True)
        monkeypatch.setattr(K, "_cus", lambda device: cus)

        monkeypatch.setattr(K, "geglu_ln_direct_ok", claims_gpu(K.geglu_ln_direct_ok))   # (the whole-tile predicate asks the tensor, not a hook)

        def pipe(h, g, b, eps, frag, bias, cff, blocked=False, variant=0, partial_tiles=False):
            self.log.append(("geglu_ln_pipe", partial_tiles, blocked, variant))
            return torch.zeros(*h.shape[:-1], cff, dtype=h.dtype)

        def direct(h, g, b, eps, frag, bias, cff, blocked=False):
            self.log.append(("geglu_ln_direct", False, blocked, None))
            return torch.zeros(*h.shape[:-1], cff, dtype=h.dtype)

        def from_blocked(xb, w, bias, residual, alpha=1.0, out=None, partial_tiles=False):
            self.log.append(("linear_from_blocked", partial_tiles))
            return torch.zeros(*xb.shape[:-1], w.shape[0], dtype=xb.dtype)

        def tail(mid, h, wc, bc, res, gn_hw=0, partial_tiles=False):
            self.log.append(("ff_tail", partial_tiles))
            return torch.zeros_like(res)
        for name, fn in (("geglu_ln_pipe", pipe), ("geglu_ln_direct", direct), ("linear_from_blocked", from_blocked), ("ff_tail", tail)):
            monkeypatch.setattr(K, name, fn)

    def take(self):
        log, self.log = self.log, []
        return log


def _ff(C):
    from synfmc_amd.models import layers as L
    torch.manual_seed(0)
    ff = L.FeedForward(C).eval().requires_grad_(False).to(torch.bfloat16)
    norm = L.LayerNorm(C).eval().requires_grad_(False).to(torch.bfloat16)
    return ff, norm


def test_forward_ln_dispatch_at_c320(monkeypatch, K):
    fake_kernels.install(monkeypatch)
    calls = _Calls(monkeypatch, K, cus=8)
    ff, norm = _ff(320)
    M = 1504                                                               # 9.4 tiles: 10 > 8 "CUs", M % 80 == 64
    h = torch.randn(M, 320).to(torch.bfloat16)
    x = torch.randn(M, 320).to(torch.bfloat16)
    wp, bp = torch.randn(320, 320).to(torch.bfloat16), torch.randn(320).to(torch.bfloat16)
    assert K.PARTIAL_TILES is False
    with torch.no_grad():
        assert not K.geglu_ln_direct_ok(h, ff.net[0].proj.weight) and K.geglu_ln_partial_ok(h, ff.net[0].proj.weight)
        assert ff.forward_ln(h, norm, h, tail=(wp, bp, x, 0)) is None and calls.take() == []          # switch off: as before, the caller's un-fused chain
        monkeypatch.setattr(K, "PARTIAL_TILES", True)
        y = ff.forward_ln(h, norm, h, tail=(wp, bp, x, 0))
        assert calls.take() == [("geglu_ln_pipe", True, True, 1), ("ff_tail", True)] and y._fmc_tail and y.shape == x.shape
        y = ff.forward_ln(h, norm, h)                                        # no tail: row-major intermediate, the ordinary output projection
        assert calls.take() == [("geglu_ln_pipe", True, False, 1)] and y.shape == h.shape and K.geglu_direct_blocked_partial_ok(h, ff.net[2].weight, h)
        r = torch.randn(M, 320).to(torch.bfloat16)                           # residual is not h: no folded tail
        ff.forward_ln(h, norm, r, tail=(wp, bp, x, 0))
        assert calls.take() == [("geglu_ln_pipe", True, False, 1)]           # (`linear_from_blocked(partial_tiles=True)` is not routed to: measured slower)
        monkeypatch.setattr(K, "_cus", lambda device: 16)                   # fewer tiles than CUs: the same
        y = ff.forward_ln(h, norm, h, tail=(wp, bp, x, 0))
        assert calls.take() == [("geglu_ln_pipe", True, False, 1)] and y.shape == h.shape and getattr(y, "_fmc_tail", None) is None
        monkeypatch.setattr(K, "_cus", lambda device: 8)
        # a pending LayerNorm / statistics on h: somebody else normalises, as before
        h2 = h.clone()
        h2._fmc_ln = (torch.zeros(M, 2), None, True)
        assert ff.forward_ln(h2, norm, h2) is None and calls.take() == []
        # whole-tile sizes never reach the new entry points, switch on
        for Mw in (1600, 1520):                                              # % 160 == 0; % 80 == 0 only
            hw_ = torch.randn(Mw, 320).to(torch.bfloat16)
            assert K.geglu_ln_direct_ok(hw_, ff.net[0].proj.weight) and not ff.ln_partial_route(hw_)
            ff.forward_ln(hw_, norm, hw_)
            log = calls.take()
            assert log and all(c[1] is False for c in log), log
        monkeypatch.setattr(K, "GEGLU_DIRECT_320", False)                    # the level's A/B switch off: neither route
        assert not K.geglu_ln_partial_ok(h, ff.net[0].proj.weight) and ff.forward_ln(h, norm, h) is None and calls.take() == []
        monkeypatch.setattr(K, "GEGLU_DIRECT_320", True)
    with torch.enable_grad():                                              # a gradient: neither route
        assert not ff.ln_partial_route(h) and ff.forward_ln(h, norm, h) is None and calls.take() == []


def test_forward_ln_dispatch_at_c640(monkeypatch, K):
    fake_kernels.install(monkeypatch)
    calls = _Calls(monkeypatch, K, cus=8)
    ff, norm = _ff(640)
    h = torch.randn(1504, 640).to(torch.bfloat16)
    with torch.no_grad():
        assert ff.forward_ln(h, norm, h) is None and calls.take() == []
        monkeypatch.setattr(K, "PARTIAL_TILES", True)
        assert K.geglu_ln_partial_ok(h, ff.net[0].proj.weight) and not K.GEGLU_PIPE_640
        assert ff.forward_ln(h, norm, h) is None and calls.take() == []      # the wrapper takes it, the model does not route to it by default (measured level)
        monkeypatch.setattr(K, "GEGLU_PIPE_640", True)
        y = ff.forward_ln(h, norm, h)                                        # the pipe kernel's 80-row form, row-major, then the ordinary projection
        assert calls.take() == [("geglu_ln_pipe", True, False, 0)] and y.shape == h.shape
        assert not K.geglu_direct_blocked_partial_ok(h, ff.net[2].weight, h)
        hw_ = torch.randn(1520, 640).to(torch.bfloat16)
        ff.forward_ln(hw_, norm, hw_)
        assert all(c[1] is False for c in calls.take())


def test_partial_predicates_follow_the_whole_tile_ones(monkeypatch, K):
    monkeypatch.setattr(K, "_ff_on_gpu", lambda t: True)
    monkeypatch.setattr(K, "_cus", lambda device: 8)
    w1, w2, wp = torch.zeros(2560, 320).bfloat16(), torch.zeros(320, 1280).bfloat16(), torch.zeros(320, 320).bfloat16()
    with torch.no_grad():
        for M in (1, 79, 1281, 1504):
            h = torch.zeros(M, 320).bfloat16()
            assert K.geglu_ln_partial_ok(h, w1) and not K.geglu_ln_direct_ok(h, w1)
            assert K.geglu_direct_blocked_partial_ok(h, w2, h) == (FFC.tiles(M) > 8)
            assert K.ff_tail_partial_ok(h, w2, wp, torch.zeros(M, 320).bfloat16()) == (FFC.tiles(M) >= 8)
            assert not K.geglu_direct_blocked_ok(h, w2, h)
        h = torch.zeros(1504, 320).bfloat16()
        assert not K.geglu_ln_partial_ok(h.float(), w1) and not K.geglu_ln_partial_ok(h, w1.float()) and not K.geglu_ln_partial_ok(h.t(), w1)
        assert not K.geglu_ln_partial_ok(torch.zeros(1504, 256).bfloat16(), torch.zeros(2048, 256).bfloat16())       # C
        assert not K.geglu_ln_partial_ok(h, torch.zeros(2 * 1000, 320).bfloat16())                                  # cff % 128
        assert not K.ff_tail_partial_ok(h, w2, wp, None) and not K.ff_tail_partial_ok(h, w2, wp, torch.zeros(1503, 320).bfloat16())
        assert K.geglu_pipe_partial_supported(1, 128, 320, 1) and K.geglu_pipe_partial_supported(1, 128, 640, 0)
        assert not K.geglu_pipe_partial_supported(1, 128, 640, 1) and not K.geglu_pipe_partial_supported(0, 128, 320, 0)
        assert not K.geglu_pipe_partial_supported(1 << 20, 1280, 320, 1)                                            # the padded intermediate: 2 GiB
    with torch.enable_grad():
        assert not K.geglu_ln_partial_ok(torch.zeros(1504, 320).bfloat16(), w1)


class _Block:
    """Stand-in for a fused attention wrapper: records (partial_tiles, statistics asked for)."""

    def __init__(self):
        self.calls = []

    def __call__(self, h, *a, **k):
        self.calls.append((bool(k.get("partial_tiles")), k.get("stats_eps") is not None))
        if k.get("stats_eps") is not None:
            return h.clone(), torch.zeros(h.numel() // h.shape[-1], 2)
        return h.clone()


def test_temporal_statistics_decision(monkeypatch, K):
    from tests.test_partial_tiles_host import _temporal_block
    fake_kernels.install(monkeypatch)
    calls = _Calls(monkeypatch, K, cus=8)
    rec = _Block()
    monkeypatch.setattr(K, "temporal_block", rec)
    blk = _temporal_block(320).to(torch.bfloat16)
    x = torch.randn(2, 16, 47, 320).to(torch.bfloat16)                     # 1504 rows
    with torch.no_grad():
        off = blk(x)
        assert rec.calls == [] and calls.take() == [] and off.shape == x.shape                        # switch off: the un-fused chain
        monkeypatch.setattr(K, "PARTIAL_TILES", True)
        on = blk(x)
        assert rec.calls == [(True, False), (True, False)] and on.shape == x.shape                  # no statistics: the feed-forward normalises itself ...
        assert calls.take() == [("geglu_ln_pipe", True, False, 1)]                                    # ... on the new entry point
        rec.calls.clear()
        # were the consuming GEMM able to take statistics at this size, the feed-forward's own route still decides
        monkeypatch.setattr(K, "lnc_ok", lambda x, w: True)
        blk(x)
        assert rec.calls == [(True, False), (True, False)] and calls.take()[0][:2] == ("geglu_ln_pipe", True)
        rec.calls.clear()
        monkeypatch.setattr(K, "GEGLU_PIPE", False)                          # no partial route: the statistics are asked for, as before
        monkeypatch.setattr(K, "resolve_pending_ln", lambda t: t)            # (the recorder's zero statistics are not applied)
        blk(x)
        assert rec.calls == [(True, False), (True, True)] and all(c[1] is False for c in calls.take())


def test_xattn_statistics_decision(monkeypatch, K):
    from synfmc_amd.models import layers as L
    fake_kernels.install(monkeypatch)
    calls = _Calls(monkeypatch, K, cus=8)
    rec = _Block()
    monkeypatch.setattr(K, "xattn_block", rec)
    monkeypatch.setattr(K, "xattn_pack_kv", lambda kv: torch.zeros(1, dtype=kv.dtype))
    torch.manual_seed(0)
    blk = L.BasicTransformerBlock(320, 8, 40, cross_attention_dim=64).eval().requires_grad_(False).to(torch.bfloat16)
    x = torch.randn(32, 47, 320).to(torch.bfloat16)                        # 1504 rows
    text = torch.randn(2, 7, 64).to(torch.bfloat16)
    with torch.no_grad():
        blk(x, encoder_hidden_states=text)
        assert rec.calls == [] and calls.take() == []
        monkeypatch.setattr(K, "PARTIAL_TILES", True)
        y = blk(x, encoder_hidden_states=text)
        assert rec.calls == [(True, False)] and y.shape == x.shape
        assert calls.take() == [("geglu_ln_pipe", True, False, 1)]
        rec.calls.clear()
        monkeypatch.setattr(K, "lnc_ok", lambda x, w: True)
        blk(x, encoder_hidden_states=text)
        assert rec.calls == [(True, False)] and calls.take()[0][:2] == ("geglu_ln_pipe", True)


# =====================================================================================================================================
# 4. what the GPU file's assertions catch
# =====================================================================================================================================
CW, KD = 8, 32                            # channels of the token stand-ins, columns of the tile-major stand-in
BAND = 200                               # rows of guard: more than one 160-row tile


def _ints(shape, seed):
    """Small integers as fp32: every sum is exact, `torch.equal` compares the plan and not a reduction order."""
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(seed)).float()


def _flat(g_view, arena):
    return (g_view.data_ptr() - arena.data_ptr()) // arena.element_size()


def _pipe_result(rows):
    """Stand-in for LayerNorm + GEGLU of `rows [n, CW]`: a row's KD results depend on that row only."""
    return rows.sum(-1, keepdim=True) * torch.arange(1, KD + 1, dtype=torch.float32) + rows[:, :1]


def _pipe_standin(g, h, tile_rows, bug=None):
    """`[M, CW]` tokens through the plan of `geglu_pipe_kernel<PARTIAL>` with a tile-major output: ceil(M / tile_rows) tiles, the source row clamped, the
    pad rows' stores dropped by a range check over the padded storage.  Loads and stores go to raw addresses of the flat arenas."""
    M = h.shape[0]
    hv = g.inp(h, BAND, 0, "h")
    _, a_h, _ = g.inputs[-1]
    h0 = _flat(hv, a_h)
    out = g.blocked_out(M, KD, torch.float32, name="out_blocked")
    _, a_out, band, _, _ = g.blocked_outputs[-1]
    n_store = (M // 160 if bug == "floor_tiles" else FFC.tiles(M)) * 160 * KD      # the buffer range, in elements
    for t in range(FFC.tiles(M, tile_rows)):
        m0 = t * tile_rows
        rl = min(tile_rows - 1, M - 1 - m0)
        for j in range(tile_rows):
            src = m0 + (j if bug == "pad_into_valid" else min(j, rl))      # (the clamp; without it a pad row reads what lies behind the tensor)
            val = _pipe_result(a_h[h0 + src * CW:h0 + (src + 1) * CW][None])[0]
            dst = m0 + j
            if j > rl:
                if bug == "store_pad":
                    pass                                                   # stored where the layout puts row m0 + j
                elif bug == "pad_into_valid":
                    dst = m0 + rl                                          # destination clamped, source not
                else:
                    continue
            if bug == "drop_last_row" and dst == M - 1:
                continue
            for kb in range(KD // 32):
                off = ((dst // 160) * (KD // 32) + kb) * 160 * 32 + (dst % 160) * 32
                if off < n_store:                                          # (the range check of the store)
                    a_out[band + off:band + off + 32] = val[kb * 32:(kb + 1) * 32]
    return {"out": FFC.from_blocked(out, M, KD)}


def _pipe_check(M, tile_rows, bug):
    h = _ints((M, CW), 1)
    got = FFC.run_surroundings(lambda g: _pipe_standin(g, h, tile_rows, bug), "cpu", f"pipe stand-in M {M} bug {bug}")
    FFC.assert_valid_rows_equal(got["out"], _pipe_result(h), f"pipe stand-in M {M} bug {bug}")


@pytest.mark.parametrize("tile_rows,M", [(80, 1), (80, 97), (80, 239), (160, 161), (160, 240), (160, 399)])
def test_right_pipe_standin_passes(tile_rows, M):
    _pipe_check(M, tile_rows, None)


@pytest.mark.parametrize("tile_rows,M", [(80, 97), (160, 241)])
def test_pipe_pad_rows_stored_are_seen_by_the_sentinels(tile_rows, M):
    with pytest.raises(EG.OutsideTouched):                                 # the pad rows of a tile-major output belong to the outside
        _pipe_check(M, tile_rows, "store_pad")


def test_pipe_last_valid_row_dropped_is_caught():
    with pytest.raises(EG.InsideUnwritten):
        _pipe_check(241, 160, "drop_last_row")


def test_pipe_pad_value_landing_in_a_valid_row_is_caught():
    with pytest.raises(EG.SurroundingsMoved):                              # what lies behind the tensor reaches row M - 1: NaN / Inf, or other bits
        _pipe_check(241, 160, "pad_into_valid")
    h = _ints((241, CW), 1)                                                # ... and under ONE fill the bit comparison sees it
    g = FFC.FFGuard("zeros")
    with pytest.raises(AssertionError, match="differ from the whole-tile result"):
        FFC.assert_valid_rows_equal(_pipe_standin(g, h, 160, "pad_into_valid")["out"], _pipe_result(h), "pad_into_valid")


def test_tile_major_range_from_the_floor_of_m_over_160_is_caught():
    with pytest.raises(EG.InsideUnwritten):                                # every store of the last tile falls outside the range and is dropped
        _pipe_check(241, 160, "floor_tiles")
    _pipe_check(320, 160, "floor_tiles")                                   # (whole tiles: floor = ceiling, nothing to see)


def _gemm_standin(g, a, res, bug=None):
    """`out = A w + res` through the plan of `gemm160p_kernel<PARTIAL>`'s epilogue: 160-row tiles of a tile-major A (whole blocks read, pad rows
    included), two passes of 80 rows through ONE staging tile -- residual rows staged (row clamped to M - 1), the pass's results written over them, then
    every (row, chunk) stored with staging row and destination row clamped to the tile's last valid row; a pass without a valid row stages nothing and
    repeats pass 0's last valid row."""
    M, Kd = a.shape
    N = res.shape[1]
    w = torch.arange(1, Kd * N + 1, dtype=torch.float32).view(Kd, N) % 7 - 3
    av = g.blocked_inp(a, name="x_blocked")
    rv = g.inp(res, BAND, 0, "residual")
    _, a_r, _ = g.inputs[-1]
    r0 = _flat(rv, a_r)
    out = g.out((M, N), torch.float32, BAND, 0, "out")
    _, a_o, _, _ = g.outputs[-1]
    o0 = _flat(out, a_o)
    for t in range(FFC.tiles(M)):
        m0 = t * 160
        blk = av[t * 160 * Kd:(t + 1) * 160 * Kd].view(Kd // 32, 160, 32).permute(1, 0, 2).reshape(160, Kd)     # the tile's A rows, pad rows as they are
        acc = blk @ w
        rl = min(159, M - 1 - m0)
        stage = torch.zeros(80, N)
        for p in range(2):
            dead = rl < 80 * p
            if not dead or bug == "residual_past_M":                       # (the mistake: the dead pass stages residual rows, read past M, over pass 0's rows)
                for r in range(80):
                    row = m0 + 80 * p + r if bug == "residual_past_M" else min(m0 + 80 * p + r, M - 1)
                    stage[r] = a_r[r0 + row * N:r0 + (row + 1) * N]
            if not dead:
                stage += acc[80 * p:80 * p + 80]
            for r in range(80):
                rt = min(80 * p + r, rl)
                rs = rt - (0 if dead else 80 * p)
                if bug == "store_pad":
                    rt, rs = 80 * p + r, r
                elif bug == "pad_into_valid" and not dead:
                    rs = r                                                 # destination clamped, staging row not
                elif bug == "drop_last_row" and 80 * p + r >= rl:
                    continue
                a_o[o0 + (m0 + rt) * N:o0 + (m0 + rt + 1) * N] = stage[rs]
    return {"out": out}


def _gemm_check(M, bug):
    a, res = _ints((M, KD), 2), _ints((M, CW), 3)
    w = torch.arange(1, KD * CW + 1, dtype=torch.float32).view(KD, CW) % 7 - 3
    got = FFC.run_surroundings(lambda g: _gemm_standin(g, a, res, bug), "cpu", f"gemm stand-in M {M} bug {bug}")
    FFC.assert_valid_rows_equal(got["out"], a @ w + res, f"gemm stand-in M {M} bug {bug}")


@pytest.mark.parametrize("M", [1, 17, 79, 80, 81, 159, 160, 161, 240, 241, 399])
def test_right_gemm_standin_passes(M):
    _gemm_check(M, None)


@pytest.mark.parametrize("M", [161, 241, 399])
def test_gemm_pad_rows_stored_are_seen_by_the_sentinels(M):
    with pytest.raises((EG.OutsideTouched, EG.SurroundingsMoved)):         # rows past M lie behind the output; what is stored there is poison-dependent
        _gemm_check(M, "store_pad")
    g = FFC.FFGuard("zeros")
    _gemm_standin(g, _ints((M, KD), 2), _ints((M, CW), 3), "store_pad")
    with pytest.raises(EG.OutsideTouched):
        g.check("store_pad")


@pytest.mark.parametrize("M", [161, 177, 240])
def test_gemm_residual_row_read_past_m_is_caught(M):
    """The last tile holds <= 80 rows: its second pass has no valid row.  Staging residual rows there (rows past M) overwrites pass 0's rounded rows, and
    the pass's redirected stores then put them into row M - 1: the surroundings move it (and under one fill the comparison sees it)."""
    with pytest.raises(EG.SurroundingsMoved):
        _gemm_check(M, "residual_past_M")
    g = FFC.FFGuard("zeros")
    a, res = _ints((M, KD), 2), _ints((M, CW), 3)
    w = torch.arange(1, KD * CW + 1, dtype=torch.float32).view(KD, CW) % 7 - 3
    with pytest.raises(AssertionError, match="differ from the whole-tile result"):
        FFC.assert_valid_rows_equal(_gemm_standin(g, a, res, "residual_past_M")["out"], a @ w + res, "residual_past_M")


@pytest.mark.parametrize("M", [161, 241])
def test_gemm_last_valid_row_dropped_is_caught(M):
    with pytest.raises(EG.InsideUnwritten):
        _gemm_check(M, "drop_last_row")


def test_gemm_pad_value_landing_in_a_valid_row_is_caught():
    with pytest.raises(EG.SurroundingsMoved):                              # the pad rows of the tile-major operand hold the poison: it reaches row M - 1
        _gemm_check(241, "pad_into_valid")

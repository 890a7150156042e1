"""The fused temporal and text cross-attention blocks at feature-map sizes that do not fill whole tiles (`fmc_temporal_block_partial_bf16`,
`fmc_xattn_block320_partial_bf16`, `fmc_xattn_block640_partial_bf16`; `hip_ops.temporal_block / xattn_block(..., partial_tiles=True)`).

A tile is 10 pixels x 16 frames (C = 320) or 5 pixels x 16 frames (C = 640) of a clip for the temporal form, 160 (80) consecutive rows of one text's
`images_per_text * hw` rows for the cross-attention form.  The last tile of a clip / of a text is partly filled: its pad rows read the tile's last
valid pixel / row again, are computed, and are never stored.  Asserted per case (the numbering of the issue):

  1. accuracy, with the gates of `test_temporal_block_fused` / `_640` / `test_xattn_block_fused_320` / `_640` and their restatements (the temporal one
     is `tests.test_gpu_edge_guards_fused._tb_case`, which takes any hw; the cross-attention one is restated here): fp32 chain `rel_inf < 2e-2`, the
     restatement with the kernel's bf16 rounding points element-wise within `2^-8 |ref| + 1.5 * 2^-8 max|ref|`, statistics to 1e-4;
  2. bit identity with the WHOLE-TILE kernel: the same tokens padded to the next whole tile with arbitrary finite rows (pixels for the temporal form,
     rows at the end of each text's segment for the cross-attention form) through the existing entry point -- every valid row, output and
     statistics, `torch.equal`;
  3. a whole-tile shape through the new entry point gives the existing entry point's bits;
  4. zeros, quiet NaN and +Inf around every input, packed weight and pose term (tests/edge_guard_common.py), output and statistics inside
     sentinel-filled arenas: finite and bit-identical across the three fills, every word inside written, every sentinel outside intact.  (A pad row
     stored in the temporal layout lands on pixel 0.. of the NEXT FRAME, inside the output: only 1 / 2 see that.  The pad rows of the last frame of
     the last clip land past the end: only the sentinels see that.);
  5. three repeated launches are bit-equal.

tests/test_partial_tiles_host.py shows, with wrong stand-ins in plain torch, that these assertions catch what they are for.  Module and model level:
`hip_ops.PARTIAL_TILES` on routes ragged sizes to the new entry points, off (the default) changes nothing."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import edge_guard_common as EG  # noqa: F401  (the helpers below come from it)
from tests.test_gpu_edge_guards import _call, _p, _rnd, _run, _tilemajor, _vec_band
from tests.test_gpu_edge_guards_fused import TB_BAND, TB_BAND_W, _tb_case
from tests.test_gpu_kernels import rel_inf

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


def _gates(out, ref_r, ref_f, what):
    """Assertion 1 on an output (CPU fp32) against the rounded and the fp32 restatement."""
    e_f = rel_inf(out, ref_f)
    err = (out - ref_r).abs()
    bound = 2.0 ** -8 * ref_r.abs() + 1.5 * 2.0 ** -8 * float(ref_r.abs().max())
    print(f"   {what}: rel-inf {e_f:.3e} (gate 2e-2), worst error in units of the fused blocks' bound {float((err / bound).max()):.3f}")
    assert e_f < 2e-2, what
    assert not bool((err > bound).any()), f"{what}: {int((err > bound).sum())} / {err.numel()} beyond the bound"


def _stats_gate(out_dev, stats, what):
    o = out_dev.float()
    mu, rstd = o.mean(-1).reshape(-1), (o.var(-1, unbiased=False) + 1e-5).rsqrt().reshape(-1)
    assert rel_inf(stats[:, 0], mu) < 1e-4 and rel_inf(stats[:, 1], rstd) < 1e-4, what


def _filler(shape, seed):
    """Arbitrary finite rows for the pad of a whole-tile launch."""
    return _rnd(shape, seed, BF16, 3.0, 1.0)


# =====================================================================================================================================
# temporal form
# =====================================================================================================================================
def _temporal(K, C, B, hw, merge, stats):
    h, gamma, bpe, bo, pt, (wq_p, wo_p, wm_p), ref_r, ref_f, s = _tb_case(C, B, hw, merge)
    rows, d, px = B * 16 * hw, C // 8, (10 if C == 320 else 5)
    what = f"temporal_block partial C {C} B {B} hw {hw} merge {merge} ln_stats {stats}"

    # ---- 4: the partial launch through the raw ABI, everything guarded -------------------------------------------------------------------------
    def fn(g):
        hd = g.inp(h.view(rows, C), TB_BAND, 0, "h")
        gd, bpd, bod = g.inp(gamma, _vec_band(C), 0, "ln_gamma"), g.inp(bpe, 2, 0, "ln_bpe"), g.inp(bo, _vec_band(C), 0, "b_out")
        wqd, wod = g.inp(wq_p.view(-1, C), TB_BAND_W, 0, "w_qkv_packed"), g.inp(wo_p.reshape(-1, C), TB_BAND_W, 0, "w_out")
        wmd = g.inp(wm_p.reshape(-1, C), TB_BAND_W, 0, "w_merge") if merge else None
        ptd = g.inp(pt.view(rows, C), TB_BAND, 0, "pose_term") if merge else None
        out = g.out((rows, C), BF16, TB_BAND, 0, "out")
        st = g.out((rows, 2), F32, TB_BAND, 0, "ln_stats") if stats else None
        _call(K, "fmc_temporal_block_partial_bf16", hd.data_ptr(), out.data_ptr(), gd.data_ptr(), bpd.data_ptr(), 1e-5, _p(wmd), _p(ptd), s, wqd.data_ptr(),
              wod.data_ptr(), bod.data_ptr(), _p(st), 1e-5 if stats else 0.0, B, 16, hw, C, 8, d ** -0.5, K._stream())
        return {"out": out, "ln_stats": st} if stats else {"out": out}
    got = _run(fn, what)
    out = got["out"].view(B, 16, hw, C)

    # ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
    _gates(out.float().cpu(), ref_r, ref_f, what)
    if stats:
        _stats_gate(got["out"], got["ln_stats"], what)

    # ---- the wrappers on plain tensors ----------------------------------------------------------------------------------------------------------
    dev = lambda t: None if t is None else t.cuda()
    gd, bpd, bod, wqd, wod = dev(gamma), dev(bpe), dev(bo), dev(wq_p), dev(wo_p.contiguous())
    wmd = dev(wm_p.contiguous()) if merge else None

    def run(hh, pp, partial):
        kw = dict(w_merge_tm=wmd, pose_term=pp, merge_scale=s) if merge else {}
        r = K.temporal_block(hh, gd, bpd, 1e-5, wqd, wod, bod, d ** -0.5, stats_eps=1e-5 if stats else None, partial_tiles=partial, **kw)
        return r if stats else (r, None)
    hd, ptd = dev(h), dev(pt)
    # ---- 5 (and the wrapper = the raw ABI) -----------------------------------------------------------------------------------------------------
    for _ in range(3):
        o_p, s_p = run(hd, ptd, True)
        assert torch.equal(o_p, out), f"{what}: repeated launches differ"
        assert not stats or torch.equal(s_p, got["ln_stats"])
    # ---- 2: padded to whole tiles through the existing entry point -----------------------------------------------------------------------------
    hwp = -(-hw // px) * px
    hp = _filler((B, 16, hwp, C), 21)
    hp[:, :, :hw] = h
    ptp = None
    if merge:
        ptp = _filler((B, 16, hwp, C), 22)
        ptp[:, :, :hw] = pt
    o_w, s_w = run(dev(hp), dev(ptp), False)
    assert torch.equal(o_w[:, :, :hw], out), f"{what}: valid rows differ from the whole-tile kernel's"
    if stats:
        assert torch.equal(s_w.view(B, 16, hwp, 2)[:, :, :hw].reshape(-1, 2), got["ln_stats"]), f"{what}: statistics differ from the whole-tile kernel's"
    # ---- 3: the whole-tile shape through the new entry point -----------------------------------------------------------------------------------
    o_n, s_n = run(dev(hp), dev(ptp), True)
    assert torch.equal(o_n, o_w) and (not stats or torch.equal(s_n, s_w)), f"{what}: a whole-tile shape through the partial entry point"
    # (the existing entry point keeps refusing the ragged size)
    if hw % px:
        with pytest.raises(ValueError):
            run(hd, ptd, False)


@pytest.mark.parametrize("stats", [True, False], ids=["ln_stats", "nostats"])
@pytest.mark.parametrize("merge", [True, False], ids=["merge", "nomerge"])
@pytest.mark.parametrize("B,hw", [(1, 1), (1, 9), (2, 11), (3, 19)])
def test_temporal_block_partial_320(K, B, hw, merge, stats):
    _temporal(K, 320, B, hw, merge, stats)


@pytest.mark.parametrize("merge", [True, False], ids=["merge", "nomerge"])
@pytest.mark.parametrize("B,hw", [(1, 1), (1, 4), (2, 6), (3, 9)])
def test_temporal_block_partial_640(K, B, hw, merge):
    _temporal(K, 640, B, hw, merge, False)


def test_temporal_block_partial_320_persistent_loop(K):
    """Two clips, CUs + 2 tiles (CUs + 3 on an odd CU count), the last tile of each clip partial: some workgroup runs a second tile, the look-ahead
    of the others has no target, and the first clip's partial tile sits in the middle of the grid."""
    per_clip = (_cus(K) + 3) // 2
    _temporal(K, 320, 2, 10 * per_clip - 3, True, True)


# =====================================================================================================================================
# text cross-attention form
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _xa_case(C, B, ipt, hw, S):
    """Inputs (CPU), packed weights and the two references of test_xattn_block_fused_320 / _640 (the same restatement, evaluated in fp32 on the device).
    The text differs per batch entry, so a tile that takes the neighbouring text misses the reference."""
    from synfmc_amd import hip_ops as K
    H, d, N = 8, C // 8, B * ipt
    h = _rnd((N, hw, C), 1, BF16, 1.5, 0.2)
    gamma, beta = _rnd((C,), 2, F32, 0.3, 1.0), _rnd((C,), 3, F32, 0.2)
    wq, wo, bo = _rnd((C, C), 5, BF16, C ** -0.5 * 1.5), _rnd((C, C), 6, BF16, C ** -0.5), _rnd((C,), 7, BF16, 0.3)
    kv = _rnd((B, S, 2 * C), 8, BF16, 1.2)
    btab = beta[None].expand(16, C).contiguous()
    f = lambda t: t.float().cuda()

    def reference(round_bf16):
        r = (lambda t: t.bfloat16().float()) if round_bf16 else (lambda t: t)
        x = r(F.layer_norm(f(h), (C,), f(gamma), f(beta), 1e-5))
        q = r(F.linear(x, f(wq))).reshape(B, ipt * hw, H, d).permute(0, 2, 1, 3)
        k = f(kv)[..., :C].reshape(B, S, H, d).permute(0, 2, 1, 3)
        v = f(kv)[..., C:].reshape(B, S, H, d).permute(0, 2, 1, 3)
        p = r(torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1))
        o = r(p @ v).permute(0, 2, 1, 3).reshape(N, hw, C)
        return (F.linear(o, f(wo), f(bo)) + f(h)).cpu()
    if C == 320:
        packed = (K.pack_xattn_q40(wq), _tilemajor(wo))
    else:
        packed = (K.pack_w_frag80(wq), K.pack_w_frag80(wo))
    frag = K.xattn_pack_kv(kv.cuda()).cpu()
    return h, gamma, btab, bo, kv, frag, packed, reference(True), reference(False)


def _xattn(K, C, B, ipt, hw, S, stats):
    h, gamma, btab, bo, kv, frag, (wq_p, wo_p), ref_r, ref_f = _xa_case(C, B, ipt, hw, S)
    N, d, T = B * ipt, C // 8, (160 if C == 320 else 80)
    rows, seg = N * hw, ipt * hw
    what = f"xattn_block partial C {C} B {B} images/text {ipt} hw {hw} S {S} ln_stats {stats}"
    name = "fmc_xattn_block320_partial_bf16" if C == 320 else "fmc_xattn_block640_partial_bf16"

    def fn(g):
        hd = g.inp(h.view(rows, C), TB_BAND, 0, "h")
        gd, btd, bod = g.inp(gamma, _vec_band(C), 0, "ln_gamma"), g.inp(btab, 2, 0, "ln_btab"), g.inp(bo, _vec_band(C), 0, "b_out")
        wqd, wod = g.inp(wq_p.view(-1, C), TB_BAND_W, 0, "w_q_packed"), g.inp(wo_p.reshape(-1, C), TB_BAND_W, 0, "w_out")
        fd = g.inp(frag.view(-1, C), TB_BAND_W, 0, "kvfrag")
        out = g.out((rows, C), BF16, TB_BAND, 0, "out")
        st = g.out((rows, 2), F32, TB_BAND, 0, "ln_stats") if stats else None
        if C == 320:
            _call(K, name, hd.data_ptr(), out.data_ptr(), gd.data_ptr(), btd.data_ptr(), 1e-5, wqd.data_ptr(), fd.data_ptr(), wod.data_ptr(), bod.data_ptr(),
                  _p(st), 1e-5 if stats else 0.0, N, hw, S, ipt, d ** -0.5, K._stream())
        else:
            _call(K, name, hd.data_ptr(), out.data_ptr(), gd.data_ptr(), btd.data_ptr(), 1e-5, wqd.data_ptr(), fd.data_ptr(), wod.data_ptr(), bod.data_ptr(),
                  N, hw, S, ipt, d ** -0.5, K._stream())
        return {"out": out, "ln_stats": st} if stats else {"out": out}
    got = _run(fn, what)
    out = got["out"].view(N, hw, C)
    _gates(out.float().cpu(), ref_r, ref_f, what)                                   # 1
    if stats:
        _stats_gate(got["out"], got["ln_stats"], what)

    gd, btd, bod, wqd, wod, kvd, fd = gamma.cuda(), btab.cuda(), bo.cuda(), wq_p.cuda(), wo_p.contiguous().cuda(), kv.cuda(), frag.cuda()

    def run(hh, per_text, partial):
        r = K.xattn_block(hh, gd, btd, 1e-5, wqd, kvd, wod, bod, d ** -0.5, per_text, stats_eps=1e-5 if stats else None, frag=fd, partial_tiles=partial)
        return r if stats else (r, None)
    hd = h.cuda()
    for _ in range(3):                                                              # 5
        o_p, s_p = run(hd, ipt, True)
        assert torch.equal(o_p, out), f"{what}: repeated launches differ"
        assert not stats or torch.equal(s_p, got["ln_stats"])
    segp = -(-seg // T) * T                                                         # 2: every text's segment padded at its end to whole tiles
    hp = _filler((B, segp, C), 23)
    hp[:, :seg] = h.view(B, seg, C)
    o_w, s_w = run(hp.cuda(), 1, False)
    assert torch.equal(o_w[:, :seg].reshape(N, hw, C), out), f"{what}: valid rows differ from the whole-tile kernel's"
    if stats:
        assert torch.equal(s_w.view(B, segp, 2)[:, :seg].reshape(-1, 2), got["ln_stats"]), f"{what}: statistics differ from the whole-tile kernel's"
    o_n, s_n = run(hp.cuda(), 1, True)                                              # 3
    assert torch.equal(o_n, o_w) and (not stats or torch.equal(s_n, s_w)), f"{what}: a whole-tile shape through the partial entry point"
    if hw % T:
        with pytest.raises(ValueError):
            run(hd, ipt, False)


@pytest.mark.parametrize("stats", [True, False], ids=["ln_stats", "nostats"])
@pytest.mark.parametrize("B,ipt,hw,S", [(2, 1, 24, 77), (2, 3, 100, 5), (3, 2, 161, 80)])
def test_xattn_block_partial_320(K, B, ipt, hw, S, stats):
    _xattn(K, 320, B, ipt, hw, S, stats)


@pytest.mark.parametrize("B,ipt,hw,S", [(2, 1, 24, 77), (2, 3, 50, 5), (3, 2, 81, 80)])
def test_xattn_block_partial_640(K, B, ipt, hw, S):
    _xattn(K, 640, B, ipt, hw, S, False)


def test_xattn_block_partial_320_persistent_loop(K):
    """Two texts, CUs + 2 tiles (CUs + 3 on an odd CU count), the last tile of each text's segment partial."""
    per_text = (_cus(K) + 3) // 2
    _xattn(K, 320, 2, 1, 160 * per_text - 17, 77, True)


# =====================================================================================================================================
# module level: the switch routes ragged sizes to the new entry points, and only the switch does
# =====================================================================================================================================
def _init(blk, norms):
    with torch.no_grad():
        for p in blk.parameters():
            if p.ndim >= 2:
                p.normal_(0, p.shape[-1] ** -0.5)
            else:
                p.normal_(0, 0.2)
        for n in norms:
            n.weight.add_(1.0)


class _Count:
    """Counts the launches of one `hip_ops` wrapper, and those that asked for partial tiles."""

    def __init__(self, K, name):
        self.K, self.name, self.calls, self.partial = K, name, 0, 0

    def __enter__(self):
        self.real = getattr(self.K, self.name)

        def counted(*a, **k):
            self.calls += 1
            self.partial += bool(k.get("partial_tiles"))
            return self.real(*a, **k)
        setattr(self.K, self.name, counted)
        return self

    def __exit__(self, *exc):
        setattr(self.K, self.name, self.real)


@pytest.mark.parametrize("C,P", [(320, 39), (640, 34)])
def test_temporal_transformer_block_partial_tiles_switch(K, C, P):
    """`TemporalTransformerBlock` as in test_temporal_transformer_block_fused_kernel_equals_the_unfused_chain, at a pixel count that fills no whole
    number of tiles.  Switch on: both attention blocks take the fused kernel, and the result is as close to the un-fused chain and to fp32 as that
    test asks.  Switch off (the default): no fused launch, and the result is the un-fused chain's, bit for bit."""
    from synfmc_amd.models import motion_module as MM
    from synfmc_amd.models.attention_processor import AttnProcessor, PoseAdaptorAttnProcessor
    torch.manual_seed(3)
    H, Fr, B = 8, 16, 2
    blk = MM.TemporalTransformerBlock(dim=C, num_attention_heads=H, attention_head_dim=C // H, attention_block_types=("Temporal_Self", "Temporal_Self"),
                                      temporal_position_encoding=True, temporal_position_encoding_max_len=32)
    blk.attention_blocks[0].set_processor(PoseAdaptorAttnProcessor(hidden_size=C, pose_feature_dim=C, query_condition=True, key_value_condition=True,
                                                                   scale=0.8))
    blk.attention_blocks[1].set_processor(AttnProcessor())
    _init(blk, list(blk.norms) + [blk.ff_norm])
    blk = blk.to("cuda", BF16).eval()
    x = (torch.randn(B, Fr, P, C) * 1.2).to("cuda", BF16)
    pose = torch.randn(B, Fr, P, C).to("cuda", BF16)
    kw = {"pose_feature": pose}
    assert not K.PARTIAL_TILES, "the switch is off by default"
    with torch.no_grad():
        assert not blk.fused_blocks_ok(x, None, kw) and blk.fused_blocks_partial_ok(x, None, kw)
        blk(x, cross_attention_kwargs=kw)                                    # (the per-shape autotuner settles on its arms in the first call)
        with _Count(MM.K, "temporal_block") as c_off:
            plain = blk(x, cross_attention_kwargs=kw)
        assert c_off.calls == 0
        MM.TEMPORAL_FUSED = False
        try:
            chain = blk(x, cross_attention_kwargs=kw)
        finally:
            MM.TEMPORAL_FUSED = True
        assert torch.equal(plain, chain)                                     # off = today's un-fused chain
        K.PARTIAL_TILES = True
        try:
            with _Count(MM.K, "temporal_block") as c_on:
                fused = blk(x, cross_attention_kwargs=kw)
        finally:
            K.PARTIAL_TILES = False
        assert c_on.calls == 2 and c_on.partial == 2                         # both attention blocks took the fused kernel
        ref = blk.float()(x.float(), cross_attention_kwargs={"pose_feature": pose.float()})
    assert rel_inf(fused, plain) < 2e-2
    e_f, e_p = rel_inf(fused, ref), rel_inf(plain, ref)
    print(f"   temporal transformer block C {C} P {P}: fused vs chain {rel_inf(fused, plain):.3e}, fused vs fp32 {e_f:.3e}, chain vs fp32 {e_p:.3e}")
    assert e_f < 2e-2 and e_f < 2.0 * e_p + 2e-3, (e_f, e_p)


@pytest.mark.parametrize("C,hw", [(320, 39), (640, 34)])
def test_basic_transformer_block_partial_tiles_switch(K, C, hw):
    """The spatial transformer block's fused text cross-attention (test_basic_transformer_block_fused_text_cross_attention_equals_the_unfused_chain)
    at a ragged hw: one fused launch with the switch on, none with it off."""
    from synfmc_amd.models import layers as L
    torch.manual_seed(5)
    H, B, Fr, S = 8, 2, 3, 77
    blk = L.BasicTransformerBlock(C, H, C // H, cross_attention_dim=768)
    _init(blk, (blk.norm1, blk.norm2, blk.norm3))
    blk = blk.to("cuda", BF16).eval()
    x = (torch.randn(B * Fr, hw, C) * 1.2).to("cuda", BF16)
    text = torch.randn(B, S, 768).to("cuda", BF16)
    assert not K.PARTIAL_TILES, "the switch is off by default"
    with torch.no_grad():
        blk(x, encoder_hidden_states=text)                                   # (the per-shape autotuner settles on its arms in the first call)
        with _Count(L.K, "xattn_block") as c_off:
            plain = blk(x, encoder_hidden_states=text)
        assert c_off.calls == 0
        L.K.XATTN_FUSED_640 = L.K.XATTN_FUSED_320 = False
        try:
            chain = blk(x, encoder_hidden_states=text)
        finally:
            L.K.XATTN_FUSED_640 = L.K.XATTN_FUSED_320 = True
        assert torch.equal(plain, chain)
        K.PARTIAL_TILES = True
        try:
            with _Count(L.K, "xattn_block") as c_on:
                fused = blk(x, encoder_hidden_states=text)
        finally:
            K.PARTIAL_TILES = False
        assert c_on.calls == 1 and c_on.partial == 1
        ref = blk.float()(x.float(), encoder_hidden_states=text.float())
    assert rel_inf(fused, plain) < 2e-2
    e_f, e_p = rel_inf(fused, ref), rel_inf(plain, ref)
    print(f"   basic transformer block C {C} hw {hw}: fused vs chain {rel_inf(fused, plain):.3e}, fused vs fp32 {e_f:.3e}, chain vs fp32 {e_p:.3e}")
    assert e_f < 2e-2 and e_f < 2.0 * e_p + 2e-3, (e_f, e_p)


# =====================================================================================================================================
# model level: the full-width U-Net + CMC + OMC at 16x64x128 (level 0: 8x16 = 128 pixels, level 1: 32 -- both ragged for all four blocks)
# =====================================================================================================================================
MH, MW = 64, 128


@pytest.fixture(scope="module")
def model64(K):
    """The case of tests/test_gpu_full_width.py on a smaller clip: the oracle in fp32 and under bf16 rounding of every layer output and weight
    (`format_err`, what the bf16 FORMAT costs on this case), and the product models in bf16."""
    import os

    from einops import rearrange

    from oracle import conditioning as OC
    from tests import common_models as CM
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ou, oe, oa, clip = CM.full_width_case(43, 143, MH, MW)
    t = torch.tensor([801])
    with torch.no_grad():
        pose_emb = rearrange(OC.to_plucker_embedding(clip["c2w"], clip["K"], (MH, MW)), "b f c h w -> b c f h w")
        pose_feats = [rearrange(x, "(b f) c h w -> b c f h w", b=1) for x in oe(pose_emb)]
        traj = OC.get_traj_features(clip["infos"], clip["masks"], oa)
        ref = ou(clip["latents"], t, clip["text"], pose_embedding_features=pose_feats, traj_features=traj).sample
        with CM.bf16_rounding(ou, oe, oa):
            pf16 = [rearrange(x, "(b f) c h w -> b c f h w", b=1) for x in oe(pose_emb)]
            tr16 = OC.get_traj_features(clip["infos"], clip["masks"], oa)
            ref16 = ou(clip["latents"], t, clip["text"], pose_embedding_features=pf16, traj_features=tr16).sample
    pu, pe, pa = CM.build_product(ou, oe, oa, CM.FULL_WIDTHS, CM.FULL_CROSS_DIM, dtype=BF16)
    format_err = rel_inf(ref16, ref)
    print(f"   16x{MH}x{MW}: bf16 format alone (rounded oracle vs fp32 oracle) {format_err:.3e}")
    assert 2e-3 < format_err < 4e-2                                         # (the sanity window of test_full_width_bf16_parity_and_format_share)
    return dict(pu=pu, pe=pe, pa=pa, clip=clip, t=t, ref=ref, format_err=format_err)


def _fused_launches(log):
    fused = [shape for family, shape, _ in log if family == "fused_block"]
    return len(fused), sum(1 for s in fused if any(isinstance(e, tuple) and e and e[0] == "partial" for e in s))


def test_full_width_unet_partial_tiles_switch_eager(K, model64):
    """Eager forward, switch off against switch on: two bf16 paths of the same model, under the format gate of tests/test_gpu_full_width.py for such a
    pair (`2 x format_err`); the fused launches are counted from `hip_ops.call_log`."""
    from einops import rearrange

    from synfmc_amd.data.dataset import to_plucker_embedding
    from synfmc_amd.models.pose_obj_adaptor import CamObjPoseAdaptor
    from synfmc_amd.util import get_traj_features_v2
    m, clip = model64, model64["clip"]
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
            counts[on] = _fused_launches(log)
    print(f"   eager 16x{MH}x{MW}: fused launches (all, partial) off {counts[False]}, on {counts[True]}; on vs off {rel_inf(outs[True], outs[False]):.3e}, "
          f"on vs fp32 oracle {rel_inf(outs[True], m['ref']):.3e}, off vs fp32 oracle {rel_inf(outs[False], m['ref']):.3e} (format {m['format_err']:.3e})")
    assert counts[False] == (0, 0)                                           # every fused-block site of this clip is ragged: none fused today
    assert counts[True][0] > 0 and counts[True][0] == counts[True][1]
    assert rel_inf(outs[True], outs[False]) < 2.0 * m["format_err"]
    assert rel_inf(outs[True], m["ref"]) < 2.5 * m["format_err"] and rel_inf(outs[True], m["ref"]) < 4e-2


def test_full_width_pipeline_partial_tiles_switch_graph(K, model64, monkeypatch):
    """`CameraObjCtrlPipeline` with a captured graph, three steps, two clips of different conditioning (every call after the capturing one refills
    the graph: `_GraphedUNet.set_conditioning`), switch off against on under the same gate; refilled back, the first clip gives its own bits again."""
    from synfmc_amd import configs as CF
    from synfmc_amd.models.pose_adaptor import features_to_video
    from synfmc_amd.pipelines.pipeline_animation_cm_om import CameraObjCtrlPipeline
    from synfmc_amd.schedulers import DDIMScheduler
    from synfmc_amd.util import stack_object_inputs
    monkeypatch.setattr(K, "DETERMINISTIC", True)      # (as test_pipeline_graph_reuse_across_clips: no vendor convolution arm, whose atomics differ run to run)
    m = model64
    clips = [m["clip"], CF.synthetic_clip(B=1, Fr=16, H=MH, W=MW, cross_dim=768, seed=144)]
    uncond = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(99))
    sk = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    pipe = CameraObjCtrlPipeline(None, None, None, m["pu"], DDIMScheduler(**sk), m["pe"])
    assert not K.PARTIAL_TILES

    def kwargs(clip):
        poses, masks = stack_object_inputs(clip["infos"], clip["masks"], "cuda")
        feats, mk = K.omc_rasterize(poses, masks, "unshuffle8", BF16)
        return dict(prompt=None, video_length=16, height=MH, width=MW, num_inference_steps=3, guidance_scale=2.0,
                    prompt_embeds=torch.cat([uncond, clip["text"]]).to("cuda", BF16), latents=clip["latents"].cuda(), output_type="latent",
                    pose_embedding=K.plucker(clip["K"].cuda(), clip["c2w"].cuda(), MH, MW, "unshuffle8", BF16), pose_embedding_unshuffled=True,
                    traj_features=features_to_video(m["pa"](feats, mk), 1))
    with torch.no_grad():
        kws = [kwargs(c) for c in clips]
        lat, counts = {}, {}
        for on in (False, True):
            K.PARTIAL_TILES = on
            try:
                K.call_log = []
                pipe(**kws[0])                                               # captures (its first step also settles the autotuned arms)
                log, K.call_log = K.call_log, None
                a = torch.as_tensor(pipe(**kws[0]).videos).float().cpu()     # replays
                b = torch.as_tensor(pipe(**kws[1]).videos).float().cpu()     # refills with the second clip's conditioning
                a2 = torch.as_tensor(pipe(**kws[0]).videos).float().cpu()    # refills back
            finally:
                K.PARTIAL_TILES, K.call_log = False, None
            print(f"   switch {'on' if on else 'off'}: the first clip again after the second, rel-inf {rel_inf(a2, a):.3e}")
            assert rel_inf(a2, a) < 1e-6, f"switch {'on' if on else 'off'}: stale per-clip state in the refilled graph"
            assert rel_inf(a, b) > 1e-3                                      # the second clip's conditioning reached the graph
            lat[on], counts[on] = (a, b), _fused_launches(log)
    assert len(pipe._runners) == 2                                           # one graph per switch setting
    e = [rel_inf(lat[True][i], lat[False][i]) for i in range(2)]
    print(f"   graph 16x{MH}x{MW}, 3 steps: fused launches at capture (all, partial) off {counts[False]}, on {counts[True]}; latents on vs off {e[0]:.3e}, "
          f"{e[1]:.3e} (gate {2.0 * m['format_err']:.3e})")
    assert counts[False] == (0, 0) and counts[True][0] > 0 and counts[True][0] == counts[True][1]
    assert all(torch.isfinite(x).all() for pair in lat.values() for x in pair)
    assert max(e) < 2.0 * m["format_err"]

"""Shared by tests/test_gpu_gemm_forward_elementwise.py (GPU) and tests/test_gemm_fwd_reference_host.py (CPU): the case table of the forward token GEMMs
(csrc/gemm_conv.hip, csrc/gemm4.hip, the fold kernel of csrc/norm_kernels.hip), a restatement of their dispatch, the two input generators, the float64
references, the element-wise bounds, a plain-torch fp32 emulation of every documented rounding chain, and the wrong stand-ins the bounds have to catch.
profiles/gemm_forward_bounds.md is the record (rounding points per form, derivations, measured shares of the bounds, the stand-in table).

Two instruments, every launch form gets both:

* EXACT runs.  Dense integer bf16 operands in [-r, r] (r per case, `exact_range`), small integer bias / residuals, alpha 0.5 or 1.  While
  `sum|terms| < 2^24` and every output is representable in bf16 (`assert_exact_conditions`, on the float64 reference), every product and every partial sum
  in ANY order is exact in fp32: the output equals the reference bit for bit whatever the tile, ring depth, split, segment boundary or summation order,
  and a dropped, doubled or mis-addressed product moves an element by at least alpha.
* ROUNDING runs.  Gaussian data as `_gemm_data` of tests/test_gpu_edge_guards.py makes it; `|got - ref| <= 2^-8 |ref| + 1e-5 sum|terms|` for every
  element (`assert_bf16_close`; `assert_f32_close` for fp32 storage), plus per form the addends derived below (GEGLU: the GELU evaluation; `_ln`: the
  row statistics; the fold: its fp32 chain).

The vendor arm (not our kernel), the MXFP8 chain (tests/test_gpu_mxfp8.py has exact tests), the convolution loader of these kernels
(tests/conv_fwd_common.py) and `fmc_linear_wgrad_bf16` / backward-data are not in this table."""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests import fused_block_common as FB
from tests.conv_fwd_common import STATS_CHAIN, STATS_REL, assert_bf16_close, assert_f32_close, check_exact, rel_inf, truncate_bf16  # noqa: F401

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
DEVICE_CUS = 256                      # the MI355X; the CPU file runs every case at this count

# ---- constants counted from the source -------------------------------------------------------------------------------------------------------------
# GELU of the bf16 GEGLU epilogues, common.h:80-93 (`fmc_gelu_fast`): the fit's absolute error, asserted on its float32 restatement by
# tests/test_gelu_fast.py; the hardware exp2 and rcp are 1 ulp each where the restatement rounds correctly: e = exp2(t) 1 ulp = 2 half-ulps, weight
# |g| s (1 - s) <= |g| / 4; r = rcp(1 + e) 2 half-ulps, weight |g| s <= |g|: 2.5, taken as 4 half-ulps of |g|.  (`make GELU_EXACT=1`: 1.5e-7.)
GELU_ABS = 2.6e-5
GELU_HW_REL = 4 * 2.0 ** -24
GELU_SLOPE = 1.13                     # max |gelu'| = 1.129
# Row statistics of gemm160p_kernel's LayerNorm epilogue (gemm_conv.hip:2270-2296), unit 2^-24 = half an fp32 ulp.  Four lanes per row, 80 values each.
# mean (:2275-2283): per lane 10 x 4 x (`lo + hi`, then `s1 +=`) = 80 roundings, two shuffle additions, the rounded constant 1.f / 320.f and the product
#   = 84, each at most 2^-24 of the row's sum |x|:  |mean - mean64| <= 84 * 2^-24 * mean|x|.
# rstd (:2286-2295): relative error of var + eps (all addends positive): `x - mean` 1, squared 2 + 1, `lo * lo + hi * hi` 1, the 40 `s2 +=` of a lane 40,
#   two shuffle additions 2, constant and product 2, `+ eps` 1, the fp32 eps against the float64 one 1 = 50; halved by the inverse square root = 25; rsqrtf
#   within 2 ulp = 4: 29, taken as 32.  The kernel centres on ITS mean: var grows by (mean - mean64)^2, added per row.
# (The same two counts as csrc/temporal_block.hip:700-723 gave tests/fused_block_common.py: the code has the same shape.)
LN_MEAN_CHAIN, LN_RSTD_CHAIN = 84, 32
LN_MEAN_REL, LN_RSTD_REL = LN_MEAN_CHAIN * 2.0 ** -24, LN_RSTD_CHAIN * 2.0 ** -24
LN_EPS = 1e-5
# gn_partials of the 160 x 320 kernels (gemm_conv.hip:1388-1414): thread t adds the pairs `a + b` of group t % GT over its rows of both 80-row passes --
# N / 32 = 10 channels per group: 5 rows x 5 pairs x 2 passes = 50 `s += a + b` = 100 roundings, then RP = 16 partials: 116; 20 channels per group: 3 rows x
# 10 pairs x 2 passes = 60 -> 120, then 32: 152.  Both within the 164 of conv_fwd_common.STATS_CHAIN, whose STATS_REL is the bound here.
assert STATS_CHAIN >= 152
# fmc_groupnorm_fold_linear (norm_kernels.hip:1141-1191).  w_out = bf16(w * (rstd * gamma)): rstd rounded from double 1, `rstd * gamma` 1, `wv * a_c` 1 = 3
# half-ulps in front of the ONE bf16 rounding.  bias_out: per addend `wv * be` 1, `wr * m_c` 1, their difference 1, the fp32 mean against the float64 one 1
# = 4 of |wv be| + |wr m_c|; the accumulation: 8 `acc +=` per 64 chunks of 8 channels, six shuffle additions, `+ bias` = 8 ceil(C / 512) + 7 of the
# running sum of |addends|.
FOLD_W_CHAIN = 3


def fold_bias_chain(C):
    return 4 + 8 * -(-C // 512) + 7


# ---- the case table ------------------------------------------------------------------------------------------------------------------------------------
# entry: C-ABI entry point without the `fmc_` prefix; tile / split_k: as the ABI takes them; shape (M, N, K); k_split: two-source seam (0: one source);
# extras: "b" bias, "a" alpha 0.5 (else 1), "r" residual, "2" residual2; geglu: the GEGLU epilogue (N counts value + gate rows); form: what else the
# entry point is asked for; want: the (kernel, form) the case exists for -- `expected_kernel` must return it; note: a fall-back the case records.
Case = namedtuple("Case", "name entry tile split_k shape k_split extras geglu form want note")

RING = {  # C-ABI tile -> (WM, WN, BK, STAGES, MI) of launch_gemm_g, gemm_conv.hip:2938-2957
    1: (2, 2, 64, 2, 2), 2: (4, 2, 64, 2, 2), 3: (4, 4, 64, 2, 2), 4: (2, 2, 32, 2, 2), 5: (4, 2, 32, 2, 2), 6: (4, 4, 32, 2, 2), 7: (4, 2, 64, 3, 2),
    8: (4, 4, 32, 4, 2), 9: (2, 2, 32, 4, 2), 10: (4, 2, 32, 4, 2), 11: (2, 5, 64, 2, 2), 12: (2, 5, 32, 4, 2),
    19: (2, 2, 64, 3, 1), 20: (2, 2, 32, 4, 1), 21: (4, 2, 64, 2, 1), 22: (2, 4, 64, 2, 1)}


def ring_tile(tile):
    wm, wn, bk, stages, mi = RING[tile]
    return 32 * mi * wm, 64 * wn, bk


def ring_name(tile):
    wm, wn, bk, stages, mi = RING[tile]
    return f"gemm_kernel<WM {wm}, WN {wn}, MI {mi}, BK {bk}, STAGES {stages}>"


def ring_per_cu(tile):
    """Co-resident workgroups per CU of a stream-K launch, launch_gemm_g :2490-2500 (the stream-K form keeps the fp32 slab: `lds`, not `lds_plain`)."""
    wm, wn, bk, stages, mi = RING[tile]
    bm, bn = 32 * mi * wm, 64 * wn
    lds = max(stages * (bm + bn) * bk * 2 + 1024, 64 * (bn + 8) * 4)
    by_waves = max(16 // (wm * wn), 1)
    return max(min(160 * 1024 // lds, by_waves), 1)


def _tiles(M, N, bm, bn):
    return -(-M // bm) * -(-N // bn)


def lockstep_chunks(nkt, tiles, g, asked):
    """S of the K-lockstep split, launch_gemm8 :2565-2577: the caller's, or the cheapest by the cost model."""
    S = asked if asked > 1 else 0
    if not S:
        best = 1e30
        for s2 in range(2, min(16, nkt // 4) + 1):
            L = -(-nkt // s2)
            if (s2 - 1) * L >= nkt:
                continue
            rounds = -(-tiles * s2 // g)
            cost = rounds * (L * 1.9 + 4.0) + tiles * s2 * 0.06
            if cost < best:
                best, S = cost, s2
    return S


def workspace_bytes(c, cus):
    """The workspace the header asks for (include/fmc_hip.h, `split_k`): what the GPU file hands over, to the byte."""
    M, N, K = c.shape
    if c.split_k > 1:
        return c.split_k * M * N * 4
    if c.split_k == 1:
        return 0
    if c.tile in (13, 14):
        tiles, g = _tiles(M, N, 256, 256), cus & ~7
        if c.split_k == -3 or c.split_k <= -16:
            return 4096 + tiles * 16 * 256 * 256 * 4                         # (S <= 16 here)
        return 4096 + g * (-(-tiles // g) + 2) * 256 * 256 * 4
    bm, bn, _ = ring_tile(c.tile)
    return 4096 + ((cus * ring_per_cu(c.tile)) & ~7) * bm * bn * 4


def expected_kernel(c, cus=DEVICE_CUS):
    """(kernel, form) the C ABI runs for `c` on a device of `cus` compute units, every A/B switch at its default and the workspace of `workspace_bytes`:
    `linear_impl`, `launch_gemm` and the launchers it calls (csrc/gemm_conv.hip), restated line by line."""
    M, N, K = c.shape
    g8 = cus & ~7
    if c.entry == "linear4_bf16":
        return "gemm4_kernel", "plain grid"                                                                    # gemm4.hip:198-215: one kernel
    if c.entry == "linear_fp8_qkv":
        return "gemm8_kernel<EPI 2, PF 4>", "plain grid"                                                       # fmc_linear_fp8_qkv (split_k 1, no stream-K)
    if c.entry in ("linear_bf16_ffblk_partial", "linear_bf16_fftail_partial"):
        assert N % 320 == 0 and -(-M // 160) * (N // 320) >= g8 >= 8                                           # ff_partial_impl
        return ("gemm160p_kernel<0, 5, 0, 0, 1, 0, 1>" if c.k_split else "gemm160p_kernel<0, 5, 0, 0, 0, 0, 1>"), "persistent, partial"    # launch_gemm160p, forms 7 | 8
    f32 = c.entry == "linear_x3_f32"
    tile = 16 if c.tile == 18 else c.tile                                                                      # linear_impl
    a_blocked = "x_blocked" in c.form or c.entry == "linear_bf16_fftail"
    a2, res2, epi = c.k_split > 0, "2" in c.extras, int(c.geglu)
    split = c.split_k if c.split_k > 1 else 1                                                                  # set_split_k
    sk, hybrid = c.split_k < 0, c.split_k == -2
    lock = 1 if c.split_k == -3 else (-c.split_k - 16 if c.split_k <= -16 else 0)
    gemm8_ok = split == 1 and (not a2 or a_blocked)                                                            # gemm8_ok (every operand here is below 2 GiB)
    g = tile
    assert 1 <= g <= 22, "the table names its tiles (tile 0 = the library's choice is not a launch form)"
    if g == 17:                                                                                                # launch_gemm
        if epi == 1 and gemm8_ok and N % 320 == 0 and M % 256 == 0 and not sk and not a2 and not f32 and g8 >= 8 and (M // 256) * (N // 320) > g8:    # gemm256p_ok
            return "gemm160p_kernel<1, 8>", "persistent 256 x 320"                                             # launch_gemm256p
        g = 16
    if g == 16:                                                                                                # launch_gemm
        if (not a2 or a_blocked) and N % 320 == 0 and not sk:                                                  # gemm8_ok with split_k set aside, gemm160_ok
            tiles = -(-M // 160) * (N // 320)
            if split > 1:
                assert epi == 0
                return "gemm160_kernel<0, 0>", "split-K + splitk_reduce_kernel"                                # launch_gemm160
            imgw = c.entry == "linear_bf16_imgw"
            if not f32 and M % 160 == 0 and g8 >= 8 and (tiles >= g8 if (a_blocked or imgw) else tiles > g8):  # launch_gemm160, g160_persistent_shape
                e0 = epi == 0                                                                                  # launch_gemm160p
                form = ((5 if "ln_stats" in c.form else 4) if e0 and imgw else 6 if e0 and a2 else 1 if "lnc" in c.form else 2 if e0 and "ln_out" in c.form
                        else 3 if e0 and "ln_stats" in c.form else 0)
                args = {0: "", 1: ", 0, 1", 2: ", 1", 3: ", 2", 4: ", 0, 0, 0, 1", 5: ", 2, 0, 0, 1", 6: ", 0, 0, 1"}[form]                             # launch_gemm160p
                return f"gemm160p_kernel<{epi}, 5{args}>", "persistent"
            return f"gemm160_kernel<0, {epi}>", "plain grid"                                                   # launch_gemm160
        g = 13
    if g in (13, 14) and not gemm8_ok:                                                                         # launch_gemm
        g = 3
    if g == 15:                                                                                                # launch_gemm, gemm_k320_ok :2801-2805
        if epi == 0 and not f32 and K == 320 and N % 320 == 0 and M % 64 == 0 and not a2 and not res2 and split == 1 and not sk:
            return "gemm_k320_kernel<2, 2, " + ("true>" if "r" in c.extras else "false>"), "persistent"       # gemm_k320_cfg default, :2821
        g = 5
    if epi == 0 and 19 <= g <= 22 and (split != 1 or res2 or sk or f32):                                       # launch_gemm
        g = 1
    if g in (13, 14):                                                                                          # launch_gemm8, :2530-2607
        name = f"gemm8_kernel<EPI {epi}, PF {4 if g == 13 else 5}>"
        tiles, nkt = _tiles(M, N, 256, 256), K // 64
        if sk and hybrid and not lock:                                                                         # :2541-2560
            t0 = (tiles // g8) * g8 if g8 >= 8 else 0
            rem = tiles - t0
            if t0 > 0 and rem > 0 and rem * nkt >= 2 * g8:
                return name, "hybrid: plain grid + stream-K (two launches)"
            if rem == 0:
                sk = False
        if sk and lock:                                                                                        # :2561-2589
            S = lockstep_chunks(nkt, tiles, g8, lock)
            L = -(-nkt // S) if S else 0
            if g8 >= 8 and S >= 2 and (S - 1) * L < nkt:
                return name, f"k-lockstep S = {S} + " + ("sk_finish_kernel" if epi == 0 else "its finishing launch")
        if sk and g8 >= 8 and tiles * nkt >= 2 * g8:                                                           # :2590-2603
            return name, "stream-K (two launches)"
        return name, "plain grid"                                                                              # :2606
    wm, wn, bk, stages, mi = RING[g]                                                                           # launch_gemm_g, :2483-2526
    bm, bn = 32 * mi * wm, 64 * wn
    if sk:
        gsk = (cus * ring_per_cu(g)) & ~7
        if stages == 2 and mi == 2 and gsk >= 8 and _tiles(M, N, bm, bn) * (K // bk) >= 4 * gsk and gsk * 4 <= 4096:      # :2507
            return ring_name(g), "stream-K (flags)"
    if split > 1:
        return ring_name(g), "split-K + splitk_reduce_kernel"                                                  # :2522-2525
    return ring_name(g), "plain grid"


def k_cuts(c, cus, kernel, form):
    """Where the launch cuts the reduction, as a function tile -> list of (k0, k1) chunks summed in this order (fp32 partials): the emulation's
    summation order.  Tiles are (row block, column block) of the kernel's geometry; an un-split launch is one tile with one chunk."""
    M, N, K = c.shape
    if "split-K" in form:
        unit = 32 if kernel.startswith("gemm160") else ring_tile(c.tile)[2]
        n = K // unit
        per = (-(-n // c.split_k) + 1) & ~1 if unit == 32 and kernel.startswith("gemm160") else -(-n // c.split_k)          # :1485 / :381
        chunks = [(s * per * unit, min(K, (s + 1) * per * unit)) for s in range(c.split_k) if s * per < n]
        return (M, N), lambda tm, tn: chunks
    if "k-lockstep" in form:
        nkt = K // 64
        S = int(form.split("S = ")[1].split(" ")[0])
        L = -(-nkt // S)
        chunks = [(s * L * 64, min(K, (s + 1) * L * 64)) for s in range(S)]
        return (M, N), lambda tm, tn: chunks
    if "stream-K" in form:
        if kernel.startswith("gemm8"):
            bm, bn, bk, g = 256, 256, 64, cus & ~7
        else:
            bm, bn, bk = ring_tile(c.tile)
            g = (cus * ring_per_cu(c.tile)) & ~7
        tiles_m, tiles_n, nk = -(-M // bm), -(-N // bn), K // bk
        t0 = 0
        if form.startswith("hybrid"):
            t0 = (tiles_m * tiles_n // g) * g
        per = -(-(tiles_m * tiles_n - t0) * nk // g)                         # equal contiguous ranges of the (tile, k-tile) space

        def cuts(tm, tn):
            t = tn * tiles_m + tm
            if t < t0:
                return [(0, K)]
            lo = (t - t0) * nk
            marks = sorted({0, nk} | {m * per - lo for m in range(lo // per, (lo + nk) // per + 1) if 0 < m * per - lo < nk})
            return [(a * bk, b * bk) for a, b in zip(marks[:-1], marks[1:])]
        return (bm, bn), cuts
    return (M, N), lambda tm, tn: [(0, K)]


def _c(name, entry, tile, shape, extras="", split_k=1, k_split=0, geglu=False, form="", want=None, note=""):
    return Case(name, entry, tile, split_k, tuple(shape), k_split, extras, geglu, form, want, note)


def table(cus=DEVICE_CUS):
    """Every launch form, at the smallest shapes that reach its edges (tests/test_gpu_edge_guards.py, tests/test_gpu_edge_guards_fused.py): M one row
    over a multiple of the tile's rows, the raggedest N the arm takes, persistent forms one tile more than CUs, the stream-K / hybrid / K-lockstep minima
    from the CU count; where those tables have a single k-tile, a K of several."""
    g8 = cus & ~7
    out = []
    L = "linear_bf16"
    # -- plain epilogue, tiles 1 - 22 (17 has no plain epilogue: it falls back to 16): bias + alpha + one residual, and two residuals
    for t in range(1, 23):
        if t <= 12:
            shp = (257, 328, 320)
        elif t in (13, 14):
            shp = (257, 264, 320)
        elif t == 15:
            shp = (64 * (cus + 1), 320, 320)
        elif t in (16, 17, 18):
            shp = (161, 640, 320)
        else:
            shp = (65, 136, 320 if t in (19, 21) else 64)
        fb1 = {17: "tile 17 is GEGLU only: falls back to tile 16"}.get(t, "")
        fb2 = {15: "two residuals: tile 15 falls back to tile 5", 17: fb1}.get(t, "two residuals: tiles 19 - 22 fall back to tile 1" if t >= 19 else "")
        out.append(_c(f"plain-t{t}-bar", L, t, shp, "bar", note=fb1))
        out.append(_c(f"plain-t{t}-r2", L, t, shp, "r2", note=fb2))
    for t in (13, 14):                                                        # one k-tile: every prefetch of the 8-phase arms is out of range
        out.append(_c(f"plain-t{t}-bar-k64", L, t, (257, 264, 64), "bar"))
    for t in (16, 18):                                                        # one 64-deep k-tile = two sub-tiles of the 160 x 320 ring of five
        out.append(_c(f"plain-t{t}-bar-k64", L, t, (161, 320, 64), "bar"))
        out.append(_c(f"persistent-t{t}-bar", L, t, (160 * (cus + 1), 320, 64), "bar", want=("gemm160p_kernel<0, 5>", "persistent")))
        out.append(_c(f"persistent-t{t}-r2-k192", L, t, (160 * (cus + 1), 320, 192), "r2", want=("gemm160p_kernel<0, 5>", "persistent")))
    out.append(_c("k320-t15-b", L, 15, (64 * (cus + 1), 320, 320), "ba", want=("gemm_k320_kernel<2, 2, false>", "persistent")))
    # -- two-source A operand (13 falls back to 3)
    for t in (1, 3, 5, 11, 13):
        out.append(_c(f"two-source-t{t}", L, t, (257, 328, 320), "bar", k_split=128, note="two-source: tile 13 falls back to tile 3" if t == 13 else ""))
        out.append(_c(f"two-source-t{t}-r2", L, t, (257, 328, 192), "r2", k_split=128))
    # -- split-K: 21 k-tiles of 64 (42 of 32) do not divide by 2 / 4 / 8; tiles 16 / 18: six sub-tiles of 32 in two ranges
    for t, M in ((1, 129), (2, 257), (9, 257)):
        for s in (2, 4, 8):
            out.append(_c(f"split-k{s}-t{t}", L, t, (M, 200, 1344), "bar", split_k=s, want=(ring_name(t), "split-K + splitk_reduce_kernel")))
    for t in (16, 18):
        out.append(_c(f"split-k2-t{t}", L, t, (161, 320, 192), "bar", split_k=2, want=("gemm160_kernel<0, 0>", "split-K + splitk_reduce_kernel")))
    # -- stream-K: the smallest reduction the arm does not hand back to the plain grid (ring: tiles * K / BK >= 4 g; 8-phase: tiles * K / 64 >= 2 g)
    for t in (1, 2, 3, 4, 5):
        bm, bn, bk = ring_tile(t)
        g = (cus * ring_per_cu(t)) & ~7
        Kd = 64 * -(-(-(-4 * g // _tiles(1025, 1032, bm, bn)) * bk) // 64)
        out.append(_c(f"stream-k-t{t}", L, t, (1025, 1032, Kd), "br", split_k=-1, want=(ring_name(t), "stream-K (flags)")))
    for t in (13, 14):
        out.append(_c(f"stream-k-t{t}", L, t, (1025, 1032, 64 * -(-2 * g8 // 25)), "br", split_k=-1,
                      want=(f"gemm8_kernel<EPI 0, PF {t - 9}>", "stream-K (two launches)")))
    rem, tiles_n = g8 // 4, 16                                                # hybrid: more tiles than CUs, the last partial round (64 tiles at 256 CUs) through stream-K
    tiles_m = (g8 + rem) // tiles_n
    assert tiles_m * tiles_n == g8 + rem
    out.append(_c("hybrid-t13", L, 13, (256 * (tiles_m - 1) + 1, 256 * (tiles_n - 1) + 8, 64 * -(-2 * g8 // rem)), "br", split_k=-2,
                  want=("gemm8_kernel<EPI 0, PF 4>", "hybrid: plain grid + stream-K (two launches)")))
    # -- K-lockstep: five k-tiles in S = 2 / 3 / 5 chunks (the last one shorter, or single k-tiles) and 17; -3: S from the cost model
    for S in (2, 3, 5):
        for Kd in (320, 1088):
            out.append(_c(f"k-lockstep-s{S}-k{Kd}", L, 13, (257, 264, Kd), "bar", split_k=-(16 + S),
                          want=("gemm8_kernel<EPI 0, PF 4>", f"k-lockstep S = {S} + sk_finish_kernel")))
    out.append(_c("k-lockstep-model-k1088", L, 13, (257, 264, 1088), "bar", split_k=-3,
                  want=("gemm8_kernel<EPI 0, PF 4>", f"k-lockstep S = {lockstep_chunks(17, 4, g8, 1)} + sk_finish_kernel")))
    # -- GEGLU: 32 + 32 interleave on tiles 1 - 14, [8 value | 8 gate] on 16 / 17 / 18
    for t in range(1, 15):
        out.append(_c(f"geglu-t{t}", L, t, (257, 448, 320), "b", geglu=True))
    out.append(_c("geglu-t13-nobias-k64", L, 13, (257, 448, 64), "", geglu=True))
    for t in (16, 18):
        out.append(_c(f"geglu-t{t}", L, t, (161, 640, 320), "b", geglu=True, want=("gemm160_kernel<0, 1>", "plain grid")))
    for t in (16, 17, 18):
        rows = 256 if t == 17 else 160
        want = ("gemm160p_kernel<1, 8>", "persistent 256 x 320") if t == 17 else ("gemm160p_kernel<1, 5>", "persistent")
        out.append(_c(f"geglu-persistent-t{t}", L, t, (rows * (cus + 1), 320, 64), "b", geglu=True, want=want))
    out.append(_c("geglu-t17-small", L, 17, (257, 640, 64), "", geglu=True, want=("gemm160_kernel<0, 1>", "plain grid"), note="M % 256: tile 17 falls back to tile 16"))
    out.append(_c("geglu-stream-k-t1", L, 1, (1025, 1088, 64 * -(-4 * 2 * cus // 81)), "b", geglu=True, split_k=-1, want=(ring_name(1), "stream-K (flags)")))
    out.append(_c("geglu-k-lockstep-t13", L, 13, (257, 320, 320), "b", geglu=True, split_k=-18,
                  want=("gemm8_kernel<EPI 1, PF 4>", "k-lockstep S = 2 + its finishing launch")))
    # -- the tile-16-only entry points
    for form, shp in (("plain-grid", (320, 640, 64)), ("persistent", (160 * (cus + 2 - cus % 2), 320, 192))):      # (whole images of two tiles)
        for tm in (0, 1):
            want = ("gemm160p_kernel<0, 5>", "persistent") if form == "persistent" else ("gemm160_kernel<0, 0>", "plain grid")
            out.append(_c(f"gn-{form}-tm{tm}", "linear_bf16_gn", 16, shp, "bar2", form="gn_partials" + (" w_tilemajor" if tm else ""), want=want))
    for mode in ("ln_out", "ln_stats"):
        for ex in ("bar", "bar2"):
            out.append(_c(f"ln-{mode}-{ex}", "linear_bf16_ln", 16, (160 * (cus + 1), 320, 64), ex, form=mode + " w_tilemajor",
                          want=("gemm160p_kernel<0, 5, " + ("1>" if mode == "ln_out" else "2>"), "persistent")))
    out.append(_c("lnc-plain", "linear_bf16_lnc", 16, (160 * (cus + 1), 320, 64), "", form="lnc w_tilemajor", want=("gemm160p_kernel<0, 5, 0, 1>", "persistent")))
    out.append(_c("lnc-geglu", "linear_bf16_lnc", 16, (160 * (cus // 2 + 1), 640, 64), "", geglu=True, form="lnc w_tilemajor",
                  want=("gemm160p_kernel<1, 5, 0, 1>", "persistent")))
    out.append(_c("ffblk-x-blocked", "linear_bf16_ffblk", 16, (160 * (cus + 1), 320, 128), "br", form="x_blocked w_tilemajor", want=("gemm160p_kernel<0, 5>", "persistent")))
    out.append(_c("ffblk-x-blocked-alpha", "linear_bf16_ffblk", 16, (160 * g8, 320, 128), "ba", form="x_blocked", want=("gemm160p_kernel<0, 5>", "persistent")))
    out.append(_c("ffblk-out-blocked", "linear_bf16_ffblk", 16, (160 * (cus // 2 + 1), 640, 64), "b", geglu=True, form="out_blocked w_tilemajor",
                  want=("gemm160p_kernel<1, 5>", "persistent")))
    out.append(_c("ffblk-out-blocked-lnc", "linear_bf16_ffblk", 16, (160 * (cus // 2 + 1), 640, 64), "", geglu=True, form="out_blocked lnc w_tilemajor",
                  want=("gemm160p_kernel<1, 5, 0, 1>", "persistent")))
    out.append(_c("ffblk-partial", "linear_bf16_ffblk_partial", 16, (160 * g8 + 1, 320, 128), "bar", form="x_blocked w_tilemajor"))
    for gn in (True, False):
        out.append(_c("fftail-" + ("gn" if gn else "plain"), "linear_bf16_fftail", 16, (160 * (g8 + (1 if gn else 0)), 320, 192), "br", k_split=128,
                      form=("gn_partials " if gn else "") + "w_tilemajor", want=("gemm160p_kernel<0, 5, 0, 0, 1>", "persistent")))
    out.append(_c("fftail-partial", "linear_bf16_fftail_partial", 16, (160 * g8 + 81, 320, 192), "br", k_split=128, form="w_tilemajor"))
    for st in (True, False):
        out.append(_c("gnfold-imgw" + ("-ln-stats" if st else ""), "linear_bf16_imgw", 16, (4 * 160 * (g8 // 4 + (1 if st else 0)), 320, 64), "",
                      form="ln_stats w_tilemajor" if st else "", want=("gemm160p_kernel<0, 5, " + ("2, 0, 0, 1>" if st else "0, 0, 0, 1>"), "persistent")))
    # -- the same entry points at exactly the smallest tile count each accepts, N = 320 (the accepted side of `g160_persistent_shape`'s two comparisons): CUs
    #    tiles where a launch of exactly one round is taken (a tile-major A, per-image weights, the partial forms: ceil), CUs + 1 where more tiles than CUs
    #    are asked.  Above: ln-* and lnc-plain (CUs + 1), ffblk-x-blocked-alpha, fftail-plain and gnfold-imgw (CUs).  fmc_linear_bf16_gn has no smallest
    #    count (the plain grid takes the rest); its images of two tiles put the persistent case at CUs + 2
    P1 = "gemm160p_kernel<1, 5"
    out.append(_c("lnc-geglu-min", "linear_bf16_lnc", 16, (160 * (g8 + 1), 320, 64), "", geglu=True, form="lnc w_tilemajor", want=(P1 + ", 0, 1>", "persistent")))
    out.append(_c("ffblk-out-blocked-min", "linear_bf16_ffblk", 16, (160 * (g8 + 1), 320, 64), "b", geglu=True, form="out_blocked w_tilemajor", want=(P1 + ">", "persistent")))
    out.append(_c("ffblk-out-blocked-lnc-min", "linear_bf16_ffblk", 16, (160 * (g8 + 1), 320, 128), "", geglu=True, form="out_blocked lnc w_tilemajor",
                  want=(P1 + ", 0, 1>", "persistent")))
    out.append(_c("ffblk-partial-min", "linear_bf16_ffblk_partial", 16, (160 * (g8 - 1) + 1, 320, 64), "bar", form="x_blocked w_tilemajor"))
    out.append(_c("fftail-gn-min", "linear_bf16_fftail", 16, (160 * g8, 320, 320), "br", k_split=256, form="gn_partials w_tilemajor",
                  want=("gemm160p_kernel<0, 5, 0, 0, 1>", "persistent")))
    out.append(_c("fftail-partial-min", "linear_bf16_fftail_partial", 16, (160 * (g8 - 1) + 81, 320, 192), "br", k_split=128, form="w_tilemajor"))
    out.append(_c("gnfold-imgw-ln-stats-min", "linear_bf16_imgw", 16, (4 * 160 * (g8 // 4), 320, 64), "", form="ln_stats w_tilemajor",
                  want=("gemm160p_kernel<0, 5, 2, 0, 0, 1>", "persistent")))
    # -- gemm4.hip: 160 x 160 tiles, 0 - 3 extras
    for n, ex in enumerate(("", "b", "bar", "bar2")):
        out.append(_c(f"linear4-extras{n}", "linear4_bf16", 0, (161, 200, 128) if n % 2 else (321, 168, 64), ex))
    # -- fp32 storage (split-bf16 x 3 operands; K is the logical K, the launch runs 3 K)
    for t, s in ((1, 1), (13, 1), (16, 1), (2, 2)):
        out.append(_c(f"x3-f32-t{t}-split{s}", "linear_x3_f32", t, (129, 320 if t == 16 else 72, 64), "bar2", split_k=s))
    # -- the e4m3 q | k | v projection: exact run only
    out.append(_c("fp8-qkv", "linear_fp8_qkv", 13, (257, 192, 128), ""))
    assert len({c.name for c in out}) == len(out)
    return out


CASES = table(DEVICE_CUS)
NAMES = [c.name for c in CASES]


def case(name, cus=DEVICE_CUS):
    return next(c for c in table(cus) if c.name == name)


def is_split_form(c, cus=DEVICE_CUS):
    return any(k in expected_kernel(c, cus)[1] for k in ("split-K", "stream-K", "k-lockstep"))


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------------------------
def interleave(w, b, block):
    """[value rows | gate rows] -> per 2 * block rows `block` value rows, then their gate rows (`synfmc_amd.models.layers.interleave_geglu`)."""
    n, k = w.shape
    wi = w.view(2, n // 2 // block, block, k).permute(1, 0, 2, 3).reshape(n, k).contiguous()
    bi = None if b is None else b.view(2, n // 2 // block, block).permute(1, 0, 2).reshape(n).contiguous()
    return wi, bi


def tilemajor(w):
    """`[N, K]` -> `[N / 320][K / 32][320][32]` (`hip_ops._w_tilemajor`)."""
    n, k = w.shape[-2:]
    return w.reshape(*w.shape[:-2], n // 320, 320, k // 32, 32).transpose(-3, -2).contiguous().view(w.shape)


def blocked(t, pad_value=float("nan")):
    """`[M, C]` -> ceil(M / 160) whole tiles `[C / 32][160][32]`; the pad rows of the last tile hold `pad_value`."""
    M, C = t.shape
    Mp = -(-M // 160) * 160
    full = torch.full((Mp, C), pad_value, dtype=t.dtype)
    full[:M] = t
    return full.view(Mp // 160, 160, C // 32, 32).permute(0, 2, 1, 3).contiguous().view(Mp, C)


def unblocked(t):
    M, C = t.shape
    return t.reshape(M // 160, C // 32, 160, 32).permute(0, 2, 1, 3).reshape(M, C)


def geglu_block(c, cus=DEVICE_CUS):
    """Rows per value / gate block of the weight order the launch wants: 8 on the 160 x 320 kernels, else 32."""
    return 8 if expected_kernel(c, cus)[0].startswith("gemm160") else 32


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return FB._gen("gemm_fwd", *key)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def exact_range(c):
    """(r, density) of the dense integer operands: the largest r whose outputs stay representable -- |alpha P| six standard deviations below 256, or
    below 128 where alpha = 0.5 puts them on the half-integer grid.  `assert_exact_conditions` decides."""
    K = c.shape[2]
    alpha = 0.5 if "a" in c.extras else 1.0
    limit = 120.0 if alpha == 0.5 else 250.0
    for r, var in ((3, 4.0), (2, 2.0), (1, 2.0 / 3.0)):
        if 6.0 * alpha * math.sqrt(K) * var <= limit:
            return r, 1.0
    return 1, min(1.0, (limit / (6.0 * alpha)) ** 2 / (K * (2.0 / 3.0) ** 2))


def _geglu_exact(c, g, M, N, K, lnc):
    """The construction of tests/fused_block_common.py `geglu_inputs` on a plain GEMM: a constant channel (x = 1), three bit channels (x in {1, 3}; {1, 9}
    under `_lnc`) and dense data channels, one of each kind of control channel per quarter of K so that four different k-tiles decide a gate.  A quarter of
    the gate columns are 0 for every row; the others are 10 + sum w_i (bit_i - 1) in {10, 12, 14, 16}.  Values: six data channels with weights +-1 per
    column, |value| <= 14, so value * gate is an integer below 256."""
    cff = N // 2
    q = K // 4
    ctl = torch.stack([torch.randint(i * q, (i + 1) * q, (1,), generator=g)[0] for i in range(4)])
    ctl = ctl[torch.randperm(4, generator=g)]
    one, bits = ctl[0], ctl[1:]
    data = torch.tensor([k for k in range(K) if k not in set(ctl.tolist())])
    x = _ints(g, -2, 2, M, K)
    if lnc:
        x = 2.0 * _ints(g, -1, 1, M, K)
    x[:, one] = 1.0
    x[:, bits] = 1.0 + (8.0 if lnc else 2.0) * _ints(g, 0, 1, M, 3)
    wv = FB._sparse_rows(g, cff, data, 6, [1.0], K)
    wg = torch.zeros(cff, K, dtype=F64)
    zero = torch.arange(cff) % 4 == 1
    if lnc:                                                                   # one bit per gate column, weight +1 on the bit and -1 on the constant: row sum 0
        pick = torch.randint(0, 4, (cff,), generator=g)
        for i in range(3):
            wg[pick == i, bits[i]] = 1.0
        wg[:, one] = -wg[:, bits].sum(-1)
        wg[zero] = 0.0
        bias = torch.cat([_ints(g, -2, 2, cff), torch.where(zero, 0.0, 10.0).to(F64)])
    else:
        wg[:, bits] = _ints(g, 0, 1, cff, 3)
        wg[zero] = 0.0
        if "b" in c.extras:
            bias = torch.cat([FB._nonzero(g, 2, (cff,)), torch.where(zero, -3.0, 4.0).to(F64)])
            wg[:, one] = torch.where(zero, 3.0, 6.0 - wg[:, bits].sum(-1))
        else:
            bias = None
            wg[:, one] = torch.where(zero, 0.0, 10.0 - wg[:, bits].sum(-1))
    return x, torch.cat([wv, wg]), bias


@functools.lru_cache(maxsize=4)
def inputs(c, instrument):
    """CPU tensors of case `c` in LOGICAL layout (GEGLU weights as [value rows | gate rows]); the GPU file packs them as the launch wants.
    instrument: "exact" | "rounding"."""
    M, N, K = c.shape
    g = _gen(c.name, instrument)
    exact = instrument == "exact"
    d = {"alpha": 0.5 if "a" in c.extras else 1.0, "x2": None, "b": None, "r": None, "r2": None}
    lnc = "lnc" in c.form
    n_out = N // 2 if c.geglu else N
    if c.entry == "linear_fp8_qkv":
        # three column blocks with scales 1, 2, 4: weights +-scale at four columns per row, x in [-2, 2]: |acc / scale| <= 8, an integer
        assert exact
        C = N // 3
        w = torch.cat([FB._sparse_rows(g, C, torch.arange(K), 4, [s], K) for s in (1.0, 2.0, 4.0)])
        d.update(x=_ints(g, -2, 2, M, K).to(BF16), w=w.to(BF16), inv_scales=torch.tensor([1.0, 0.5, 0.25]))
        return d
    if c.entry == "linear_x3_f32":
        if exact:
            r, _ = exact_range(c)
            d.update(x=_ints(g, -r, r, M, K).float(), w=_ints(g, -r, r, N, K).float(), b=_ints(g, -2, 2, N).float(), r=_ints(g, -2, 2, M, N).float(),
                     r2=_ints(g, -2, 2, M, N).float())
        else:
            d.update(x=torch.randn(M, K, generator=g), w=torch.randn(N, K, generator=g) * K ** -0.5, b=torch.randn(N, generator=g),
                     r=torch.randn(M, N, generator=g), r2=torch.randn(M, N, generator=g))
        d["alpha"] = 0.5 if exact else 0.7
        return d
    if exact and c.geglu:
        x, w, b = _geglu_exact(c, g, M, N, K, lnc)
    elif exact:
        r, dens = exact_range(c)
        x, w = _ints(g, -r, r, M, K), _ints(g, -r, r, N, K)
        if dens < 1.0:
            w = w * (torch.rand(N, K, generator=g, dtype=F64) < dens)
        b = _ints(g, -2, 2, N) if "b" in c.extras else None
    else:
        x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5
        b = torch.randn(N, generator=g) if ("b" in c.extras or lnc) else None
    if lnc:
        # `ln_stats` is an INPUT of the consumer: integer (even) means and power-of-two rstd in the exact run, the rows' own statistics otherwise;
        # w = W diag(gamma) rounded to bf16, c = its row sums, lb = W beta + b (`hip_ops._ln_folded_weight`)
        if exact:
            mean = 2.0 * _ints(g, -1, 1, M)
            rstd = torch.tensor([0.25, 0.5])[torch.randint(0, 2, (M,), generator=g)].to(F64) if c.geglu else \
                torch.tensor([0.25, 0.5, 1.0])[torch.randint(0, 3, (M,), generator=g)].to(F64)
            if not c.geglu:
                x, w = _ints(g, -2, 2, M, K), _ints(g, -2, 2, N, K)
                b = _ints(g, -2, 2, N)
            wg = w.to(BF16)
            lb = b
        else:
            x = (x + 0.5).to(BF16).to(F64)                                    # (a row mean to cancel in acc - mean c)
            gamma, beta = torch.randn(K, generator=g) * 0.3 + 1.0, torch.randn(K, generator=g) * 0.2
            mean, rstd = x.mean(-1), (x.var(-1, unbiased=False) + LN_EPS).rsqrt()
            wg = (w.float() * gamma[None, :]).to(BF16)
            lb = w.to(BF16).float() @ beta + b.to(BF16).float()
        d.update(x=x.to(BF16), w=wg, ln_stats=torch.stack([mean, rstd], -1).float().contiguous(), ln_c=wg.float().sum(1).contiguous(),
                 ln_bias=lb.float().contiguous())
        return d
    if c.entry == "linear_bf16_imgw":
        # per-image weights.  Rounding: the fold's own inputs (tests/test_gpu_edge_guards_fused.py: group means up to +-6) -- the GPU file runs the fold and
        # hands ITS outputs on; exact: integer weights and fp32 bias rows of our own (the fold's rstd is no power of two)
        n_img, G = 4, 32
        hw = M // n_img
        d.update(n_img=n_img, img_rows=hw, G=G, eps=1e-6)
        if exact:
            r, _ = exact_range(c)
            d.update(x=x.to(BF16), w_img=_ints(g, -r, r, n_img, N, K).to(BF16), bias_img=_ints(g, -8, 8, n_img, N).float())
            return d
        base = torch.randn(n_img, hw, K, generator=g) * (0.5 + torch.rand(n_img, 1, K, generator=g))
        shift = (torch.rand(n_img, 1, G, generator=g) * 12.0 - 6.0).repeat_interleave(K // G, dim=2)
        xb = (base + shift).to(BF16)
        v = xb.float().view(n_img, 4, hw // 4, G, K // G)
        d.update(x=xb.view(M, K), w=w.to(BF16), b=(torch.randn(N, generator=g) * 0.2).to(BF16), gamma=torch.randn(K, generator=g) * 0.3 + 1.0,
                 beta=torch.randn(K, generator=g) * 0.3, partials=torch.stack([v.sum(dim=(2, 4)), (v * v).sum(dim=(2, 4))], dim=-1).contiguous(), splits=4)
        return d
    if c.k_split:
        x, x2 = x[:, :c.k_split].contiguous(), x[:, c.k_split:].contiguous()
        d["x2"] = x2.to(BF16)
    d.update(x=x.to(BF16), w=w.to(BF16), b=None if b is None else b.to(BF16))
    if "ln_" in c.form and c.entry == "linear_bf16_ln":
        frames, inner = 3, 160
        d.update(pe_frames=frames, pe_inner=inner)
        if exact:
            # the rows leaving the GEMM are `c0 +- a` (FB.balanced_rows): residual = target - alpha (x W^T + b) - residual2, an integer
            gamma, beta = FB._nonzero(g, 2, (N,)), FB._offsets(g, (N,))
            pe = 6.0 * _ints(g, -1, 1, frames, N)
            pe[1] = pe[0] + 6.0 * (1 - 2 * (pe[0] > 0).to(F64))               # rows 0 and 1 differ in EVERY channel
            target, _ = FB.balanced_rows(torch.zeros(M, N, dtype=F64), g)
            r2 = _ints(g, -2, 2, M, N) if "2" in c.extras else None
            xa = d["x"].double()
            res = target - d["alpha"] * (xa @ d["w"].double().t() + (0 if b is None else d["b"].double())) - (0 if r2 is None else r2)
            d.update(r=res.to(BF16), r2=None if r2 is None else r2.to(BF16), gamma=gamma.float(), beta=beta.float(), pe=pe.float(), target=target)
            assert bool((d["r"].double() == res).all()), f"{c.name}: the balancing residual is not representable in bf16"
            return d
        d.update(gamma=torch.randn(N, generator=g) * 0.3 + 1.0, beta=torch.randn(N, generator=g) * 0.2, pe=torch.randn(frames, N, generator=g))
    if "r" in c.extras:
        d["r"] = (_ints(g, -2, 2, M, n_out) if exact else torch.randn(M, n_out, generator=g)).to(BF16)
    if "2" in c.extras:
        d["r2"] = (_ints(g, -2, 2, M, n_out) if exact else torch.randn(M, n_out, generator=g)).to(BF16)
    return d


# ---- the float64 reference ------------------------------------------------------------------------------------------------------------------------------
def _xa(d):
    return d["x"] if d.get("x2") is None else torch.cat([d["x"], d["x2"]], -1)


def gelu64(g):
    return F.gelu(g)


def compose_geglu(y, m):
    """(ref, mag, extra) of value * gelu(gate) from the float64 pre-activations `y` and their sum|terms| `m` ([.., value | gate]): one rounding of the
    product (2^-8 |ref|, in assert_bf16_close) + the fp32 accumulation of value and gate (1e-5 mag: |gelu(g)| mag_v + GELU_SLOPE |v| mag_g) + |value| times
    the GELU evaluation error (GELU_ABS + GELU_HW_REL |g|) + four fp32 roundings of the bias adds and the product."""
    (v, g), (mv, mg) = y.chunk(2, -1), m.chunk(2, -1)
    ref = v * gelu64(g)
    return ref, gelu64(g).abs() * mv + GELU_SLOPE * v.abs() * mg, v.abs() * (GELU_ABS + GELU_HW_REL * g.abs()) + 4 * 2.0 ** -24 * ref.abs()


def reference(c, d):
    """float64 on the operands as stored -> dict(ref, mag, extra or None [, pre: the pre-activations of a GEGLU launch]).  `mag` = sum|terms| with every
    epilogue addend."""
    if c.entry == "linear_bf16_imgw":
        n_img, hw = d["n_img"], d["img_rows"]
        x = d["x"].double().view(n_img, hw, -1)
        ref = torch.einsum("imc,inc->imn", x, d["w_img"].double()) + d["bias_img"].double()[:, None, :]
        mag = torch.einsum("imc,inc->imn", x.abs(), d["w_img"].double().abs()) + d["bias_img"].double().abs()[:, None, :]
        return {"ref": ref.reshape(n_img * hw, -1), "mag": mag.reshape(n_img * hw, -1), "extra": None}
    xa, w = _xa(d).double(), d["w"].double()
    P, Pm = xa @ w.t(), xa.abs() @ w.abs().t()
    if c.entry == "linear_fp8_qkv":
        return {"ref": P, "mag": Pm, "extra": None}
    if "lnc" in c.form:
        mean, rstd = d["ln_stats"].double()[:, :1], d["ln_stats"].double()[:, 1:]
        cc, lb = d["ln_c"].double(), d["ln_bias"].double()
        y, m = rstd * (P - mean * cc) + lb, rstd * (Pm + (mean * cc).abs()) + lb.abs()
    else:
        b = 0.0 if d["b"] is None else d["b"].double()
        y, m = d["alpha"] * (P + b), abs(d["alpha"]) * (Pm + (0.0 if d["b"] is None else d["b"].double().abs()))
    if c.geglu:
        ref, mag, extra = compose_geglu(y, m)
        return {"ref": ref, "mag": mag, "extra": extra, "pre": y}
    for t in (d["r"], d["r2"]):
        if t is not None:
            y, m = y + t.double(), m + t.double().abs()
    return {"ref": y, "mag": m, "extra": None}


def ln_reference(out, d, M):
    """float64 LayerNorm (+ the positional row of the tile's frame) of the kernel's OWN bf16 rows `out` -> (ref, mag, extra): one rounding, four fp32
    roundings of `(x - m) * rs * g + b` (inside 1e-5 mag) and the statistics term |gamma| rstd (dm + |x - mean| drstd) from the counted LN_*_REL."""
    o = out.detach().double().cpu()
    mean, var = o.mean(-1, keepdim=True), o.var(-1, unbiased=False, keepdim=True)
    rstd = (var + LN_EPS).rsqrt()
    rows = (torch.arange(M) // d["pe_inner"]) % d["pe_frames"]
    g, bpe = d["gamma"].double(), d["beta"].double() + d["pe"].double()[rows]
    core = (o - mean) * rstd * g
    dm = LN_MEAN_REL * o.abs().mean(-1, keepdim=True)
    extra = g.abs() * rstd * (dm + (o - mean).abs() * (LN_RSTD_REL + 0.5 * dm * dm * rstd * rstd))
    return core + bpe, core.abs() + bpe.abs(), extra


def ln_stats_shares(stats, out, eps=LN_EPS):
    """(worst mean error, worst rstd error) of `ln_stats [M, 2]` in units of their counted bounds, against the float64 statistics of `out`'s rows."""
    o = out.detach().double().cpu()
    mean = o.mean(-1)
    rstd = (((o - mean[:, None]) ** 2).mean(-1) + eps).rsqrt()
    s = stats.detach().double().cpu().reshape(-1, 2)
    dm = LN_MEAN_REL * o.abs().mean(-1)
    e_mean = ((s[:, 0] - mean).abs() / dm.clamp_min(1e-300)).max()
    e_rstd = ((s[:, 1] - rstd).abs() / (rstd * (LN_RSTD_REL + 0.5 * dm * dm * rstd * rstd))).max()
    return float(e_mean), float(e_rstd)


def check_ln_stats(stats, out, what=""):
    e_mean, e_rstd = ln_stats_shares(stats, out)
    print(f"   {what}: ln_stats mean {e_mean:.3f} of {LN_MEAN_CHAIN} x 2^-24 mean|x|, rstd {e_rstd:.3f} of {LN_RSTD_CHAIN} x 2^-24 (+ the mean's share)")
    assert e_mean <= 1.0 and e_rstd <= 1.0, f"{what}: ln_stats beyond the counted bounds: mean {e_mean:.3f}, rstd {e_rstd:.3f}"
    return max(e_mean, e_rstd)


def gn_hw(c):
    """Rows per image of a launch that writes gn_partials: two 160-row tiles per image under fmc_linear_bf16_gn (so that slots can be told apart from
    their sum), one under fmc_linear_bf16_fftail (CUs + 1 tiles)."""
    return 320 if c.entry == "linear_bf16_gn" else 160


def gn_tile_stats(out, hw):
    """out `[M, N]` bf16 -> (partials `[M / hw][hw / 160][32][2]` = (sum, sum of squares) per image, 160-row tile and group of N / 32 channels in
    float64, the same sums over the absolute values)."""
    M, N = out.shape
    o = out.detach().double().cpu().view(M // hw, hw // 160, 160, 32, N // 32)
    want = torch.stack([o.sum((2, 4)), (o * o).sum((2, 4))], -1)
    return want, torch.stack([o.abs().sum((2, 4)), (o * o).sum((2, 4))], -1)


def check_gn_partials(parts, out, hw, exact, what=""):
    want, mag = gn_tile_stats(out, hw)
    got = parts.detach().double().cpu().reshape(want.shape)
    if exact:
        assert float(want[..., 1].max()) < 2.0 ** 24
        check_exact(got, want, what + " gn_partials")
        return 0.0
    err, bound = (got - want).abs(), STATS_REL * mag
    bad = ~(err <= bound)
    assert not bool(bad.any()), (f"{what} gn_partials: {int(bad.sum())} / {bad.numel()} entries beyond {STATS_REL:.2e} * sum|addends|, first at "
                                 f"(image, tile, group, which) {tuple(bad.nonzero()[0].tolist())}")
    return float((err / bound.clamp_min(1e-300)).max())


def fold_reference(d, N, K):
    """float64 of fmc_groupnorm_fold_linear from the same partials -> (w_ref [n_img, N, K], a [n_img, K], mean [n_img, K])."""
    n_img, G, hw = d["n_img"], d["G"], d["img_rows"]
    s = d["partials"].double().sum(1)
    cnt = hw * (K // G)
    mean = s[..., 0] / cnt
    rstd = 1.0 / torch.sqrt((s[..., 1] / cnt - mean * mean).clamp_min(0) + d["eps"])
    a = rstd.repeat_interleave(K // G, 1) * d["gamma"].double()[None, :]
    return d["w"].double()[None] * a[:, None, :], a, mean.repeat_interleave(K // G, 1)


def check_fold(w_out, bias_out, d, N, K, what=""):
    """w_out element-wise against float64 `W diag(rstd gamma)`: one bf16 rounding + FOLD_W_CHAIN half-ulps of fp32; bias_out against float64 from the
    kernel's OWN rounded w_out (the header's contract) under `fold_bias_chain`.  Returns the two largest shares."""
    w_ref, _, mean = fold_reference(d, N, K)
    w_got = w_out.detach().double().cpu().view(w_ref.shape)
    e_w = (w_got - w_ref).abs() / ((2.0 ** -8 + FOLD_W_CHAIN * 2.0 ** -24) * w_ref.abs()).clamp_min(1e-300)
    assert float(e_w.max()) <= 1.0, f"{what}: w_out beyond one bf16 rounding + {FOLD_W_CHAIN} x 2^-24, worst {float(e_w.max()):.3f} at {tuple(int(i) for i in (e_w == e_w.max()).nonzero()[0])}"
    terms_b, terms_m = d["w"].double()[None] * d["beta"].double()[None, None, :], w_got * mean[:, None, :]
    b_ref = (terms_b - terms_m).sum(-1) + d["b"].double()[None, :]
    b_mag = (terms_b.abs() + terms_m.abs()).sum(-1) + d["b"].double().abs()[None, :]
    e_b = (bias_out.detach().double().cpu().view(b_ref.shape) - b_ref).abs() / (fold_bias_chain(K) * 2.0 ** -24 * b_mag).clamp_min(1e-300)
    assert float(e_b.max()) <= 1.0, f"{what}: bias_out beyond {fold_bias_chain(K)} x 2^-24 sum|addends|, worst {float(e_b.max()):.3f}"
    return float(e_w.max()), float(e_b.max())


def emulate_fold(d, N, K, tm=False):
    """gn_fold_linear_kernel in plain torch: statistics in float64 rounded to fp32, `bf16(w * (rstd * gamma))`, the bias from the ROUNDED weight in fp32."""
    G, hw = d["G"], d["img_rows"]
    s = d["partials"].double().sum(1)
    cnt = hw * (K // G)
    mean = s[..., 0] / cnt
    rstd = (1.0 / torch.sqrt((s[..., 1] / cnt - mean * mean).clamp_min(0) + float(torch.tensor(d["eps"], dtype=F32)))).float()
    mean = mean.float().repeat_interleave(K // G, 1)
    a = rstd.repeat_interleave(K // G, 1) * d["gamma"][None, :]
    wr = (d["w"].float()[None] * a[:, None, :]).to(BF16)
    bias = (d["w"].float()[None] * d["beta"][None, None, :] - wr.float() * mean[:, None, :]).sum(-1) + d["b"].float()[None, :]
    return wr, bias


def with_fold(d, w_out, bias_out):
    """The inputs of the imgw launch of a rounding run: the fold's own outputs (row-major here)."""
    return dict(d, w_img=w_out.detach().cpu(), bias_img=bias_out.detach().cpu())


def fp8_reference(d, N):
    """(e4m3 bytes, amax per block) of the exact q | k | v run."""
    acc = _xa(d).double() @ d["w"].double().t()
    C = N // 3
    scaled = acc * d["inv_scales"].double().repeat_interleave(C)[None, :]
    assert bool((scaled == scaled.round()).all()) and float(scaled.abs().max()) <= 16
    return scaled.float().to(torch.float8_e4m3fn).view(torch.uint8), acc.abs().view(-1, 3, C).amax((0, 2)).float()


def is_bf16(t):
    return bool((t.float().to(BF16).double() == t.double()).all())


def assert_exact_conditions(c, d, r):
    """What the exact instrument rests on, asserted on the float64 reference: sum|terms| < 2^24 (every partial sum in any order is exact in fp32) and
    every value a kernel rounds is representable in bf16 (fp32 storage: an integer or half-integer below 2^24)."""
    what = c.name
    assert float(r["mag"].max()) < 2.0 ** 24, f"{what}: sum|terms| reaches {float(r['mag'].max())}"
    if c.entry == "linear_x3_f32":
        assert bool((2 * r["ref"] == (2 * r["ref"]).round()).all())
        for k in ("x", "w"):
            assert is_bf16(d[k]), f"{what}: {k} has a low part"
        return
    if c.entry == "linear_fp8_qkv":
        fp8_reference(d, c.shape[1])
        return
    assert is_bf16(r["ref"]), f"{what}: {int((r['ref'].float().to(BF16).double() != r['ref']).sum())} outputs are not representable in bf16 (max |v| {float(r['ref'].abs().max())})"
    if c.geglu:
        v, gate = r["pre"].chunk(2, -1)
        assert bool(((gate == 0) | ((gate >= 10) & (gate <= 16) & (gate == gate.round()))).all()), what
        assert bool((gate == 0).any()) and len(gate[gate > 0].unique()) >= 2, what
        ints = torch.arange(10, 17, dtype=F32)
        assert torch.equal(FB.gelu_fast_f32(ints), ints) and float(FB.gelu_fast_f32(torch.zeros(1))) == 0.0      # the fp32 restatement of fmc_gelu_fast
        assert float(v.abs().max()) < 16 and bool((4 * v == (4 * v).round()).all()), what
    if "gn_partials" in c.form:
        assert float(gn_tile_stats(r["ref"].to(BF16), gn_hw(c))[0][..., 1].max()) < 2.0 ** 24, what
    if c.entry == "linear_bf16_ln":
        # the LayerNorm output: within 1e-5 |gamma| (+ fp32 slack) of a nonzero integer below 256, far from every rounding tie
        assert bool((r["ref"] == d["target"]).all()), what
        pre, _, _ = ln_reference(r["ref"].to(BF16), d, c.shape[0])
        assert float((pre - pre.round()).abs().max()) < 1e-4 and float(pre.round().abs().min()) >= 1 and float(pre.abs().max()) < 256, what
        assert float(FB.ln_tie_distance(pre).min()) > 0.49, what


# ---- the fp32 emulation of the documented rounding chains (plain torch, CPU) and the wrong stand-ins ---------------------------------------------------
FAULTS = {  # name: (what it is, does the gate `rel_inf < 1e-2` pass it on the gap data -- filled in by the CPU file, recorded in the profile)
    "truncate": "the output truncated to bf16 instead of rounded",
    "partial_bf16": "a stream-K / K-lockstep partial held in bf16",
    "splitk_partial_bf16": "a split-K partial rounded to bf16",
    "ragged_chunk": "the ragged last k-chunk counted twice and the chunk before it dropped",
    "segment_twice": "a stream-K segment (the last of its tile) summed twice",
    "bias_plus8": "the bias of column n + 8 in the ragged column tail",
    "pad_residual": "a pad row's residual added to the last valid row",
    "seam_off": "the two-source seam one k-tile off (the first k-tile of x2 never read)",
    "alpha_after_residual": "alpha applied after the residual",
    "geglu_swap16": "value and gate swapped inside one 16-row group of the weight order",
    "pe_next_frame": "the positional row of the next frame in the _ln epilogue",
    "gn_slots_swapped": "the gn_partials slots of two tiles of one image exchanged",
    "tilemajor_subtiles": "two 32-deep sub-tiles of the tile-major weight exchanged",
}
GAP = 2.0 ** -7                       # the scale of the affected operand part in the gap data (`gap_inputs`)


def applies(fault, c, cus=DEVICE_CUS):
    kernel, form = expected_kernel(c, cus)
    M, N, K = c.shape
    plain = not c.geglu and c.entry not in ("linear_fp8_qkv", "linear_x3_f32") and "lnc" not in c.form and c.entry != "linear_bf16_imgw"
    if c.entry == "linear_fp8_qkv":
        return False
    return {
        "truncate": c.entry != "linear_x3_f32",
        "partial_bf16": "stream-K" in form or "k-lockstep" in form,
        "splitk_partial_bf16": "split-K" in form and c.entry != "linear_x3_f32",
        "ragged_chunk": ("split-K" in form or "k-lockstep" in form) and c.entry != "linear_x3_f32",      # (the fp32-storage emulation has no cuts)
        "segment_twice": "stream-K" in form,
        "bias_plus8": plain and "b" in c.extras and N % 64 != 0,
        "pad_residual": plain and "r" in c.extras and M % 32 != 0,
        "seam_off": c.k_split > 0,
        "alpha_after_residual": plain and "a" in c.extras and "r" in c.extras,
        "geglu_swap16": c.geglu and "lnc" not in c.form,
        "pe_next_frame": "ln_out" in c.form,
        "gn_slots_swapped": "gn_partials" in c.form and gn_hw(c) >= 320,
        "tilemajor_subtiles": (c.tile == 18 or "w_tilemajor" in c.form) and K >= 64 and c.entry != "linear_bf16_imgw",
    }[fault]


def gap_inputs(c, fault):
    """The rounding inputs with the operand part the fault touches scaled by GAP = 2^-7: the faulty output then stays within 1e-2 of the tensor maximum --
    the gate the suite had -- while the affected elements leave their own bound."""
    d = dict(inputs(c, "rounding"))
    M, N, K = c.shape
    sc = lambda t: (t.float() * GAP).to(t.dtype)
    if fault == "bias_plus8":
        d["b"] = d["b"].clone()
        d["b"][N - 16:] = sc(d["b"][N - 16:])
    elif fault in ("pad_residual", "alpha_after_residual"):
        d["r"] = sc(d["r"])
        d["pad_row"] = sc(torch.randn(d["r"].shape[1], generator=_gen("pad", c.name)).to(BF16))
    elif fault == "seam_off":
        d["x2"] = d["x2"].clone()
        d["x2"][:, :64] = sc(d["x2"][:, :64])
    elif fault in ("ragged_chunk", "segment_twice"):
        d["x"] = sc(d["x"])                                                   # every product is small against bias and residual
    elif fault == "geglu_swap16":
        cff = N // 2
        d["w"], d["b"] = d["w"].clone(), None if d["b"] is None else d["b"].clone()
        d["w"][:8] = sc(d["w"][:8])                                           # the value rows of output columns 0 .. 7
        if d["b"] is not None:
            d["b"][:8] = sc(d["b"][:8])
    elif fault == "pe_next_frame":
        d["pe"] = d["pe"] * GAP
    elif fault == "tilemajor_subtiles":
        d["x"] = d["x"].clone()
        d["x"][:, :64] = sc(d["x"][:, :64])
    return d


def _product32(c, d, cus, fault):
    """x W^T in fp32 with the launch's cuts of the reduction: one fp32 partial per chunk, summed in chunk order."""
    xa, w = _xa(d).float(), d["w"].float()
    M, N, K = c.shape
    if fault == "seam_off":
        xa = xa.clone()
        xa[:, c.k_split:c.k_split + 64] = 0.0
    if fault == "tilemajor_subtiles":                                         # sub-tiles 0 and 1 of every 320-row block change places: W's columns [0, 32) <-> [32, 64)
        w = torch.cat([w[:, 32:64], w[:, :32], w[:, 64:]], 1)
    kernel, form = expected_kernel(c, cus)
    (bm, bn), cuts = k_cuts(c, cus, kernel, form)
    if (bm, bn) == (M, N) and len(cuts(0, 0)) == 1:
        return xa @ w.t()
    out = torch.empty(M, N)
    for tm in range(-(-M // bm)):
        for tn in range(-(-N // bn)):
            chunks = list(cuts(tm, tn))
            if fault == "ragged_chunk" and len(chunks) >= 2:
                chunks = chunks[:-2] + [chunks[-1], chunks[-1]]
            if fault == "segment_twice" and len(chunks) >= 2:
                chunks = chunks + [chunks[-1]]
            xs, ws = xa[tm * bm:(tm + 1) * bm], w[tn * bn:(tn + 1) * bn]
            acc = None
            for k0, k1 in chunks:
                p = xs[:, k0:k1] @ ws[:, k0:k1].t()
                if fault in ("partial_bf16", "splitk_partial_bf16") and len(chunks) >= 2:
                    p = p.to(BF16).float()
                acc = p if acc is None else acc + p
            out[tm * bm:(tm + 1) * bm, tn * bn:(tn + 1) * bn] = acc
    return out


def emulate(c, d, cus=DEVICE_CUS, fault=None):
    """What the kernels document, in plain torch: products of bf16 values summed in fp32 (per chunk of a split form, the chunks then in order); (acc + bias)
    * alpha, then the residuals, in fp32; ONE rounding to bf16.  Tile 15 puts the bias into the accumulator first (the same fp32 expression).  GEGLU: (value
    + bias) * fmc_gelu_fast(gate + bias) in fp32, one rounding.  `_lnc`: rstd * (acc - mean * c) + ln_bias.  `_ln`: two-pass fp32 statistics of the ROUNDED
    rows, `(x - m) * rs * g + (beta + pe)`, one rounding.  gn_partials: fp32 sums of the rounded outputs.  fp32 storage: three split products in fp32.
    -> dict of what the launch writes."""
    M, N, K = c.shape
    rnd = truncate_bf16 if fault == "truncate" else (lambda t: t.to(BF16))
    res = {}
    if c.entry == "linear_x3_f32":
        x, w = d["x"], d["w"]
        xh, wh = x.to(BF16).float(), w.to(BF16).float()
        xl, wl = (x - xh).to(BF16).float(), (w - wh).to(BF16).float()
        y = xh @ wh.t() + (xh @ wl.t() + xl @ wh.t())
        y = (y + d["b"]) * torch.tensor(d["alpha"], dtype=F32) + d["r"] + d["r2"]
        return {"out": y}
    if c.entry == "linear_bf16_imgw":
        n_img, hw = d["n_img"], d["img_rows"]
        y = torch.einsum("imc,inc->imn", d["x"].float().view(n_img, hw, K), d["w_img"].float()) + d["bias_img"][:, None, :]
        res["out"] = rnd(y.reshape(M, N))
        if "ln_stats" in c.form:
            res["ln_stats"] = _ln_stats32(res["out"])
        return res
    acc = _product32(c, d, cus, fault)
    if c.entry == "linear_fp8_qkv":
        y = acc * d["inv_scales"].repeat_interleave(N // 3)[None, :]
        return {"out": y.to(torch.float8_e4m3fn).view(torch.uint8), "amax": acc.abs().view(M, 3, N // 3).amax((0, 2))}
    if "lnc" in c.form:
        y = d["ln_stats"][:, 1:] * (acc - d["ln_stats"][:, :1] * d["ln_c"]) + d["ln_bias"]
    else:
        b = d["b"]
        if fault == "bias_plus8" and b is not None:
            b = b.clone()
            b[N - 16:N - 8] = d["b"][N - 8:]
        y = acc if b is None else acc + b.float()
        if not c.geglu:
            r = d["r"]
            if fault == "alpha_after_residual":
                y, r = y + r.float(), None
            y = y * torch.tensor(d["alpha"], dtype=F32)
            for t in (r, d["r2"]):
                if t is not None:
                    y = y + t.float()
            if fault == "pad_residual":
                pad = d["pad_row"] if "pad_row" in d else torch.ones(y.shape[1], dtype=BF16)
                y[M - 1] = y[M - 1] + pad.float()
    if c.geglu:
        v, g = y.chunk(2, -1)
        if fault == "geglu_swap16":
            v, g = v.clone(), g.clone()
            v[:, :8], g[:, :8] = y.chunk(2, -1)[1][:, :8], y.chunk(2, -1)[0][:, :8]
        y = v * FB.gelu_fast_f32(g)
    res["out"] = rnd(y)
    if "gn_partials" in c.form:
        hw = gn_hw(c)
        o = res["out"].float().view(M // hw, hw // 160, 160, 32, N // 32)
        res["gn_partials"] = torch.stack([o.sum((2, 4)), (o * o).sum((2, 4))], -1)
        if fault == "gn_slots_swapped":                                       # the two tiles of the last image
            res["gn_partials"][-1] = res["gn_partials"][-1].flip(0)
    if c.entry == "linear_bf16_ln":
        st = _ln_stats32(res["out"])
        if "ln_stats" in c.form:
            res["ln_stats"] = st
        else:
            rows = (torch.arange(M) // d["pe_inner"] + (1 if fault == "pe_next_frame" else 0)) % d["pe_frames"]
            o = res["out"].float()
            res["ln_out"] = rnd((o - st[:, :1]) * st[:, 1:] * d["gamma"].float() + (d["beta"].float() + d["pe"].float()[rows]))
    return res


def _ln_stats32(out):
    """gemm160p_kernel's two-pass row statistics in fp32 (the rounded constant 1.f / 320.f, centred variance)."""
    o = out.float()
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(o.shape[-1]), dtype=F32)
    mean = o.sum(-1, keepdim=True) * inv
    dl = o - mean
    return torch.cat([mean, torch.rsqrt((dl * dl).sum(-1, keepdim=True) * inv + torch.tensor(LN_EPS, dtype=F32))], -1)


# ---- the two instruments, as both files apply them ---------------------------------------------------------------------------------------------------------
def check(c, d, got, instrument, what=None):
    """Every assertion of one launch: `got` = dict of what it wrote (CPU or GPU tensors), `d` its inputs.  Returns {name: largest err / bound}."""
    what = what or f"{c.name} [{instrument}]"
    M, N, K = c.shape
    exact = instrument == "exact"
    shares = {}
    for k, v in got.items():
        if v.dtype.is_floating_point:
            assert bool(torch.isfinite(v.float()).all()), f"{what}: {k} has {int((~torch.isfinite(v.float())).sum())} unwritten or non-finite elements"
    if c.entry == "linear_fp8_qkv":
        want, amax = fp8_reference(d, N)
        check_exact(got["out"].cpu().to(torch.int32), want.to(torch.int32), what + " e4m3 bytes")
        if "amax" in got:
            check_exact(got["amax"].cpu(), amax, what + " amax")
        return shares
    r = reference(c, d)
    out = got["out"].detach().cpu()
    if exact:
        assert_exact_conditions(c, d, r)
        check_exact(out, r["ref"].float() if c.entry == "linear_x3_f32" else r["ref"].to(BF16), what)
    elif c.entry == "linear_x3_f32":
        shares["out"] = assert_f32_close(out, r["ref"], r["mag"], what)
    else:
        shares["out"] = assert_bf16_close(out, r["ref"], r["mag"], what, extra=r["extra"])
    if "gn_partials" in got:
        shares["gn_partials"] = check_gn_partials(got["gn_partials"], out, gn_hw(c), exact, what)
    if "ln_stats" in got:
        shares["ln_stats"] = check_ln_stats(got["ln_stats"], out, what)
    if "ln_out" in got:
        ref, mag, extra = ln_reference(out, d, M)
        if exact:
            check_exact(got["ln_out"].detach().cpu(), ref.round().to(BF16), what + " ln_out")
        else:
            shares["ln_out"] = assert_bf16_close(got["ln_out"], ref, mag, what + " ln_out", extra=extra)
    return shares


def old_gate(c, d, got):
    """The gate the suite had for most arms: rel_inf(got, ref) < 1e-2, relative to the largest element of the tensor (side outputs: the same)."""
    r = reference(c, d)
    ok = rel_inf(got["out"].float(), r["ref"]) < 1e-2
    if "ln_out" in got:
        ok = ok and rel_inf(got["ln_out"].float(), ln_reference(got["out"], d, c.shape[0])[0]) < 1e-2
    if "gn_partials" in got:
        want, _ = gn_tile_stats(got["out"], gn_hw(c))                         # (the old gate: the sum over an image's tiles, 1e-4)
        ok = ok and rel_inf(got["gn_partials"].double().reshape(want.shape).sum(1), want.sum(1)) < 1e-4
    return ok

"""The host surface of the token GEMMs and the 3x3 GEMM convolutions as data (tools/record_gemm_host_surface.py writes it to
tests/golden/gemm_host_surface.json, tests/test_gemm_host_surface.py asserts that the tree reproduces the file): the (return code, message) of refused
calls to the fourteen entry points of csrc/gemm_conv.hip, what the Python predicates of the tile-16 forms return over a row-count axis, and what
`linear()` / `geglu_linear()` hand to recording stand-ins at the shipped shapes.  Nothing here launches: every recorded call breaks at least one argument
check (pointers are made-up integers), the predicates and routes see storage-less tensors.

Without a GPU the library counts 256 CUs (`fmc_cu_count`'s fall-back), so the tile-count clauses of the persistent form sit at 255 / 256 / 257 tiles."""
import itertools

import torch

from tests import fake_kernels
from tests.fused_host_surface_common import REFUSALS, claims_gpu, tensor  # noqa: F401  (REFUSALS: re-exported to the recorder and the test)
from tests.halo_host_surface_common import _Table, rle, same_table, unrle  # noqa: F401  (same_table, unrle: re-exported to the test)

BF16, F32 = torch.bfloat16, torch.float32
CUS = 256                                           # what the library sees on a host without a GPU

# ---- 1. errors ----------------------------------------------------------------------------------------------------------------------------------------
X, W, BIAS, RES, OUT, WS, X2, RES2, GNP, LNO, GAMMA, BETA, PE, STATS, LNC, LNB, BIMG, TEMB, INV, AMAX = (0x10000 * k for k in range(1, 21))
_LIN = ("x", "w", "bias", "residual", "out", "M", "N", "K", "ldx", "ldres", "ldo", "alpha")
_CONV = ("x", "w", "bias", "temb", "residual", "out", "n_img", "H", "Wd", "Cin", "Cout", "temb_row_stride", "temb_img_div", "upsample2x")
SIGS = {
    "fmc_linear_bf16": _LIN + ("epilogue", "tile", "split_k", "workspace", "workspace_bytes", "x2", "ldx2", "k_split", "residual2", "stream"),
    "fmc_linear_bf16_gn": _LIN + ("residual2", "gn_partials", "gn_hw", "w_tilemajor", "stream"),
    "fmc_linear_bf16_ln": _LIN + ("residual2", "ln_out", "ln_gamma", "ln_beta", "ln_eps", "ln_pe", "ln_pe_inner", "ln_pe_frames", "ln_stats", "w_tilemajor", "stream"),
    "fmc_linear_bf16_lnc": ("x", "w", "out", "M", "N", "K", "ldx", "ldo", "epilogue", "lnc_stats", "ln_c", "ln_bias", "w_tilemajor", "stream"),
    "fmc_linear_bf16_ffblk": ("x", "w", "bias", "residual", "out", "M", "N", "K", "ldres", "alpha", "epilogue", "x_blocked", "out_blocked", "lnc_stats", "ln_c",
                              "ln_bias", "w_tilemajor", "stream"),
    "fmc_linear_bf16_imgw": ("x", "w", "bias_img", "out", "M", "N", "K", "ldx", "ldo", "img_rows", "ln_stats", "ln_eps", "w_tilemajor", "stream"),
    "fmc_linear_bf16_fftail": ("x", "x2", "w", "bias", "residual", "out", "M", "N", "K", "k_split", "ldx2", "ldres", "gn_partials", "gn_hw", "w_tilemajor", "stream"),
    "fmc_linear_x3_f32": _LIN + ("epilogue", "tile", "split_k", "workspace", "workspace_bytes", "residual2", "stream"),
    "fmc_linear_bf16_ffblk_partial": ("x", "w", "bias", "residual", "out", "M", "N", "K", "ldres", "alpha", "w_tilemajor", "stream"),
    "fmc_linear_bf16_fftail_partial": ("x", "x2", "w", "bias", "residual", "out", "M", "N", "K", "k_split", "ldx2", "ldres", "gn_partials", "gn_hw", "w_tilemajor",
                                       "stream"),
    "fmc_conv3x3_bf16": _CONV + ("tile", "split_k", "workspace", "workspace_bytes", "stream"),
    "fmc_conv3x3_bf16_gn": _CONV + ("gn_partials", "w_tilemajor", "stream"),
    "fmc_conv3x3_x3_f32": _CONV + ("tile", "split_k", "workspace", "workspace_bytes", "stream"),
    "fmc_linear_fp8_qkv": ("x", "w", "out", "M", "N", "K", "ldx", "inv_scales", "amax_bits", "stream"),
}
M_MORE, M_SAME, M_LESS = 160 * (CUS + 1), 160 * CUS, 160 * (CUS - 1)          # N = 320: one tile per 160 rows
_COMMON = dict(x=X, w=W, bias=None, residual=None, out=OUT, N=320, K=64, ldx=64, ldres=0, ldo=320, alpha=1.0, epilogue=0, tile=0, split_k=1, workspace=None,
               workspace_bytes=0, x2=None, ldx2=0, k_split=0, residual2=None, stream=None, w_tilemajor=0, gn_partials=None, gn_hw=0, ln_out=None, ln_gamma=None,
               ln_beta=None, ln_eps=1e-5, ln_pe=None, ln_pe_inner=1, ln_pe_frames=1, ln_stats=None, lnc_stats=None, ln_c=None, ln_bias=None, x_blocked=0,
               out_blocked=0, bias_img=None, img_rows=0, temb=None, n_img=1, H=16, Wd=10, Cin=64, Cout=320, temb_row_stride=0, temb_img_div=1, upsample2x=0,
               inv_scales=INV, amax_bits=AMAX)
# per entry point: a call that every argument check accepts (never made: each recorded row changes it into a refused one)
BASES = {
    "fmc_linear_bf16": dict(M=320),
    "fmc_linear_bf16_gn": dict(M=320, gn_partials=GNP, gn_hw=160),
    "fmc_linear_bf16_ln": dict(M=M_MORE, ln_out=LNO, ln_gamma=GAMMA, ln_beta=BETA),
    "fmc_linear_bf16_lnc": dict(M=M_MORE, lnc_stats=STATS, ln_c=LNC, ln_bias=LNB),
    "fmc_linear_bf16_ffblk": dict(M=M_SAME, x_blocked=1),
    "fmc_linear_bf16_imgw": dict(M=M_SAME, bias_img=BIMG, img_rows=160),
    "fmc_linear_bf16_fftail": dict(M=M_SAME, K=128, k_split=64, ldx2=64, x2=X2, residual=RES, ldres=320),
    "fmc_linear_x3_f32": dict(M=320, K=192, ldx=192),
    "fmc_linear_bf16_ffblk_partial": dict(M=M_LESS + 1),
    "fmc_linear_bf16_fftail_partial": dict(M=M_LESS + 1, K=128, k_split=64, ldx2=64, x2=X2, residual=RES, ldres=320),
    "fmc_conv3x3_bf16": {}, "fmc_conv3x3_bf16_gn": dict(gn_partials=GNP), "fmc_conv3x3_x3_f32": dict(Cin=192),
    "fmc_linear_fp8_qkv": dict(M=256, N=192, inv_scales=INV),
}
# rows past 2 GiB at K = 1280 (dense rows): 838 880 = 160 * 5243 is the first multiple of 160 whose M * 1280 * 2 bytes reach 2^31; weights past 2 GiB
BIG_A = dict(M=838880, K=1280, ldx=1280)
BIG_W = dict(N=327680, K=3328, ldx=3328, ldo=327680)
_PTRS = ("x", "w", "out", "bias", "residual", "residual2", "x2", "temb", "gn_partials", "ln_out", "ln_gamma", "ln_beta", "ln_pe", "ln_stats", "lnc_stats", "ln_c",
         "ln_bias", "bias_img", "workspace", "inv_scales", "amax_bits")
_VALUE = dict(x=X, w=W, out=OUT, bias=BIAS, residual=RES, residual2=RES2, x2=X2, temb=TEMB, gn_partials=GNP, ln_out=LNO, ln_gamma=GAMMA, ln_beta=BETA, ln_pe=PE,
              ln_stats=STATS, lnc_stats=STATS, ln_c=LNC, ln_bias=LNB, bias_img=BIMG, workspace=WS, inv_scales=INV, amax_bits=AMAX)


UNCHECKED = ("gn_partials", "ln_gamma", "ln_beta", "ln_pe", "lnc_stats", "inv_scales", "amax_bits")


def error_calls():
    """[(entry point, label, arguments)]"""
    rows = []

    def row(name, label, **over):
        a = dict(_COMMON, **BASES[name])
        if "ldx" not in BASES[name] and "K" in over and "ldx" not in over:
            over = dict(over, ldx=over["K"])                  # (dense rows follow K unless the row is about the stride)
        a.update(over)
        rows.append((name, label, [a[k] for k in SIGS[name]]))

    for name, sig in SIGS.items():
        conv, partial, f32 = "conv" in name, "partial" in name, "f32" in name
        base = dict(_COMMON, **BASES[name])
        with_res = dict(residual=RES, ldres=320) if "ldres" in sig else dict(residual=RES)
        # -- every pointer position: NULL where the entry point needs it, and 4 and 8 bytes off.  (Inherited, not derived: `UNCHECKED` pointers are passed on
        #    as they come, the fp32 statistics may sit on 8 bytes, an optional pointer counts only with what it belongs to)
        for p in (k for k in _PTRS if k in sig and k not in UNCHECKED):
            extra = with_res if p == "residual2" and "residual" in sig else {}
            if p == "ln_stats" and name == "fmc_linear_bf16_ln":
                extra = dict(ln_out=None)                         # (exactly one of ln_out / ln_stats)
            if p == "workspace":
                extra = dict(split_k=2, workspace_bytes=1 << 30)
            if p in ("ln_c", "ln_bias") and name == "fmc_linear_bf16_ffblk":
                extra = dict(x_blocked=0, out_blocked=1, epilogue=1, M=M_MORE, lnc_stats=STATS, ln_c=LNC, ln_bias=LNB)
            if p in ("x", "w", "out") or p in BASES[name] and p != "residual":
                row(name, f"null {p}", **{p: None})
            row(name, f"misaligned {p} (+4)", **dict(extra, **{p: _VALUE[p] + 4}))
            if p != "ln_stats":
                row(name, f"misaligned {p} (+8)", **dict(extra, **{p: _VALUE[p] + 8}))
        if "residual2" in sig:
            row(name, "residual2 without residual", residual2=RES2)
        # -- the common shape check, one clause at a time
        if conv:
            for k in ("n_img", "H", "Wd", "Cin", "Cout"):
                row(name, f"{k} 0", **{k: 0})
            row(name, "Cin 96", Cin=96 if not f32 else 99)
            if f32:
                row(name, "Cin 32 * 3", Cin=96)
            row(name, "Cout 324", Cout=324)
            row(name, "Cout 12", Cout=12)
            row(name, "temb: div 0", temb=TEMB, temb_img_div=0)
            if not f32:
                row(name, "temb: stride 324", temb=TEMB, temb_row_stride=324)
            row(name, "temb: stride 322", temb=TEMB, temb_row_stride=322)
            row(name, "resample mode 3", upsample2x=3)
            row(name, "resample mode -1", upsample2x=-1)
            row(name, "upsample, odd H", upsample2x=1, H=15)
            row(name, "upsample, odd W", upsample2x=1, Wd=9)
            row(name, "null x, Cin 0", x=None, Cin=0)
            row(name, "Cin 0, misaligned w", Cin=0, w=W + 8)
            row(name, "misaligned out, temb div 0", out=OUT + 8, temb=TEMB, temb_img_div=0)
            row(name, "temb div 0, resample mode 3", temb=TEMB, temb_img_div=0, upsample2x=3)
            if "gn_partials" in sig:
                row(name, "H W 159", H=53, Wd=3)
                row(name, "Cout 640 + 8", Cout=648)
                row(name, "x of 2 GiB", n_img=1024, H=128, Wd=128, Cin=64)
                row(name, "x of 2 GiB when read 2x2", n_img=256, H=128, Wd=128, Cin=64, upsample2x=2)
                row(name, "w of 2 GiB", Cout=327680, Cin=384)
                row(name, "tile-major: Cout 640 + 8", Cout=648, w_tilemajor=1)
                row(name, "H W 159, resample mode 3", H=53, Wd=3, upsample2x=3)
                row(name, "temb div 0, H W 159", temb=TEMB, temb_img_div=0, H=53, Wd=3)
        else:
            for k in ("M", "N", "K"):
                row(name, f"{k} 0", **{k: 0})
            row(name, "M -160", M=-160)
            row(name, "K 96", K=96 if not f32 else 99)
            row(name, "N 324", N=324, ldo=328)
            row(name, "null x, M 0", x=None, M=0)
            row(name, "M 0, misaligned w", M=0, w=W + 8)
            if "ldx" in sig:
                row(name, "ldx + 4", ldx=base["ldx"] + 4)
            if "ldo" in sig:
                if not f32:
                    row(name, "ldo + 4", ldo=324)
                row(name, "ldo + 2", ldo=322)
            if "ldres" in sig:
                if not f32:
                    row(name, "ldres + 4", **dict(with_res, ldres=324))
                row(name, "ldres + 2", **dict(with_res, ldres=322))
                if "x2" not in sig:
                    row(name, "ldres + 4 without residual (reaches the next check)", ldres=324, x=X + 8)
            if "epilogue" in sig:
                row(name, "epilogue 2", epilogue=2)
                row(name, "epilogue -1", epilogue=-1)
                row(name, "GEGLU: N 328", epilogue=1, N=328, ldo=164)
                if "residual" in sig:
                    row(name, "GEGLU with a residual", epilogue=1, **with_res)
                row(name, "epilogue 2, misaligned out", epilogue=2, out=OUT + 8)
        # -- tile range, split_k codes and the workspace checks of set_split_k (the entry points that have the arguments)
        if "tile" in sig:
            row(name, "tile -1", tile=-1)
            row(name, "tile 23", tile=23)
            row(name, "tile 23, split_k 17", tile=23, split_k=17)
            row(name, "misaligned out, tile 23", out=OUT + 8, tile=23)
            for sk in (-16, -17, -81, -1000):
                row(name, f"split_k {sk}", split_k=sk, workspace=WS, workspace_bytes=1 << 30)
            for sk in (-1, -2, -3, -18):
                if f32:
                    row(name, f"split_k {sk}", split_k=sk, workspace=WS, workspace_bytes=1 << 30)
                    continue
                row(name, f"split_k {sk}: null workspace", split_k=sk, workspace_bytes=1 << 30)
                row(name, f"split_k {sk}: misaligned workspace", split_k=sk, workspace=WS + 8, workspace_bytes=1 << 30)
                row(name, f"split_k {sk}: workspace of 8191 bytes", split_k=sk, workspace=WS, workspace_bytes=8191)
            row(name, "split_k 17", split_k=17, workspace=WS, workspace_bytes=1 << 40)
            row(name, "split_k 2: null workspace", split_k=2, workspace_bytes=1 << 30)
            need = 2 * (160 * 320 if conv else 320 * 320) * 4
            row(name, "split_k 2: workspace one byte short", split_k=2, workspace=WS, workspace_bytes=need - 1)
            row(name, "split_k 17, null workspace", split_k=17)
            row(name, "split_k 2: null workspace, one byte short", split_k=2, workspace_bytes=need - 1)
            if "epilogue" in sig:
                row(name, "split_k 2 with GEGLU", split_k=2, epilogue=1, workspace=WS, workspace_bytes=1 << 30)
            # tile 18's conditions (a later check than the tile range: the pairs pin the accepted side of everything before it)
            if not f32:
                wide = dict(Cout=648) if conv else dict(N=648, ldo=648)
                row(name, "tile 18: width 640 + 8", tile=18, **wide)
                row(name, "tile 18: stream-K", tile=18, split_k=-1, workspace=WS, workspace_bytes=1 << 30)
                row(name, "tile 18: split_k 0", tile=18, split_k=0)
                row(name, "tile 18: width 640 + 8, split_k 17", tile=18, split_k=17, **wide)
                row(name, "tile 18: split_k 17 (reaches set_split_k)", tile=18, split_k=17)
                if conv:
                    row(name, "tile 18: x of 2 GiB", tile=18, n_img=1024, H=128, Wd=128)
                    row(name, "tile 18: w of 2 GiB", tile=18, Cout=327680, Cin=384)
                else:
                    row(name, "tile 18: two-source operand", tile=18, K=128, ldx=64, x2=X2, ldx2=64, k_split=64)
                    row(name, "tile 18: x of 2 GiB", tile=18, **BIG_A)
                    row(name, "tile 18: x of 838 860 rows, the last count below 2 GiB (reaches set_split_k)", tile=18, **dict(BIG_A, M=838860), split_k=17)
                    row(name, "tile 18: w of 2 GiB", tile=18, **BIG_W)
            else:
                row(name, "tile 18", tile=18)
        if name == "fmc_linear_bf16":
            two = dict(K=128, ldx=64, x2=X2, ldx2=64, k_split=64)
            for label, over in (("k_split 0", dict(k_split=0)), ("k_split K", dict(k_split=128)), ("k_split 32", dict(k_split=32)), ("ldx2 + 4", dict(ldx2=68)),
                                ("misaligned x2", dict(x2=X2 + 8)), ("k_split 0, tile 23", dict(k_split=0, tile=23)),
                                ("residual2 without residual, k_split 0", dict(k_split=0, residual2=RES2))):
                row(name, "two-source: " + label, **dict(two, **over))
            row(name, "two-source accepted, tile 23", **two, tile=23)
        if name == "fmc_linear_x3_f32":
            row(name, "K3 194", K=194)
            row(name, "K3 3 * 20", K=60)
            row(name, "K3 194, null x", K=194, x=None)
        if name == "fmc_conv3x3_x3_f32":
            row(name, "Cin3 194", Cin=194)
            row(name, "Cin3 194, null x", Cin=194, x=None)
        if name == "fmc_linear_fp8_qkv":
            row(name, "null inv_scales", inv_scales=None)
            row(name, "N 200", N=200)
            row(name, "N 320", N=320)
            row(name, "x of 2 GiB", M=1 << 24)
            row(name, "w of 2 GiB", N=327744, K=3328)
        # -- the tile-16 forms: every clause of the entry's own block alone, on the refused side of its boundary
        t16 = []
        if name == "fmc_linear_bf16_gn":
            t16 = [("gn_hw 0", dict(gn_hw=0)), ("gn_hw 80", dict(gn_hw=80)), ("gn_hw 320 at M 480", dict(M=480, gn_hw=320)), ("N 640 + 8", dict(N=648, ldo=648)),
                   ("x of 2 GiB", BIG_A), ("w of 2 GiB", BIG_W), ("tile-major: accepted by the partials' check, refused by none (alpha 2)", None),
                   ("gn_hw 80, misaligned out", dict(gn_hw=80, out=OUT + 8)), ("gn_hw 80, residual2 without residual", dict(gn_hw=80, residual2=RES2))]
        if name == "fmc_linear_bf16_ln":
            stats = dict(ln_out=None, ln_gamma=None, ln_beta=None, ln_stats=STATS)
            t16 = [("both ln_out and ln_stats", dict(ln_stats=STATS)), ("neither", dict(ln_out=None)), ("null gamma", dict(ln_gamma=None)), ("null beta", dict(ln_beta=None)),
                   ("N 640", dict(N=640, ldo=640)), ("M + 1", dict(M=M_MORE + 1)), ("as many tiles as CUs", dict(M=M_SAME)), ("one tile fewer", dict(M=M_LESS)),
                   ("statistics: as many tiles as CUs", dict(stats, M=M_SAME)), ("statistics: misaligned by 4", dict(stats, ln_stats=STATS + 4)),
                   ("pe: inner 80", dict(ln_pe=PE, ln_pe_inner=80)), ("pe: inner 0", dict(ln_pe=PE, ln_pe_inner=0)), ("pe: no frame", dict(ln_pe=PE, ln_pe_inner=160, ln_pe_frames=0)),
                   ("x of 2 GiB", BIG_A), ("as many tiles as CUs, tile-major weight of N 640", dict(M=M_SAME, N=640, ldo=640, w_tilemajor=1)),
                   ("both, as many tiles as CUs", dict(ln_stats=STATS, M=M_SAME)), ("residual2 without residual, N 640", dict(residual2=RES2, N=640, ldo=640)),
                   ("alpha 2 is accepted: N 640", dict(alpha=2.0, N=640, ldo=640))]
        if name == "fmc_linear_bf16_lnc":
            t16 = [("null ln_c, N 640 + 8", dict(ln_c=None, N=648, ldo=648)), ("N 640 + 8", dict(N=648, ldo=648)), ("M + 1", dict(M=M_MORE + 1)),
                   ("as many tiles as CUs", dict(M=M_SAME)), ("one tile fewer", dict(M=M_LESS)), ("as many tiles as CUs at N 640", dict(M=M_SAME // 2, N=640, ldo=640)),
                   ("GEGLU: as many tiles as CUs", dict(M=M_SAME // 2, epilogue=1, N=640, ldo=320)), ("x of 2 GiB", BIG_A), ("w of 2 GiB", dict(BIG_W, M=M_MORE)),
                   ("misaligned out, as many tiles as CUs", dict(out=OUT + 8, M=M_SAME)), ("epilogue 2, as many tiles as CUs", dict(epilogue=2, M=M_SAME))]
        if name == "fmc_linear_bf16_ffblk":
            outb = dict(x_blocked=0, out_blocked=1, epilogue=1, M=M_MORE)
            lnc = dict(lnc_stats=STATS, ln_c=LNC, ln_bias=LNB)
            t16 = [("neither operand tile-major", dict(x_blocked=0)), ("neither, null x", dict(x_blocked=0, x=None)), ("N 640 + 8", dict(N=648)), ("M + 1", dict(M=M_SAME + 1)),
                   ("x tile-major: one tile fewer than CUs", dict(M=M_LESS)), ("x tile-major: GEGLU", dict(epilogue=1)), ("x tile-major: K 96 (refused earlier)", dict(K=96)),
                   ("x tile-major: intermediate of 2 GiB", dict(M=838880, K=1280)), ("out tile-major: as many tiles as CUs", dict(outb, M=M_SAME)),
                   ("out tile-major: plain epilogue", dict(outb, epilogue=0)), ("out tile-major: N / 2 = 160 + 8 (refused earlier)", dict(outb, N=336)),
                   ("out tile-major: N 960 (N / 2 % 32)", dict(outb, N=960 + 64)), ("out tile-major: intermediate of 2 GiB", dict(outb, M=838880 * 2, N=1280)),
                   ("both tile-major", dict(outb, x_blocked=1)), ("LayerNorm statistics: as many tiles as CUs (the consumer's check)", dict(outb, **lnc, M=M_SAME)),
                   ("LayerNorm statistics on more tiles, plain epilogue (reaches the intermediate's check)", dict(outb, **lnc, epilogue=0)),
                   ("LayerNorm statistics with a bias", dict(outb, **lnc, bias=BIAS)), ("LayerNorm statistics without ln_c", dict(outb, **dict(lnc, ln_c=None))),
                   ("LayerNorm statistics: misaligned ln_bias", dict(outb, **dict(lnc, ln_bias=LNB + 8))),
                   ("x tile-major with LayerNorm statistics: as many tiles as CUs", dict(lnc)), ("out tile-major with a residual", dict(outb, residual=RES, ldres=160)),
                   ("one tile fewer, misaligned w", dict(M=M_LESS, w=W + 8)), ("one tile fewer, tile-major weight of N 640 + 8", dict(M=M_LESS, N=648, w_tilemajor=1))]
        if name == "fmc_linear_bf16_imgw":
            t16 = [("null bias_img, M + 1", dict(bias_img=None, M=M_SAME + 1)), ("N 640 + 8", dict(N=648, ldo=648)), ("M + 1", dict(M=M_SAME + 1)),
                   ("one tile fewer than CUs", dict(M=M_LESS)), ("images of 80 rows", dict(img_rows=80)), ("images of 240 rows", dict(img_rows=240)),
                   ("images of 0 rows", dict(img_rows=0)), ("images of 320 rows at an odd tile count", dict(M=M_MORE, img_rows=320)), ("x of 2 GiB", dict(BIG_A, img_rows=160)),
                   ("all weights of 2 GiB", dict(M=160 * 26215, K=128, img_rows=160)), ("all weights one image short of 2 GiB, one statistic misaligned (the LayerNorm's check)",
                                                                                      dict(M=160 * 26214, K=128, img_rows=160, ln_stats=STATS + 4)),
                   ("statistics: as many tiles as CUs, misaligned by 4 (the LayerNorm's check)", dict(ln_stats=STATS + 4)),
                   ("statistics: one tile fewer", dict(ln_stats=STATS, M=M_LESS)), ("statistics: N 640", dict(ln_stats=STATS, N=640, ldo=640, M=M_SAME // 2)),
                   ("one tile fewer, misaligned x", dict(M=M_LESS, x=X + 8))]
        if name == "fmc_linear_bf16_fftail":
            gn = dict(gn_partials=GNP, gn_hw=160)
            t16 = [("null x2", dict(x2=None)), ("null x2, null w", dict(x2=None, w=None)), ("N 640 + 8", dict(N=648, ldres=648)), ("M + 1", dict(M=M_SAME + 1)),
                   ("one tile fewer than CUs", dict(M=M_LESS)), ("k_split 32 (K % 32 holds: the two-source check)", dict(k_split=32, K=96)),
                   ("k_split 0", dict(k_split=0)), ("k_split K", dict(k_split=128)), ("ldx2 + 4", dict(ldx2=68)), ("misaligned x2, one tile fewer", dict(x2=X2 + 8, M=M_LESS)),
                   ("intermediate of 2 GiB", dict(M=838880, K=1280 + 64, k_split=1280)), ("x2 of 2 GiB", dict(M=838880, K=128 + 1280, k_split=128, ldx2=1280)),
                   ("partials: gn_hw 80", dict(gn, gn_hw=80)), ("partials: one tile fewer than CUs (the intermediate's check)", dict(gn, M=M_LESS)),
                   ("partials: gn_hw 80, one tile fewer", dict(gn, gn_hw=80, M=M_LESS)), ("gn_hw without partials, one tile fewer", dict(gn_hw=160, M=M_LESS)),
                   ("one tile fewer, tile-major weight", dict(M=M_LESS, w_tilemajor=1))]
        if partial:
            tail = "fftail" in name
            t16 = [("N 640 + 8", dict(N=648)), ("M 160 * (CUs - 1): one tile fewer than CUs", dict(M=M_LESS)), ("one tile fewer at N 640", dict(M=160 * 127, N=640)),
                   ("weight of 2 GiB", dict(BIG_W, K=3328)), ("padded intermediate of 2 GiB", dict(M=838721, K=1280 + (64 if tail else 0), k_split=1280 if tail else 0)),
                   ("ldres + 4", dict(residual=RES, ldres=324)), ("one tile fewer, misaligned x", dict(M=M_LESS, x=X + 8)), ("null x, one tile fewer", dict(M=M_LESS, x=None))]
            if tail:
                t16 += [("null x2", dict(x2=None)), ("partials", dict(gn_partials=GNP, gn_hw=160)), ("gn_hw alone", dict(gn_hw=160)), ("null x2, partials", dict(x2=None, gn_partials=GNP)),
                        ("partials, null w", dict(gn_partials=GNP, w=None)), ("k_split 0", dict(k_split=0)), ("k_split K", dict(k_split=128)), ("k_split 32", dict(k_split=32, K=96)),
                        ("ldx2 + 4", dict(ldx2=68)), ("ldx2 short of K - k_split", dict(ldx2=56)), ("x2 of 2 GiB", dict(M=838861, K=128 + 1280, k_split=128, ldx2=1280))]
        for label, over in t16:
            if over is not None:
                row(name, label, **over)
    return rows


def errors(L):
    """Rows `[entry point (index in `names`), label, index]`, values `[return code, message]`."""
    t, names = _Table(), []
    for name, label, args in error_calls():
        rc = int(getattr(L, name)(*args))
        msg = L.fmc_last_error()
        if name not in names:
            names.append(name)
        t.add((names.index(name), label), [rc, msg.decode() if msg else ""])
    return dict(t.data(), names=names)


# ---- 2. predicates: one row per (function, arguments other than M); its value: the results over `MS` as runs ---------------------------------------------
# every multiple of 160 up to 260 tiles with its neighbours (the CU thresholds at 8 and 256 CUs lie inside), the M >= 16384 gate, and the sizes around 2 GiB:
# M * 1280 and M * 320 elements of bf16, exact and padded to whole tiles
MS = sorted({m + d for m in range(160, 160 * 261, 160) for d in (-1, 0, 1)} | {16383, 16384, 16385}
            | {m + d for m in (838720, 838860, 838880, 3355360, 3355440, 3355520) for d in (-1, 0, 1)})
# (8 CUs, and the configurations that change one operand property or switch: the tile counts where something is decided, with their neighbours, and the same large sizes)
MS_EDGES = sorted({160 * t + d for t in (1, 2, 3, 4, 5, 7, 8, 9, 10, 64, 102, 103, 127, 128, 129, 255, 256, 257, 258) for d in (-1, 0, 1)} | {m for m in MS if m > 160 * 261})
SWITCHES_OFF = ("LN_EPILOGUE", "GN_EPILOGUE", "GN_FOLD", "FF_BLOCKED", "FF_TAIL", "GEGLU_DIRECT_BLOCKED", "W_TILEMAJOR", "LINEAR4")
VARIANTS = {"base": {}, "x fp32": dict(x_dtype=F32), "w fp32": dict(w_dtype=F32), "x strided": dict(x_tr=True), "w strided": dict(w_tr=True), "grad": dict(grad=True),
            "plain tensors": dict(claims=False), "residual fp32": dict(res_dtype=F32), "residual strided": dict(res_tr=True), "no residual": dict(res=None)}


def predicates(K, monkeypatch):
    L = K._lib.load()
    t, names = _Table(), []

    axis = [MS]

    def line(name, key, fn, xs=None):
        if name not in names:
            names.append(name)
        t.add([names.index(name)] + list(key), rle([fn(x) for x in (axis[0] if xs is None else xs)]))

    # no tensors, no state
    for Kd in (320, 1280, 2560):
        line("ff_blocked_numel", [Kd], lambda M: K.ff_blocked_numel(M, Kd))
    line("_decode_arm", [], lambda a: list(K._decode_arm(a, 7)), xs=list(range(0, 720)))
    for N, Kd, ldx in itertools.product((320, 640, 1280, 328, 64), (320, 1280, 64, 96), (0, 4)):
        line("fmc_linear4_supported", [N, Kd, ldx], lambda M: int(L.fmc_linear4_supported(M, N, Kd, Kd + ldx)))

    configs = [("", cus, g160, "base") for cus in (8, 256) for g160 in ("1", "0", "2")] + [("", 8, "1", v) for v in VARIANTS if v != "base"]
    configs += [(off, 8, "1", "base") for off in SWITCHES_OFF]
    for off, cus, g160, vname in configs:
        v = VARIANTS[vname]
        claims = v.get("claims", True)
        with monkeypatch.context() as mp, torch.set_grad_enabled(v.get("grad", False)):
            mp.setattr(K, "_cus", lambda device: cus)
            mp.setenv("FMC_G160_PERSIST", g160)
            if off:
                mp.setattr(K, off, False)
            key = [off, cus, g160, vname]
            axis[0] = MS if vname == "base" and not off and cus == 256 else MS_EDGES
            xd, wd = v.get("x_dtype", BF16), v.get("w_dtype", BF16)
            x = lambda M, C: tensor((M, C), xd, claims, v.get("x_tr", False))
            w = lambda N, C: tensor((N, C), wd, claims, v.get("w_tr", False))
            res = lambda M, N: None if "res" in v else tensor((M, N), v.get("res_dtype", BF16), claims, v.get("res_tr", False))
            if vname in ("base", "grad") and not off.startswith(("FF_", "GEGLU", "LN_", "GN_FOLD")):
                for N, Kd in ((320, 1280), (640, 640), (1280, 5120), (328, 1280), (320, 512)):
                    line("split_arms", key + [N, Kd], lambda M: list(K.split_arms(M, N, Kd)))
                for N, Kd, hw in ((320, 320, 2560), (320, 320, 2400), (640, 320, 160), (320, 96, 2560), (328, 320, 2560)):
                    line("gn_emit_ok", key + [N, Kd, hw], lambda M: int(bool(K.gn_emit_ok(M, N, Kd, hw, xd))))
            for N, Kd in ((320, 320), (640, 320), (320, 1280), (328, 320), (320, 96)):
                line("linear_supported", key + [N, Kd], lambda M: int(bool(K.linear_supported(x(M, Kd), w(N, Kd)))), xs=MS[:4])
                line("lnc_ok", key + [N, Kd], lambda M: int(bool(K.lnc_ok(x(M, Kd), w(N, Kd)))))
                for stats_only, pe_inner in ((False, 0), (True, 0), (False, 160), (False, 80)) if (N, Kd) == (320, 320) else ((False, 0),):
                    pe = tensor((16, 320), F32, claims) if pe_inner else None
                    ln = K.LnSpec(tensor((320,), F32, claims), tensor((320,), F32, claims), 1e-5, pe, pe_inner or 1, 16, "key", stats_only)
                    line("ln_emit_ok", key + [N, Kd, stats_only, pe_inner], lambda M: int(bool(K.ln_emit_ok(x(M, Kd), w(N, Kd), res(M, N), None, ln))))
            # x [n_img, hw, C] with the partial sums of 32 groups; M = n_img * hw: hw = 160, so that every multiple of 160 on the axis is a whole image count
            for N, C, with_ln in ((320, 320, 0), (320, 320, 1), (640, 320, 1), (640, 640, 0), (328, 320, 0)):
                def fold(M):
                    if M % 160:
                        return -1
                    n_img = M // 160
                    xs_ = tensor((n_img, 160, C), xd, claims, v.get("x_tr", False))
                    ln = K.LnSpec(None, None, 1e-5, None, 1, 1, "key", True) if with_ln else None
                    return int(bool(K.gn_fold_ok(xs_, (tensor((n_img, 1, 32), F32), C), 32, w(N, C), ln)))
                line("gn_fold_ok", key + [N, C, with_ln], fold)
            for C, Cff, N2 in ((320, 1280, 320), (640, 2560, 640), (320, 1280, 328), (320, 1200, 320)):
                line("ff_blocked_ok", key + [C, Cff, N2], lambda M: int(bool(K.ff_blocked_ok(x(M, C), w(2 * Cff, C), w(N2, Cff), res(M, N2)))))
                for any_rows in (False, True):
                    line("_geglu_blocked_ok", key + [C, Cff, N2, any_rows], lambda M: int(bool(K._geglu_blocked_ok(x(M, C), w(N2, Cff), res(M, C), any_rows))))
                    line("_ff_tail_ok", key + [C, Cff, N2, any_rows], lambda M: int(bool(K._ff_tail_ok(x(M, C), w(C, Cff), w(N2, C), res(M, N2), any_rows))))
    axis[0] = MS
    return dict(t.data(), names=names)


# ---- 3. routes: what `linear()` and `geglu_linear()` hand to the wrappers ----------------------------------------------------------------------------------
LEVELS = ((81920, 320, 2560), (20480, 640, 640), (5120, 1280, 160))          # (rows, width, pixels per image) of the three U-Net levels at 16 x 320 x 512
ROUTE_SWITCHES = [dict(arm=a) for a in (0, -1, 544, 512, 13, 700)] + [dict(arm=544, **{off: False}) for off in ("LN_EPILOGUE", "W_TILEMAJOR", "FF_BLOCKED", "FF_TAIL",
                                                                                                               "GN_EPILOGUE", "LINEAR4")]
WRAPPERS = ("linear_bf16", "linear4_bf16", "linear_lnc", "linear_ln", "linear_gn", "linear_f32", "vendor_linear", "resolve_pending_ln")


class Received:
    """Recording stand-ins: `[wrapper, tile, x2 given, gn_hw, ln ("out" | "stats" | None), geglu]`."""

    def __init__(self, monkeypatch, K, cus=256):
        fake_kernels.install(monkeypatch)
        self.log = []
        monkeypatch.setattr(K, "_cus", lambda device: cus)
        monkeypatch.setattr(K, "vendor_linear_ok", lambda *a, **k: False)
        for name in ("lnc_ok", "ln_emit_ok", "linear_supported"):
            monkeypatch.setattr(K, name, getattr(K, name))          # (asked with tensors that answer `is_cuda` with True, below)

        def result(x, weight, geglu=False):
            return torch.empty(*x.shape[:-1], weight.shape[0] // (2 if geglu else 1), dtype=x.dtype, device="meta")

        def note(name, tile=None, x2=None, gn_hw=0, ln=None, geglu=False):
            self.log.append([name, tile, x2 is not None, int(gn_hw), None if ln is None else ("stats" if ln.stats_only else "out"), bool(geglu)])

        def linear_bf16(x, weight, bias=None, residual=None, alpha=1.0, geglu=False, tile=0, split_k=1, x2=None, residual2=None, out=None):
            note("linear_bf16", tile, x2, geglu=geglu)
            return result(x, weight, geglu)

        def linear4_bf16(x, weight, bias=None, residual=None, alpha=1.0, residual2=None):
            note("linear4_bf16")
            return result(x, weight)

        def linear_lnc(x, weight, bias, pend, geglu=False):
            note("linear_lnc", geglu=geglu)
            return result(x, weight, geglu)

        def linear_ln(x, weight, bias, residual, alpha, residual2, ln):
            note("linear_ln", ln=ln)
            return result(x, weight)

        def linear_gn(x, weight, bias, residual, alpha, residual2, hw):
            note("linear_gn", gn_hw=hw)
            return result(x, weight)

        def resolve(x):
            if getattr(x, "_fmc_pending_ln", None) is not None:
                note("resolve_pending_ln")
                return x.view(x.shape)
            return x
        for name, fn in (("linear_bf16", linear_bf16), ("linear4_bf16", linear4_bf16), ("linear_lnc", linear_lnc), ("linear_ln", linear_ln), ("linear_gn", linear_gn),
                         ("resolve_pending_ln", resolve)):
            monkeypatch.setattr(K, name, fn)

    def take(self):
        log, self.log = self.log, []
        return log


def routes(K, monkeypatch):
    """Rows `[switch set (index in `switches`), case, index]`: the value holds, per level in order, the index (in `launches`) of what the stand-ins received
    (nothing received: the vendor library's arm), as runs."""
    calls = Received(monkeypatch, K)
    t, launches, at, switches = _Table(), [], {}, []

    def launch_id(detail):
        if repr(detail) not in at:
            at[repr(detail)] = len(launches)
            launches.append(detail)
        return at[repr(detail)]

    on = lambda *shape, dtype=BF16: tensor(shape, dtype, True)

    def pending(x):
        x._fmc_pending_ln = (on(x.shape[0], 2, dtype=F32), on(x.shape[1], dtype=F32), on(x.shape[1], dtype=F32), 1e-5)
        return x

    def spec(C, stats_only):
        return K.LnSpec(on(C, dtype=F32), on(C, dtype=F32), 1e-5, None, 1, 1, "key", stats_only)

    cases = {
        "proj": lambda M, C, hw: K.linear(on(M, C), on(C, C), on(C), on(M, C)),
        "proj, pending LayerNorm": lambda M, C, hw: K.linear(pending(on(M, C)), on(C, C), on(C)),
        "proj, pending LayerNorm and a residual": lambda M, C, hw: K.linear(pending(on(M, C)), on(C, C), on(C), on(M, C)),
        "to 320, ln": lambda M, C, hw: K.linear(on(M, C), on(320, C), on(320), on(M, 320), ln=spec(320, False)),
        "to 320, ln statistics": lambda M, C, hw: K.linear(on(M, C), on(320, C), on(320), on(M, 320), ln=spec(320, True)),
        "proj, ln at the level's width": lambda M, C, hw: K.linear(on(M, C), on(C, C), on(C), on(M, C), ln=spec(C, False)),
        "proj, gn_hw": lambda M, C, hw: K.linear(on(M, C), on(C, C), on(C), on(M, C), gn_hw=hw),
        "proj, gn_hw and ln": lambda M, C, hw: K.linear(on(M, C), on(320, C), on(320), None, gn_hw=hw, ln=spec(320, False)),
        "proj, x2": lambda M, C, hw: K.linear(on(M, C), on(C, 2 * C), on(C), x2=on(M, C)),
        "proj, x2 and gn_hw": lambda M, C, hw: K.linear(on(M, C), on(C, 2 * C), on(C), x2=on(M, C), gn_hw=hw),
        "ff2": lambda M, C, hw: K.linear(on(M, 4 * C), on(C, 4 * C), on(C), on(M, C)),
        "proj, fp32": lambda M, C, hw: K.linear(on(M, C, dtype=F32), on(C, C, dtype=F32), None),
        "geglu": lambda M, C, hw: K.geglu_linear(on(M, C), on(8 * C, C), on(8 * C), on(8 * C, C), on(8 * C), on(8 * C, C), on(8 * C)),
        "geglu without the 160-row order": lambda M, C, hw: K.geglu_linear(on(M, C), on(8 * C, C), on(8 * C), on(8 * C, C), on(8 * C)),
        "geglu, pending LayerNorm": lambda M, C, hw: K.geglu_linear(pending(on(M, C)), on(8 * C, C), on(8 * C), on(8 * C, C), on(8 * C), on(8 * C, C), on(8 * C)),
        "geglu, pending LayerNorm, without the 160-row order": lambda M, C, hw: K.geglu_linear(pending(on(M, C)), on(8 * C, C), on(8 * C), on(8 * C, C), on(8 * C)),
    }
    for sw in ROUTE_SWITCHES:
        with monkeypatch.context() as mp, torch.no_grad():
            for k, v in sw.items():
                if k == "arm":
                    mp.setattr(K, "_pick", lambda *a, _v=v, **kw: _v)
                else:
                    mp.setattr(K, k, v)
            mp.setattr(K, "F32_GEMM", False)
            switches.append(sorted(sw.items()))
            for case, fn in cases.items():
                seq = []
                for M, C, hw in LEVELS:
                    fn(M, C, hw)
                    seq.append(launch_id(calls.take()))
                t.add([len(switches) - 1, case], rle(seq))
    data = t.data()
    data["launches"], data["switches"] = launches, switches
    return data


def surface(K, monkeypatch):
    with monkeypatch.context() as mp:
        pred = predicates(K, mp)
    with monkeypatch.context() as mp:
        rt = routes(K, mp)
    return {"predicates": pred, "errors": errors(K._lib.load()), "routes": rt}

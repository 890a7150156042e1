"""The host surface of the fused attention blocks and the feed-forward chain as data (tools/record_fused_host_surface.py writes it to
tests/golden/fused_host_surface.json, tests/test_fused_host_surface.py asserts that the tree reproduces the file): what every predicate and count of these
families returns over a grid, the (return code, message) of refused calls to the launch and pack entry points, and the launches the two transformer blocks
and `FeedForward.forward_ln` make over the shipped and ragged sizes.  Nothing here launches: the refused calls fail their argument checks (pointers are
made-up integers), the predicates and the routes see storage-less tensors, the routes run on recording stand-ins.

How a host without a GPU reaches the conditions behind the device test, the same way before and after any host-side change:
  * predicates are recorded in three states: plain tensors with `hip_ops._on_gpu` (and `_ff_on_gpu`, where a tree still has it) as it is; plain tensors with
    the hook patched to True; tensors that answer `is_cuda` with True, hook as it is.  The second state shows which predicate consults the hook;
  * in the routes the hook is patched to True and the whole-tile predicates the models ask by name (`WHOLE_PREDICATES`) are wrapped so that they see their
    first argument as a tensor that answers `is_cuda` with True."""
import itertools

import torch

from tests import fake_kernels
from tests.halo_host_surface_common import _OnDevice, _Table, rle, same_table, unrle  # noqa: F401  (rle / same_table / unrle: re-exported to the test)

BF16, F32 = torch.bfloat16, torch.float32
HWS = list(range(1, 171))
# rows of the feed-forward: step 7 is coprime to 160 and runs 243 values (every remainder of 5, 10, 80, 160), the multiples of 80 with their neighbours, and
# the sizes around 2 GiB: M * 1280 and ceil(M / 160) * 160 * 1280 elements of bf16 (the intermediate, exact and padded), M * 320 (the tokens)
MS = sorted(set(range(1, 1701, 7)) | {m + d for m in range(80, 1701, 80) for d in (-1, 0, 1)}) + [838719, 838720, 838721, 838860, 838861, 838880, 3355443, 3355444]
STATES = ("plain", "hook", "claims")
SWITCHES_OFF = ("TEMPORAL_FUSED_640", "XATTN_FUSED_320", "XATTN_FUSED_640", "GEGLU_DIRECT_320", "GEGLU_DIRECT_640", "GEGLU_PIPE", "GEGLU_PIPE_640",
                "GEGLU_DIRECT_BLOCKED", "FF_BLOCKED", "FF_TAIL")


def tensor(shape, dtype=BF16, claims=False, transposed=False):
    """A storage-less tensor; `transposed`: the same shape, not contiguous."""
    if transposed:
        t = torch.empty(*shape[:-2], shape[-1], shape[-2], dtype=dtype, device="meta").transpose(-1, -2)
    else:
        t = torch.empty(*shape, dtype=dtype, device="meta")
    return t.as_subclass(_OnDevice) if claims else t


def claims_gpu(predicate):
    """`predicate` seeing its first argument as a tensor that answers `is_cuda` with True: a whole-tile predicate's other conditions on a CPU tensor."""
    return lambda h, *a: predicate(h.as_subclass(_OnDevice), *a)


def _hooks(monkeypatch, K):
    monkeypatch.setattr(K, "_on_gpu", lambda t: True)
    if hasattr(K, "_ff_on_gpu"):
        monkeypatch.setattr(K, "_ff_on_gpu", lambda t: True)


# ---- 1. predicates and counts: one row per (function, state, arguments other than hw / M); its value: the results over `HWS` or `MS` as runs ----
# variants of the operands, one changed at a time: (dtype, not contiguous, grad enabled, past 2 GiB)
ATT_VARIANTS = {"base": {}, "fp32": dict(dtype=F32), "strided": dict(transposed=True), "grad": dict(grad=True), "big": dict(big=True), "frames 15": dict(frames=15)}


def predicates(K, monkeypatch):
    L = K._lib.load()
    t, names = _Table(), []

    def line(name, key, xs, fn):
        if name not in names:
            names.append(name)
        t.add([names.index(name)] + list(key), rle([int(fn(x)) for x in xs]))

    # counts (no tensors, no state)
    for C in (320, 640):
        line("temporal_tile_count", [C], HWS, lambda hw: K.temporal_tile_count(3, hw, C))
        for ipt in (1, 3):
            line("xattn_tile_count", [C, ipt], HWS, lambda hw: K.xattn_tile_count(6, hw, ipt, C))
        line("geglu_pipe_variant", [C], MS, lambda M: K.geglu_pipe_variant(M, C))
        line("geglu_pipe_partial_variant", [C], [0], lambda _: K.geglu_pipe_partial_variant(C))
    for rows in (80, 160):
        line("ff_tile_count", [rows], MS, lambda M: K.ff_tile_count(M, rows))
    for Kd in (1280, 2560):
        line("ff_blocked_numel", [Kd], MS, lambda M: K.ff_blocked_numel(M, Kd))
    # the pipe's shape rule: the two exported predicates and the Python restatement of the partial one
    for C, cff, variant in itertools.product((256, 320, 640), (1280, 2560, 1000, 0), (0, 1, 2, -1)):
        line("fmc_geglu_pipe_supported", [C, cff, variant], MS, lambda M: L.fmc_geglu_pipe_supported(M, cff, C, variant))
        line("fmc_geglu_pipe_partial_supported", [C, cff, variant], MS, lambda M: L.fmc_geglu_pipe_partial_supported(M, cff, C, variant))
        line("geglu_pipe_partial_supported", [C, cff, variant], MS, lambda M: K.geglu_pipe_partial_supported(M, cff, C, variant))

    def attention(state):
        claims = state == "claims"
        # one operand or switch changed at a time: every variant at 8 heads, the other widths, head counts and switches on the base variant
        configs = [("", C, 8, v) for C in (320, 640) for v in ATT_VARIANTS] + [("", 256, 8, "base")] + [("", C, 4, "base") for C in (320, 640)]
        configs += [(off, C, 8, "base") for off in ("TEMPORAL_FUSED_640", "XATTN_FUSED_320", "XATTN_FUSED_640") for C in (320, 640)]
        for off, C, heads, vname in configs:
            v = ATT_VARIANTS[vname]
            dt, tr, big, fr = v.get("dtype", BF16), v.get("transposed", False), v.get("big", False), v.get("frames", 16)
            with monkeypatch.context() as mp, torch.set_grad_enabled(v.get("grad", False)):
                if off:
                    mp.setattr(K, off, False)
                # (`big`: 1311 | 655 clips of 16 frames, 20972 | 10486 images -- the tensor passes 2 GiB at hw = 160 | 161)
                mk = lambda hw: tensor((((655 if C == 640 else 1311) if big else 2), fr, hw, C), dt, claims, tr)
                for name in ("temporal_block_supported", "temporal_block_partial_supported"):
                    line(name, [state, off, C, heads, vname], HWS, lambda hw: getattr(K, name)(mk(hw), heads))
                if fr != 16:
                    continue
                mk = lambda hw: tensor((((10486 if C == 640 else 20972) if big else 6), hw, C), dt, claims, tr)
                base = vname == "base" and not off and heads == 8
                for name, S in itertools.product(("xattn_block_supported", "xattn_block640_supported", "xattn_block_partial_supported"), (1, 77, 80, 81)):
                    if base or (S == 77 and "640_" not in name):
                        line(name, [state, off, C, heads, vname, S], HWS, lambda hw: getattr(K, name)(mk(hw), S, heads))

    FF_VARIANTS = {"base": {}, "h fp32": dict(h_dtype=F32), "w fp32": dict(w_dtype=F32), "h strided": dict(h_tr=True), "grad": dict(grad=True),
                   "no residual": dict(res=None), "residual fp32": dict(res_dtype=F32), "residual strided": dict(res_tr=True), "tail short": dict(tail_rows=-1),
                   "cff + 32": dict(cff_add=32), "cff 1000": dict(cff=1000), "w2 strided": dict(w2_tr=True)}
    FF_OFF = [s_ for s_ in SWITCHES_OFF if not s_.startswith(("TEMPORAL", "XATTN"))]

    def feed_forward(state):
        claims = state == "claims"
        # (switch off, CUs, FMC_G160_PERSIST, C, width of the tail / the second GEMM, variant): every variant at 8 CUs and width 320, the rest on the base variant
        configs = [("", 8, "1", C, 320, v) for C in (320, 640) for v in FF_VARIANTS] + [("", 8, "1", 256, 320, "base")]
        configs += [("", cus, "1", C, n_out, "base") for C in (320, 640) for cus, n_out in ((8, 10240), (256, 10240), (256, 320))]
        configs += [(off, 8, "1", C, 320, "base") for off in FF_OFF for C in (320, 640)] + [("", 8, "0", C, 320, "base") for C in (320, 640)]
        for off, cus, g160, C, n_out, vname in configs:
            v = FF_VARIANTS[vname]
            with monkeypatch.context() as mp, torch.set_grad_enabled(v.get("grad", False)):
                mp.setattr(K, "_cus", lambda device: cus)
                mp.setenv("FMC_G160_PERSIST", g160)
                if off:
                    mp.setattr(K, off, not getattr(K, off) if off == "GEGLU_PIPE_640" else False)
                cff = v.get("cff", 4 * C + v.get("cff_add", 0))
                w1 = tensor((2 * cff, C), v.get("w_dtype", BF16), claims)
                w2 = tensor((C, cff), v.get("w_dtype", BF16), claims, v.get("w2_tr", False))
                wp = tensor((n_out, C), v.get("w_dtype", BF16), claims)
                w2n = tensor((n_out, cff), v.get("w_dtype", BF16), claims, v.get("w2_tr", False))      # the second GEMM of the blocked pair: `[N2, Cff]`
                key = [state, off, cus, g160, C, n_out, vname]
                h = lambda M: tensor((M, C), v.get("h_dtype", BF16), claims, v.get("h_tr", False))
                res = lambda M: None if "res" in v else tensor((M, C), v.get("res_dtype", BF16), claims, v.get("res_tr", False))
                tres = lambda M: None if "res" in v else tensor((M + v.get("tail_rows", 0), n_out), v.get("res_dtype", BF16), claims, v.get("res_tr", False))
                if n_out == 320:                                      # (these three do not see the tail's width)
                    for name in ("geglu_ln_direct_ok", "geglu_ln_partial_ok", "geglu_ln_pipe_ok"):
                        line(name, key, MS, lambda M: getattr(K, name)(h(M), w1))
                for name in ("geglu_direct_blocked_ok", "geglu_direct_blocked_partial_ok"):
                    line(name, key, MS, lambda M: getattr(K, name)(h(M), w2n, res(M)))
                for name in ("ff_tail_ok", "ff_tail_partial_ok"):
                    line(name, key, MS, lambda M: getattr(K, name)(h(M), w2, wp, tres(M)))

    for state in STATES:
        with monkeypatch.context() as mp:
            if state == "hook":
                _hooks(mp, K)
            attention(state)
            feed_forward(state)
    return dict(t.data(), names=names)


# ---- 2. errors: refused calls of the eight launch and the two pack entry points.  Every row breaks at least one argument check, so none reaches its launch ----
H, OUT, GAMMA, BPE, WM, POSE, WQKV, WOUT, BOUT, STATS, KV, WPK, BIAS = (0x10000 * k for k in range(1, 14))
SIGS = {
    "fmc_temporal_block_bf16": ("h", "out", "gamma", "bpe", "eps", "w_merge", "pose", "merge_scale", "w_qkv", "w_out", "b_out", "stats", "stats_eps", "n", "frames",
                                "hw", "C", "heads", "scale", "stream"),
    "fmc_xattn_block320_bf16": ("h", "out", "gamma", "bpe", "eps", "w_qkv", "kv", "w_out", "b_out", "stats", "stats_eps", "n", "hw", "keys", "ipt", "scale", "stream"),
    "fmc_xattn_block640_bf16": ("h", "out", "gamma", "bpe", "eps", "w_qkv", "kv", "w_out", "b_out", "n", "hw", "keys", "ipt", "scale", "stream"),
    "fmc_geglu_pipe_ln_bf16": ("h", "out", "gamma", "bpe", "eps", "w_qkv", "bias", "M", "cff", "C", "blocked", "variant", "stream"),
}
for _n in list(SIGS):
    SIGS[_n.replace("_bf16", "_partial_bf16")] = SIGS[_n]
PACKS = {"fmc_xattn_pack_kv": 1280, "fmc_xattn_pack_kv40": 640}
BASE = dict(h=H, out=OUT, gamma=GAMMA, bpe=BPE, eps=1e-5, w_merge=None, pose=None, merge_scale=1.0, w_qkv=WQKV, w_out=WOUT, b_out=BOUT, stats=None, stats_eps=0.0,
            n=2, frames=16, hw=40, C=320, heads=8, scale=0.125, stream=None, kv=KV, keys=77, ipt=1, bias=BIAS, M=1600, cff=1280, blocked=0, variant=0)
REFUSALS = (-1, -3, -5)                             # FMC_E_SHAPE, FMC_E_ALIGN, FMC_E_NULL: the argument checks' codes (FMC_E_LAUNCH = -4 would be a launch)


def error_calls():
    """[(entry point, label, arguments)]"""
    rows = []

    def row(name, label, **over):
        a = dict(BASE, **over)
        rows.append((name, label, [a[k] for k in SIGS[name]]))

    for name, sig in SIGS.items():
        partial, pipe, temporal = "_partial" in name, "geglu" in name, "temporal" in name
        widths = (320, 640) if (temporal or pipe) else (640 if "640" in name else 320,)
        for C in widths:
            at = dict(C=C, hw=(160 if C == 320 else 80)) if not pipe else dict(C=C, cff=4 * C)
            ptrs = [k for k in ("h", "out", "gamma", "bpe", "w_qkv", "kv", "w_out") if k in sig]
            for k in ptrs:
                row(name, f"C {C}: null {k}", **at, **{k: None})
                row(name, f"C {C}: misaligned {k}", **at, **{k: BASE[k] + 8})
            if pipe:
                row(name, f"C {C}: misaligned bias", **at, bias=BIAS + 4)
                row(name, f"C {C}: null h, bad variant", **at, h=None, variant=2)
                row(name, f"C {C}: variant 2", **at, variant=2)
                row(name, f"C {C}: variant -1", **at, variant=-1)
                row(name, f"C {C}: variant 2, misaligned out", **at, variant=2, out=OUT + 8)
                row(name, f"C {C}: cff 1000", **dict(at, cff=1000))
                row(name, f"C {C}: cff 0", **dict(at, cff=0))
                row(name, f"C {C}: no row", **at, M=0)
                row(name, f"C {C}: cff 1000, misaligned h", **dict(at, cff=1000), h=H + 8)
                row(name, f"C {C}: intermediate of 2 GiB", **dict(at, cff=1280), M=838880)
                row(name, f"C {C}: padded intermediate of 2 GiB", **dict(at, cff=1280), M=838721)
                row(name, f"C {C}: tokens of 2 GiB", **dict(at, cff=128), M=3355520)
                if C == 640:
                    row(name, "C 640: variant 1", **at, variant=1)
                if not partial:
                    row(name, f"C {C}: ragged M 1504", **at, M=1504)
                    row(name, f"C {C}: tile-major at M 1520", **at, M=1520, blocked=1)
                    row(name, f"C {C}: ragged M 1504, misaligned gamma", **at, M=1504, gamma=GAMMA + 4)
                    if C == 320:
                        row(name, "C 320: variant 1 at M 1520", **at, M=1520, variant=1)
                continue
            row(name, f"C {C}: misaligned b_out", **at, b_out=BOUT + 8)
            row(name, f"C {C}: null h, no pixel", **dict(at, hw=0), h=None)
            row(name, f"C {C}: no pixel", **dict(at, hw=0))
            row(name, f"C {C}: no image", **at, n=0)
            if not partial:
                row(name, f"C {C}: ragged hw", **dict(at, hw=39 if C == 320 else 34))
                row(name, f"C {C}: ragged hw, misaligned out", **dict(at, hw=39 if C == 320 else 34), out=OUT + 8)
            if "stats" in sig and C == 320:
                row(name, "C 320: misaligned statistics", **at, stats=STATS + 4)
            if temporal:
                big = dict(at, n=1311, hw=160) if C == 320 else dict(at, n=655, hw=165)
                row(name, f"C {C}: tensor of 2 GiB", **big)
                row(name, f"C {C}: tensor of 2 GiB, misaligned h", **big, h=H + 8)
                row(name, f"C {C}: merge without pose term", **at, w_merge=WM)
                row(name, f"C {C}: pose term without merge", **at, pose=POSE)
                row(name, f"C {C}: misaligned merge", **at, w_merge=WM + 8, pose=POSE)
                row(name, f"C {C}: misaligned pose term", **at, w_merge=WM, pose=POSE + 8)
                row(name, f"C {C}: merge without pose term, tensor of 2 GiB", **big, w_merge=WM)
                row(name, f"C {C}: merge without pose term, misaligned out", **at, w_merge=WM, out=OUT + 8)
                row(name, f"C {C}: 15 frames", **at, frames=15)
                row(name, f"C {C}: 4 heads", **at, heads=4)
                row(name, f"C {C}: 15 frames, merge without pose term", **at, frames=15, w_merge=WM)
                row(name, f"C {C}: null out, 15 frames", **at, frames=15, out=None)
                if C == 640:
                    row(name, "C 640: statistics", **at, stats=STATS)
                    row(name, "C 640: statistics, merge without pose term", **at, stats=STATS, w_merge=WM)
                    row(name, "C 640: statistics, tensor of 2 GiB", **big, stats=STATS)
                    row(name, "C 640: statistics, misaligned h", **at, stats=STATS, h=H + 8)
                    row(name, "C 256", **dict(at, C=256))
                    if not partial:
                        row(name, "C 640: ragged hw, tensor of 2 GiB", **dict(big, hw=164))
                        row(name, "C 640: ragged hw, statistics", **dict(at, hw=34), stats=STATS)
            else:
                big = dict(at, n=20972 if C == 320 else 10486, hw=160 if C == 320 else 240)
                row(name, f"C {C}: tensor of 2 GiB", **big)
                row(name, f"C {C}: tensor of 2 GiB, misaligned h", **big, h=H + 8)
                row(name, f"C {C}: no key", **at, keys=0)
                row(name, f"C {C}: 81 keys", **at, keys=81)
                row(name, f"C {C}: 7 images of 3 per text", **at, n=7, ipt=3)
                row(name, f"C {C}: 0 images per text", **at, ipt=0)
                row(name, f"C {C}: null kv, 81 keys", **at, kv=None, keys=81)
                row(name, f"C {C}: 81 keys, tensor of 2 GiB", **big, keys=81)
                row(name, f"C {C}: 81 keys, misaligned w_out", **at, keys=81, w_out=WOUT + 8)
    for name, width in PACKS.items():
        def prow(label, kv=KV, out=OUT, batch=2, S=77, ld=None):
            rows.append((name, label, [kv, out, batch, S, S * width if ld is None else ld, None]))
        prow("null kv", kv=None)
        prow("null out", out=None)
        prow("misaligned kv", kv=KV + 4)
        prow("misaligned out", out=OUT + 8)
        prow("no token", S=0)
        prow("81 tokens", S=81)
        prow("no batch", batch=0)
        prow("short batch stride", ld=77 * width - 1)
        prow("null kv, 81 tokens", kv=None, S=81)
        prow("81 tokens, misaligned out", S=81, out=OUT + 8)
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


# ---- 3. routes: the launches of the two transformer blocks and of `FeedForward.forward_ln` ----
WHOLE_PREDICATES = ("temporal_block_supported", "xattn_block_supported", "geglu_ln_direct_ok", "geglu_ln_pipe_ok")
ROUTE_SWITCHES = [dict(PARTIAL_TILES=pt, GEGLU_PIPE=gp, GEGLU_PIPE_640=g6, FP8_FF=f8) for pt in (False, True) for gp in (True, False) for g6 in (False, True)
                  for f8 in (False, True)]
ROUTE_SWITCHES += [dict(PARTIAL_TILES=pt, GEGLU_PIPE=True, GEGLU_PIPE_640=False, FP8_FF=False, lnc_ok=True) for pt in (False, True)]
# (where the feed-forward does not normalise its input itself the attention block in front of it is asked for row statistics: the pipe off with the
#  consuming GEMM said to take them, and the level's own switch off)
ROUTE_SWITCHES += [dict(PARTIAL_TILES=pt, GEGLU_PIPE=False, GEGLU_PIPE_640=False, FP8_FF=False, lnc_ok=True) for pt in (False, True)]
ROUTE_SWITCHES += [dict(PARTIAL_TILES=pt, GEGLU_PIPE=True, GEGLU_PIPE_640=False, FP8_FF=False, GEGLU_DIRECT_320=False) for pt in (False, True)]
BLOCK_SIZES = [(320, hw) for hw in (39, 40, 47, 2560)] + [(640, hw) for hw in (34, 35, 640)]
FF_ROWS = (1504, 1520, 1600)


class Launches:
    """Recording stand-ins for the five wrappers (and `geglu_ln_direct`): `[wrapper, partial_tiles, statistics asked for, blocked, variant, gn_hw]`."""

    def __init__(self, monkeypatch, K, cus=8):
        fake_kernels.install(monkeypatch)
        self.log = []
        _hooks(monkeypatch, K)
        monkeypatch.setattr(K, "_cus", lambda device: cus)
        monkeypatch.setattr(K, "resolve_pending_ln", lambda t: t)          # (the stand-ins' statistics are not applied)
        monkeypatch.setattr(K, "xattn_pack_kv", lambda kv: torch.zeros(1, dtype=kv.dtype, device=kv.device))
        for name in WHOLE_PREDICATES:
            monkeypatch.setattr(K, name, claims_gpu(getattr(K, name)))

        def block(name):
            def fn(h, *a, **k):
                asked = k.get("stats_eps") is not None
                self.log.append([name, bool(k.get("partial_tiles")), asked, None, None, None])
                out = torch.zeros_like(h)
                return (out, torch.zeros(h.numel() // h.shape[-1], 2, device=h.device)) if asked else out
            return fn

        def pipe(h, g, b, eps, frag, bias, cff, blocked=False, variant=0, partial_tiles=False):
            self.log.append(["geglu_ln_pipe", bool(partial_tiles), None, bool(blocked), int(variant), None])
            return torch.zeros(*h.shape[:-1], cff, dtype=h.dtype, device=h.device)

        def direct(h, g, b, eps, frag, bias, cff, blocked=False):
            self.log.append(["geglu_ln_direct", False, None, bool(blocked), None, None])
            return torch.zeros(*h.shape[:-1], cff, dtype=h.dtype, device=h.device)

        def from_blocked(xb, w, bias, residual, alpha=1.0, out=None, partial_tiles=False):
            self.log.append(["linear_from_blocked", bool(partial_tiles), None, None, None, None])
            return torch.zeros(*xb.shape[:-1], w.shape[0], dtype=xb.dtype, device=xb.device)

        def tail(mid, h, wc, bc, res, gn_hw=0, partial_tiles=False):
            self.log.append(["ff_tail", bool(partial_tiles), None, None, None, int(gn_hw)])
            return torch.zeros_like(res)
        for name, fn in (("temporal_block", block("temporal_block")), ("xattn_block", block("xattn_block")), ("geglu_ln_pipe", pipe), ("geglu_ln_direct", direct),
                         ("linear_from_blocked", from_blocked), ("ff_tail", tail)):
            monkeypatch.setattr(K, name, fn)

    def take(self):
        log, self.log = self.log, []
        return log


def _modules(C):
    from synfmc_amd.models import layers as L
    from synfmc_amd.models.attention_processor import _PoseMerge  # noqa: F401
    from tests.test_partial_tiles_host import _temporal_block
    meta = lambda m: m.eval().requires_grad_(False).to(BF16).to("meta")
    torch.manual_seed(0)
    return dict(plain=meta(_temporal_block(C)), camera=meta(_temporal_block(C, pose_proc=True)),
                basic=meta(L.BasicTransformerBlock(C, 8, C // 8, cross_attention_dim=64)), ff=meta(L.FeedForward(C)), norm=meta(L.LayerNorm(C)))


def routes(K, monkeypatch):
    """Rows `[switch set (index in `switches`), case, index]`: the value holds, per size in order, the index (in `launches`) of what the stand-ins received
    plus how the call ended, as runs."""
    from synfmc_amd.models.attention_processor import _PoseMerge
    calls = Launches(monkeypatch, K)
    monkeypatch.setattr(_PoseMerge, "_pose_term", lambda self, pose, w, b, s: torch.zeros_like(pose))
    t, launches, at, switches = _Table(), [], {}, []

    def launch_id(detail):
        if repr(detail) not in at:
            at[repr(detail)] = len(launches)
            launches.append(detail)
        return at[repr(detail)]

    def ended(y):
        return "none" if y is None else ("tail" if getattr(y, "_fmc_tail", False) else "plain")

    mods = {C: _modules(C) for C in (320, 640)}
    for sw in ROUTE_SWITCHES:
        with monkeypatch.context() as mp:
            for k, v in sw.items():
                mp.setattr(K, k, (lambda x, w: True) if k == "lnc_ok" else v)
            switches.append(sorted((k, v) for k, v in sw.items()))
            key = [len(switches) - 1]
            with torch.no_grad():
                for case in ("plain", "camera"):
                    seq = []
                    for C, hw in BLOCK_SIZES:
                        x = tensor((2, 16, hw, C))
                        kw = {"pose_feature": tensor((2, 16, hw, C))} if case == "camera" else {}
                        for tail in (None, (tensor((C, C)), tensor((C,)), tensor((32, hw, C)), hw)):
                            y = mods[C][case](x, cross_attention_kwargs=kw, tail=tail)
                            seq.append(launch_id(calls.take() + [ended(y)]))
                    t.add(key + ["temporal " + case], rle(seq))
                seq = []
                for C, hw in BLOCK_SIZES:
                    x, text = tensor((6, hw, C)), tensor((2, 7, 64))
                    for tail in (None, (tensor((C, C)), tensor((C,)), tensor((6, hw, C)), hw)):
                        y = mods[C]["basic"](x, encoder_hidden_states=text, tail=tail)
                        seq.append(launch_id(calls.take() + [ended(y)]))
                t.add(key + ["basic"], rle(seq))
                seq = []
                for C, M, with_tail, own_residual in itertools.product((320, 640), FF_ROWS, (False, True), (True, False)):
                    h = tensor((M, C))
                    tail = (tensor((C, C)), tensor((C,)), tensor((M, C)), 160) if with_tail else None
                    y = mods[C]["ff"].forward_ln(h, mods[C]["norm"], h if own_residual else tensor((M, C)), tail=tail)
                    seq.append(launch_id(calls.take() + [ended(y)]))
                t.add(key + ["forward_ln"], rle(seq))
    data = t.data()
    data["launches"], data["switches"] = launches, switches
    return data


def surface(K, monkeypatch):
    with monkeypatch.context() as mp:
        pred = predicates(K, mp)
    return {"predicates": pred, "errors": errors(K._lib.load()), "routes": routes(K, monkeypatch)}

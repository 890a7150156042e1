"""The host surface of the attention kernels as data (tools/record_attn_host_surface.py writes it to tests/golden/attn_host_surface.json,
tests/test_attn_host_surface.py asserts that the tree reproduces the file): the (return code, message) of refused calls to the eight entry points of
csrc/spatial_attn.hip, csrc/spatial_attn_bwd.hip, csrc/temporal_attn.hip and csrc/attn_generic.hip, and every argument the attention wrappers of
`hip_ops` hand to the library, forward and backward, with the library replaced by a recorder.  Nothing here launches: every recorded call of part 1
breaks at least one argument check (pointers are made-up integers), part 2 never reaches the library.

What part 1 cannot hold, because the entry points ACCEPT it and a recorded row must be refused (each is pinned from the accepted side instead, paired
with a fault that a later check refuses):

* `fmc_temporal_attn_fp8_bwd` checks no pointer alignment (no later check exists: nothing is recorded), and takes strides that are 8 mod 16;
* `fmc_spatial_attn_fwd` does not check `B % kv_batch_div` (the backward does);
* `fmc_temporal_attn_fwd` reports a bad `F` from inside its dispatcher, after the stride and alignment checks;
* temporal head widths 104 and 136 are built (`(D + 31) / 32` k-steps), the spatial ones are not;
* the backward's two "does not fit LDS" refusals cannot be reached: with D <= 160, at most 32 tile rows and 4-byte elements the seven tiles of one
  head take 7 * 32 * 168 * 4 = 150 528 bytes, below both the 150 KiB of the search and the 160 KiB of the refusal (`lds_refusal_unreachable`);
* lse, dvec, key_keep, the fp8 scales and the three pointers of `fmc_fp8_scales_roll` are passed on without an alignment check."""
import ctypes

import torch

from tests.gemm_host_surface_common import REFUSALS, _Table, rle, same_table, tensor, unrle  # noqa: F401  (re-exported to the recorder and the test)

BF16, F32 = torch.bfloat16, torch.float32
ATTN_REFUSALS = REFUSALS + (-2,)                    # and FMC_E_DTYPE

# ---- 1. errors ----------------------------------------------------------------------------------------------------------------------------------------
Q, K_, V, O, DO, LSE, DVEC, DQ, DK, DV, SCALES, KEEP, AMAX, SCALE, INV = (0x10000 * k for k in range(1, 16))
_SP_STR = ("q_batch_stride", "q_row_stride", "kv_batch_stride", "kv_row_stride", "o_batch_stride", "o_row_stride")
_TA_STR = ("clip_stride", "frame_stride", "pix_stride")
_TA_BWD_STR = _TA_STR + ("do_clip_stride", "do_frame_stride", "do_pix_stride", "dq_clip_stride", "dq_frame_stride", "dq_pix_stride")
_TA_SIZES = ("n_clips", "n_pix", "F", "H", "D")
SIGS = {
    "fmc_spatial_attn_fwd": ("q", "k", "v", "o", "lse", "B", "H", "Sq", "Skv", "D") + _SP_STR + ("kv_batch_div", "scale", "dtype", "stream"),
    "fmc_spatial_attn_bwd": ("q", "k", "v", "o", "d_o", "lse", "dvec", "dq", "dk", "dv", "B", "H", "Sq", "Skv", "D") + _SP_STR
                            + ("dq_batch_stride", "dq_row_stride", "dkv_batch_stride", "dkv_row_stride", "kv_batch_div", "scale", "dtype", "stream"),
    "fmc_temporal_attn_fwd": ("q", "k", "v", "o") + _TA_SIZES + _TA_STR + ("o_clip_stride", "o_frame_stride", "o_pix_stride", "scale", "dtype", "stream"),
    "fmc_temporal_attn_bwd": ("q", "k", "v", "d_o", "dq", "dk", "dv") + _TA_SIZES + _TA_BWD_STR + ("scale", "dtype", "stream"),
    "fmc_temporal_attn_fp8_fwd": ("q", "k", "v", "o", "scales") + _TA_SIZES + _TA_STR + ("o_clip_stride", "o_frame_stride", "o_pix_stride", "scale", "stream"),
    "fmc_temporal_attn_fp8_bwd": ("q", "k", "v", "scales", "d_o", "dq", "dk", "dv") + _TA_SIZES + _TA_BWD_STR + ("scale", "stream"),
    "fmc_attention_fwd": ("q", "k", "v", "o", "key_keep", "B", "H", "Sq", "Skv", "D") + _SP_STR + ("scale", "causal", "dtype", "stream"),
    "fmc_fp8_scales_roll": ("amax", "scale_out", "inv_scale", "margin", "stream"),
}
# a call that every argument check accepts (never made: each recorded row changes it into a refused one).  Spatial: 4 batch entries on 2 texts of 64 keys,
# 2 heads of 40; temporal: 2 clips of 3 pixels and 16 frames in the fused native layout [B, F, P, 3 C], 2 heads of 40; generic: head width 64
_C = 80
BASE = dict(q=Q, k=K_, v=V, o=O, d_o=DO, lse=LSE, dvec=DVEC, dq=DQ, dk=DK, dv=DV, scales=SCALES, key_keep=None, amax=AMAX, scale_out=SCALE, inv_scale=INV,
            B=4, H=2, Sq=64, Skv=64, D=40, q_batch_stride=64 * _C, q_row_stride=_C, kv_batch_stride=64 * 2 * _C, kv_row_stride=2 * _C, o_batch_stride=64 * _C,
            o_row_stride=_C, dq_batch_stride=64 * _C, dq_row_stride=_C, dkv_batch_stride=64 * 2 * _C, dkv_row_stride=2 * _C, kv_batch_div=2, scale=0.125, dtype=0,
            causal=0, stream=None, margin=1.25, n_clips=2, n_pix=3, F=16, clip_stride=16 * 3 * 3 * _C, frame_stride=3 * 3 * _C, pix_stride=3 * _C,
            o_clip_stride=16 * 3 * _C, o_frame_stride=3 * _C, o_pix_stride=_C, do_clip_stride=16 * 3 * _C, do_frame_stride=3 * _C, do_pix_stride=_C,
            dq_clip_stride=16 * 3 * 3 * _C, dq_frame_stride=3 * 3 * _C, dq_pix_stride=3 * _C)
BASES = {name: {} for name in SIGS}
BASES["fmc_attention_fwd"] = dict(D=64, q_batch_stride=64 * 128, q_row_stride=128, kv_batch_stride=64 * 128, kv_row_stride=128, o_batch_stride=64 * 128,
                                  o_row_stride=128)
BASES["fmc_temporal_attn_fp8_fwd"] = BASES["fmc_temporal_attn_fp8_bwd"] = dict(clip_stride=16 * 3 * 3 * _C, frame_stride=3 * 3 * _C, pix_stride=3 * _C)   # (bytes: 720, 240)
_PTRS = ("q", "k", "v", "o", "d_o", "lse", "dvec", "dq", "dk", "dv", "scales", "key_keep", "amax", "scale_out", "inv_scale")
OPTIONAL = {"fmc_spatial_attn_fwd": ("lse",), "fmc_attention_fwd": ("key_keep",)}            # NULL is a value of the interface
UNALIGNED_OK = ("lse", "dvec", "scales", "key_keep", "amax", "scale_out", "inv_scale")       # passed on as they come
HEAD_WIDTHS = (4, 12, 104, 136, 168)


def lds_refusal_unreachable():
    """The largest LDS size the backward's head-group search can see (one head, D = 160, 32 tile rows, fp32) against its two bounds."""
    worst = 7 * 32 * (160 + 8) * 4
    return worst <= 150 * 1024 and worst <= 160 * 1024


def error_calls():
    """[(entry point, label, arguments)]"""
    rows = []

    def row(name, label, **over):
        a = dict(BASE, **BASES[name])
        a.update(over)
        rows.append((name, label, [a[k] for k in SIGS[name]]))

    for name, sig in SIGS.items():
        base = dict(BASE, **BASES[name])
        temporal, fp8, bwd, roll = "temporal" in name, "fp8" in name and "roll" not in name, name.endswith("_bwd"), "roll" in name
        checks_alignment = not roll and name != "fmc_temporal_attn_fp8_bwd"
        strides = [k for k in sig if k.endswith("_stride")]
        later = {strides[0]: base[strides[0]] + 4} if strides else {}                   # a fault of the stride check: what an ACCEPTED shape is paired with
        # -- every pointer: NULL, and 4 and 8 bytes off
        for p in (k for k in _PTRS if k in sig):
            if p not in OPTIONAL.get(name, ()):
                row(name, f"null {p}", **{p: None})
            elif later:
                row(name, f"null {p} is accepted (reaches the stride check)", **{p: None}, **later)
            if checks_alignment and p not in UNALIGNED_OK:
                for off in (4, 8):
                    row(name, f"misaligned {p} (+{off})", **{p: base[p] + off})
        if "dk" in sig and not temporal:
            row(name, "dk and dv null together are accepted (reaches the stride check)", dk=None, dv=None, **later)
            row(name, "dk and dv null together, misaligned dq", dk=None, dv=None, dq=DQ + 8)
        if roll:
            row(name, "all three null", amax=None, scale_out=None, inv_scale=None)
            continue
        # -- every size at 0, the head widths, the frame counts
        sizes = _TA_SIZES if temporal else ("B", "H", "Sq", "Skv", "D")
        for k in sizes:
            row(name, f"{k} 0", **{k: 0})
            row(name, f"{k} -1", **{k: -1})
        for d in HEAD_WIDTHS:
            built = temporal and d % 8 == 0 and d <= 160
            if built:
                row(name, f"D {d} is built (reaches the stride check)", D=d, **later)
            else:
                row(name, f"D {d}", D=d)
        if temporal:
            row(name, "F 33", F=33)
            row(name, "F 32 is accepted (reaches the stride check)", F=32, **later)
        # -- every stride
        for s in strides:
            row(name, f"{s} + 4", **{s: base[s] + 4})
            if name == "fmc_temporal_attn_fp8_fwd" and s in _TA_STR:
                row(name, f"{s} + 8", **{s: base[s] + 8})
        if "kv_batch_div" in sig:
            row(name, "kv_batch_div 0", kv_batch_div=0)
            row(name, "kv_batch_div -2", kv_batch_div=-2)
            if bwd:
                row(name, "kv_batch_div 3 does not divide B", kv_batch_div=3)
            else:
                row(name, "kv_batch_div 3 does not divide B: accepted (reaches the stride check)", kv_batch_div=3, **later)
        if "dtype" in sig:
            row(name, "dtype 2", dtype=2)
            row(name, "dtype -1", dtype=-1)
            row(name, "fp32: D 104" if not temporal else "fp32: F 33", dtype=1, **(dict(F=33) if temporal else dict(D=104)))
        if name == "fmc_attention_fwd":
            row(name, "B H 65536", B=256, H=256)
            row(name, "D 160", D=160)
        if name == "fmc_temporal_attn_fp8_fwd":                      # (the fp8 backward has no such clause: it stages bf16 rows)
            row(name, "no head group: H 1, D 40", H=1, D=40)
            row(name, "no head group: H 3, D 8", H=3, D=8)
            row(name, "no head group, frame stride + 4", H=1, D=40, frame_stride=base["frame_stride"] + 4)
        # -- pairs of faults: the order of the checks
        row(name, "null q, D 4", q=None, D=4)
        row(name, "null v, misaligned q", v=None, **({"q": Q + 8} if checks_alignment else {strides[0]: base[strides[0]] + 4}))
        if "dtype" in sig:
            row(name, "null k, dtype 2", k=None, dtype=2)
            row(name, "dtype 2, D 4", dtype=2, D=4)
            row(name, "dtype 2, misaligned q", dtype=2, q=Q + 8)
        row(name, "D 4, stride + 4", D=4, **later)
        row(name, "H 0, stride + 4", H=0, **later)
        if checks_alignment:
            row(name, "D 4, misaligned o" if "o" in sig else "D 4, misaligned dq", D=4, **({"o": O + 8} if "o" in sig else {"dq": DQ + 8}))
            row(name, "stride + 4, misaligned q", q=Q + 8, **later)
            row(name, "last stride + 4, misaligned v", v=V + 4, **{strides[-1]: base[strides[-1]] + 4})
        if temporal:
            row(name, "F 33, D 168", F=33, D=168)
            row(name, "F 0, stride + 4", F=0, **later)
            if checks_alignment:
                row(name, "F 33, misaligned q", F=33, q=Q + 8)
                row(name, "F 0, misaligned k", F=0, k=K_ + 4)
        if name == "fmc_temporal_attn_fp8_fwd":
            row(name, "q stride + 8, o stride + 4", clip_stride=base["clip_stride"] + 8, o_pix_stride=base["o_pix_stride"] + 4)
            row(name, "o stride + 4, misaligned q", o_clip_stride=base["o_clip_stride"] + 4, q=Q + 8)
            row(name, "no head group, misaligned q", H=1, D=40, q=Q + 8)
        if name == "fmc_spatial_attn_fwd":
            row(name, "D 104, kv_batch_div 3", D=104, kv_batch_div=3)
            row(name, "D 104, fp32", D=104, dtype=1)
        if name == "fmc_spatial_attn_bwd":
            row(name, "dk null alone, dtype 2", dk=None, dtype=2)
            row(name, "kv_batch_div 3, stride + 4", kv_batch_div=3, **later)
            row(name, "D 104 (not built: the dispatcher's refusal, after every check)", D=104)
            row(name, "D 136, fp32", D=136, dtype=1)
            row(name, "D 104, misaligned dv", D=104, dv=DV + 8)
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


# ---- 2. wrapper calls: every argument the attention wrappers hand to the library ---------------------------------------------------------------------------
class Recorder:
    """Stands where `_lib.load()` returns the library: a call of an entry point is logged as `[name, arguments]` and answers 0.  A pointer argument is
    logged as `[tensor, byte offset]`: the case's named operands, or `empty <shape> <dtype> #<i>` for the i-th tensor of that shape and type the
    wrappers allocated (so the record does not depend on the order in which a wrapper allocates tensors of different shapes).  The
    `*_supported` questions go to the real library."""

    def __init__(self, monkeypatch, K):
        from synfmc_amd import _lib
        self.real, self.sigs = _lib.load(), _lib.SIGNATURES
        self.log, self.known, self.keep = [], [], []
        monkeypatch.setattr(K._lib, "load", lambda: self)
        monkeypatch.setattr(K, "_dev", lambda *ts: None)
        monkeypatch.setattr(K, "_stream", lambda: None)
        empty, seen = torch.empty, {}

        def recording_empty(*a, **kw):
            t = empty(*a, **kw)
            what = f"{list(t.shape)} {str(t.dtype).replace('torch.', '')}"
            seen[what] = seen.get(what, 0) + 1
            self.name(t, f"empty {what} #{seen[what]}")
            return t
        monkeypatch.setattr(torch, "empty", recording_empty)
        self.reset = lambda: (seen.clear(), self.known.clear(), self.keep.clear())

    def name(self, t, label):
        s = t.untyped_storage()
        if s.nbytes():
            self.known.append((s.data_ptr(), s.nbytes(), label))
            self.keep.append(t)                          # (alive until the case ends: an address is not handed out twice)
        return t

    def where(self, p):
        if p is None:
            return None
        for base, n, label in self.known:
            if base <= p < base + n:
                return [label, p - base]
        return ["?", None]                               # (a copy the wrapper made, the fp8 scales of the call: its address is not the record)

    def __getattr__(self, fn):
        if fn.endswith("_supported") or fn == "fmc_last_error":
            return getattr(self.real, fn)
        types = self.sigs[fn][1]

        def call(*args):
            assert len(args) == len(types), fn
            self.log.append([fn, [self.where(a) if t is ctypes.c_void_p else a for a, t in zip(args, types)]])
            return 0
        return call

    def take(self):
        log, self.log = self.log, []
        self.reset()
        return log


def wrapper_cases(K, rec):
    """[(label, thunk)]: each thunk runs one wrapper, forward and (where it says so) backward, on CPU tensors."""
    B, S, Skv, H, D = 4, 24, 7, 2, 8
    C = H * D

    def t(label, *shape, dtype=BF16, grad=False):
        return rec.name(torch.zeros(*shape, dtype=dtype), label).requires_grad_(grad)

    def back(out):
        out.backward(rec.name(torch.ones(out.shape, dtype=out.dtype), "d_o"))

    def s3(x):
        return x[..., :C], x[..., C:2 * C], x[..., 2 * C:]

    cases = []
    add = lambda label, fn: cases.append((label, fn))
    for dtype, tag in ((BF16, "bf16"), (F32, "fp32")):
        qkv_sp = lambda grad=False, dtype=dtype: t("qkv", B, S, 3 * C, dtype=dtype, grad=grad)
        sep = lambda grad=(False, False, False), bkv=B, dtype=dtype: (t("q", B, S, C, dtype=dtype, grad=grad[0]), t("k", bkv, Skv, C, dtype=dtype, grad=grad[1]),
                                                                    t("v", bkv, Skv, C, dtype=dtype, grad=grad[2]))
        add(f"{tag} spatial_attention: separate", lambda sep=sep: K.spatial_attention(*sep(), H))
        add(f"{tag} spatial_attention: separate, scale, return_lse", lambda sep=sep: K.spatial_attention(*sep(), H, 0.25, return_lse=True))
        add(f"{tag} spatial_attention: fused slices", lambda f=qkv_sp: K.spatial_attention(*s3(f()), H))
        add(f"{tag} spatial_attention: 2 texts for 4 entries", lambda sep=sep: K.spatial_attention(*sep(bkv=2), H))
        add(f"{tag} spatial_attention: grad q k v, return_lse (no autograd node)", lambda sep=sep: K.spatial_attention(*sep((True, True, True)), H, return_lse=True))
        add(f"{tag} spatial_attention: backward q k v", lambda sep=sep: back(K.spatial_attention(*sep((True, True, True)), H)))
        add(f"{tag} spatial_attention: backward q only", lambda sep=sep: back(K.spatial_attention(*sep((True, False, False)), H, 0.5)))
        add(f"{tag} spatial_attention: backward k only, 1 text", lambda sep=sep: back(K.spatial_attention(*sep((False, True, False), bkv=1), H)))
        add(f"{tag} spatial_attention: backward through fused slices", lambda f=qkv_sp: back(K.spatial_attention(*s3(f(True)), H)))
        add(f"{tag} self_attention_qkv spatial", lambda f=qkv_sp: K.self_attention_qkv(f(), H, 0.3, False))
        add(f"{tag} self_attention_qkv spatial: backward", lambda f=qkv_sp: back(K.self_attention_qkv(f(True), H, 0.3, False)))
        for lay, shape in (("native", (2, 5, 3)), ("nfc", (6, 5))):
            qkv_t = lambda grad=False, shape=shape, dtype=dtype: t("qkv", *shape, 3 * C, dtype=dtype, grad=grad)
            sep_t = lambda grad=False, shape=shape, dtype=dtype: tuple(t(n, *shape, C, dtype=dtype, grad=grad) for n in "qkv")
            add(f"{tag} temporal_attention {lay}: fused slices", lambda f=qkv_t: K.temporal_attention(*s3(f()), H))
            add(f"{tag} temporal_attention {lay}: separate, scale", lambda f=sep_t: K.temporal_attention(*f(), H, 0.2))
            add(f"{tag} temporal_attention {lay}: backward through fused slices", lambda f=qkv_t: back(K.temporal_attention(*s3(f(True)), H)))
            add(f"{tag} temporal_attention {lay}: backward, separate", lambda f=sep_t: back(K.temporal_attention(*f(True), H, 0.2)))
            add(f"{tag} self_attention_qkv temporal {lay}", lambda f=qkv_t: K.self_attention_qkv(f(), H, 0.3, True))
            add(f"{tag} self_attention_qkv temporal {lay}: backward", lambda f=qkv_t: back(K.self_attention_qkv(f(True), H, 0.3, True)))
        for bkv, what in ((B, "a text per entry"), (2, "2 texts for 4 entries"), (1, "1 text for 4 entries")):
            qkv_c = lambda gq=False, gkv=False, bkv=bkv, dtype=dtype: (t("q", B, S, C, dtype=dtype, grad=gq), t("kv", bkv, Skv, 2 * C, dtype=dtype, grad=gkv))
            add(f"{tag} cross_attention_q_kv, {what}", lambda f=qkv_c: K.cross_attention_q_kv(*f(), H, 0.3))
            add(f"{tag} cross_attention_q_kv, {what}: backward, frozen kv", lambda f=qkv_c: back(K.cross_attention_q_kv(*f(True, False), H, 0.3)))
            add(f"{tag} cross_attention_q_kv, {what}: backward, trainable kv", lambda f=qkv_c: back(K.cross_attention_q_kv(*f(True, True), H, 0.3)))
            add(f"{tag} cross_attention_q_kv, {what}: backward, kv only", lambda f=qkv_c: back(K.cross_attention_q_kv(*f(False, True), H, 0.3)))
        Hg, Dg = 2, 32
        Cg = Hg * Dg
        gen = lambda dtype=dtype: tuple(t(n, 2, S if n == "q" else Skv, Cg, dtype=dtype) for n in "qkv")
        add(f"{tag} attention: separate", lambda f=gen: K.attention(*f(), Hg))
        add(f"{tag} attention: causal, key_keep, scale", lambda f=gen: K.attention(*f(), Hg, 0.1, causal=True, key_keep=t("keep", 2, Skv, dtype=torch.uint8)))
        add(f"{tag} attention: fused slices", lambda dtype=dtype: K.attention(*(lambda x: (x[..., :Cg], x[..., Cg:2 * Cg], x[..., 2 * Cg:]))(t("qkv", 2, S, 3 * Cg, dtype=dtype)), Hg))
    # fp8: x [.., 64] through a [192, 64] projection (2 heads of 32); the scale state counts as calibrated (the calibration is a bf16 `linear`)
    for lay, shape in (("native", (2, 5, 3)), ("nfc", (6, 5))):
        def fp8(gx, gw, shape=shape):
            scales = K.Fp8QKVScales("cpu")
            scales.calibrated = True
            for n in ("amax", "scale", "inv_scale"):
                rec.name(getattr(scales, n), f"scales.{n}")
            return K.temporal_attention_fp8(t("x", *shape, 64, grad=gx), t("w", 192, 64, grad=gw), scales, 2, 0.3)
        add(f"temporal_attention_fp8 {lay}", lambda f=fp8: f(False, False))
        add(f"temporal_attention_fp8 {lay}: backward, frozen weight", lambda f=fp8: back(f(True, False)))
        add(f"temporal_attention_fp8 {lay}: backward, trainable weight", lambda f=fp8: back(f(True, True)))
    return cases


def calls(K, monkeypatch):
    """Rows `[case, index]`, values: the ordered calls `[entry point, arguments]` the case made."""
    t = _Table()
    with monkeypatch.context() as mp:
        rec = Recorder(mp, K)
        for label, fn in wrapper_cases(K, rec):
            rec.take()
            fn()
            t.add([label], rec.take())
    return t.data()


def surface(K, monkeypatch):
    return {"errors": errors(K._lib.load()), "calls": calls(K, monkeypatch)}

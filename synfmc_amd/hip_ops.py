"""Tensor-level entry points of the hand-written gfx950 kernels (through the C ABI).

PyTorch is plumbing here: it owns device memory and the stream; every function below hands raw
device pointers + sizes + the current `hipStream_t` to `libfmc_hip.so`.  No CPU / eager fallback:
CPU tensors raise.

Layout: activations are channels-last.  `[N, S, C]` "tokens" are what the kernels see; a
`b c f h w` video in `torch.channels_last_3d` memory format *is* `[(b f), (h w), c]` tokens.
"""
from __future__ import annotations

import atexit
import ctypes
import math
import os
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import FMC_BF16, FMC_F32
from .derived import derived_on_owner

_DT = {torch.bfloat16: FMC_BF16, torch.float32: FMC_F32}


def _dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"fmc kernels take bf16 or fp32 activations, got {t.dtype}") from None


def _dev(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("fmc HIP kernels need device (cuda/hip) tensors; there is no CPU fallback")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_ws_cache = {}
_ws_retired = []


def _workspace(device, nbytes: int) -> torch.Tensor:
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        if ws is not None:
            _ws_retired.append(ws)      # a captured HIP graph may have baked its address: never hand it back
        ws = torch.empty(max(nbytes // 4 + 1, 1 << 16), dtype=torch.float32, device=device)
        _ws_cache[key] = ws
    return ws


# --------------------------------------------------------------------------------------------
# GroupNorm (+SiLU)
# --------------------------------------------------------------------------------------------
def groupnorm_silu_raw(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float,
                       act: bool, x2: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """x `[N, S, C]` contiguous -> (y, stats `[N, G, 2]`).  With `x2 [N, S, C2]` the normalised tensor is the channel
    concat `[x, x2]` (never materialised); y is `[N, S, C + C2]`."""
    _dev(x, gamma, beta, x2)
    assert x.ndim == 3 and x.is_contiguous(), "groupnorm: x must be contiguous [N, S, C] tokens"
    N, S, C1 = x.shape
    C = C1
    if x2 is not None:
        assert x2.is_contiguous() and x2.shape[:2] == x.shape[:2] and x2.dtype == x.dtype
        C = C1 + x2.shape[2]
    lib = _lib.load()
    y = torch.empty(N, S, C, dtype=x.dtype, device=x.device)
    stats = torch.empty(N, groups, 2, dtype=torch.float32, device=x.device)
    ws = _workspace(x.device, lib.fmc_groupnorm_workspace_bytes(N, C, groups))
    _lib.check(lib.fmc_groupnorm_silu_fwd(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                          stats.data_ptr(), ws.data_ptr(), N, S, C, groups, float(eps), int(act),
                                          _dt(x), _p(x2), C1 if x2 is not None else 0, _stream()),
               "fmc_groupnorm_silu_fwd")
    return y, stats


# GroupNorm statistics out of the producing GEMM / conv epilogue (fmc_linear_bf16_gn / fmc_conv3x3_bf16_gn -> fmc_groupnorm_apply_fwd).
# A producer that emitted them tags its output tensor: `out._fmc_gn = (partials [n_img, hw / 160, 32, 2], C)`; views made by the layout helpers
# carry the tag, any arithmetic on the tensor makes a new, untagged one.  FMC_GN_EPILOGUE=0: A/B switch.
GN_EPILOGUE = os.environ.get("FMC_GN_EPILOGUE", "1") != "0"
gn_epilogue_calls = {"emitted": 0, "consumed": 0}
GN_MIN_HW = 2048                    # below that the single-pass GroupNorm kernel reads x once anyway


def gn_emit_ok(M: int, N: int, Kd: int, hw: int, dtype) -> bool:
    return (GN_EPILOGUE and dtype == torch.bfloat16 and hw >= GN_MIN_HW and hw % 160 == 0 and M % hw == 0 and N % 320 == 0 and Kd % 64 == 0
            and not torch.is_grad_enabled())


def carry_gn(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    tag = getattr(src, "_fmc_gn", None)
    if tag is not None:
        dst._fmc_gn = tag
    return dst


def groupnorm_apply(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, act: bool,
                    partials: torch.Tensor) -> torch.Tensor:
    """GroupNorm(+SiLU) of `[N, S, C]` tokens whose per-(image, tile, group) sums the producer already wrote (`partials [N, splits, G, 2]`)."""
    _dev(x, gamma, beta, partials)
    N, S, C = x.shape
    assert x.is_contiguous() and partials.shape[0] == N and partials.shape[2] == groups and partials.dtype == torch.float32
    y = torch.empty_like(x)
    stats = torch.empty(N, groups, 2, dtype=torch.float32, device=x.device)
    gn_epilogue_calls["consumed"] += 1
    _lib.check(_lib.load().fmc_groupnorm_apply_fwd(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(),
                                                   partials.data_ptr(), partials.shape[1], N, S, C, groups, float(eps), int(act), _dt(x),
                                                   _stream()), "fmc_groupnorm_apply_fwd")
    return y


class _GroupNormSiLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, act):
        y, stats = groupnorm_silu_raw(x, gamma, beta, groups, eps, act)
        ctx.save_for_backward(x, gamma, beta, stats)
        ctx.groups, ctx.act = groups, act
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, stats = ctx.saved_tensors
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            return (*_gn_param_backward(ctx, dy, None), None, None, None)
        dy = dy.contiguous()
        N, S, C = x.shape
        lib = _lib.load()
        dx = torch.empty_like(x)
        ws = _workspace(x.device, lib.fmc_groupnorm_workspace_bytes(N, C, ctx.groups))
        _lib.check(lib.fmc_groupnorm_silu_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), gamma.data_ptr(),
                                              beta.data_ptr(), stats.data_ptr(), ws.data_ptr(), N, S, C, ctx.groups,
                                              int(ctx.act), _dt(x), _stream()), "fmc_groupnorm_silu_bwd")
        return dx, None, None, None, None, None


def groupnorm_silu_bwd_params(dy, x, gamma, beta, stats, groups: int, act: bool, want_dx: bool = True, addend=None,
                              dgamma=None, dbeta=None, accumulate: bool = False):
    """(dX or None, dgamma, dbeta) of GroupNorm(+SiLU) over `[N, S, C]` tokens (`fmc_groupnorm_silu_bwd_params`): dX as
    `fmc_groupnorm_silu_bwd_add` computes it (`addend` added), the affine gradients in fp32 `[C]` (written into `dgamma` / `dbeta`
    when given, added to them with `accumulate`).  `want_dx=False` skips the dX pass."""
    _dev(dy, x, gamma, beta, stats, addend)
    dy = dy if dy.is_contiguous() else dy.contiguous()
    assert x.is_contiguous() and dy.shape == x.shape and dy.dtype == x.dtype
    assert (dgamma is None) == (dbeta is None), "pass both dgamma and dbeta or neither"
    N, S, C = x.shape
    lib = _lib.load()
    dx = torch.empty_like(x) if want_dx else None
    if dgamma is None:
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        accumulate = False
    ws = _workspace(x.device, lib.fmc_groupnorm_silu_bwd_params_workspace_bytes(N, S, C, groups))
    _lib.check(lib.fmc_groupnorm_silu_bwd_params(dy.data_ptr(), x.data_ptr(), _p(dx), dgamma.data_ptr(), dbeta.data_ptr(), gamma.data_ptr(),
                                                 beta.data_ptr(), stats.data_ptr(), _p(addend), int(accumulate), ws.data_ptr(), N, S, C, groups,
                                                 int(act), _dt(x), _stream()), "fmc_groupnorm_silu_bwd_params")
    return dx, dgamma, dbeta


def _gn_param_backward(ctx, dy, addend):
    """The norm's gamma / beta train: (dX or None, dgamma, dbeta) from one statistics pass (+ the dX pass when x needs a gradient)."""
    x, gamma, beta, stats = ctx.saved_tensors
    dx, dg, db = groupnorm_silu_bwd_params(dy, x, gamma, beta, stats, ctx.groups, ctx.act,
                                           want_dx=ctx.needs_input_grad[0] or addend is not None, addend=addend)
    return dx, (dg.to(gamma.dtype) if ctx.needs_input_grad[1] else None), (db.to(beta.dtype) if ctx.needs_input_grad[2] else None)


def _gn_backward(ctx, dy, addend):
    x, gamma, beta, stats = ctx.saved_tensors
    dy = dy.contiguous()
    N, S, C = x.shape
    lib = _lib.load()
    dx = torch.empty_like(x)
    ws = _workspace(x.device, lib.fmc_groupnorm_workspace_bytes(N, C, ctx.groups))
    _lib.check(lib.fmc_groupnorm_silu_bwd_add(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(),
                                              ws.data_ptr(), N, S, C, ctx.groups, int(ctx.act), _p(addend), _dt(x), _stream()),
               "fmc_groupnorm_silu_bwd_add")
    return dx


class _GroupNormSiLUSkip(torch.autograd.Function):
    """`(h, GroupNorm(h))` as ONE autograd node for `h + f(norm(h))`: the backward receives the gradient along the skip and the one through
    the norm together and returns `d_skip + dX(norm)` from the norm's backward kernel (`fmc_groupnorm_silu_bwd_add`) -- autograd would
    otherwise sum the two with an elementwise launch per residual connection (303 per OMC-stage step)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, act):
        y, stats = groupnorm_silu_raw(x, gamma, beta, groups, eps, act)
        ctx.save_for_backward(x, gamma, beta, stats)
        ctx.groups, ctx.act = groups, act
        ctx.set_materialize_grads(False)
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, d_skip, dy):
        if dy is None:
            return d_skip, None, None, None, None, None
        add = None
        if d_skip is not None:
            add = d_skip if d_skip.is_contiguous() else d_skip.contiguous()
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:          # trainable gamma / beta: the skip gradient rides in the same dX pass
            return (*_gn_param_backward(ctx, dy, add), None, None, None)
        return _gn_backward(ctx, dy, add), None, None, None, None, None


def groupnorm_silu_skip(x, gamma, beta, groups: int, eps: float, act: bool):
    """(x for the skip connection, GroupNorm(+SiLU)(x)) -- one autograd node when x needs a gradient, the plain pair otherwise.
    Trainable gamma / beta (`train_mm`) get their gradients from either (`fmc_groupnorm_silu_bwd_params`)."""
    if torch.is_grad_enabled() and x.requires_grad and x.is_cuda and x.is_contiguous():
        return _GroupNormSiLUSkip.apply(x, gamma, beta, groups, eps, act)
    return x, groupnorm_silu(x, gamma, beta, groups, eps, act)


def groupnorm_silu(x, gamma, beta, groups: int, eps: float, act: bool, x2=None, gn_tag=None) -> torch.Tensor:
    """GroupNorm over `[N, S, C]` tokens (statistics per sample and group over S x C/G) + optional SiLU.
    gamma/beta: fp32 `[C]`.  `x2`: second channel block (the result normalises `cat([x, x2], -1)` without building it).
    `gn_tag`: the `_fmc_gn` tag of the tensor x is a view of -- its producer's partial sums replace the statistics pass."""
    if (gn_tag is not None and x2 is None and groups == 32 and gn_tag[1] == x.shape[-1] and gn_tag[0].shape[0] == x.shape[0]
            and gn_tag[0].shape[1] <= 64 and not torch.is_grad_enabled()):       # (any split of the pixels: 160-row tiles, the halo conv's 10 x 32 tiles)
        return groupnorm_apply(x, gamma, beta, groups, eps, act, gn_tag[0])
    if torch.is_grad_enabled() and (x.requires_grad or (x2 is not None and x2.requires_grad) or gamma.requires_grad or beta.requires_grad):
        if x2 is not None:
            x = torch.cat([x, x2], dim=-1)
        return _GroupNormSiLU.apply(x, gamma, beta, groups, eps, act)
    return groupnorm_silu_raw(x, gamma, beta, groups, eps, act, x2)[0]


# --------------------------------------------------------------------------------------------
# LayerNorm (+ positional encoding), GEGLU
# --------------------------------------------------------------------------------------------
class _LayerNorm(torch.autograd.Function):
    """gamma / beta here are the fp32 views the kernel reads; their grads come back in fp32."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, pe, pe_inner, pe_frames):
        ctx.save_for_backward(x, gamma)
        ctx.eps = eps
        return _layernorm_raw(x, gamma, beta, eps, pe, pe_inner, pe_frames)

    @staticmethod
    def backward(ctx, dy):
        x, gamma = ctx.saved_tensors
        dy = dy.contiguous()
        C = x.shape[-1]
        M = x.numel() // C
        dx = torch.empty_like(x)
        want_p = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dg = torch.zeros(C, dtype=torch.float32, device=x.device) if want_p else None
        db = torch.zeros(C, dtype=torch.float32, device=x.device) if want_p else None
        _lib.check(_lib.load().fmc_layernorm_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), dx.data_ptr(), _p(dg),
                                                 _p(db), M, C, float(ctx.eps), _dt(x), _stream()), "fmc_layernorm_bwd")
        return dx, dg, db, None, None, None, None


def _ln_backward(ctx, dy, addend):
    x, gamma = ctx.saved_tensors
    dy = dy.contiguous()
    C = x.shape[-1]
    M = x.numel() // C
    dx = torch.empty_like(x)
    want_p = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
    dg = torch.zeros(C, dtype=torch.float32, device=x.device) if want_p else None
    db = torch.zeros(C, dtype=torch.float32, device=x.device) if want_p else None
    _lib.check(_lib.load().fmc_layernorm_bwd_add(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), dx.data_ptr(), _p(dg), _p(db), _p(addend), M, C,
                                                 float(ctx.eps), _dt(x), _stream()), "fmc_layernorm_bwd_add")
    return dx, dg, db


class _LayerNormSkip(torch.autograd.Function):
    """`(h, LayerNorm(h) [+ pe])` as ONE autograd node (see _GroupNormSiLUSkip): backward = `d_skip + dX(norm)` in `fmc_layernorm_bwd_add`."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, pe, pe_inner, pe_frames):
        ctx.save_for_backward(x, gamma)
        ctx.eps = eps
        ctx.set_materialize_grads(False)
        return x.view_as(x), _layernorm_raw(x, gamma, beta, eps, pe, pe_inner, pe_frames)

    @staticmethod
    def backward(ctx, d_skip, dy):
        if dy is None:
            return d_skip, None, None, None, None, None, None
        add = None
        if d_skip is not None:
            add = d_skip if d_skip.is_contiguous() else d_skip.contiguous()
        dx, dg, db = _ln_backward(ctx, dy, add)
        return dx, dg, db, None, None, None, None


def layernorm_skip(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
                   pe: Optional[torch.Tensor] = None, pe_inner: int = 1, pe_frames: int = 1):
    """(x for the skip connection, LayerNorm(x)) -- one autograd node when x needs a gradient."""
    if torch.is_grad_enabled() and x.requires_grad and x.is_cuda and x.is_contiguous():
        return _LayerNormSkip.apply(x, gamma, beta, eps, pe, pe_inner, pe_frames)
    return x, layernorm(x, gamma, beta, eps, pe, pe_inner, pe_frames)


LAZY_RESIDUAL = os.environ.get("FMC_LAZY_RESIDUAL", "1") != "0"    # A/B switch: the residual add behind a vendor-arm projection rides in the next LayerNorm


def layernorm_add(x: torch.Tensor, addend: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
                  pe: Optional[torch.Tensor] = None, pe_inner: int = 1, pe_frames: int = 1):
    """`h = x + addend` (rounded to the storage type, as a separate add would) and `LayerNorm(h) (+ pe)` in one pass: returns (h, y)."""
    _dev(x, addend, gamma, beta, pe)
    assert x.is_contiguous() and addend.is_contiguous() and x.shape == addend.shape and x.dtype == addend.dtype
    C = x.shape[-1]
    M = x.numel() // C
    h, y = torch.empty_like(x), torch.empty_like(x)
    _lib.check(_lib.load().fmc_layernorm_add_fwd(x.data_ptr(), addend.data_ptr(), h.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                 _p(pe), M, C, float(eps), int(pe_inner), int(pe_frames), _dt(x), _stream()), "fmc_layernorm_add_fwd")
    return h, y


def resolve_pending_add(x: torch.Tensor) -> torch.Tensor:
    """A projection output whose residual add was left to its consumer (`linear(..., lazy_residual=True)` on the vendor arm): the sum."""
    r = getattr(x, "_fmc_pending_add", None)
    return x if r is None else torch.add(r, x)


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
              pe: Optional[torch.Tensor] = None, pe_inner: int = 1, pe_frames: int = 1) -> torch.Tensor:
    """LayerNorm over the last dim of contiguous tokens; optionally adds `pe[(row // pe_inner) % pe_frames]`
    (fp32 `[>=pe_frames, C]`) after normalising."""
    if torch.is_grad_enabled() and (x.requires_grad or gamma.requires_grad or beta.requires_grad):
        return _LayerNorm.apply(x, gamma, beta, eps, pe, pe_inner, pe_frames)
    return _layernorm_raw(x, gamma, beta, eps, pe, pe_inner, pe_frames)


def _layernorm_raw(x, gamma, beta, eps, pe, pe_inner, pe_frames):
    _dev(x, gamma, beta, pe)
    assert x.is_contiguous()
    C = x.shape[-1]
    M = x.numel() // C
    y = torch.empty_like(x)
    _lib.check(_lib.load().fmc_layernorm_fwd(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _p(pe), M,
                                             C, float(eps), int(pe_inner), int(pe_frames), _dt(x), _stream()),
               "fmc_layernorm_fwd")
    return y


class _Geglu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _geglu_raw(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        cff = x.shape[-1] // 2
        dx = torch.empty_like(x)
        _lib.check(_lib.load().fmc_geglu_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel() // (2 * cff), cff,
                                             _dt(x), _stream()), "fmc_geglu_bwd")
        return dx


def geglu(x: torch.Tensor) -> torch.Tensor:
    """`a * gelu_erf(g)` with `a, g = x.chunk(2, -1)`; x contiguous `[..., 2*Cff]`."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _Geglu.apply(x)
    return _geglu_raw(x)


def _geglu_raw(x: torch.Tensor) -> torch.Tensor:
    _dev(x)
    assert x.is_contiguous()
    cff = x.shape[-1] // 2
    M = x.numel() // (2 * cff)
    y = torch.empty(*x.shape[:-1], cff, dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().fmc_geglu_fwd(x.data_ptr(), y.data_ptr(), M, cff, _dt(x), _stream()), "fmc_geglu_fwd")
    return y


# --------------------------------------------------------------------------------------------
# attention
# --------------------------------------------------------------------------------------------
def _rows(t: torch.Tensor) -> Tuple[int, int]:
    """(batch stride, row stride) in elements of a `[B, S, C]` view whose last dim is dense."""
    assert t.ndim == 3 and t.stride(2) == 1, "attention operands must be [B, S, C] with a dense channel dim"
    return t.stride(0), t.stride(1)


def _split3(qkv: torch.Tensor):
    """The q | k | v slices of a fused `[.., 3C]` tensor."""
    C = qkv.shape[-1] // 3
    return qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]


def _split2(kv: torch.Tensor):
    """The k | v slices of a fused `[.., 2C]` tensor."""
    C = kv.shape[-1] // 2
    return kv[..., :C], kv[..., C:]


def _spatial_bwd(q, k, v, o, lse, d_o, dq, dk, dv, kbs, div, heads, scale, unwritten=(0, 0)) -> None:
    """`fmc_spatial_attn_bwd` into dq and dk / dv (both None: a frozen key/value side).  o and `d_o` are dense `[B, Sq, C]`; `kbs`: the batch stride K / V
    are read with, `div`: the batch entries that share one of them; `unwritten`: the strides named for dk / dv when there is none (inherited: each
    caller has its own pair, the kernels read neither)."""
    B, Sq, C = q.shape
    dvec = torch.empty(B, heads, Sq, dtype=torch.float32, device=q.device)
    dkb, dkr = (dk.stride(0), dk.stride(1)) if dk is not None else unwritten
    _lib.check(_lib.load().fmc_spatial_attn_bwd(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), dvec.data_ptr(), dq.data_ptr(), _p(dk), _p(dv), B, heads, Sq,
        k.shape[1], C // heads, q.stride(0), q.stride(1), kbs, k.stride(1), Sq * C, C, dq.stride(0), dq.stride(1), dkb, dkr, div, float(scale), _dt(q), _stream()),
        "fmc_spatial_attn_bwd")


class _SpatialAttention(torch.autograd.Function):
    """q `[B,S,C]`, kv-side tensors `[Bkv,Skv,C]` (strided slices allowed).  Grads come back as dense tensors."""

    @staticmethod
    def forward(ctx, q, k, v, heads, scale):
        o, lse = _spatial_attention_raw(q, k, v, heads, scale, True)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.heads, ctx.scale = heads, scale
        return o

    @staticmethod
    def backward(ctx, d_o):
        q, k, v, o, lse = ctx.saved_tensors
        dq = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        need_kv = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dk = torch.empty(k.shape, dtype=q.dtype, device=q.device) if need_kv else None
        dv = torch.empty(k.shape, dtype=q.dtype, device=q.device) if need_kv else None
        _spatial_bwd(q, k, v, o, lse, d_o.contiguous(), dq, dk, dv, k.stride(0), q.shape[0] // k.shape[0], ctx.heads, ctx.scale,
                     unwritten=(k.shape[1] * k.shape[2], k.shape[2]))
        return dq, dk, dv, None, None


def spatial_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: Optional[float] = None,
                      return_lse: bool = False):
    """softmax(Q K^T * scale) V per (batch, head); differentiable (fmc_spatial_attn_bwd)."""
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad) and not return_lse:
        sc = (q.shape[-1] // heads) ** -0.5 if scale is None else scale
        return _SpatialAttention.apply(q, k, v, heads, sc)
    return _spatial_attention_raw(q, k, v, heads, scale, return_lse)


def _spatial_attention_raw(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: Optional[float] = None,
                           return_lse: bool = False):
    """softmax(Q K^T * scale) V per (batch, head).  q `[B, Sq, H*D]`, k/v `[Bkv, Skv, H*D]` (strided views of a
    fused projection are fine; B must be a multiple of Bkv: batch b reads kv batch b // (B // Bkv))."""
    _dev(q, k, v)
    B, Sq, C = q.shape
    Bkv, Skv, _ = k.shape
    assert C % heads == 0 and k.shape == v.shape and k.shape[2] == C and B % Bkv == 0
    assert k.stride() == v.stride(), "k and v must share strides (slices of one fused projection)"
    D = C // heads
    scale = D ** -0.5 if scale is None else scale
    o = torch.empty(B, Sq, C, dtype=q.dtype, device=q.device)
    lse = torch.empty(B, heads, Sq, dtype=torch.float32, device=q.device) if return_lse else None
    qb, qr = _rows(q)
    kb, kr = _rows(k)
    _lib.check(_lib.load().fmc_spatial_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), _p(lse), B,
                                                heads, Sq, Skv, D, qb, qr, kb, kr, Sq * C, C, B // Bkv, float(scale),
                                                _dt(q), _stream()), "fmc_spatial_attn_fwd")
    return (o, lse) if return_lse else o


def attention_ok(head_dim: int) -> bool:
    return head_dim in (32, 64, 128, 256, 512)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: Optional[float] = None, causal: bool = False,
              key_keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(Q K^T scale + mask) V per (batch, head) on `fmc_attention_fwd` (csrc/attn_generic.hip): head widths 32 .. 512 and masked scores -- the VAE
    mid block's single head of width 512 and CLIP's causal text attention (once per clip, no autograd).  q `[B, Sq, H D]`, k / v
    `[B, Skv, H D]` (strided views of a fused projection are fine), `key_keep [B, Skv]` bool / uint8 (True = attend) or None."""
    _dev(q, k, v, key_keep)
    B, Sq, C = q.shape
    Bk, Skv, _ = k.shape
    assert C % heads == 0 and k.shape == v.shape and k.shape[2] == C and Bk == B and k.stride() == v.stride() and q.dtype == k.dtype == v.dtype
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        raise NotImplementedError("hip_ops.attention is forward-only (VAE / text encoder are frozen in every FMC stage)")
    D = C // heads
    if not _lib.load().fmc_attention_supported(D):
        raise ValueError(f"hip_ops.attention: head width {D} (supported: 32, 64, 128, 256, 512)")
    scale = D ** -0.5 if scale is None else scale
    o = torch.empty(B, Sq, C, dtype=q.dtype, device=q.device)
    keep = None
    if key_keep is not None:
        keep = key_keep.to(torch.uint8).contiguous()
        assert tuple(keep.shape) == (B, Skv)
    qb, qr = _rows(q)
    kb, kr = _rows(k)
    _lib.check(_lib.load().fmc_attention_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), _p(keep), B, heads, Sq, Skv, D, qb, qr, kb, kr,
                                             Sq * C, C, float(scale), int(causal), _dt(q), _stream()), "fmc_attention_fwd")
    return o


def _tstrides(t):
    """(clips, pixels, frames, clip stride, frame stride, pixel stride) of the native `[B, F, P, C]` layout or of `[N, F, C]` (one clip of N pixels)."""
    if t.ndim == 4:
        return t.shape[0], t.shape[2], t.shape[1], t.stride(0), t.stride(1), t.stride(2)
    return 1, t.shape[0], t.shape[1], 0, t.stride(1), t.stride(0)


def _temporal_bwd(q, k, v, d_o, dqkv, heads, scale, scales=None) -> None:
    """`fmc_temporal_attn_bwd` into the slices of the fused `[.., 3C]` gradient `dqkv`; with `scales` (the three fp8 scales of the forward) q, k, v are
    e4m3 bytes and the call is `fmc_temporal_attn_fp8_bwd` (bf16 `d_o` and gradients)."""
    dq, dk, dv = _split3(dqkv)
    B, P, F, cs, fs, ps = _tstrides(q)
    args = (d_o.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, P, F, heads, q.shape[-1] // heads, cs, fs, ps, *_tstrides(d_o)[3:], *_tstrides(dq)[3:],
            float(scale))
    L = _lib.load()
    if scales is None:
        _lib.check(L.fmc_temporal_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), *args, _dt(q), _stream()), "fmc_temporal_attn_bwd")
    else:
        _lib.check(L.fmc_temporal_attn_fp8_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), scales.data_ptr(), *args, _stream()), "fmc_temporal_attn_fp8_bwd")


class _TemporalAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, heads, scale):
        ctx.save_for_backward(q, k, v)
        ctx.heads, ctx.scale = heads, scale
        return _temporal_attention_raw(q, k, v, heads, scale)

    @staticmethod
    def backward(ctx, d_o):
        q, k, v = ctx.saved_tensors
        dqkv = torch.empty(*q.shape[:-1], 3 * q.shape[-1], dtype=q.dtype, device=q.device)   # fused [.., 3C] gradient
        _temporal_bwd(q, k, v, d_o.contiguous(), dqkv, ctx.heads, ctx.scale)
        return (*_split3(dqkv), None, None)


class _SelfAttentionQKV(torch.autograd.Function):
    """Self attention on the fused projection output `qkv [.., 3C]`; the backward kernels write dQ | dK | dV straight
    into ONE `[.., 3C]` gradient through their stride arguments.  (Passing the three slices through autograd instead
    costs, per attention, three zero-fills of the fused shape, three slice copies and two adds.)"""

    @staticmethod
    def forward(ctx, qkv, heads, scale, temporal):
        q, k, v = _split3(qkv)
        ctx.heads, ctx.scale, ctx.temporal = heads, scale, temporal
        if temporal:
            ctx.save_for_backward(qkv)
            return _temporal_attention_raw(q, k, v, heads, scale)
        o, lse = _spatial_attention_raw(q, k, v, heads, scale, True)
        ctx.save_for_backward(qkv, o, lse)
        return o

    @staticmethod
    def backward(ctx, d_o):
        qkv = ctx.saved_tensors[0]
        q, k, v = _split3(qkv)
        d_o = d_o.contiguous()
        dqkv = torch.empty(qkv.shape, dtype=qkv.dtype, device=qkv.device)
        if ctx.temporal:
            _temporal_bwd(q, k, v, d_o, dqkv, ctx.heads, ctx.scale)
        else:
            _, o, lse = ctx.saved_tensors
            _spatial_bwd(q, k, v, o, lse, d_o, *_split3(dqkv), k.stride(0), 1, ctx.heads, ctx.scale)
        return dqkv, None, None, None


class _CrossAttentionQKV(torch.autograd.Function):
    """Cross attention with the fused `kv [Bkv, Skv, 2C]` projection; one fused dK | dV gradient."""

    @staticmethod
    def forward(ctx, q, kv, heads, scale):
        o, lse = _spatial_attention_raw(q, *_split2(kv), heads, scale, True)
        ctx.save_for_backward(q, kv, o, lse)
        ctx.heads, ctx.scale = heads, scale
        return o

    @staticmethod
    def backward(ctx, d_o):
        q, kv, o, lse = ctx.saved_tensors
        B, Bkv = q.shape[0], kv.shape[0]
        k, v = _split2(kv)
        dq = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        div, kbs = B // Bkv, k.stride(0)
        if not ctx.needs_input_grad[1]:
            # frozen to_k / to_v on a constant text embedding (every FMC training stage): no dK / dV kernel at all
            dkv = None
        elif Bkv == 1 and div > 1:
            # one text for all frames: per-frame partial dK | dV (batch stride 0 on K / V keeps B x heads workgroups
            # busy instead of `heads`), summed over the frames afterwards
            dkv, div, kbs = torch.empty(B, *kv.shape[1:], dtype=q.dtype, device=q.device), 1, 0
        else:
            dkv = torch.empty(kv.shape, dtype=q.dtype, device=q.device)
        dk, dv = _split2(dkv) if dkv is not None else (None, None)
        _spatial_bwd(q, k, v, o, lse, d_o.contiguous(), dq, dk, dv, kbs, div, ctx.heads, ctx.scale, unwritten=(0, kv.shape[2]))
        if dkv is not None and dkv.shape[0] != Bkv:
            dkv = dkv.sum(0, keepdim=True, dtype=torch.float32).to(q.dtype)
        return dq, dkv, None, None


def self_attention_qkv(qkv: torch.Tensor, heads: int, scale: float, temporal: bool) -> torch.Tensor:
    """Attention on a fused `[.., 3C]` projection (q | k | v); differentiable with a single fused gradient."""
    if torch.is_grad_enabled() and qkv.requires_grad:
        return _SelfAttentionQKV.apply(qkv, heads, scale, temporal)
    q, k, v = _split3(qkv)
    return _temporal_attention_raw(q, k, v, heads, scale) if temporal else _spatial_attention_raw(q, k, v, heads, scale)


def cross_attention_q_kv(q: torch.Tensor, kv: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """Cross attention with a fused `[.., 2C]` (k | v) projection; differentiable with a fused dK | dV gradient."""
    if torch.is_grad_enabled() and (q.requires_grad or kv.requires_grad):
        return _CrossAttentionQKV.apply(q, kv, heads, scale)
    return _spatial_attention_raw(q, *_split2(kv), heads, scale)


def temporal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int,
                       scale: Optional[float] = None) -> torch.Tensor:
    """Attention over the frame axis (see `_temporal_attention_raw`); differentiable (fmc_temporal_attn_bwd)."""
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        sc = (q.shape[-1] // heads) ** -0.5 if scale is None else scale
        return _TemporalAttention.apply(q, k, v, heads, sc)
    return _temporal_attention_raw(q, k, v, heads, scale)


def _temporal_attention_raw(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int,
                            scale: Optional[float] = None) -> torch.Tensor:
    """Attention over the frame axis.  Accepts the native layout `[B, F, P, C]` (frames outer, pixels inner: the
    channels-last video) or the reference layout `[N, F, C]` (`(b h w) f c`).  q/k/v may be strided slices of a
    fused QKV tensor (same strides for all three).  Returns a contiguous tensor of q's shape."""
    _dev(q, k, v)
    assert q.shape == k.shape == v.shape and q.stride() == k.stride() == v.stride() and q.stride(-1) == 1
    C = q.shape[-1]
    D = C // heads
    scale = D ** -0.5 if scale is None else scale
    o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    if q.ndim not in (3, 4):
        raise ValueError("temporal_attention expects [B, F, P, C] or [N, F, C]")
    _lib.check(_lib.load().fmc_temporal_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), *_tstrides(q)[:3], heads, D, *_tstrides(q)[3:],
                                                 *_tstrides(o)[3:], float(scale), _dt(q), _stream()), "fmc_temporal_attn_fwd")
    return o


# --------------------------------------------------------------------------------------------
# fp8 (e4m3) temporal attention: QKV projection with an fp8 epilogue + attention on fp8 MFMA (BASELINE configs[4])
# --------------------------------------------------------------------------------------------
FP8_MAX = 448.0


class Fp8QKVScales:
    """Per-attention-module scale state for the fp8 q | k | v tensors (delayed scaling: the scales of call t come from the
    running |max| the projection's epilogue recorded in call t - 1).  Everything lives on the device and is updated by
    device ops only, so a captured HIP graph replays it.  `margin` leaves headroom for a max that grows between calls
    (values beyond it saturate at +-448 * scale)."""

    def __init__(self, device, margin: float = 1.25):
        self.margin = margin
        self.amax = torch.zeros(3, dtype=torch.float32, device=device)       # float bit patterns, written by atomicMax
        self.scale = torch.ones(3, dtype=torch.float32, device=device)
        self.inv_scale = torch.ones(3, dtype=torch.float32, device=device)
        self.calibrated = False

    def calibrate(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> None:
        """First call: take the maxima from a bf16 projection."""
        self.amax.copy_(torch.stack([q.abs().amax(), k.abs().amax(), v.abs().amax()]).float())
        self.calibrated = True

    def roll(self) -> None:
        """scale <- margin * amax / 448, inv_scale <- 1 / scale, then restart the running max: one tiny launch."""
        _lib.check(_lib.load().fmc_fp8_scales_roll(self.amax.data_ptr(), self.scale.data_ptr(), self.inv_scale.data_ptr(),
                                                   float(self.margin), _stream()), "fmc_fp8_scales_roll")


def linear_fp8_qkv(x: torch.Tensor, weight: torch.Tensor, scales: Fp8QKVScales) -> torch.Tensor:
    """`x @ weight^T` -> `[..., 3C]` e4m3 bytes (torch.float8_e4m3fn), block b scaled by `scales.inv_scale[b]`; records |max|."""
    _dev(x, weight)
    N, Kd = weight.shape
    assert x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and weight.is_contiguous()
    assert N % 192 == 0 and Kd % 64 == 0, "fp8 QKV projection needs C % 64 == 0 and K % 64 == 0"
    M, ldx = _rows2d(x)
    out = torch.empty(*x.shape[:-1], N, dtype=torch.float8_e4m3fn, device=x.device)
    _lib.check(_lib.load().fmc_linear_fp8_qkv(x.data_ptr(), weight.data_ptr(), out.data_ptr(), M, N, Kd, ldx,
                                              scales.inv_scale.data_ptr(), scales.amax.data_ptr(), _stream()),
               "fmc_linear_fp8_qkv")
    return out


def _temporal_fp8_raw(qkv8: torch.Tensor, scale_dev: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    q, k, v = _split3(qkv8)
    C = q.shape[-1]
    o = torch.empty(*qkv8.shape[:-1], C, dtype=torch.bfloat16, device=qkv8.device)
    _lib.check(_lib.load().fmc_temporal_attn_fp8_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), scale_dev.data_ptr(), *_tstrides(q)[:3], heads,
                                                     C // heads, *_tstrides(q)[3:], *_tstrides(o)[3:], float(scale), _stream()), "fmc_temporal_attn_fp8_fwd")
    return o


class _TemporalAttentionFp8(torch.autograd.Function):
    """Projection (fp8 epilogue) + fp8 temporal attention as ONE autograd node: x -> o.  Backward: the attention backward
    kernel dequantises the saved e4m3 q | k | v while staging them (straight-through w.r.t. the quantisation), writes one
    fused bf16 dQ | dK | dV, and the projection's input gradient is `dqkv @ W` (frozen weight) -- or dW as well when the
    weight trains (camera encoder)."""

    @staticmethod
    def forward(ctx, x, weight, scales, heads, scale):
        qkv8 = linear_fp8_qkv(x, weight, scales)
        sc = scales.scale.clone()                     # the scales THIS call used (the state rolls on)
        ctx.save_for_backward(x, weight, qkv8, sc)
        ctx.heads, ctx.scale = heads, scale
        return _temporal_fp8_raw(qkv8, sc, heads, scale)

    @staticmethod
    def backward(ctx, d_o):
        x, weight, qkv8, sc = ctx.saved_tensors
        dqkv = torch.empty(qkv8.shape, dtype=torch.bfloat16, device=qkv8.device)
        _temporal_bwd(*_split3(qkv8), d_o.contiguous(), dqkv, ctx.heads, ctx.scale, scales=sc)
        dx = None
        if ctx.needs_input_grad[0]:                  # frozen weight: own GEMM on the cached W^T; a training weight: plain matmul
            dx = torch.matmul(dqkv, weight) if weight.requires_grad else linear_backward_data(dqkv, weight)
        dw = None
        if ctx.needs_input_grad[1]:
            dw = torch.matmul(dqkv.reshape(-1, dqkv.shape[-1]).t(), x.reshape(-1, x.shape[-1]))
        return dx, dw, None, None, None


def temporal_attention_fp8(x: torch.Tensor, weight: torch.Tensor, scales: Fp8QKVScales, heads: int, scale: float):
    """o = temporal_attention(split(x @ W_qkv^T)) with e4m3 q | k | v (native `[B, F, P, C]` tokens or `[N, F, C]`).
    The first call on a fresh `scales` runs the bf16 path once to calibrate the maxima."""
    if not scales.calibrated:
        with torch.no_grad():
            scales.calibrate(*_split3(linear(x.detach(), weight.detach())))
    scales.roll()
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
        return _TemporalAttentionFp8.apply(x, weight, scales, heads, scale)
    qkv8 = linear_fp8_qkv(x, weight, scales)
    return _temporal_fp8_raw(qkv8, scales.scale, heads, scale)


# --------------------------------------------------------------------------------------------
# conditioning
# --------------------------------------------------------------------------------------------
def plucker(K: torch.Tensor, c2w: torch.Tensor, H: int, W: int, layout: str = "bfhwc",
            dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Pluecker embedding on device.  K `[B, F, 4]`, c2w `[B, F, 3|4, 4]` (fp32).
    layout "bfhwc": `[B,F,H,W,6]` (= ray_condition); "bcfhw": `[B,6,F,H,W]`;
    "unshuffle8": `[B*F, H/8, W/8, 384]` channels-last with PixelUnshuffle(8) applied."""
    _dev(K, c2w)
    B, F = K.shape[:2]
    K = K.to(torch.float32).contiguous()
    c2w = c2w.to(torch.float32).contiguous()
    rows = c2w.shape[2]
    code = {"bfhwc": 0, "bcfhw": 1, "unshuffle8": 2}[layout]
    shape = {0: (B, F, H, W, 6), 1: (B, 6, F, H, W), 2: (B * F, H // 8, W // 8, 384)}[code]
    out = torch.empty(shape, dtype=dtype, device=K.device)
    _lib.check(_lib.load().fmc_plucker_fwd(K.data_ptr(), c2w.data_ptr(), out.data_ptr(), B, F, H, W, rows, code,
                                           _dt(out), _stream()), "fmc_plucker_fwd")
    return out


def gaussian_circle_masks(circles: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """circles `[..., 3]` = (cx, cy, radius) pixels -> Gaussian circle masks `[..., H, W]` fp32 (dataset.py:5365-5380)."""
    _dev(circles)
    c = circles.to(torch.float32).contiguous()
    out = torch.empty(*c.shape[:-1], H, W, dtype=torch.float32, device=c.device)
    _lib.check(_lib.load().fmc_gaussian_circle_mask_fwd(c.data_ptr(), out.data_ptr(), c.numel() // 3, H, W, _stream()),
               "fmc_gaussian_circle_mask_fwd")
    return out


def omc_rasterize(poses: torch.Tensor, masks: torch.Tensor, layout: str = "planar",
                  dtype: torch.dtype = torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """poses `[BF, n_obj, 12]`, masks `[BF, n_obj, H, W]` (fp32) -> (features, mask).
    "planar": features `[BF,13,H,W]`, mask `[BF,1,H,W]`; "unshuffle8": features `[BF,H/8,W/8,832]`, mask `[BF,H,W]`."""
    _dev(poses, masks)
    BF, n_obj, H, W = masks.shape
    poses = poses.to(torch.float32).contiguous()
    masks = masks.to(torch.float32).contiguous()
    code = {"planar": 0, "unshuffle8": 2}[layout]
    feat = torch.empty((BF, 13, H, W) if code == 0 else (BF, H // 8, W // 8, 832), dtype=dtype, device=masks.device)
    mout = torch.empty((BF, 1, H, W) if code == 0 else (BF, H, W), dtype=torch.float32, device=masks.device)
    _lib.check(_lib.load().fmc_omc_rasterize_fwd(poses.data_ptr(), masks.data_ptr(), feat.data_ptr(), mout.data_ptr(),
                                                 BF, n_obj, H, W, code, _dt(feat), _stream()), "fmc_omc_rasterize_fwd")
    return feat, mout


def _mask_modulate_raw(x, mask_in, h, w, want_mask):
    N, S, C = x.shape
    y = torch.empty_like(x)
    mo = torch.empty(N, h, w, dtype=torch.float32, device=x.device) if want_mask else None
    _lib.check(_lib.load().fmc_mask_modulate_fwd(x.data_ptr(), mask_in.data_ptr(), y.data_ptr(), _p(mo), N, h, w, C,
                                                 mask_in.shape[1], mask_in.shape[2], _dt(x), _stream()),
               "fmc_mask_modulate_fwd")
    return y, mo


class _MaskModulate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask_in, h, w):
        y, mo = _mask_modulate_raw(x, mask_in, h, w, True)
        ctx.save_for_backward(mask_in)
        ctx.hw = (h, w)
        ctx.mark_non_differentiable(mo)
        return y, mo

    @staticmethod
    def backward(ctx, dy, _dmo):
        (mask_in,) = ctx.saved_tensors
        dx, _ = _mask_modulate_raw(dy.contiguous(), mask_in, ctx.hw[0], ctx.hw[1], False)
        return dx, None, None, None


def mask_modulate(x: torch.Tensor, mask_in: torch.Tensor, h: int, w: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """`x * nearest(mask_in -> h x w)`; x `[N, h*w, C]` tokens, mask_in `[N, Hin, Win]` fp32.
    Returns (y, resampled mask `[N, h, w]`)."""
    _dev(x, mask_in)
    assert x.is_contiguous() and mask_in.is_contiguous() and mask_in.dtype == torch.float32
    assert x.shape[1] == h * w
    if torch.is_grad_enabled() and x.requires_grad:
        return _MaskModulate.apply(x, mask_in, h, w)
    return _mask_modulate_raw(x, mask_in, h, w, True)


class _FeatureAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, t, skip):
        ctx.skip, ctx.tshape = skip, t.shape
        return _feature_add_raw(h, t, skip, False)

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        return dy, dy.reshape(-1)[ctx.skip:].reshape(ctx.tshape), None


def _feature_add_raw(h, t, skip, inplace):
    out = h if inplace else torch.empty_like(h)
    _lib.check(_lib.load().fmc_feature_add_fwd(h.data_ptr(), t.data_ptr(), out.data_ptr(), h.numel(), skip, _dt(h),
                                               _stream()), "fmc_feature_add_fwd")
    return out


def feature_add(h: torch.Tensor, t: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """`h + t` where `t` covers only the LAST `t.numel()` elements of `h` (the conditioned half under
    classifier-free guidance; the leading elements get nothing added)."""
    _dev(h, t)
    assert h.is_contiguous() and t.is_contiguous() and h.dtype == t.dtype and t.numel() <= h.numel()
    skip = h.numel() - t.numel()
    if torch.is_grad_enabled() and (h.requires_grad or t.requires_grad):
        out = _FeatureAdd.apply(h, t, skip)
        return out
    return _feature_add_raw(h, t, skip, inplace)


def cfg_ddim_step(eps: torch.Tensor, x: torch.Tensor, guidance: float, alpha_t: float, alpha_prev: float,
                  has_uncond: bool) -> torch.Tensor:
    """Fused classifier-free-guidance combine + DDIM(eta=0) update.  eps `[2B, ...]` (uncond || cond) or `[B, ...]`;
    x fp32 latents `[B, ...]`.  Returns the new fp32 latents."""
    _dev(eps, x)
    assert x.dtype == torch.float32 and x.is_contiguous() and eps.is_contiguous()
    n = x.numel()
    assert eps.numel() == (2 * n if has_uncond else n)
    out = torch.empty_like(x)
    _lib.check(_lib.load().fmc_cfg_ddim_step(eps.data_ptr(), x.data_ptr(), out.data_ptr(), n, int(has_uncond),
                                             float(guidance), float(alpha_t), float(alpha_prev), _dt(eps), _stream()),
               "fmc_cfg_ddim_step")
    return out


def sampler_step_elems_per_trip() -> int:
    return int(_lib.load().fmc_sampler_step_elems_per_trip())


def sampler_step(eps: torch.Tensor, x: torch.Tensor, *, guidance: float = 1.0, has_uncond: bool = False, m_x: float = 0.0,
                 m_e: float = 0.0, m_clamp: float = 0.0, c_x: float = 1.0, c_e: float = 0.0, c_m: float = 0.0, c_n: float = 0.0,
                 c_h=(), hist=(), noise: Optional[torch.Tensor] = None, x_out: Optional[torch.Tensor] = None,
                 m_out: Optional[torch.Tensor] = None, x_in: Optional[torch.Tensor] = None, in_scale: float = 1.0) -> torch.Tensor:
    """Fused classifier-free-guidance combine + one sampler step (`fmc_sampler_step`; the formula is in include/fmc_hip.h).
    eps `[2B, ...]` (uncond || cond) or `[B, ...]`, x fp32 latents `[B, ...]`, `hist` up to three fp32 tensors like x with their
    coefficients `c_h`, `noise` like x in eps's dtype.  `x_out` may be x, `m_out` may be one of `hist`; `x_in` `[B or 2B, ...]`
    receives `in_scale * x'` in its own dtype (the next model input).  Returns `x_out` (a new tensor when not given)."""
    _dev(eps, x, noise, x_out, m_out, x_in, *hist)
    n = x.numel()
    assert x.dtype == torch.float32 and x.is_contiguous() and eps.is_contiguous()
    assert eps.numel() == (2 * n if has_uncond else n)
    assert len(hist) == len(c_h) <= 3 and all(h.dtype == torch.float32 and h.is_contiguous() and h.numel() == n for h in hist)
    assert noise is None or (noise.dtype == eps.dtype and noise.is_contiguous() and noise.numel() == n)
    assert m_out is None or (m_out.dtype == torch.float32 and m_out.is_contiguous() and m_out.numel() == n)
    if x_out is None:
        x_out = torch.empty_like(x)
    assert x_out.dtype == torch.float32 and x_out.is_contiguous() and x_out.numel() == n
    in_reps = 0
    if x_in is not None:
        assert x_in.is_contiguous() and x_in.numel() in (n, 2 * n)
        in_reps = x_in.numel() // n
    coef = _lib.SamplerCoef(float(guidance), float(m_x), float(m_e), float(m_clamp), float(c_x), float(c_e), float(c_m), float(c_n),
                            (ctypes.c_float * 3)(*[float(c) for c in c_h]), float(in_scale))
    hp = [h.data_ptr() for h in hist] + [None] * (3 - len(hist))
    _log_call("sampler_step", (n, int(has_uncond), len(hist), noise is not None, in_reps), 0.0)
    _lib.check(_lib.load().fmc_sampler_step(eps.data_ptr(), x.data_ptr(), _p(noise), hp[0], hp[1], hp[2], x_out.data_ptr(), _p(m_out),
                                            _p(x_in), n, int(has_uncond), len(hist), in_reps, coef, _dt(eps),
                                            _dt(x_in) if x_in is not None else _dt(eps), _stream()), "fmc_sampler_step")
    return x_out


def _window_view(t: torch.Tensor, what: str):
    """`[R, W, B, C, F, ...]` with the trailing `[B, C, F, ...]` block dense -> (stride_r, stride_w) in elements."""
    assert t.ndim >= 6, f"{what}: [R, W, B, C, F, ...]"
    assert t[0, 0].is_contiguous(), f"{what}: every [B, C, F, ...] block has to be dense"
    return int(t.stride(0)), int(t.stride(1))


def window_step(eps: torch.Tensor, x: torch.Tensor, *, overlap: int, guidance: float = 1.0, m_x: float = 0.0, m_e: float = 0.0,
                m_clamp: float = 0.0, c_x: float = 1.0, c_e: float = 0.0, c_m: float = 0.0, c_n: float = 0.0, c_h=(), hist=(),
                noise: Optional[torch.Tensor] = None, x_out: Optional[torch.Tensor] = None, m_out: Optional[torch.Tensor] = None,
                x_in: Optional[torch.Tensor] = None, in_scale: float = 1.0) -> torch.Tensor:
    """Sliding windows: the average of the windows' guided predictions + one sampler step (`fmc_window_step`; the formula is in
    include/fmc_hip.h).  eps `[R, W, B, C, F, ...]` with R = 2 (uncond, cond) or 1, x fp32 latents `[B, C, Ftot, ...]` with
    `Ftot = W (F - overlap) + overlap`; `hist`, `noise`, `m_out` like x.  eps and `x_in` `[R', W, B, C, F, ...]` (R' = 1 or 2) may be
    any view whose `[B, C, F, ...]` blocks are dense: `[W, R, B, ...]` storage is `t.transpose(0, 1)`.  `x_in` receives
    `in_scale * x'` at every covering window's own frame.  Returns `x_out` (a new tensor when not given)."""
    _dev(eps, x, noise, x_out, m_out, x_in, *hist)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.ndim >= 4
    R, W, B, C, F = (int(v) for v in eps.shape[:5])
    e_sr, e_sw = _window_view(eps, "eps")
    stride = F - int(overlap)
    hw = int(math.prod(x.shape[3:]))
    assert R in (1, 2) and tuple(x.shape[:2]) == (B, C) and tuple(eps.shape[5:]) == tuple(x.shape[3:])
    if stride < 1 or overlap < 0:
        raise ValueError(f"window_step: overlap {overlap} of windows of {F} frames")
    assert x.shape[2] == (W - 1) * stride + F, f"window_step: {W} windows of {F} frames overlapping by {overlap} cover " \
                                               f"{(W - 1) * stride + F} frames, the latents hold {x.shape[2]}"
    n = x.numel()
    assert len(hist) == len(c_h) <= 3 and all(h.dtype == torch.float32 and h.is_contiguous() and h.numel() == n for h in hist)
    assert noise is None or (noise.dtype == eps.dtype and noise.is_contiguous() and noise.numel() == n)
    assert m_out is None or (m_out.dtype == torch.float32 and m_out.is_contiguous() and m_out.numel() == n)
    if x_out is None:
        x_out = torch.empty_like(x)
    assert x_out.dtype == torch.float32 and x_out.is_contiguous() and x_out.numel() == n
    in_reps, i_sr, i_sw = 0, 0, 0
    if x_in is not None:
        assert tuple(x_in.shape[1:]) == tuple(eps.shape[1:]) and x_in.shape[0] in (1, 2)
        in_reps = int(x_in.shape[0])
        i_sr, i_sw = _window_view(x_in, "x_in")
    coef = _lib.SamplerCoef(float(guidance), float(m_x), float(m_e), float(m_clamp), float(c_x), float(c_e), float(c_m), float(c_n),
                            (ctypes.c_float * 3)(*[float(c) for c in c_h]), float(in_scale))
    hp = [h.data_ptr() for h in hist] + [None] * (3 - len(hist))
    _log_call("window_step", (n, W, F, int(overlap), R, len(hist), noise is not None, in_reps), 0.0)
    _lib.check(_lib.load().fmc_window_step(eps.data_ptr(), e_sr, e_sw, x.data_ptr(), _p(noise), hp[0], hp[1], hp[2], x_out.data_ptr(),
                                           _p(m_out), _p(x_in), i_sr, i_sw, B * C, F, stride, W, hw, int(R == 2), len(hist), in_reps, coef,
                                           _dt(eps), _dt(x_in) if x_in is not None else _dt(eps), _stream()), "fmc_window_step")
    return x_out


# --------------------------------------------------------------------------------------------
# bf16 MFMA GEMM / implicit 3x3 conv with fused epilogues
# --------------------------------------------------------------------------------------------
ARM_160 = 512
ARM_256 = 528                       # C-ABI tile 17: persistent 256 x 320 tiles, GEGLU projections only (falls back to tile 16)
ARM_SMALLM = 600                    # C-ABI tiles 19 .. 22: 64 x 128 (4 waves, 64- / 32-deep k-tiles), 128 x 128 and 64 x 256 (8 waves) with 32 x 64 per wave, for M <= 2560 (round 4)
ARM_G4 = 700                        # `fmc_linear4_bf16` (csrc/gemm4.hip, round 5): 160 x 160 tiles, 4 waves, software-pipelined -- the M <= 5120 projections of the inner levels
ARM_160B = 544                      # C-ABI tile 18: tile 16 reading the weight pre-packed tile-major (`_w_tilemajor`): linear 1-KiB operand requests


def _decode_arm(tile: int, split_k: int):
    """autotune arm id -> (C-ABI tile id, split_k).  Ids 16..127 encode split-K (geometry + 16 log2(split)), 128+ / 256+ stream-K and its
    hybrid; ARM_160 (512) is the C-ABI tile 16, the 160 x 320 kernel."""
    if ARM_SMALLM <= tile < ARM_SMALLM + 4:            # 600 .. 603: the small-M tiles of 32 x 64 per wave (C-ABI tiles 19 .. 22)
        return 19 + tile - ARM_SMALLM, 1
    if tile == ARM_256:
        return 17, 1
    if ARM_160B <= tile < ARM_160B + 5:                # 544 + log2(split): the same on the tile-major weight copy
        return 18, 1 << (tile - ARM_160B)
    if ARM_160 <= tile < ARM_160 + 5:                  # 512 + log2(split): the 160 x 320 kernel, split-K 1 / 2 / 4 / 8 / 16
        return 16, 1 << (tile - ARM_160)
    if tile >= 384:
        return tile - 384, -3                           # k-lockstep split on the 8-phase arms (round 4): chunks of every tile's reduction, an XCD's CUs on the same chunk
    if tile >= 256:
        return tile - 256, -2                           # whole rounds on the plain grid, the last partial round stream-K (8-phase arms)
    if tile >= 128:
        return tile - 128, -1                           # stream-K
    if tile >= 16:
        return tile & 15, 1 << (tile >> 4)
    return tile, split_k


_sk_ws = {}


def _streamk_workspace(device):
    """[4 KiB of flags | fp32 partial tiles] for the stream-K arms: zero on first use, handed back zeroed by the kernel.
    One per (device, stream): two streams running stream-K launches at once must not share flags / partial slots."""
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    ws = _sk_ws.get(key)
    if ws is None:
        # (8-phase arms: <= 7 slots per CU.)  Only the flag words must start at zero; the partial slots are written before they are
        # read.  A full torch.zeros here was a 486 MB fill -- and, first reached under graph capture (the capture stream is a new
        # key), one that was replayed with every step: 60 us of the 16x320x512 step.
        ws = torch.empty((4096 + 1856 * 256 * 256 * 4) // 4, dtype=torch.float32, device=device)
        ws[:1024].zero_()
        _sk_ws[key] = ws
    return ws.data_ptr(), ws.numel() * 4


def prepare_streamk_workspace(stream) -> None:
    """Create and zero the stream-K workspace of `stream` EAGERLY.  Call before capturing a HIP graph on that stream: first reached under
    capture, the flag words' zero fill is only recorded into THAT graph, and a second graph captured on the same stream and replayed first
    would run the flag-based stream-K arms on uninitialised flags."""
    with torch.cuda.stream(stream):
        _streamk_workspace(torch.device("cuda", torch.cuda.current_device()))
    stream.synchronize()


def release_streamk_workspace(stream) -> None:
    """Drop the workspace of a stream that is going away (a discarded graph runner): 486 MB per key otherwise stay allocated."""
    dev = getattr(getattr(stream, "device", None), "index", None)          # the stream's own device, not whichever is current when a runner dies
    _sk_ws.pop((torch.cuda.current_device() if dev is None else dev, stream.cuda_stream), None)


def _splitk_workspace(device, split_k: int, M: int, N: int):
    if split_k < 0:                                     # -1 / -2 / -3 / <= -16: the stream-K forms
        return _streamk_workspace(device)
    if split_k <= 1:
        return None, 0
    nbytes = split_k * M * N * 4
    return _workspace(device, nbytes).data_ptr(), nbytes


def split_arms(M: int, N: int, Kd: int):
    """extra autotune arms for problems whose 128x128 output tiles cannot fill the 256 CUs: split-K 2 / 4 (/ 8)"""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles > 320 or Kd < 1024:
        return ()
    arms = [t + 16 * si for si in (1, 2) for t in (1, 2, 9)]
    if tiles <= 128 and Kd >= 4096:
        arms += [1 + 16 * 3, 9 + 16 * 3]
    if N % 320 == 0:                                    # 160 x 320 tiles with split-K: as many workgroups as CUs, whole rounds
        t160 = ((M + 159) // 160) * (N // 320)
        arms += [(ARM_160B if W_TILEMAJOR else ARM_160) + si for si in (1, 2, 3, 4) if 128 <= t160 * (1 << si) <= 512 and Kd // 32 >= 8 * (1 << si)]
    return tuple(arms)


W_TILEMAJOR = os.environ.get("FMC_W_TILEMAJOR", "1") != "0"      # A/B switch: the 160 x 320 kernels read weights pre-packed tile-major (tile 18)


def _w_tilemajor(weight: torch.Tensor) -> torch.Tensor:
    """`[N, K]` projection weight -> `[N / 320][K / 32][320][32]`: what tile 18 reads (a W piece of a sub-tile = one contiguous KiB)."""
    N, Kd = weight.shape
    return derived_on_owner(weight, "_fmc_wtm", "lin",
                            lambda: weight.detach().reshape(N // 320, 320, Kd // 32, 32).permute(0, 2, 1, 3).contiguous())


def _w_tilemajor_conv(weight_cl: torch.Tensor) -> torch.Tensor:
    """Channels-last 3x3 filter (physically `[Cout][3][3][Cin]`) -> `[Cout / 320][Cin / 64][9 taps][2 halves][320][32]`: the conv kernel's own
    sub-tile order (64-channel chunk, tap, 32-channel half)."""
    def build():
        cout, cin = weight_cl.shape[:2]
        w = weight_cl.detach().permute(0, 2, 3, 1).reshape(cout // 320, 320, 9, cin // 64, 2, 32)      # [nt][row][tap][chunk][half][32]
        return w.permute(0, 3, 2, 4, 1, 5).contiguous()                                                # [nt][chunk][tap][half][row][32]
    return derived_on_owner(weight_cl, "_fmc_wtm", "conv", build)


def pack_temporal_qkv(w_qkv: torch.Tensor, heads: int = 8) -> torch.Tensor:
    """Fused temporal `[3 C, C]` projection (rows q | k | v, heads contiguous inside each) -> the MFMA-fragment order of `fmc_temporal_block_bf16`
    (C = 320, d = 40): per head [q: blocks q[0:16], q[16:32], tail = (q[32:40] | k[32:40])][k: k[0:16], k[16:32]][v: v[0:16], v[16:32], (v[32:40] | 0)],
    every part as [k-step C / 32][block][lane = 16 * (k chunk of 8) + row][8]: the fragment of one 16-row block and k-step is one contiguous KiB,
    a head's 30 (part, k-step) steps one contiguous 80-KiB stream."""
    C3, C = w_qkv.shape
    assert C3 == 3 * C and C == 320 and heads == 8, "the fused temporal block exists for C = 320, 8 heads"
    d = C // heads
    w = w_qkv.detach()
    q, k, v = w[:C].view(heads, d, C), w[C:2 * C].view(heads, d, C), w[2 * C:].view(heads, d, C)
    z = torch.zeros(heads, 8, C, dtype=w.dtype, device=w.device)
    parts = [torch.stack([q[:, 0:16], q[:, 16:32], torch.cat([q[:, 32:40], k[:, 32:40]], 1)], 1),        # [H, 3, 16, C]
             torch.stack([k[:, 0:16], k[:, 16:32]], 1),
             torch.stack([v[:, 0:16], v[:, 16:32], torch.cat([v[:, 32:40], z], 1)], 1)]
    out = []
    for blk in parts:                                   # [H, nb, 16 rows, C] -> [H, ks, nb, kq, row, 8]
        nb = blk.shape[1]
        out.append(blk.reshape(heads, nb, 16, C // 32, 4, 8).permute(0, 3, 1, 4, 2, 5).reshape(heads, -1))
    return torch.cat(out, 1).contiguous().view(-1)


def pack_w_frag80(w: torch.Tensor) -> torch.Tensor:
    """`[640, 640]` projection weight -> the MFMA-fragment order of the C = 640 fused temporal block (`temporal_block640.hip`): wave w owns output columns
    80 w .. 80 w + 79; per wave [k-step K / 32][block of 16 rows][lane = 16 * (k chunk of 8) + row][8]: the fragment of one block and k-step is one contiguous
    KiB, a wave's 100 (k-step, block) fragments one contiguous 100-KiB stream that never passes through LDS."""
    N, Kd = w.shape
    assert N == 640 and Kd == 640, "the C = 640 fused temporal block"
    return w.detach().reshape(8, 5, 16, Kd // 32, 4, 8).permute(0, 3, 1, 4, 2, 5).contiguous().view(-1)


def pack_temporal_qkv80(w_qkv: torch.Tensor, heads: int = 8) -> torch.Tensor:
    """Fused temporal `[3 C, C]` projection at C = 640 (d = 80 = five whole 16-row blocks per head and part, no padding): per head [q | k | v], every part
    as [k-step][block][lane][8] like `pack_w_frag80`."""
    C3, C = w_qkv.shape
    assert C3 == 3 * C and C == 640 and heads == 8, "the C = 640 fused temporal block: 8 heads x 80"
    w = w_qkv.detach()
    parts = [w[i * C:(i + 1) * C].reshape(heads, 5, 16, C // 32, 4, 8).permute(0, 3, 1, 4, 2, 5).reshape(heads, -1) for i in range(3)]
    return torch.cat(parts, 1).contiguous().view(-1)


def temporal_block_supported(h: torch.Tensor, heads: int) -> bool:
    """`[B, F, hw, C]` bf16 tokens the fused block takes: F = 16, 8 heads, C = 320 with hw % 10 == 0 or C = 640 with hw % 5 == 0, inference."""
    return _temporal_block_ok(h, heads, any_rows=False)


TEMPORAL_FUSED_640 = os.environ.get("FMC_TEMPORAL_FUSED_640", "1") != "0"      # A/B switch: the 20x32-level blocks on the un-fused chain


def temporal_block(h: torch.Tensor, ln_gamma: torch.Tensor, ln_bpe: torch.Tensor, ln_eps: float, w_qkv_packed: torch.Tensor,
                   w_out_tm: torch.Tensor, b_out: Optional[torch.Tensor], scale: float, w_merge_tm: Optional[torch.Tensor] = None,
                   pose_term: Optional[torch.Tensor] = None, merge_scale: float = 1.0, stats_eps: Optional[float] = None, partial_tiles: bool = False):
    """One attention block of the temporal transformer in one launch (`fmc_temporal_block_bf16`): LayerNorm (+ pe) -> [Camera-Adapter merge] ->
    q | k | v -> attention over the frames -> out-projection + bias + h.  Returns `out` or `(out, ln_stats)` when `stats_eps` is given.
    C = 320: `w_qkv_packed = pack_temporal_qkv(..)`, `w_out_tm` / `w_merge_tm` = `_w_tilemajor(..)`.  C = 640: `pack_temporal_qkv80`, `pack_w_frag80`, no statistics.
    `partial_tiles=True`: `fmc_temporal_block_partial_bf16` -- any hw >= 1, the last tile of a clip partly filled (`temporal_tile_count`)."""
    _dev(h, ln_gamma, ln_bpe, w_qkv_packed, w_out_tm, b_out, w_merge_tm, pose_term)
    B, F, hw, C = h.shape
    assert h.is_contiguous() and ln_gamma.dtype == torch.float32 and ln_bpe.dtype == torch.float32 and tuple(ln_bpe.shape) == (F, C) and ln_bpe.is_contiguous()
    assert (w_merge_tm is None) == (pose_term is None)
    assert pose_term is None or (pose_term.shape == h.shape and pose_term.is_contiguous() and pose_term.dtype == h.dtype)
    out = torch.empty_like(h)
    stats = torch.empty(B * F * hw, 2, dtype=torch.float32, device=h.device) if stats_eps is not None else None
    _log_call("fused_block", ("temporal", B * F * hw, C, w_merge_tm is not None) + ((("partial", temporal_tile_count(B, hw, C)),) if partial_tiles else ()),
              2.0 * B * F * hw * C * C * (5 if w_merge_tm is not None else 4) + 4.0 * B * F * hw * F * C)
    name, fn = _entry("fmc_temporal_block_bf16", partial_tiles)
    _lib.check(fn(h.data_ptr(), out.data_ptr(), ln_gamma.data_ptr(), ln_bpe.data_ptr(), float(ln_eps), _p(w_merge_tm),
                  _p(pose_term), float(merge_scale), w_qkv_packed.data_ptr(), w_out_tm.data_ptr(), _p(b_out),
                  _p(stats), float(stats_eps or 0.0), B, F, hw, C, 8, float(scale), _stream()), name)
    return out if stats is None else (out, stats)


XATTN_FUSED_640 = os.environ.get("FMC_XATTN_FUSED_640", "1") != "0"      # A/B switch: the 20x32-level text cross-attention as one launch
XATTN_FUSED_320 = os.environ.get("FMC_XATTN_FUSED_320", "1") != "0"      # ... and the 40x64-level one


def pack_xattn_q40(w_q: torch.Tensor, heads: int = 8) -> torch.Tensor:
    """`to_q [320, 320]` of a text cross-attention (8 heads x 40) -> the fragment order phase D of the fused block reads: per head [10 k-steps][3 blocks =
    q[0:16], q[16:32], (q[32:40] | 8 zero rows)][lane = 16 * (k chunk of 8) + row][8] (the q part of `pack_temporal_qkv`, the shared tail block's k half empty)."""
    C, Ci = w_q.shape
    assert C == 320 and Ci == 320 and heads == 8
    q = w_q.detach().view(heads, 40, Ci)
    z = torch.zeros(heads, 8, Ci, dtype=q.dtype, device=q.device)
    blk = torch.stack([q[:, 0:16], q[:, 16:32], torch.cat([q[:, 32:40], z], 1)], 1)            # [H, 3, 16, C]
    return blk.reshape(heads, 3, 16, Ci // 32, 4, 8).permute(0, 3, 1, 4, 2, 5).contiguous().view(-1)


def xattn_block_supported(h: torch.Tensor, kv_tokens: int, heads: int) -> bool:
    """`[images, hw, C]` bf16 tokens the fused text cross-attention block takes: 8 heads, at most 80 text tokens, inference; C = 640 with hw % 80 == 0
    or C = 320 with hw % 160 == 0."""
    return _xattn_block_ok(h, kv_tokens, heads, any_rows=False)


xattn_block640_supported = xattn_block_supported


def xattn_pack_kv(kv: torch.Tensor) -> torch.Tensor:
    """`kv [B, S, 2 C]` (the text's fused k | v projection, C = 320 | 640, S <= 80) -> the K / V^T MFMA fragments the fused text cross-attention block
    reads (`fmc_xattn_pack_kv40` / `fmc_xattn_pack_kv`).  Constant over the denoising steps of a clip: packed once per clip (`Attention.text_kv`)."""
    _dev(kv)
    B, S, C2 = kv.shape
    C = C2 // 2
    assert C in (320, 640) and kv.stride(2) == 1 and kv.stride(1) == C2 and S <= 80
    L = _lib.load()
    if C == 640:
        frag = torch.empty(B * 8 * 12800, dtype=kv.dtype, device=kv.device)
        _lib.check(L.fmc_xattn_pack_kv(kv.data_ptr(), frag.data_ptr(), B, S, kv.stride(0), _stream()), "fmc_xattn_pack_kv")
    else:
        frag = torch.empty(B * 8 * 7680, dtype=kv.dtype, device=kv.device)
        _lib.check(L.fmc_xattn_pack_kv40(kv.data_ptr(), frag.data_ptr(), B, S, kv.stride(0), _stream()), "fmc_xattn_pack_kv40")
    return frag


def xattn_block(h: torch.Tensor, ln_gamma: torch.Tensor, ln_btab: torch.Tensor, ln_eps: float, w_q_packed: torch.Tensor, kv: torch.Tensor,
                w_out_packed: torch.Tensor, b_out: Optional[torch.Tensor], scale: float, images_per_text: int, stats_eps: Optional[float] = None,
                frag: Optional[torch.Tensor] = None, partial_tiles: bool = False):
    """`to_out(softmax(to_q(LayerNorm(h)) k^T scale) v) + b + h` in one launch; `kv [B, S, 2 C]` = the text's fused k | v projection (packed into MFMA
    fragments by one tiny launch); `ln_btab [16, C]` fp32 rows = the LayerNorm beta.  C = 640: `fmc_xattn_block640_bf16`, weights `pack_w_frag80`;
    C = 320: `fmc_xattn_block320_bf16`, `pack_xattn_q40` / `_w_tilemajor`, and `stats_eps` adds the (mean, rstd) of the output rows: `(out, stats)`.
    `partial_tiles=True`: the `_partial` entry points -- any hw >= 1, the last tile of a text's `images_per_text * hw` rows partly filled (`xattn_tile_count`)."""
    _dev(h, ln_gamma, ln_btab, w_q_packed, kv, w_out_packed, b_out)
    N, hw, C = h.shape
    B, S, C2 = kv.shape
    assert C in (320, 640) and C2 == 2 * C and kv.stride(2) == 1 and kv.stride(1) == C2 and N % images_per_text == 0 and N // images_per_text == B
    out = torch.empty_like(h)
    _log_call("fused_block", ("xattn", N * hw, C, S) + ((("partial", xattn_tile_count(N, hw, images_per_text, C)),) if partial_tiles else ()),
              2.0 * N * hw * C * C * 2 + 4.0 * N * hw * S * C)
    if frag is None:
        frag = xattn_pack_kv(kv)
    assert frag.numel() == B * 8 * (12800 if C == 640 else 7680) and frag.dtype == h.dtype
    assert C == 320 or stats_eps is None
    stats = torch.empty(N * hw, 2, dtype=torch.float32, device=h.device) if stats_eps is not None else None
    name, fn = _entry("fmc_xattn_block%d_bf16" % C, partial_tiles)
    _lib.check(fn(h.data_ptr(), out.data_ptr(), ln_gamma.data_ptr(), ln_btab.data_ptr(), float(ln_eps), w_q_packed.data_ptr(), frag.data_ptr(),
                  w_out_packed.data_ptr(), _p(b_out), *((_p(stats), float(stats_eps or 0.0)) if C == 320 else ()), N, hw, S, images_per_text,
                  float(scale), _stream()), name)
    return out if stats is None else (out, stats)


xattn_block640 = xattn_block


# ---- the fused attention blocks at any feature-map size: partly filled last tiles (csrc/temporal_block.hip: PARTIAL) -----------------------------------
# One switch opts the models in (`TemporalTransformerBlock.forward`, `BasicTransformerBlock.forward`); read at call time.  Off by default: the whole-tile
# predicates, wrappers and entry points behave as before, and ragged sizes keep the un-fused chain (profiles/partial_tiles.md has the numbers).
PARTIAL_TILES = os.environ.get("FMC_PARTIAL_TILES", "0") not in ("", "0")


# ---- MXFP8 feed-forward (csrc/gemm_mxfp8.hip): block-scaled e4m3 operands on v_mfma_scale_f32_32x32x64_f8f6f4 ---------------------------------------------
# One switch opts `FeedForward.forward_ln` in (inference, bf16, no pending tag); read at call time.  Off by default: a step launches what it launched before.
# The chain is LayerNorm + quantise -> GEGLU GEMM (MXFP8 out) -> output GEMM (bias + residual, bf16 out); profiles/mxfp8_ff.md has the numbers.
FP8_FF = os.environ.get("FMC_FP8_FF", "0") not in ("", "0")
# the widths `ff_mxfp8_ok` does NOT route: a level is listed where the slowest run of the new chain did not beat the fastest run of the bf16 chain
# (tools/mxfp8_ff_rates.py; profiles/mxfp8_ff.md: all three widths of the full-size U-Net at the bench clip, 0.35 / 0.27 / 0.24 ms against 0.24 / 0.22 / 0.22 ms --
#  the first version of the kernel reaches 0.6 - 1.0 PFLOP/s and its epilogues are not hidden; other widths, which nobody has measured, are routed)
MXFP8_FF_SLOWER = (320, 640, 1280)


def mxfp8_supported(M: int, N: int, K: int, geglu: bool) -> bool:
    """The domain of `linear_mxfp8` (`fmc_linear_mxfp8_supported`): N output columns (GEGLU: inner), K % 64 == 0, N % 64 == 0, operands below 2 GiB."""
    return M >= 1 and N >= 64 and K >= 64 and K % 64 == 0 and N % 64 == 0 and M * K < (1 << 31) and (2 if geglu else 1) * N * K < (1 << 31) \
        and M * N * (1 if geglu else 2) < (1 << 31)


def mxfp8_pack_weight(w: torch.Tensor, geglu: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """w `[N, K]` bf16 -> (e4m3 bytes `[N, K]` uint8, E8M0 scales `[N, K / 32]` uint8) in the row order `linear_mxfp8` wants; `geglu`: value and gate
    rows interleaved in 32-row blocks.  Once per weight version (`derived`)."""
    _dev(w)
    assert w.ndim == 2 and w.dtype == torch.bfloat16
    w = w.detach().contiguous()
    N, Kd = w.shape
    wq = torch.empty(N, Kd, dtype=torch.uint8, device=w.device)
    ws = torch.empty(N, Kd // 32, dtype=torch.uint8, device=w.device)
    _lib.check(_lib.load().fmc_mxfp8_pack_weight(w.data_ptr(), wq.data_ptr(), ws.data_ptr(), N, Kd, N // 2 if geglu else 0, _stream()), "fmc_mxfp8_pack_weight")
    return wq, ws


def layernorm_mxfp8(h: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float = 1e-5) -> Tuple[torch.Tensor, torch.Tensor]:
    """MXFP8 of LayerNorm(h) over the last dim in one pass: (bytes `[M, C]`, scales `[M, C / 32]`), M = the rows of `h`.  `gamma is None`: the rows of
    `h` quantised as they are.  `h` bf16 with a dense last dim and one row stride."""
    _dev(h, gamma, beta)
    assert h.dtype == torch.bfloat16 and h.stride(-1) == 1
    C = h.shape[-1]
    if h.ndim != 2:
        assert h.is_contiguous()
        h = h.view(-1, C)
    M = h.shape[0]
    xq = torch.empty(M, C, dtype=torch.uint8, device=h.device)
    xs = torch.empty(M, C // 32, dtype=torch.uint8, device=h.device)
    _lib.check(_lib.load().fmc_layernorm_mxfp8_fwd(h.data_ptr(), _p(gamma), _p(beta), xq.data_ptr(), xs.data_ptr(), M, C, h.stride(0) if M > 1 else C,
                                                   float(eps), _stream()), "fmc_layernorm_mxfp8_fwd")
    _log_call("mxfp8", ("ln", M, C), 0.0)
    return xq, xs


def linear_mxfp8(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, bias: Optional[torch.Tensor] = None,
                 residual: Optional[torch.Tensor] = None, geglu: bool = False):
    """`dq(xq, xs) @ dq(wq, ws)^T + bias (+ residual)` -> bf16 `[M, N]`, or with `geglu` (weights packed with `geglu=True`, bias `[2 inner]`) the GEGLU
    product as MXFP8: (bytes `[M, inner]`, scales `[M, inner / 32]`), ready to be the next call's `xq, xs`."""
    _dev(xq, xs, wq, ws, bias, residual)
    M, Kd = xq.shape
    N = wq.shape[0] // 2 if geglu else wq.shape[0]
    assert xq.is_contiguous() and xs.is_contiguous() and wq.is_contiguous() and ws.is_contiguous() and wq.shape[1] == Kd
    assert bias is None or (bias.dtype == torch.bfloat16 and bias.is_contiguous() and bias.numel() == wq.shape[0])
    lib = _lib.load()
    if geglu:
        assert residual is None
        oq = torch.empty(M, N, dtype=torch.uint8, device=xq.device)
        osc = torch.empty(M, N // 32, dtype=torch.uint8, device=xq.device)
        _lib.check(lib.fmc_linear_mxfp8(xq.data_ptr(), xs.data_ptr(), wq.data_ptr(), ws.data_ptr(), _p(bias), None, oq.data_ptr(), osc.data_ptr(), M, N, Kd,
                                        0, 0, 1, _stream()), "fmc_linear_mxfp8")
        _log_call("mxfp8", ("geglu", M, N, Kd), 4.0 * M * N * Kd)
        return oq, osc
    if residual is not None:
        assert residual.dtype == torch.bfloat16 and residual.is_contiguous() and residual.numel() == M * N
    out = torch.empty(M, N, dtype=torch.bfloat16, device=xq.device)
    _lib.check(lib.fmc_linear_mxfp8(xq.data_ptr(), xs.data_ptr(), wq.data_ptr(), ws.data_ptr(), _p(bias), _p(residual), out.data_ptr(), None, M, N, Kd,
                                    N, N, 0, _stream()), "fmc_linear_mxfp8")
    _log_call("mxfp8", ("linear", M, N, Kd), 2.0 * M * N * Kd)
    return out


def ff_mxfp8_ok(h: torch.Tensor, w_proj: torch.Tensor, w_out: torch.Tensor, residual: Optional[torch.Tensor]) -> bool:
    """What the MXFP8 feed-forward chain takes: bf16 tokens `h [..., C]` (contiguous) on the GPU, no gradient, GEGLU weight `[2 inner, C]`, output weight
    `[C_out, inner]`, both bf16 and inside `mxfp8_supported`, a width outside `MXFP8_FF_SLOWER`, and a residual (or None) that is a plain bf16 tensor of the output's size."""
    C = h.shape[-1]
    M = h.numel() // max(C, 1)
    if not (_on_gpu(h) and h.dtype == torch.bfloat16 and h.is_contiguous() and not torch.is_grad_enabled() and w_proj.dtype == torch.bfloat16
            and w_out.dtype == torch.bfloat16 and w_proj.ndim == 2 and w_out.ndim == 2 and w_proj.shape[1] == C and w_proj.shape[0] % 2 == 0
            and w_out.shape[1] == w_proj.shape[0] // 2 and C not in MXFP8_FF_SLOWER and C <= 2048):
        return False
    inner, n_out = w_out.shape[1], w_out.shape[0]
    if residual is not None and not (residual.dtype == torch.bfloat16 and residual.is_contiguous() and residual.numel() == M * n_out
                                     and getattr(residual, "_fmc_pending_add", None) is None and getattr(residual, "_fmc_pending_ln", None) is None):
        return False
    return mxfp8_supported(M, inner, C, True) and mxfp8_supported(M, n_out, inner, False)


# ---- tile forms of the fused blocks and the feed-forward chain: what a tile holds, and whether the last one may be partly filled --------------------------
# pixels (x 16 frames) of a clip; rows of a text's segment; rows of the GEMMs that read the feed-forward's intermediate; rows its LayerNorm + GEGLU kernels step by
_TILE_UNITS = {"temporal": {320: 10, 640: 5}, "xattn": {320: 160, 640: 80}, "ff": 160, "ff_ln": 80}


def _tile_units(C: int, kind: str) -> int:
    """What a tile of form `kind` holds at width C."""
    units = _TILE_UNITS[kind]
    if isinstance(units, int):
        return units
    assert C in (320, 640)
    return units[C]


class TileForm(NamedTuple):
    """`units` pixels or rows per tile; `any_rows`: any count >= 1, the last tile partly filled (the `_partial` entry points) -- else the count divides."""
    units: int
    any_rows: bool

    def takes(self, n: int) -> bool:
        return n >= 1 if self.any_rows else n % self.units == 0

    def tiles(self, n: int) -> int:                         # (the ceiling: n / units where the count divides)
        return -(-n // self.units)


def _tile_form(kind: str, C: int, any_rows: bool) -> TileForm:
    return TileForm(_tile_units(C, kind), any_rows)


def _g160_persistent(M: int, N: int, device, at_least: bool, any_rows: bool = False) -> bool:
    """Tile 16's persistent form takes (M, N) on this device (csrc/gemm_conv.hip: `g160_persistent_shape`): `FMC_G160_PERSIST` not 0 (read per call), N a
    multiple of 320, M of 160 (`any_rows`: any M, the last tile partly filled), and strictly more 160 x 320 tiles than CUs -- `at_least`: as many
    suffice.  Which of the two a form asks is inherited, not derived: each call site says so."""
    form = TileForm(_TILE_UNITS["ff"], any_rows)
    if os.environ.get("FMC_G160_PERSIST", "1") == "0" or N % 320 or not form.takes(M):
        return False
    tiles = form.tiles(M) * (N // 320)
    return tiles >= _cus(device) if at_least else tiles > _cus(device)


def _below_2gib(numel: int) -> bool:
    """`numel` bf16 elements stay below 2 GiB: the kernels' 32-bit operand offsets."""
    return numel * 2 < (1 << 31)


def _entry(whole: str, partial: bool):
    """(name, function) in C of a launch entry point: `whole` or its partial-tile twin (`..._partial_bf16`, `fmc_linear_bf16_<form>_partial`)."""
    name = whole if not partial else (whole[:-5] + "_partial_bf16" if whole.endswith("_bf16") else whole + "_partial")
    return name, getattr(_lib.load(), name)


def temporal_tile_count(n_clips: int, hw: int, C: int) -> int:
    """Tiles (= the grid before the persistent cap at C = 320) of `fmc_temporal_block_partial_bf16`: ceil(hw / 10 | 5) per clip."""
    return n_clips * _tile_form("temporal", C, True).tiles(hw)


def temporal_tile(t: int, hw: int, C: int):
    """Tile t of the temporal form -> (clip, first pixel, valid pixels): the kernel's `tile_row0` / `tile_valid`."""
    px = _tile_units(C, "temporal")
    per_clip = -(-hw // px)
    clip, p0 = t // per_clip, (t % per_clip) * px
    return clip, p0, min(px, hw - p0)


def xattn_tile_count(n_images: int, hw: int, images_per_text: int, C: int) -> int:
    """Tiles of `fmc_xattn_block320 | 640_partial_bf16`: a segment = the `images_per_text * hw` rows of one text, ceil(rows / 160 | 80) tiles each."""
    return (n_images // images_per_text) * _tile_form("xattn", C, True).tiles(images_per_text * hw)


def xattn_tile(t: int, seg_rows: int, C: int):
    """Tile t of the text cross-attention form -> (segment = text, first global row, valid rows); a tile never holds rows of two texts."""
    rows = _tile_units(C, "xattn")
    per_seg = -(-seg_rows // rows)
    seg, r0 = t // per_seg, (t % per_seg) * rows
    return seg, seg * seg_rows + r0, min(rows, seg_rows - r0)


def _on_gpu(t: torch.Tensor) -> bool:
    """(its own function so that the host tests can exercise every other condition of the partial-tile predicates below on CPU tensors)"""
    return t.is_cuda


def _temporal_block_ok(h: torch.Tensor, heads: int, any_rows: bool) -> bool:
    # (inherited, not derived, here and in `_xattn_block_ok`: the whole-tile predicate asks the tensor itself, the partial-tile one the hook above)
    return ((_on_gpu(h) if any_rows else h.is_cuda) and h.dtype == torch.bfloat16 and h.ndim == 4 and h.is_contiguous() and h.shape[1] == 16 and heads == 8
            and (h.shape[3] == 320 or (h.shape[3] == 640 and TEMPORAL_FUSED_640)) and _tile_form("temporal", h.shape[3], any_rows).takes(h.shape[2])
            and h.numel() * 2 < (1 << 31) and not torch.is_grad_enabled())


def _xattn_block_ok(h: torch.Tensor, kv_tokens: int, heads: int, any_rows: bool) -> bool:
    if not ((_on_gpu(h) if any_rows else h.is_cuda) and h.dtype == torch.bfloat16 and h.ndim == 3 and h.is_contiguous() and heads == 8 and 0 < kv_tokens <= 80
            and h.numel() * 2 < (1 << 31) and not torch.is_grad_enabled()):
        return False
    C = h.shape[2]
    return bool(((XATTN_FUSED_640 and C == 640) or (XATTN_FUSED_320 and C == 320)) and _tile_form("xattn", C, any_rows).takes(h.shape[1]))


def temporal_block_partial_supported(h: torch.Tensor, heads: int) -> bool:
    """`temporal_block_supported` without the divisibility of hw: what `temporal_block(..., partial_tiles=True)` takes."""
    return _temporal_block_ok(h, heads, any_rows=True)


def xattn_block_partial_supported(h: torch.Tensor, kv_tokens: int, heads: int) -> bool:
    """`xattn_block_supported` without the divisibility of hw: what `xattn_block(..., partial_tiles=True)` takes."""
    return _xattn_block_ok(h, kv_tokens, heads, any_rows=True)


GEGLU_DIRECT_640 = os.environ.get("FMC_GEGLU_DIRECT_640", "1") != "0"      # A/B switch: LayerNorm + GEGLU projection of the 20x32 level with the A operand resident
GEGLU_DIRECT_320 = os.environ.get("FMC_GEGLU_DIRECT_320", "1") != "0"      # ... and of the 40x64 level


def pack_geglu_frag80(w: torch.Tensor) -> torch.Tensor:
    """GEGLU projection `[2 Cff, C]` (value rows, then gate rows; C = 640 | 320) -> `fmc_geglu640_ln_bf16` / `fmc_geglu320_ln_bf16`'s fragment order:
    [Cff / (40 NW) chunks][NW = C / 80 waves][C / 32 k-steps][5 blocks][lane][8]; wave w of chunk c owns gated columns 40 NW c + 40 w .. + 39, its 80 weight
    rows ordered [v 0-15 | v 16-31 | v 32-39, g 32-39 | g 0-15 | g 16-31] so that value and gate of a column share a lane in four of the five blocks."""
    two_cff, Kd = w.shape
    cff, nw = two_cff // 2, Kd // 80
    assert Kd in (320, 640) and cff % (40 * nw) == 0
    nc = cff // (40 * nw)
    base = (torch.arange(nc, device=w.device)[:, None] * (40 * nw) + torch.arange(nw, device=w.device)[None, :] * 40)[..., None]      # [nc, nw, 1]
    r = torch.arange(16, device=w.device)
    idx = torch.cat([base + r, base + 16 + r, base + 32 + r[:8], cff + base + 32 + r[:8], cff + base + r, cff + base + 16 + r], -1)    # [nc, nw, 80]
    wp = w.detach()[idx.reshape(-1)].reshape(nc, nw, 5, 16, Kd // 32, 4, 8)
    return wp.permute(0, 1, 4, 2, 5, 3, 6).contiguous().view(-1)


GEGLU_PIPE = os.environ.get("FMC_GEGLU_PIPE", "1") != "0"        # A/B switch: the software-pipelined LayerNorm + GEGLU kernel (csrc/geglu_pipe.hip) where it applies
GEGLU_PIPE_640 = os.environ.get("FMC_GEGLU_PIPE_640", "0") == "1"  # ... also at C = 640 (80-row form only: 130 vs 136 us isolated)


def pack_geglu_frag(w: torch.Tensor, group: int = 32) -> torch.Tensor:
    """GEGLU projection `[2 Cff, C]` (value rows, then gate rows) -> `fmc_geglu_pipe_ln_bf16`'s fragment order: per group of `group` (32 | 16) gated columns
    the 2 x group weight rows [value blocks of 16 | gate blocks of 16] (value and gate of a column share a lane), as
    [Cff / group][C / 32 k-steps][group / 8 blocks][lane = 16 kq + row][8]."""
    two_cff, Kd = w.shape
    cff, nb = two_cff // 2, group // 8
    assert Kd % 32 == 0 and cff % group == 0 and group in (16, 32)
    base = (torch.arange(cff // group, device=w.device) * group)[:, None]                                                            # [ng, 1]
    r = torch.arange(group, device=w.device)
    idx = torch.cat([base + r, cff + base + r], -1)                                                                                  # [ng, 2 group]
    wp = w.detach()[idx.reshape(-1)].reshape(cff // group, nb, 16, Kd // 32, 4, 8)                                                   # [ng, block, row, ks, kq, 8]
    return wp.permute(0, 3, 1, 4, 2, 5).contiguous().view(-1)


def geglu_pipe_variant(M: int, C: int) -> int:
    """1 = the 160-row form (C = 320, M % 160 == 0: each weight fragment serves twice the rows), else 0 = the 80-row form.  FMC_GEGLU_PIPE_VARIANT forces."""
    env = os.environ.get("FMC_GEGLU_PIPE_VARIANT")
    if env is not None:
        return int(env)
    return 1 if (C == 320 and M % 160 == 0) else 0


def geglu_ln_pipe_ok(h: torch.Tensor, weight: torch.Tensor) -> bool:
    C = h.shape[-1]
    M = h.numel() // C
    return bool(GEGLU_PIPE and h.is_cuda and h.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and h.is_contiguous() and weight.shape[1] == C
                and not torch.is_grad_enabled()
                and _lib.load().fmc_geglu_pipe_supported(M, weight.shape[0] // 2, C, geglu_pipe_variant(M, C)))


def geglu_ln_pipe(h: torch.Tensor, ln_gamma: torch.Tensor, ln_beta: torch.Tensor, ln_eps: float, w_packed: torch.Tensor, bias: Optional[torch.Tensor],
                  cff: int, blocked: bool = False, variant: int = 0, partial_tiles: bool = False) -> torch.Tensor:
    """`GEGLU(LayerNorm(h))` on `fmc_geglu_pipe_ln_bf16` (the gate of chunk c - 1 in the shadow of chunk c's MFMAs): `[..., C] -> [..., cff]`, `w_packed` =
    `pack_geglu_frag(weight, 32 if variant == 0 else 16)`.  `blocked`: tile-major `[M / 160][cff / 32][160][32]` for `linear_from_blocked`.
    `partial_tiles`: any row count on `fmc_geglu_pipe_ln_partial_bf16`; with `blocked` the result owns padded storage (see `linear_from_blocked`)."""
    _dev(h, ln_gamma, ln_beta, w_packed, bias)
    C = h.shape[-1]
    M = h.numel() // C
    if partial_tiles and blocked:          # ceil(M / 160) whole tiles; the tensor handed on is the [..., cff]-shaped head of that storage
        out = torch.empty(ff_blocked_numel(M, cff), dtype=h.dtype, device=h.device)[:M * cff].view(*h.shape[:-1], cff)
    else:
        out = torch.empty(*h.shape[:-1], cff, dtype=h.dtype, device=h.device)
    _log_call("geglu_direct", (M, 2 * cff, C) + (("partial",) if partial_tiles else ()), 2.0 * M * 2 * cff * C)
    name, fn = _entry("fmc_geglu_pipe_ln_bf16", partial_tiles)
    _lib.check(fn(h.data_ptr(), out.data_ptr(), ln_gamma.data_ptr(), ln_beta.data_ptr(), float(ln_eps), w_packed.data_ptr(), _p(bias), M, cff, C, int(blocked),
                  int(variant), _stream()), name)
    return out


# ---- the feed-forward chain at any row count: partly filled last tile (csrc/geglu_pipe.hip, csrc/gemm_conv.hip: PARTIAL) --------------------------------
# M is one flat row count: ceil(M / 160) tiles, only the last one ragged.  Taken by `FeedForward.forward_ln` with `PARTIAL_TILES` on.
def ff_tile_count(M: int, rows: int = _TILE_UNITS["ff"]) -> int:
    return TileForm(rows, True).tiles(M)


def ff_blocked_numel(M: int, K: int) -> int:
    """Elements of the tile-major intermediate: ceil(M / 160) WHOLE tiles of `[K / 32][160][32]`."""
    form = _tile_form("ff", 0, True)
    return form.tiles(M) * form.units * K


def _ff_on_gpu(t: torch.Tensor) -> bool:
    """(as `_on_gpu`, for `geglu_ln_partial_ok`: the host tests exercise every other condition of it on CPU tensors)"""
    return t.is_cuda


def geglu_pipe_partial_supported(M: int, cff: int, C: int, variant: int) -> bool:
    """What `geglu_ln_pipe(..., partial_tiles=True)` takes of a shape: the rule is written once, in csrc/geglu_pipe.hip (`pipe_shape_ok`)."""
    return bool(_lib.load().fmc_geglu_pipe_partial_supported(M, cff, C, variant))


def geglu_pipe_partial_variant(C: int) -> int:
    """The 160-row form at C = 320 (every weight fragment serves twice the rows), the 80-row form at C = 640."""
    return 1 if C == 320 else 0


def _geglu_ln_ok(h: torch.Tensor, weight: torch.Tensor, any_rows: bool) -> bool:
    C = h.shape[-1]
    M = h.numel() // max(C, 1)
    cff = weight.shape[0] // 2
    # (inherited, not derived: the whole-tile predicate asks the tensor itself, the partial-tile one this family's own hook)
    if not ((_ff_on_gpu(h) if any_rows else h.is_cuda) and h.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and h.is_contiguous() and weight.shape[1] == C
            and _tile_form("ff_ln", C, any_rows).takes(M) and h.numel() * 2 < (1 << 31) and not torch.is_grad_enabled()):
        return False
    if not ((GEGLU_DIRECT_640 and C == 640) or (GEGLU_DIRECT_320 and C == 320)):
        return False
    # inherited, not derived: whole tiles ask for the direct kernels' chunks of cff and leave `GEGLU_PIPE` to `geglu_ln_pipe_ok`; a partly filled tile exists
    # on the pipe kernel alone, so its switch and its shape rule (cff % 128, the padded sizes) decide
    if any_rows:
        return bool(GEGLU_PIPE and geglu_pipe_partial_supported(M, cff, C, geglu_pipe_partial_variant(C)))
    return cff % (320 if C == 640 else 160) == 0


def geglu_ln_partial_ok(h: torch.Tensor, weight: torch.Tensor) -> bool:
    """`geglu_ln_direct_ok` without the divisibility of M: what `geglu_ln_pipe(..., partial_tiles=True)` takes (both levels on the pipe kernel)."""
    return _geglu_ln_ok(h, weight, any_rows=True)


def _geglu_blocked_ok(h: torch.Tensor, w2: torch.Tensor, residual, any_rows: bool) -> bool:
    C = h.shape[-1]
    M = h.numel() // C
    N2, Cff = w2.shape
    # inherited, not derived: Cff % 32 on whole tiles, Cff % 64 and the weight's own 2 GiB bound on partly filled ones; strictly more tiles than CUs.  (The
    # intermediate's bound is the padded count in both: on whole tiles that IS M * Cff)
    return (GEGLU_DIRECT_BLOCKED and FF_BLOCKED and C == 320 and Cff % (64 if any_rows else 32) == 0 and _g160_persistent(M, N2, h.device, False, any_rows)
            and _below_2gib(ff_blocked_numel(M, Cff)) and (not any_rows or _below_2gib(N2 * Cff)) and w2.dtype == torch.bfloat16 and w2.is_contiguous()
            and (residual is None or (residual.is_contiguous() and residual.dtype == h.dtype)))


def geglu_direct_blocked_partial_ok(h: torch.Tensor, w2: torch.Tensor, residual) -> bool:
    """`geglu_direct_blocked_ok` without `M % 160 == 0`: ceil(M / 160) tiles, more of them than CUs, the padded intermediate below 2 GiB."""
    return _geglu_blocked_ok(h, w2, residual, any_rows=True)


def _ff_tail_ok(h: torch.Tensor, w2: torch.Tensor, wp: torch.Tensor, tail_residual: Optional[torch.Tensor], any_rows: bool) -> bool:
    C = h.shape[-1]
    M = h.numel() // C
    # inherited, not derived: as many tiles as CUs suffice where the blocked pair asks more; the folded weight's own 2 GiB bound on partly filled tiles only
    return (FF_TAIL and not torch.is_grad_enabled() and h.dtype == torch.bfloat16 and h.is_contiguous() and wp.dtype == torch.bfloat16 and w2.dtype == torch.bfloat16
            and wp.ndim == 2 and wp.shape[1] == w2.shape[0] == C and C % 64 == 0 and w2.shape[1] % 64 == 0
            and _g160_persistent(M, wp.shape[0], h.device, True, any_rows) and _below_2gib(ff_blocked_numel(M, max(w2.shape[1], C)))
            and (not any_rows or _below_2gib(wp.shape[0] * (w2.shape[1] + C)))
            and tail_residual is not None and tail_residual.dtype == h.dtype and tail_residual.is_contiguous() and tail_residual.numel() == M * wp.shape[0])


def ff_tail_partial_ok(h: torch.Tensor, w2: torch.Tensor, wp: torch.Tensor, tail_residual: Optional[torch.Tensor]) -> bool:
    """`ff_tail_ok` without `M % 160 == 0`: at least as many tiles (ceil) as CUs, the padded intermediate below 2 GiB."""
    return _ff_tail_ok(h, w2, wp, tail_residual, any_rows=True)


def _blocked_storage_ok(xb: torch.Tensor, M: int, K: int) -> bool:
    return (xb.untyped_storage().nbytes() - xb.storage_offset() * xb.element_size()) >= ff_blocked_numel(M, K) * xb.element_size()


def geglu_ln_direct_ok(h: torch.Tensor, weight: torch.Tensor) -> bool:
    return _geglu_ln_ok(h, weight, any_rows=False)


GEGLU_DIRECT_BLOCKED = os.environ.get("FMC_GEGLU_DIRECT_BLOCKED", "1") != "0"   # A/B switch: the level-0 feed-forward's intermediate tile-major (below)


def geglu_direct_blocked_ok(h: torch.Tensor, w2: torch.Tensor, residual) -> bool:
    """Level 0 (C = 320): `geglu_ln_direct(..., blocked=True)` + `linear_from_blocked` -- the second GEMM (K = 1280, N = 320) streams a 210-MB operand in
    128-byte row pieces 2560 bytes apart when it is row-major; tile-major it requests contiguous 10-KiB blocks (113 -> 99 us isolated,
    tools/scratch/r05/bench_ffblk.py).  No gain measured at C = 640 (74.6 / 75.2 us), so only this level takes it."""
    return _geglu_blocked_ok(h, w2, residual, any_rows=False)


def geglu_ln_direct(h: torch.Tensor, ln_gamma: torch.Tensor, ln_beta: torch.Tensor, ln_eps: float, w_packed: torch.Tensor, bias: Optional[torch.Tensor],
                    cff: int, blocked: bool = False) -> torch.Tensor:
    """`GEGLU(LayerNorm(h))` in one launch (`fmc_geglu640_ln_bf16` / `fmc_geglu320_ln_bf16`): `[..., C] -> [..., cff]`.  `blocked`: the result is laid
    out tile-major `[M / 160][cff / 32][160][32]` for `linear_from_blocked` (same shape, private to the feed-forward)."""
    _dev(h, ln_gamma, ln_beta, w_packed, bias)
    C = h.shape[-1]
    M = h.numel() // C
    out = torch.empty(*h.shape[:-1], cff, dtype=h.dtype, device=h.device)
    _log_call("geglu_direct", (M, 2 * cff, C), 2.0 * M * 2 * cff * C)
    fn = _lib.load().fmc_geglu640_ln_bf16 if C == 640 else _lib.load().fmc_geglu320_ln_bf16
    _lib.check(fn(h.data_ptr(), out.data_ptr(), ln_gamma.data_ptr(), ln_beta.data_ptr(), float(ln_eps), w_packed.data_ptr(), _p(bias), M, cff, int(blocked),
                  _stream()), "fmc_geglu_ln_bf16")
    return out


def linear_supported(x: torch.Tensor, weight: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and x.stride(-1) == 1
            and weight.shape[1] % 64 == 0 and weight.shape[0] % 8 == 0 and weight.is_contiguous())


def _rows2d(t: torch.Tensor):
    """(M, row stride) of a tensor whose leading dims collapse to uniformly strided rows with a dense last dim."""
    C = t.shape[-1]
    if t.is_contiguous():
        return t.numel() // C, C
    assert t.ndim == 2 and t.stride(1) == 1, "strided operands must be 2-D [M, C] views"
    return t.shape[0], t.stride(0)


# ---- what the token-GEMM wrappers below share: the residuals' stride with its assertions, the packed weight, the log line and the call --------------------------
def _ldres(out: torch.Tensor, residual, residual2=None) -> int:
    """Row stride of the residual(s) of `out` (0 without one): they have the output's shape, and the second one the first one's stride."""
    ldres = 0
    if residual is not None:
        assert residual.shape == out.shape
        ldres = _rows2d(residual)[1]
    if residual2 is not None:
        assert residual is not None and residual2.shape == out.shape and _rows2d(residual2)[1] == ldres
    return ldres


def _packed(weight: torch.Tensor):
    """(the weight as tile 16 is to read it, the entry points' `w_tilemajor` flag): packed tile-major unless `W_TILEMAJOR` is off."""
    return (_w_tilemajor(weight), 1) if W_TILEMAJOR else (weight, 0)


def _own_linear(entry: str, form: str, M: int, N: int, Kd: int, n_res: int, *args) -> None:
    """The `own_linear` log line of a launch and the call of `entry` with `args` + the stream."""
    _log_call("own_linear", (M, N, Kd, form, n_res), 2.0 * M * N * Kd)
    _lib.check(getattr(_lib.load(), entry)(*args, _stream()), entry)


VENDOR_DIRECT = os.environ.get("FMC_VENDOR_DIRECT", "1") != "0"      # A/B switch: the vendor arm through fmc_vendor_linear_bf16 (bias + residual in the GEMM)
VENDOR_ALGO = int(os.environ.get("FMC_VENDOR_ALGO", "-1"))           # >= 0: this heuristic candidate for every problem (clamped to the list); default: per problem, from the arm table
_vendor_seen = {}                                                     # problem -> candidate count (a first call plans: never under stream capture)
vendor_direct_calls = {"direct": 0, "with_residual": 0}


_vendor_ws = {}                                                       # (device, stream handle) -> workspace tensor: two streams never share split-K scratch
_vendor_inited = set()


def _vendor_init(device_index: int) -> None:
    """hipBLASLt handle of the device, created once through the ABI's explicit `fmc_vendor_init` and dropped at interpreter exit."""
    if device_index not in _vendor_inited:
        _lib.check(_lib.load().fmc_vendor_init(), "fmc_vendor_init")
        if not _vendor_inited:
            atexit.register(_vendor_shutdown)
        _vendor_inited.add(device_index)


def _vendor_shutdown() -> None:
    _vendor_ws.clear()
    try:
        if _vendor_inited and torch.cuda.is_available():
            cur = torch.cuda.current_device()
            for d in sorted(_vendor_inited):
                torch.cuda.set_device(d)
                _lib.load().fmc_vendor_destroy()
            torch.cuda.set_device(cur)
    except Exception:                                                 # interpreter teardown: the driver frees what is left
        pass
    _vendor_inited.clear()


def _vendor_workspace(device: torch.device):
    """The caller-owned scratch `fmc_vendor_linear_bf16` wants: one torch allocation per (device, stream).  Under stream capture the buffer comes out
    of the graph's private pool and lives as long as the graph's memory does; the entry is keyed by the capture stream, which eager work never uses."""
    key = (device.index, _stream())
    ws = _vendor_ws.get(key)
    if ws is None:
        ws = _vendor_ws[key] = torch.empty(int(_lib.load().fmc_vendor_workspace_bytes()), dtype=torch.uint8, device=device)
    return ws


def vendor_version() -> int:
    """hipBLASLt's version number (the `("valgo", ...)` entries of an arm table index ITS heuristic's candidate list)."""
    _vendor_init(torch.cuda.current_device())
    return int(_lib.load().fmc_vendor_version())


def vendor_linear_ok(x: torch.Tensor, weight: torch.Tensor, bias, residual) -> bool:
    if not (VENDOR_DIRECT and x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and weight.is_contiguous() and x.stride(-1) == 1
            and (x.is_contiguous() or x.ndim == 2) and (bias is None or (bias.dtype == torch.bfloat16 and bias.is_contiguous()))
            and (residual is None or (residual.dtype == torch.bfloat16 and residual.stride(-1) == 1 and (residual.is_contiguous() or residual.ndim == 2)))
            and not torch.is_grad_enabled()):
        return False
    N, Kd = weight.shape
    M, ldx = _rows2d(x)
    ldres = 0
    if residual is not None:
        # the library reads C as a full [M, N] matrix: a broadcastable residual ([1, S, N], [N]) must take the torch path, which broadcasts
        if tuple(residual.shape) != (*x.shape[:-1], N):
            return False
        ldres = _rows2d(residual)[1]
        if ldres % 8 or residual.data_ptr() % 16:
            return False
    if ldx % 8 or x.data_ptr() % 16 or weight.data_ptr() % 16 or (bias is not None and bias.data_ptr() % 2):
        return False                                                  # un-aligned views: F.linear accepts them, the direct call would raise FMC_E_ALIGN
    key = (x.device.index, M, N, Kd, ldx, ldres, bias is not None, residual is not None)
    return key in _vendor_seen or not torch.cuda.is_current_stream_capturing()


def vendor_linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`x @ weight^T + bias + residual` as one hipBLASLt launch (`fmc_vendor_linear_bf16`): the library arm of `linear` without the separate torch add."""
    _dev(x, weight, bias, residual)
    N, Kd = weight.shape
    M, ldx = _rows2d(x)
    _vendor_init(x.device.index)
    out = torch.empty(*x.shape[:-1], N, dtype=x.dtype, device=x.device)
    ws = _vendor_workspace(x.device)
    ldres = 0 if residual is None else _rows2d(residual)[1]
    key = (x.device.index, M, N, Kd, ldx, ldres, bias is not None, residual is not None)
    n = _vendor_seen.get(key)
    if n is None:
        n = _lib.load().fmc_vendor_linear_candidates(M, N, Kd, ldx, ldres, N, int(bias is not None), int(residual is not None))
        if n <= 0:
            _lib.check(n if n < 0 else -1, "fmc_vendor_linear_candidates")
        _vendor_seen[key] = n
    # which of the heuristic's candidates: its first choice is not the fastest on every shape (5120 x 3840 x 1280: 62 us, the second candidate 52 us --
    # tools/scratch/r05/bench_vendor_algos.py: 0.25 ms per step over the ten main shapes).  Chosen once per problem by timing, kept in the arm table
    # (`("valgo", ...)` keys: the tracked default table holds them like the GEMM / conv arms, so a fresh box runs the measured candidates without tuning)
    akey = ("valgo", M, N, Kd, ldx, ldres, bias is not None, residual is not None)
    if not _cache_state["loaded"]:
        load_autotune_table()
    algo = VENDOR_ALGO if VENDOR_ALGO >= 0 else _choice.get(akey)
    if algo is None:
        if AUTOTUNE and n > 1 and not torch.cuda.is_current_stream_capturing():
            times = {}
            for a in range(n):
                call = lambda a=a: _lib.load().fmc_vendor_linear_bf16(x.data_ptr(), weight.data_ptr(), _p(bias), _p(residual), out.data_ptr(), M, N, Kd, ldx,
                                                                      ldres, N, a, ws.data_ptr(), ws.numel(), _stream())
                for _ in range(5):
                    call()
                best = float("inf")
                for _ in range(3):                      # min of 3 event-bracketed bursts
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(10):
                        call()
                    e1.record()
                    e1.synchronize()
                    best = min(best, e0.elapsed_time(e1) / 10)
                times[a] = round(best, 4)
            algo = min(times, key=times.get)
            _choice[akey] = algo
            _tune_log[akey] = times
            _cache_state["dirty"] = True
        else:
            algo = 0
    _lib.check(_lib.load().fmc_vendor_linear_bf16(x.data_ptr(), weight.data_ptr(), _p(bias), _p(residual), out.data_ptr(), M, N, Kd, ldx, ldres, N,
                                                  min(int(algo), n - 1), ws.data_ptr(), ws.numel(), _stream()), "fmc_vendor_linear_bf16")
    vendor_direct_calls["direct"] += 1
    vendor_direct_calls["with_residual"] += residual is not None
    _log_call("vendor", (M, N, Kd, bias is not None, residual is not None), 2.0 * M * N * Kd)
    return out


def linear4_bf16(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                 alpha: float = 1.0, residual2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`alpha * (x @ weight^T + bias) + residual [+ residual2]` on `fmc_linear4_bf16` (160 x 160 tiles, 4 waves, software-pipelined: the small-M
    projections of the 10x16 / 5x8 levels).  x `[..., K]` (dense last dim, uniformly strided rows), weight `[N, K]` contiguous."""
    _dev(x, weight, bias, residual, residual2)
    N, Kd = weight.shape
    assert weight.is_contiguous() and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
    M, ldx = _rows2d(x)
    out = torch.empty(*x.shape[:-1], N, dtype=x.dtype, device=x.device)
    ldres = _ldres(out, residual, residual2)
    _own_linear("fmc_linear4_bf16", "g4", M, N, Kd, (residual is not None) + (residual2 is not None),
                x.data_ptr(), weight.data_ptr(), _p(bias), _p(residual), _p(residual2), out.data_ptr(), M, N, Kd, ldx, ldres, N, float(alpha))
    return out


def linear_bf16(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None, alpha: float = 1.0, geglu: bool = False,
                tile: int = 0, split_k: int = 1, x2: Optional[torch.Tensor] = None,
                residual2: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`alpha * (x @ weight^T + bias) + residual [+ residual2]` (or the GEGLU gate, see fmc_linear_bf16) on the bf16 MFMA kernel.
    x `[..., K]`, weight `[N, K]`; residual has the output's shape.  `tile` may also be an autotune arm id
    (`tile + 16 * log2(split_k)`).  `x2 [..., K2]`: the A operand is the concat `[x, x2]` (weight `[N, K + K2]`),
    never materialised.  `out`: a 2-D `[M, N]` view (e.g. a column slice of a wider tensor) to write instead of a new tensor."""
    tile, split_k = _decode_arm(tile, split_k)
    _dev(x, weight, bias, residual, x2)
    N, Kd = weight.shape
    if tile == 18:
        M0 = x.numel() // x.shape[-1]
        if x2 is not None or N % 320 or split_k < 1 or not _below_2gib(M0 * max(Kd, N)) or not _below_2gib(N * Kd):
            tile = 16                                   # (not a case tile 16 takes on a packed weight: row-major, with tile 16's own fall-backs)
        else:
            weight = _w_tilemajor(weight)
    M, ldx = _rows2d(x)
    ldx2, k_split = 0, 0
    if x2 is not None:
        M2, ldx2 = _rows2d(x2)
        k_split = x.shape[-1]
        assert M2 == M and k_split + x2.shape[-1] == Kd
    n_out = N // 2 if geglu else N
    ldo = n_out
    if out is None:
        out = torch.empty(*x.shape[:-1], n_out, dtype=x.dtype, device=x.device)
    else:
        assert out.dtype == x.dtype and out.shape[-1] == n_out and _rows2d(out)[0] == M and tile != 18
        ldo = _rows2d(out)[1]
    ldres = _ldres(out, residual, residual2)
    ws, ws_bytes = _splitk_workspace(x.device, split_k, M, N)
    _own_linear("fmc_linear_bf16", "geglu" if geglu else f"t{tile}", M, N, Kd, (residual is not None) + (residual2 is not None),
                x.data_ptr(), weight.data_ptr(), _p(bias), _p(residual), out.data_ptr(), M, N, Kd, ldx, ldres, ldo, float(alpha), int(geglu), int(tile),
                int(split_k), ws, ws_bytes, _p(x2), ldx2, k_split, _p(residual2))
    return out


def conv3x3_supported(x: torch.Tensor, weight: torch.Tensor, stride, padding) -> bool:
    s2 = tuple(stride) == (2, 2) and x.shape[-1] % 2 == 0 and x.shape[-2] % 2 == 0
    return (x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
            and tuple(weight.shape[2:]) == (3, 3) and (tuple(stride) == (1, 1) or s2) and tuple(padding) == (1, 1)
            and weight.shape[1] % 64 == 0 and weight.shape[0] % 8 == 0)


def conv3x3_bf16(x_nhwc: torch.Tensor, weight_cl: torch.Tensor, bias: Optional[torch.Tensor] = None,
                 temb: Optional[torch.Tensor] = None, residual_nhwc: Optional[torch.Tensor] = None,
                 tile: int = 0, split_k: int = 1, temb_div: int = 1, upsample: bool = False,
                 stride2: bool = False) -> torch.Tensor:
    """x `[N, H, W, Cin]` contiguous, weight `[Cout, Cin, 3, 3]` in channels_last memory format (physically
    `[Cout, 3, 3, Cin]`), temb `[N // temb_div, Cout]` (rows may be strided: a column slice of a wider matrix),
    residual `[N, H, W, Cout]` -> `[N, H, W, Cout]`."""
    _dev(x_nhwc, weight_cl, bias, temb, residual_nhwc)
    n, h, w, cin = x_nhwc.shape
    if upsample:                                        # x is the half-resolution source of a nearest 2x upsample
        h, w = 2 * h, 2 * w
    if stride2:                                         # 3x3 / stride 2 / pad 1 (even input size): output is half-size
        assert not upsample and h % 2 == 0 and w % 2 == 0
        h, w = h // 2, w // 2
    cout = weight_cl.shape[0]
    assert x_nhwc.is_contiguous() and weight_cl.is_contiguous(memory_format=torch.channels_last)
    assert temb is None or (temb.stride(1) == 1 and temb.shape == (n // temb_div, cout) and n % temb_div == 0)
    assert residual_nhwc is None or (residual_nhwc.is_contiguous() and residual_nhwc.shape == (n, h, w, cout))
    out = torch.empty(n, h, w, cout, dtype=x_nhwc.dtype, device=x_nhwc.device)
    tile, split_k = _decode_arm(tile, split_k)
    if tile == 18:
        if cout % 320 or cin % 64 or split_k < 1 or x_nhwc.numel() * 2 >= (1 << 31) or weight_cl.numel() * 2 >= (1 << 31):
            tile = 16
        else:
            weight_cl = _w_tilemajor_conv(weight_cl)
    ws, ws_bytes = _splitk_workspace(x_nhwc.device, split_k, n * h * w, cout)
    _lib.check(_lib.load().fmc_conv3x3_bf16(x_nhwc.data_ptr(), weight_cl.data_ptr(), _p(bias), _p(temb),
                                            _p(residual_nhwc), out.data_ptr(), n, h, w, cin, cout,
                                            0 if temb is None else temb.stride(0), int(temb_div), 2 if stride2 else int(upsample),
                                            int(tile),
                                            int(split_k), ws, ws_bytes, _stream()),
               "fmc_conv3x3_bf16")
    return out


LN_EPILOGUE = os.environ.get("FMC_LN_EPILOGUE", "1") != "0"      # A/B switch: the consumer's LayerNorm out of the producing GEMM's epilogue
ln_epilogue_calls = {"emitted": 0, "consumed": 0}


class LnSpec:
    """The LayerNorm a GEMM output feeds (`fmc_linear_bf16_ln`): fp32 gamma / beta, eps, optional positional-encoding table `[>= frames, C]`
    with `pe[(row // pe_inner) % pe_frames]` added after normalising; `key` identifies the consumer (module, pe arguments)."""
    __slots__ = ("gamma", "beta", "eps", "pe", "pe_inner", "pe_frames", "key", "stats_only")

    def __init__(self, gamma, beta, eps, pe, pe_inner, pe_frames, key, stats_only: bool = False):
        self.gamma, self.beta, self.eps, self.pe, self.pe_inner, self.pe_frames, self.key = gamma, beta, eps, pe, pe_inner, pe_frames, key
        self.stats_only = stats_only                    # the consumer is a GEMM that applies the norm itself (`linear_lnc`): only (mean, rstd) per row


_cu_count = {}


def _cus(device) -> int:
    n = _cu_count.get(device.index)
    if n is None:
        n = _cu_count[device.index] = torch.cuda.get_device_properties(device).multi_processor_count & ~7
    return n


def ln_emit_ok(x: torch.Tensor, weight: torch.Tensor, residual, residual2, ln: LnSpec) -> bool:
    N, Kd = weight.shape
    M = x.numel() // x.shape[-1]
    return (LN_EPILOGUE and not torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
            and x.is_contiguous() and weight.is_contiguous() and N == 320 and Kd % 64 == 0
            and _g160_persistent(M, N, x.device, at_least=False)                       # (inherited, not derived: N == 320 -- whole rows in a tile; more tiles than CUs)
            and ln.gamma.numel() == 320 and ln.gamma.dtype == torch.float32 and ln.beta.dtype == torch.float32
            and (ln.pe is None or (ln.pe.dtype == torch.float32 and ln.pe.is_contiguous() and ln.pe.shape[-1] == 320 and ln.pe_inner % 160 == 0
                                   and ln.pe.shape[0] >= ln.pe_frames))
            and (residual is None or (residual.is_contiguous() and residual.dtype == x.dtype))
            and (residual2 is None or residual2.is_contiguous()) and _below_2gib(M * max(Kd, 320)))


def carry_ln(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    tag = getattr(src, "_fmc_ln", None)
    if tag is not None:
        dst._fmc_ln = tag
    return dst


def take_ln(x: torch.Tensor, key) -> Optional[torch.Tensor]:
    """LayerNorm(x) if x's producer already wrote it for exactly this consumer, else None."""
    tag = getattr(x, "_fmc_ln", None)
    if tag is None or tag[1] != key or torch.is_grad_enabled() or tag[2]:
        return None
    ln_epilogue_calls["consumed"] += 1
    return tag[0].view(x.shape)


def take_ln_stats(x: torch.Tensor, key) -> Optional[torch.Tensor]:
    """(mean, rstd) `[M, 2]` fp32 of x's rows if x's producer wrote them for exactly this consumer, else None."""
    tag = getattr(x, "_fmc_ln", None)
    if tag is None or tag[1] != key or torch.is_grad_enabled() or not tag[2]:
        return None
    return tag[0]


def pending_ln(x: torch.Tensor, stats: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    """x itself (a fresh view, so the tag stays off the residual stream's tensor) marked "LayerNorm still to be applied": the next
    `linear` / `geglu_linear` applies it in its epilogue (`linear_lnc`) or, where it cannot, materialises it first (`resolve_pending_ln`).
    Only call sites whose consumer is one of those two may ask for this (LayerNorm.forward(defer=True))."""
    v = x.view(x.shape)
    v._fmc_pending_ln = (stats, gamma, beta, eps)
    return v


def resolve_pending_ln(x: torch.Tensor) -> torch.Tensor:
    pend = getattr(x, "_fmc_pending_ln", None)
    if pend is None:
        return x
    ln_epilogue_calls["materialised"] = ln_epilogue_calls.get("materialised", 0) + 1
    return _layernorm_raw(x.contiguous(), pend[1], pend[2], pend[3], None, 1, 1)


def _ln_folded_weight(weight: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor):
    """(W diag(gamma) in bf16, c[n] = sum_k of it, W beta + bias) for `fmc_linear_bf16_lnc`; cached on the tensor that owns W's storage."""
    def build():
        w32 = weight.detach().float()
        wg = (w32 * gamma.float()[None, :]).to(torch.bfloat16).contiguous()
        b = w32 @ beta.float()
        if bias is not None:
            b = b + bias.detach().float()
        return wg, wg.float().sum(dim=1).contiguous(), b.contiguous()
    tag = (gamma.data_ptr(), gamma._version, beta.data_ptr(), beta._version, None if bias is None else (bias.data_ptr(), bias._version))
    return derived_on_owner(weight, "_fmc_lnw", tag, build)


def lnc_ok(x: torch.Tensor, weight: torch.Tensor) -> bool:
    N, Kd = weight.shape
    M = x.numel() // x.shape[-1]
    return (LN_EPILOGUE and not torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
            and x.is_contiguous() and Kd % 64 == 0 and _g160_persistent(M, N, x.device, at_least=False)      # (inherited, not derived: more tiles than CUs)
            and _below_2gib(M * max(Kd, 320)) and _below_2gib(N * Kd))


def linear_lnc(x: torch.Tensor, weight: torch.Tensor, bias, pend, geglu: bool = False) -> torch.Tensor:
    """`LayerNorm(x) @ weight^T + bias` (or its GEGLU) with the norm applied in the GEMM's epilogue from the producer's (mean, rstd)."""
    stats, gamma, beta, _ = pend
    wg, c, b = _ln_folded_weight(weight, bias, gamma, beta)
    _dev(x, wg, c, b, stats)
    N, Kd = weight.shape
    M, ldx = _rows2d(x)
    n_out = N // 2 if geglu else N
    out = torch.empty(*x.shape[:-1], n_out, dtype=x.dtype, device=x.device)
    ln_epilogue_calls["consumed"] += 1
    wt, tilemajor = _packed(wg)
    _own_linear("fmc_linear_bf16_lnc", "lnc-geglu" if geglu else "lnc", M, N, Kd, 0,
                x.data_ptr(), wt.data_ptr(), out.data_ptr(), M, N, Kd, ldx, n_out, int(geglu), stats.data_ptr(), c.data_ptr(), b.data_ptr(), tilemajor)
    return out


def linear_ln(x: torch.Tensor, weight: torch.Tensor, bias, residual, alpha: float, residual2, ln: LnSpec) -> torch.Tensor:
    """`linear_bf16` on the persistent 160 x 320 kernel that also writes the consumer's LayerNorm: out carries `_fmc_ln = (ln_out, key)`."""
    _dev(x, weight, bias, residual, ln.gamma, ln.beta, ln.pe)
    N, Kd = weight.shape
    M, ldx = _rows2d(x)
    out = torch.empty(*x.shape[:-1], N, dtype=x.dtype, device=x.device)
    ldres = 0 if residual is None else _rows2d(residual)[1]
    ln_epilogue_calls["emitted"] += 1
    if ln.stats_only:
        stats = torch.empty(M, 2, dtype=torch.float32, device=x.device)
        ln_out = None
    else:
        stats, ln_out = None, torch.empty_like(out)
    wt, tilemajor = _packed(weight)
    _own_linear("fmc_linear_bf16_ln", "ln", M, N, Kd, (residual is not None) + (residual2 is not None),
                x.data_ptr(), wt.data_ptr(), _p(bias), _p(residual), out.data_ptr(), M, N, Kd, ldx, ldres, N, float(alpha), _p(residual2), _p(ln_out),
                ln.gamma.data_ptr(), ln.beta.data_ptr(), float(ln.eps), _p(ln.pe), int(ln.pe_inner), int(ln.pe_frames), _p(stats), tilemajor)
    out._fmc_ln = (stats, ln.key, True) if ln.stats_only else (ln_out, ln.key, False)
    return out


GN_FOLD = os.environ.get("FMC_GN_FOLD", "1") != "0"             # A/B switch: the GroupNorm in front of a transformer's proj_in folded into per-image weights (below)
GN_FOLD_MAX_BYTES = 8 << 20                                       # ... while the per-image weights stay small next to the tensor (level 0: 32 x 200 KB)


def gn_fold_ok(x: torch.Tensor, gn_tag, groups: int, weight: torch.Tensor, ln: Optional[LnSpec]) -> bool:
    """`proj(GroupNorm(x))` without the normalised tensor (`linear_gnfold`): x `[n_img, hw, C]` whose producer left the GroupNorm partial sums (`gn_tag`)."""
    if not GN_FOLD or gn_tag is None or torch.is_grad_enabled() or x.ndim != 3 or weight.ndim != 2:
        return False
    n_img, hw, C = x.shape
    N = weight.shape[0]
    M = n_img * hw
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and weight.dtype == torch.bfloat16 and weight.is_contiguous() and weight.shape[1] == C
            and groups == 32 and gn_tag[1] == C and gn_tag[0].shape[0] == n_img and gn_tag[0].shape[1] <= 64 and gn_tag[0].shape[2] == groups
            and hw % 160 == 0 and C % 64 == 0 and _g160_persistent(M, N, x.device, at_least=True)      # (inherited, not derived: as many tiles as CUs suffice)
            and n_img * N * C * 2 <= GN_FOLD_MAX_BYTES and _below_2gib(M * max(C, N)) and (ln is None or (LN_EPILOGUE and ln.stats_only and N == 320)))


def linear_gnfold(x: torch.Tensor, gn_tag, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, weight: torch.Tensor, bias,
                  ln: Optional[LnSpec] = None) -> torch.Tensor:
    """`GroupNorm(x) @ weight^T + bias` with the norm folded into per-image weights: `fmc_groupnorm_fold_linear` turns the producer's partial sums into
    `W'_img = W diag(rstd_img gamma)` (bf16) and an fp32 bias row per image (built from the ROUNDED W': the mean cancels exactly), `fmc_linear_bf16_imgw`
    runs the projection on the raw tensor -- the apply pass (read + write of x) disappears.  `ln` (statistics only): as `linear_ln`."""
    part = gn_tag[0]
    _dev(x, part, gamma, beta, weight, bias)
    n_img, hw, C = x.shape
    N = weight.shape[0]
    M = n_img * hw
    lib = _lib.load()
    w_img = torch.empty(n_img, N, C, dtype=torch.bfloat16, device=x.device)
    b_img = torch.empty(n_img, N, dtype=torch.float32, device=x.device)
    gn_epilogue_calls["consumed"] += 1
    _lib.check(lib.fmc_groupnorm_fold_linear(part.data_ptr(), int(part.shape[1]), gamma.data_ptr(), beta.data_ptr(), weight.data_ptr(), _p(bias),
                                             w_img.data_ptr(), b_img.data_ptr(), n_img, hw, C, int(groups), N, float(eps), int(W_TILEMAJOR), _stream()),
               "fmc_groupnorm_fold_linear")
    out = torch.empty(n_img, hw, N, dtype=x.dtype, device=x.device)
    stats = None
    if ln is not None:
        stats = torch.empty(M, 2, dtype=torch.float32, device=x.device)
        ln_epilogue_calls["emitted"] += 1
    _own_linear("fmc_linear_bf16_imgw", "gn-fold", M, N, C, 0, x.data_ptr(), w_img.data_ptr(), b_img.data_ptr(), out.data_ptr(), M, N, C, C, N, hw, _p(stats),
                float(ln.eps) if ln is not None else 0.0, int(W_TILEMAJOR))           # (the fold kernel above has written w_img in that layout)
    if ln is not None:
        out._fmc_ln = (stats, ln.key, True)
    return out


FF_BLOCKED = os.environ.get("FMC_FF_BLOCKED", "1") != "0"        # A/B switch: tile-major intermediate between the two GEMMs of a feed-forward


def ff_blocked_ok(x: torch.Tensor, w1_il160: Optional[torch.Tensor], w2: torch.Tensor, residual) -> bool:
    """Both GEMMs of the feed-forward on tile 16 with the `[M / 160][Cff / 32][160][32]` intermediate (`fmc_linear_bf16_ffblk`)?"""
    if not FF_BLOCKED or w1_il160 is None or torch.is_grad_enabled():
        return False
    N1, Kd = w1_il160.shape
    N2, Cff = w2.shape
    M = x.numel() // x.shape[-1]
    return (x.is_cuda and x.dtype == torch.bfloat16 and w1_il160.dtype == torch.bfloat16 and w2.dtype == torch.bfloat16 and x.is_contiguous()
            and w1_il160.is_contiguous() and w2.is_contiguous() and N1 == 2 * Cff and Cff % 160 == 0 and N2 % 320 == 0 and Kd % 64 == 0
            and M >= 16384 and _g160_persistent(M, N1, x.device, at_least=False)          # (inherited, not derived: the GEGLU that writes tile-major asks more tiles than CUs)
            and _below_2gib(M * Cff) and (residual is None or (residual.is_contiguous() and residual.dtype == x.dtype)))


def geglu_linear_blocked(x: torch.Tensor, weight_il160: torch.Tensor, bias_il160) -> torch.Tensor:
    """GEGLU projection whose gated output is written tile-major (private to the feed-forward's second GEMM, `linear_from_blocked`).
    A pending LayerNorm on x (LayerNorm.forward(defer=True)) is applied in the epilogue as in `linear_lnc`."""
    pend = getattr(x, "_fmc_pending_ln", None)
    N, Kd = weight_il160.shape
    M = x.numel() // Kd
    out = torch.empty(*x.shape[:-1], N // 2, dtype=x.dtype, device=x.device)
    if pend is not None:
        stats, gamma, beta, _ = pend
        w, c, b = _ln_folded_weight(weight_il160, bias_il160, gamma, beta)
        _dev(x, w, c, b, stats)
        ln_epilogue_calls["consumed"] += 1
        bias, lnc = None, (stats.data_ptr(), c.data_ptr(), b.data_ptr())
    else:
        _dev(x, weight_il160, bias_il160)
        w, bias, lnc = weight_il160, _p(bias_il160), (None, None, None)
    wt, tilemajor = _packed(w)
    _own_linear("fmc_linear_bf16_ffblk", "geglu-blocked", M, N, Kd, 0, x.data_ptr(), wt.data_ptr(), bias, None, out.data_ptr(), M, N, Kd, 0, 1.0, 1, 0, 1, *lnc, tilemajor)
    return out


def linear_from_blocked(xb: torch.Tensor, weight: torch.Tensor, bias, residual, alpha: float = 1.0, out: Optional[torch.Tensor] = None,
                        partial_tiles: bool = False) -> torch.Tensor:
    """`alpha * (x @ weight^T + bias) + residual` for an x in the tile-major layout of `geglu_linear_blocked`; `out`: a contiguous `[M, N]` destination.
    `partial_tiles` (`fmc_linear_bf16_ffblk_partial`; also `ff_tail`): any M.  The shape contract of the tile-major intermediate then, stated once: the
    tensor has the logical shape `[..., K]` with M rows, and is the HEAD of a storage of `ff_blocked_numel(M, K)` = ceil(M / 160) * 160 * K elements that
    the data spans in tile order -- what `geglu_ln_pipe(..., blocked=True, partial_tiles=True)` returns.  It is passed on as it is: a copy (`clone`,
    `contiguous`) keeps M * K elements and loses the last tile.  The pad rows of that tile are never written and may hold anything."""
    _dev(xb, weight, bias, residual, out)
    N, Kd = weight.shape
    M = xb.numel() // Kd
    if out is None:
        out = torch.empty(*xb.shape[:-1], N, dtype=xb.dtype, device=xb.device)
    assert out.is_contiguous() and out.numel() == M * N and out.dtype == xb.dtype
    wt, tilemajor = _packed(weight)
    assert not partial_tiles or _blocked_storage_ok(xb, M, Kd), "linear_from_blocked: the tile-major operand does not own its padded storage"
    # (the whole-tile entry point is the general blocked GEMM: no GEGLU, no LayerNorm epilogue -- the arguments the partial one does not have)
    _own_linear(_entry("fmc_linear_bf16_ffblk", partial_tiles)[0], "from-blocked-partial" if partial_tiles else "from-blocked", M, N, Kd, int(residual is not None),
                xb.data_ptr(), wt.data_ptr(), _p(bias), _p(residual), out.data_ptr(), M, N, Kd, 0 if residual is None else N, float(alpha),
                *(() if partial_tiles else (0, 1, 0, None, None, None)), tilemajor)
    return out


FF_TAIL = os.environ.get("FMC_FF_TAIL", "1") != "0"             # A/B switch: feed-forward output projection + proj_out as one product (below)


def ff_tail_ok(h: torch.Tensor, w2: torch.Tensor, wp: torch.Tensor, tail_residual: Optional[torch.Tensor]) -> bool:
    """`proj_out(ff2(g) + b2 + h) + bp + x` as ONE launch on the tile-major intermediate (`ff_tail`): the level-0 transformers, where both GEMMs are
    HBM passes (K = 1280 and K = 320 on 81 920 rows) -- the folded product reads g, h and x once and writes once, the block's output is never stored."""
    return _ff_tail_ok(h, w2, wp, tail_residual, any_rows=False)


def fold_ff_tail(w2: torch.Tensor, b2: Optional[torch.Tensor], wp: torch.Tensor, bp: Optional[torch.Tensor]):
    """([Wp W2 | Wp] as bf16 [N, Cff + C], Wp b2 + bp as bf16 [N] or None): folded in fp32, rounded once."""
    with torch.no_grad():
        wpf = wp.detach().float()
        wc = torch.cat([wpf @ w2.detach().float(), wpf], dim=1).to(torch.bfloat16).contiguous()
        bc = None
        if b2 is not None or bp is not None:
            bc = (wpf @ b2.detach().float()) if b2 is not None else torch.zeros(wp.shape[0], dtype=torch.float32, device=wp.device)
            if bp is not None:
                bc = bc + bp.detach().float()
            bc = bc.to(torch.bfloat16).contiguous()
    return wc, bc


def ff_tail(mid_blocked: torch.Tensor, h: torch.Tensor, w_cat: torch.Tensor, b_cat: Optional[torch.Tensor], tail_residual: torch.Tensor,
            gn_hw: int = 0, partial_tiles: bool = False) -> torch.Tensor:
    """`[g | h] @ w_cat^T + b_cat + tail_residual` (`fmc_linear_bf16_fftail`): g = `mid_blocked`, the tile-major gated intermediate; `h` row-major `[M, C]`.
    With `gn_hw` the 160-row tiles also leave the consumer GroupNorm's partial sums (as `linear_gn`).  Returns `[..., N]` in `tail_residual`'s shape.
    `partial_tiles`: any M on `fmc_linear_bf16_fftail_partial` (`mid_blocked` as `linear_from_blocked` describes; no GroupNorm partial sums)."""
    _dev(mid_blocked, h, w_cat, b_cat, tail_residual)
    N, Kd = w_cat.shape
    C = h.shape[-1]
    M = h.numel() // C
    assert mid_blocked.numel() == M * (Kd - C) and tail_residual.numel() == M * N
    out = torch.empty_like(tail_residual)
    assert not partial_tiles or _blocked_storage_ok(mid_blocked, M, Kd - C), "ff_tail: the tile-major operand does not own its padded storage"
    part = None
    if gn_hw and not partial_tiles and gn_emit_ok(M, N, Kd, gn_hw, h.dtype):
        part = torch.empty(M // gn_hw, gn_hw // 160, 32, 2, dtype=torch.float32, device=h.device)
        gn_epilogue_calls["emitted"] += 1
    wt, tilemajor = _packed(w_cat)
    _own_linear(_entry("fmc_linear_bf16_fftail", partial_tiles)[0], "ff-tail-partial" if partial_tiles else "ff-tail", M, N, Kd, 1,
                mid_blocked.data_ptr(), h.data_ptr(), wt.data_ptr(), _p(b_cat), tail_residual.data_ptr(), out.data_ptr(), M, N, Kd, Kd - C, C, N, _p(part),
                int(gn_hw if part is not None else 0), tilemajor)
    if part is not None:
        out._fmc_gn = (part, N)
    return out


def linear_gn(x: torch.Tensor, weight: torch.Tensor, bias, residual, alpha: float, residual2, hw: int):
    """`linear_bf16` on the 160 x 320 kernel + the GroupNorm partial sums of the output: (out, partials [M / hw, hw / 160, 32, 2])."""
    _dev(x, weight, bias, residual)
    N, Kd = weight.shape
    M, ldx = _rows2d(x)
    out = torch.empty(*x.shape[:-1], N, dtype=x.dtype, device=x.device)
    part = torch.empty(M // hw, hw // 160, 32, 2, dtype=torch.float32, device=x.device)
    ldres = 0 if residual is None else _rows2d(residual)[1]
    gn_epilogue_calls["emitted"] += 1
    wt, tilemajor = _packed(weight)
    _own_linear("fmc_linear_bf16_gn", "gn", M, N, Kd, (residual is not None) + (residual2 is not None),
                x.data_ptr(), wt.data_ptr(), _p(bias), _p(residual), out.data_ptr(), M, N, Kd, ldx, ldres, N, float(alpha), _p(residual2), part.data_ptr(), int(hw), tilemajor)
    out._fmc_gn = (part, N)
    return out


def conv3x3_gn(x_nhwc: torch.Tensor, weight_cl: torch.Tensor, bias, temb, residual_nhwc, temb_div: int, upsample: bool, stride2: bool):
    n, h, w, cin = x_nhwc.shape
    if upsample:
        h, w = 2 * h, 2 * w
    if stride2:
        h, w = h // 2, w // 2
    cout = weight_cl.shape[0]
    out = torch.empty(n, h, w, cout, dtype=x_nhwc.dtype, device=x_nhwc.device)
    part = torch.empty(n, (h * w) // 160, 32, 2, dtype=torch.float32, device=x_nhwc.device)
    gn_epilogue_calls["emitted"] += 1
    wt = _w_tilemajor_conv(weight_cl) if W_TILEMAJOR else weight_cl
    _lib.check(_lib.load().fmc_conv3x3_bf16_gn(x_nhwc.data_ptr(), wt.data_ptr(), _p(bias), _p(temb), _p(residual_nhwc), out.data_ptr(),
                                               n, h, w, cin, cout, 0 if temb is None else temb.stride(0), int(temb_div),
                                               2 if stride2 else int(upsample), part.data_ptr(), int(W_TILEMAJOR), _stream()), "fmc_conv3x3_bf16_gn")
    return out, (part, cout)


# --------------------------------------------------------------------------------------------
# 3x3 convolution with the input halo resident in LDS and GroupNorm + SiLU applied while it is staged (csrc/conv_halo.hip; SURVEY.md
# section 8 f1).  `conv(silu(norm(x)))` of diffusers' ResnetBlock2D as: statistics (out of the producer's epilogue, or one read of x) ->
# `fmc_groupnorm_coef` (per-(image, channel) scale / shift) -> `fmc_conv3x3_halo_bf16` reading the RAW x.  FMC_CONV_HALO=0: A/B switch.
# --------------------------------------------------------------------------------------------
CONV_HALO = os.environ.get("FMC_CONV_HALO", "1") != "0"
CONV_HALO_MIN_TILES = int(os.environ.get("FMC_CONV_HALO_MIN_TILES", "200"))     # workgroups below which the ring / stream-K arms keep the shape
LINEAR4 = os.environ.get("FMC_LINEAR4", "1") != "0"            # A/B switch: `fmc_linear4_bf16` is a candidate arm of the projections
CONV_HALO4 = os.environ.get("FMC_CONV_HALO4", "1") != "0"       # A/B switch: the 4-wave form on the 10x16 / 5x8 levels
CONV_GN_FUSED = os.environ.get("FMC_CONV_GN_FUSED", "0") == "1"   # GroupNorm + SiLU in the conv's operand path instead of a separate apply pass (measured slower)
conv_halo_calls = {"conv": 0, "gn_fused": 0, "stats_pass": 0, "stats_from_producer": 0}


def conv3x3_halo_supported(n: int, h: int, w: int, cin: int, cin1: int, cout: int, upsample: bool) -> bool:
    return bool(_lib.load().fmc_conv3x3_halo_supported(n, h, w, cin, cin1, cout, int(upsample)))


# ---- the halo convolutions at any image width: partly filled column tiles (include/fmc_hip.h: fmc_conv3x3_halo*_partial_*).  The wrappers take
# `partial_tiles=True`; `conv3x3`, `conv3x3_upfold_arm` and `shortcut_fold_ok` ask for it only with `PARTIAL_TILES` on, and only where
# `partial_conv_routed` says that the launch measured faster than the route the shape takes without (profiles/partial_tiles.md section 17;
# tools/partial_conv_rates.py).  The kinds -- "halo4": a width that is no multiple of 8 (ring kernel / vendor arm today) on conv_halo4's row blocks;
# "halo": a width that is no multiple of 32 on the 10 x 32 tiles (conv_halo4's whole row blocks today where W % 8 == 0);  "halo_sc": the shortcut fold
# on them;  "upfold_halo" / "upfold_halo4": the phase mode of the upsample sites.  FMC_PARTIAL_CONV names the kinds that may be routed at all (A/B).
PARTIAL_CONV_ROUTED = frozenset(k for k in os.environ.get("FMC_PARTIAL_CONV", "halo,halo_sc,halo4,upfold_halo4").split(",") if k)
PARTIAL_CONV_RULES = True           # False: every shape of a routed kind goes to the partial launch (the measurement itself, tests)


def partial_conv_routed(kind: str, n: int, h: int, w: int, cin: int, cout: int) -> bool:
    """The routing decisions of profiles/partial_tiles.md section 17 in closed form (h x w: the launch's own image -- the SOURCE of a fold).  Every
    measured (shape, kind) pair that cleared "median below the parent route's by more than the legs' spread" at 16x256x384 is routed, none that did not is;
    where one bound had to separate the two, marginal wins (3 - 8 %, 16x512x768) fall on the unrouted side."""
    if kind not in PARTIAL_CONV_ROUTED:
        return False
    if not PARTIAL_CONV_RULES:
        return True
    macs = n * h * w * cin * cout                          # per filter tap
    if kind in ("halo", "halo_sc"):
        # 10 x 32 tiles: at least three quarters of the last column tile filled (W = 24, 48; W = 12 and 6 measured 0.26 - 0.92 of the parent route) ...
        if 4 * w < 3 * 32 * ((w + 31) // 32):
            return False
        # ... and a launch small enough that the tile shape still matters: against conv_halo4's 10 x 16 row blocks (W % 16 == 0) and with the shortcut
        # the gain is gone from 10e9 multiply-adds per tap on (1.00 - 1.03), against its 5 x 8 row blocks (W = 24) from 30e9 on
        return macs <= (7e9 if kind == "halo_sc" or w % 16 == 0 else 21e9)
    if kind == "halo4":
        # against the ring kernel's arms: ahead (1.06 - 1.20) up to 1280 input channels and 2^21 input elements, level or behind (0.94 - 1.05) beyond
        return cin <= 1280 and n * h * w * cin <= (1 << 21)
    return True                                            # the folds: 1.42 - 1.71 on conv_halo4's row blocks at every source measured


def conv3x3_halo_partial_supported(n: int, h: int, w: int, cin: int, cin1: int, cout: int, upsample: bool) -> bool:
    return bool(_lib.load().fmc_conv3x3_halo_partial_supported(n, h, w, cin, cin1, cout, int(upsample)))


class HaloRoute(NamedTuple):
    """One halo launch.  `kernel`: "halo" (10 x 32-pixel tiles, csrc/conv_halo.hip), "halo4" / "halo4w" (row blocks on 4 / 8 waves, csrc/conv_halo4.hip);
    `partial`: the `*_partial_*` entry points (a partly filled last column tile); `tw`: the row-block width of a partial conv_halo4 launch (a whole-tile
    one picks its own: None); `split`: workgroups per tile over the reduction; `bn`: output channels per tile."""
    kernel: str
    partial: bool = False
    tw: Optional[int] = None
    split: int = 1
    bn: int = 160

    @property
    def arm(self) -> str:                                   # what `conv3x3_upfold_arm` answers
        return self.kernel + ("_partial" if self.partial else "")
    @property
    def mark(self) -> tuple:                                # behind the shape of a `call_log` entry: bench.py tells the partial launches' shapes by it
        return () if not self.partial else (("partial",) if self.kernel == "halo" else (("partial", self.tw),))
    @property
    def tail(self) -> tuple:                                # the entry point's arguments between the operands and the stream
        return () if self.kernel == "halo" else (int(self.kernel == "halo4w"),) + ((self.tw,) if self.partial else ())

    def entry(self, form: str, what: str):                  # (name, function) in C: `form` "" (plain) / "_sc" / "_fold", `what` "supported" / "bf16"
        name = "fmc_conv3x3_%s%s%s_%s" % ("halo" if self.kernel == "halo" else "halo4", form, "_partial" if self.partial else "", what)
        return name, getattr(_lib.load(), name)


def _halo4_tw(h: int, w: int, wide: bool, tw: Optional[int] = None) -> int:
    """The row-block width of a partial conv_halo4 launch: the caller's, else the library's choice for the image (`fmc_conv3x3_halo4_partial_tw`)."""
    return int(_lib.load().fmc_conv3x3_halo4_partial_tw(h, w, int(wide))) if tw is None else int(tw)


def _halo_tiles(route: HaloRoute, n: int, h: int, w: int, cout: int, phases: int = 1):
    """(workgroups before any split over the reduction, statistics slots per image) of a launch on `n` images `h x w` (the SOURCE of a fold, which
    has `phases` = 4 channel-tile sets and slots per pixel tile): what is held against `CONV_HALO_MIN_TILES` and what sizes the partials."""
    L = _lib.load()
    if route.kernel == "halo":
        per = (L.fmc_conv3x3_halo_partial_tiles_per_image if route.partial else L.fmc_conv3x3_halo_tiles_per_image)(h, w)
        return n * per * phases * (cout // 160), phases * per
    wide = int(route.kernel == "halo4w")
    if route.partial:
        return (phases * L.fmc_conv3x3_halo4_partial_tiles(n, h, w, cout, wide, int(route.tw)),
                phases * L.fmc_conv3x3_halo4_partial_row_blocks_per_image(h, w, int(route.tw)))
    return phases * L.fmc_conv3x3_halo4_tiles(n, h, w, cout, wide), phases * L.fmc_conv3x3_halo4_row_blocks_per_image(h, w)


def _halo_route(n: int, h: int, w: int, cin: int, cout: int, upsample: bool) -> Optional[HaloRoute]:
    """The halo launch of a plain stride-1 convolution with output `h x w`, or None.  In this order: the 10 x 32-pixel tiles (1.75 - 1.95 x the ring
    kernels wherever they fill the chip; tools/scratch/r05/bench_halo.py), whole, then partial; conv_halo4's row blocks (the two inner levels), split over
    the reduction where the tiles alone would leave most of the chip idle, whole, then partial (`PARTIAL_TILES`, a routed kind, a width the whole ones refuse)."""
    for kernel, partial in (("halo", False), ("halo", True), ("halo4", False), ("halo4", True)) if CONV_HALO else ():
        if (kernel == "halo4" and not CONV_HALO4) or (partial and not (PARTIAL_TILES and partial_conv_routed(kernel, n, h, w, cin, cout)
                                                                      and w % (32 if kernel == "halo" else 8))):
            continue
        route = HaloRoute(kernel, partial, bn=160 if kernel == "halo" else 80)
        if not route.entry("", "supported")[1](n, h, w, cin, cin, cout, int(upsample), *route.tail[:1]):
            continue
        if kernel == "halo4":
            tw = _halo4_tw(h, w, False) if partial else None
            route = route._replace(tw=tw, split=conv3x3_halo4_split(n, h, w, cin, cout, tw=tw))
        if _halo_tiles(route, n, h, w, cout)[0] * route.split >= CONV_HALO_MIN_TILES:
            return route
    return None


def _halo_emit_gn(route: HaloRoute, emit_gn: bool, h: int, w: int, cout: int) -> bool:
    """A halo launch with output `h x w` leaves the statistics of the GroupNorm that consumes it: asked for, no gradient, whole groups of an even number of
    channels per channel tile; conv_halo4 only where that norm would otherwise read its input twice (the large feature maps) and without a split."""
    return bool(emit_gn and GN_EPILOGUE and cout % 64 == 0 and route.bn % (cout // 32) == 0 and not torch.is_grad_enabled()
                and (route.kernel == "halo" or (h * w >= GN_MIN_HW and route.split == 1)))


def _w_packed(weight_cl: torch.Tensor, key: str, factor: int, fn: str, *args) -> torch.Tensor:
    """Channels-last 3x3 filter (physically `[Cout][3][3][Cin]`) -> a halo kernel's sub-tile order, cached on the weight per version under `key`:
    `factor` = 9 taps, or 16 for the folded filter of the phase mode; `fn(filter, packed, Cin, Cout, *args, stream)` is the C pack routine."""
    def build():
        cout, cin = weight_cl.shape[:2]
        assert weight_cl.is_contiguous(memory_format=torch.channels_last)
        out = torch.empty(cout * factor * cin, dtype=weight_cl.dtype, device=weight_cl.device)
        _lib.check(getattr(_lib.load(), fn)(weight_cl.data_ptr(), out.data_ptr(), cin, cout, *args, _stream()), fn)
        return out
    return derived_on_owner(weight_cl, "_fmc_wtm", key, build)


def _w_halo_packed(weight_cl: torch.Tensor) -> torch.Tensor:
    """The filter in `conv_halo_kernel`'s sub-tile order (`fmc_conv3x3_halo_pack_weight`: 160-channel tiles), cached on the weight."""
    return _w_packed(weight_cl, "halo", 9, "fmc_conv3x3_halo_pack_weight")


# ---- a ResnetBlock2D's 1x1 shortcut inside conv2's reduction (inference): conv2(a) + Ws [x | skip] + b2 + bs is one sum over K = 9 Cout + Cin_x
# whose last Cin_x channels are multiplied at the centre tap only -- the shortcut GEMM, its [M, Cout] write and conv2's residual read go away, and
# the shortcut product is not rounded to bf16 (include/fmc_hip.h: fmc_conv3x3_halo_sc_bf16; the 10 x 32-pixel-tile kernel only) ----
SHORTCUT_FOLD = os.environ.get("FMC_SHORTCUT_FOLD", "1") != "0"   # A/B switch: 0 = the shortcut as its own GEMM, added in conv2's epilogue
shortcut_fold_calls = {"folded": 0}


def conv3x3_halo_sc_supported(n: int, h: int, w: int, cin: int, cout: int, cin_sc: int, cin_sc1: int) -> bool:
    return bool(_lib.load().fmc_conv3x3_halo_sc_supported(n, h, w, cin, cout, cin_sc, cin_sc1))


def conv3x3_halo_sc_partial_supported(n: int, h: int, w: int, cin: int, cout: int, cin_sc: int, cin_sc1: int) -> bool:
    return bool(_lib.load().fmc_conv3x3_halo_sc_partial_supported(n, h, w, cin, cout, cin_sc, cin_sc1))


def _shortcut_route(n: int, h: int, w: int, cin: int, cout: int, cin_sc: int, cs1: int) -> Optional[HaloRoute]:
    """The launch of conv2 with the shortcut (`cin_sc` channels, `cs1` in the first source) in its reduction, or None: where the plain convolution goes to
    the 10 x 32-pixel tiles (the same conditions) and the sources fit them; with `PARTIAL_TILES` and the kind routed, a width the whole tiles refuse too."""
    for partial in (False, True):
        if partial and not (PARTIAL_TILES and partial_conv_routed("halo_sc", n, h, w, cin, cout) and w % 32):
            continue
        route = HaloRoute("halo", partial)
        if route.entry("_sc", "supported")[1](n, h, w, cin, cout, cin_sc, cs1) and _halo_tiles(route, n, h, w, cout)[0] >= CONV_HALO_MIN_TILES:
            return route
    return None


def _w_halo_sc_packed(weight_cl: torch.Tensor, w_sc: torch.Tensor, bn: int = 160) -> torch.Tensor:
    """The 3x3 filter and the 1x1 shortcut filter `[Cout, Cin_sc]` in one sub-tile order (`fmc_conv3x3_halo_sc_pack_weight`), cached on the 3x3
    weight per version of both.  The entry holds the shortcut weight, so an equal pointer is the same live storage."""
    def build():
        cout, cin = weight_cl.shape[:2]
        assert weight_cl.is_contiguous(memory_format=torch.channels_last) and w_sc.is_contiguous() and w_sc.shape[0] == cout
        out = torch.empty(cout * (9 * cin + w_sc.shape[1]), dtype=weight_cl.dtype, device=weight_cl.device)
        _lib.check(_lib.load().fmc_conv3x3_halo_sc_pack_weight(weight_cl.data_ptr(), w_sc.data_ptr(), out.data_ptr(), cin, cout, w_sc.shape[1], bn,
                                                               _stream()), "fmc_conv3x3_halo_sc_pack_weight")
        return out, w_sc
    return derived_on_owner(weight_cl, "_fmc_wtm", ("halo_sc", bn, w_sc.data_ptr(), w_sc._version, w_sc.storage_offset(), tuple(w_sc.shape)), build)[0]


def _shortcut_fold_route(x_nchw: torch.Tensor, weight_cl: torch.Tensor, xs: torch.Tensor, xs2: Optional[torch.Tensor]) -> Optional[HaloRoute]:
    """conv2 of a ResnetBlock2D takes the block's 1x1 shortcut into its reduction: inference on channels-last bf16 images of one size, on the launch
    `_shortcut_route` names.  The one decision `shortcut_fold_ok` and the `shortcut=` branch of `conv3x3` share."""
    if not (SHORTCUT_FOLD and CONV_HALO and not torch.is_grad_enabled() and x_nchw.is_cuda and weight_cl.dtype == torch.bfloat16
            and all(t is None or (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous()) for t in (x_nchw, xs, xs2))
            and weight_cl.is_contiguous(memory_format=torch.channels_last)):
        return None
    n, cin, h, w = x_nchw.shape
    cout = weight_cl.shape[0]
    if weight_cl.shape[1] != cin or xs.shape[0] != n or tuple(xs.shape[2:]) != (h, w) or (xs2 is not None and (xs2.shape[0] != n or tuple(xs2.shape[2:]) != (h, w))):
        return None
    cs1 = xs.shape[1]
    return _shortcut_route(n, h, w, cin, cout, cs1 + (xs2.shape[1] if xs2 is not None else 0), cs1)


def shortcut_fold_ok(x_nchw: torch.Tensor, weight_cl: torch.Tensor, xs: torch.Tensor, xs2: Optional[torch.Tensor]) -> bool:
    return _shortcut_fold_route(x_nchw, weight_cl, xs, xs2) is not None


def _gn_tagged(y, want: bool, cout: int):
    """A halo launch's result in `conv3x3` -- `(out, partials)` with `want`, else `out` -- as NCHW view; the statistics go with it as `_fmc_gn` for
    the GroupNorm that consumes it."""
    if not want:
        return y.permute(0, 3, 1, 2)
    y, part = y
    gn_epilogue_calls["emitted"] += 1
    y = y.permute(0, 3, 1, 2)
    y._fmc_gn = (part, cout)
    return y


def _halo_args(x_nhwc, weight_cl, temb, residual_nhwc, temb_div, upsample, x2_nhwc):
    """The shape checks `conv3x3_halo` and `conv3x3_halo4` share -> `(n, h, w, c1, cin, cout)`, h x w the OUTPUT size."""
    n, hs, ws, c1 = x_nhwc.shape
    h, w = (2 * hs, 2 * ws) if upsample else (hs, ws)
    cout, cin = weight_cl.shape[:2]
    assert x_nhwc.is_contiguous() and x_nhwc.dtype == torch.bfloat16 and weight_cl.dtype == torch.bfloat16
    if x2_nhwc is not None:
        assert x2_nhwc.is_contiguous() and x2_nhwc.shape[:3] == x_nhwc.shape[:3] and x2_nhwc.dtype == x_nhwc.dtype and c1 + x2_nhwc.shape[3] == cin
    else:
        assert c1 == cin
    assert temb is None or (temb.stride(1) == 1 and temb.shape == (n // temb_div, cout) and n % temb_div == 0)
    assert residual_nhwc is None or (residual_nhwc.is_contiguous() and residual_nhwc.shape == (n, h, w, cout))
    return n, h, w, c1, cin, cout


def groupnorm_coef(partials: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, hw: int, C: int, groups: int, eps: float,
                   want_stats: bool = False):
    """Partial (sum, sum of squares) `[N, splits, G, 2]` -> per-(image, channel) `(scale, shift)` `[N, C, 2]` of the GroupNorm (+ `[N, G, 2]` mean / rstd)."""
    _dev(partials, gamma, beta)
    N, splits, G, _ = partials.shape
    assert G == groups and partials.dtype == torch.float32 and partials.is_contiguous() and gamma.dtype == torch.float32
    coef = torch.empty(N, C, 2, dtype=torch.float32, device=partials.device)
    stats = torch.empty(N, G, 2, dtype=torch.float32, device=partials.device) if want_stats else None
    _lib.check(_lib.load().fmc_groupnorm_coef(partials.data_ptr(), splits, gamma.data_ptr(), beta.data_ptr(), coef.data_ptr(), _p(stats), N, hw, C,
                                              groups, float(eps), _stream()), "fmc_groupnorm_coef")
    return (coef, stats) if want_stats else coef


def conv3x3_halo4_supported(n: int, h: int, w: int, cin: int, cin1: int, cout: int, upsample: bool, wide: bool = False) -> bool:
    return bool(_lib.load().fmc_conv3x3_halo4_supported(n, h, w, cin, cin1, cout, int(upsample), int(wide)))


def _w_halo4_packed(weight_cl: torch.Tensor, wide: bool = False) -> torch.Tensor:
    return _w_packed(weight_cl, "halo4w" if wide else "halo4", 9, "fmc_conv3x3_halo4_pack_weight", int(wide))


def conv3x3_halo4_partial_supported(n: int, h: int, w: int, cin: int, cin1: int, cout: int, upsample: bool, wide: bool = False) -> bool:
    return bool(_lib.load().fmc_conv3x3_halo4_partial_supported(n, h, w, cin, cin1, cout, int(upsample), int(wide)))


def conv3x3_halo4_split(n: int, h: int, w: int, cin: int, cout: int, cus: int = 256, wide: bool = False, tw: Optional[int] = None) -> int:
    """Workgroups per tile: 1 where the tiles fill the chip, else the divisor of the chunk count that brings the launch closest to one round.
    `tw`: the row-block geometry of a partial-tile launch (the tile count is then that launch's)."""
    tiles = _halo_tiles(HaloRoute("halo4w" if wide else "halo4", tw is not None, tw), n, h, w, cout)[0]
    if tiles >= (3 * cus) // 4:
        return 1
    nchunk = cin // 64
    best = 1
    for s in range(2, min(nchunk, 16) + 1):
        if nchunk % s == 0 and tiles * s <= cus + cus // 8:
            best = s
    return best


def conv3x3_halo4(x_nhwc: torch.Tensor, weight_cl: torch.Tensor, bias=None, temb=None, residual_nhwc=None, temb_div: int = 1, upsample: bool = False,
                  x2_nhwc: Optional[torch.Tensor] = None, emit_gn: bool = False, split_k: Optional[int] = None, wide: bool = False,
                  partial_tiles: bool = False, tw: Optional[int] = None):
    """`conv3x3` on the small feature maps (images 8 / 16 / 32 pixels wide; csrc/conv_halo4.hip): arguments and results as `conv3x3_halo` without the
    GroupNorm operand path; the statistics partials are per (image, row block of 5 / 10 rows).
    `partial_tiles`: any width >= 1, on row blocks `tw` = 16 or 8 pixels wide (None: `fmc_conv3x3_halo4_partial_tw`) with a partly filled last block
    per image row; the partials are per (image, row block) of that geometry."""
    _dev(x_nhwc, weight_cl, bias, temb, residual_nhwc, x2_nhwc)
    n, h, w, c1, cin, cout = _halo_args(x_nhwc, weight_cl, temb, residual_nhwc, temb_div, upsample, x2_nhwc)
    assert partial_tiles or tw is None, "conv3x3_halo4: the whole-tile launch picks its own row blocks"
    tw = _halo4_tw(h, w, wide, tw) if partial_tiles else None
    route = HaloRoute("halo4w" if wide else "halo4", bool(partial_tiles), tw)
    wp = _w_halo4_packed(weight_cl, wide)
    out = torch.empty(n, h, w, cout, dtype=x_nhwc.dtype, device=x_nhwc.device)
    if split_k is None:
        split_k = 1 if emit_gn else conv3x3_halo4_split(n, h, w, cin, cout, wide=wide, tw=tw)
    ws, ws_bytes = (None, 0) if split_k <= 1 else _splitk_workspace(x_nhwc.device, split_k, n * h * w, cout)
    part = torch.empty(n, _halo_tiles(route, n, h, w, cout)[1], 32, 2, dtype=torch.float32, device=x_nhwc.device) if emit_gn else None
    conv_halo_calls["conv4"] = conv_halo_calls.get("conv4", 0) + 1
    if call_log is not None:
        call_log.append(("conv_halo4", (n, h, w, cin, cout, bool(upsample)) + route.mark, 2.0 * n * h * w * cout * 9 * cin))
    name, fn = route.entry("", "bf16")
    _lib.check(fn(x_nhwc.data_ptr(), _p(x2_nhwc), c1, wp.data_ptr(), _p(bias), _p(temb), _p(residual_nhwc), out.data_ptr(), n, h, w, cin, cout,
                  0 if temb is None else temb.stride(0), int(temb_div), int(upsample), _p(part), int(split_k), ws, ws_bytes, *route.tail, _stream()), name)
    return (out, part) if emit_gn else out


def groupnorm_partials(x: torch.Tensor, groups: int, x2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The statistics pass of a GroupNorm alone: x `[N, S, C]` (+ `x2 [N, S, C2]`: channel concat read in place) -> partial (sum, sum of squares)
    `[N, splits, G, 2]` (one read of x, no write)."""
    _dev(x, x2)
    N, S, C1 = x.shape
    C = C1 + (x2.shape[2] if x2 is not None else 0)
    assert x.is_contiguous() and (x2 is None or (x2.is_contiguous() and x2.shape[:2] == x.shape[:2] and x2.dtype == x.dtype))
    L = _lib.load()
    part = torch.empty(N, L.fmc_groupnorm_partial_splits(S, C), groups, 2, dtype=torch.float32, device=x.device)
    conv_halo_calls["stats_pass"] += 1
    _lib.check(L.fmc_groupnorm_partials(x.data_ptr(), _p(x2), C1 if x2 is not None else 0, part.data_ptr(), N, S, C, groups, _dt(x), _stream()),
               "fmc_groupnorm_partials")
    return part


def conv3x3_halo(x_nhwc: torch.Tensor, weight_cl: torch.Tensor, bias=None, temb=None, residual_nhwc=None, temb_div: int = 1, upsample: bool = False,
                 x2_nhwc: Optional[torch.Tensor] = None, gn_coef: Optional[torch.Tensor] = None, gn_act: bool = True, emit_gn: bool = False,
                 shortcut=None, partial_tiles: bool = False):
    """`conv3x3(act(x * scale + shift))` on channels-last bf16 images: x `[N, Hs, Ws, C1]` (+ `x2 [N, Hs, Ws, C2]`: channel concat read in place),
    filter `[Cout, C1 + C2, 3, 3]` channels-last, `gn_coef [N, C1 + C2, 2]` fp32 or None (plain convolution).  Returns out `[N, H, W, Cout]`, or
    `(out, partials [N, tiles, 32, 2])` with `emit_gn` (statistics of the output for the GroupNorm that consumes it).
    `shortcut = (xs [N, H, W, Cs1], xs2 [N, H, W, Cs2] | None, w_sc [Cout, Cs1 + Cs2], b_sc [Cout] | None)`: `+ w_sc . [xs | xs2] + b_sc` in the same
    reduction (plain convolution of one source without temb / residual / upsample only).
    `partial_tiles`: any width >= 1, ceil(W / 32) column tiles per image row with a partly filled last one (the `*_partial_*` entry points)."""
    _dev(x_nhwc, weight_cl, bias, temb, residual_nhwc, x2_nhwc, gn_coef)
    n, h, w, c1, cin, cout = _halo_args(x_nhwc, weight_cl, temb, residual_nhwc, temb_div, upsample, x2_nhwc)
    assert gn_coef is None or (gn_coef.shape == (n, cin, 2) and gn_coef.dtype == torch.float32 and gn_coef.is_contiguous())
    route = HaloRoute("halo", bool(partial_tiles))
    part = torch.empty(n, _halo_tiles(route, n, h, w, cout)[1], 32, 2, dtype=torch.float32, device=x_nhwc.device) if emit_gn else None
    if shortcut is not None:
        xs, xs2, w_sc, b_sc = shortcut
        _dev(xs, xs2, w_sc, b_sc)
        assert temb is None and residual_nhwc is None and x2_nhwc is None and gn_coef is None and not upsample
        cs1, cin_sc = xs.shape[3], w_sc.shape[1]
        assert xs.is_contiguous() and xs.dtype == torch.bfloat16 and xs.shape[:3] == (n, h, w) and w_sc.shape[0] == cout and w_sc.dtype == torch.bfloat16
        assert (cs1 == cin_sc) if xs2 is None else (xs2.is_contiguous() and xs2.dtype == xs.dtype and xs2.shape == (n, h, w, cin_sc - cs1))
        assert b_sc is None or (b_sc.shape == (cout,) and b_sc.dtype == torch.bfloat16 and b_sc.is_contiguous())
        wp = _w_halo_sc_packed(weight_cl, w_sc)
        out = torch.empty(n, h, w, cout, dtype=x_nhwc.dtype, device=x_nhwc.device)
        conv_halo_calls["conv"] += 1
        shortcut_fold_calls["folded"] += 1
        if call_log is not None:      # (a shape of its own: the longer launches do not enter the plain shapes' per-shape averages)
            call_log.append(("conv_halo", (n, h, w, cin, cout, False, cin_sc) + route.mark, 2.0 * n * h * w * cout * (9 * cin + cin_sc)))
        # the shortcut bias rides as a one-row "temb" shared by all images: bias + temb are summed in fp32
        name, fn = route.entry("_sc", "bf16")
        _lib.check(fn(x_nhwc.data_ptr(), wp.data_ptr(), _p(bias), _p(b_sc), out.data_ptr(), xs.data_ptr(), _p(xs2), cs1, cin_sc,
                      n, h, w, cin, cout, cout, n, _p(part), _stream()), name)
        return (out, part) if emit_gn else out
    wp = _w_halo_packed(weight_cl)
    out = torch.empty(n, h, w, cout, dtype=x_nhwc.dtype, device=x_nhwc.device)
    conv_halo_calls["conv"] += 1
    conv_halo_calls["gn_fused"] += gn_coef is not None
    if call_log is not None:
        call_log.append(("conv_halo", (n, h, w, cin, cout, bool(upsample)) + route.mark, 2.0 * n * h * w * cout * 9 * cin))
    name, fn = route.entry("", "bf16")
    _lib.check(fn(x_nhwc.data_ptr(), _p(x2_nhwc), c1, wp.data_ptr(), _p(bias), _p(temb), _p(residual_nhwc), out.data_ptr(),
                  n, h, w, cin, cout, 0 if temb is None else temb.stride(0), int(temb_div), int(upsample), _p(gn_coef),
                  int(gn_act), _p(part), _stream()), name)
    return (out, part) if emit_gn else out


# ---- the nearest-2x upsample convolutions in PHASE MODE (inference): conv3x3(upsample2x(src)) = four 2x2-tap convolutions of src, one per output
# parity, on a filter folded once per weight version (include/fmc_hip.h: fmc_conv3x3_upfold_pack_weight) -- 4 taps per output instead of 9 ----
UPS_FOLD = os.environ.get("FMC_UPS_FOLD", "1") != "0"             # A/B switch: 0 = the 9-tap launch with the upsample in the halo addressing
UPS_FOLD_MIN_WS = int(os.environ.get("FMC_UPS_FOLD_MIN_WS", "8"))     # narrowest SOURCE image that takes the folded path (per-site A/B: 16 keeps the 5x8 -> 10x16 site on 9 taps)
UPS_FOLD_WIDE = os.environ.get("FMC_UPS_FOLD_WIDE", "0") == "1"   # the 8-wave (160-channel) form of conv_halo4 for sources narrower than 32 pixels


def upsample_fold_weights(weight: torch.Tensor) -> torch.Tensor:
    """`[Cout, Cin, 3, 3]` -> `Wf[py, px, a, b, Cout, Cin]` with
    `conv3x3(nearest2x(src))[2i+py, 2j+px] = sum_{a,b} Wf[py,px,a,b] . src_padded_by_1[i+py+a, j+px+b]`: the filter rows (columns) that read the same
    source pixel are summed -- parity 0: a=0 <- w[0], a=1 <- w[1]+w[2]; parity 1: a=0 <- w[0]+w[1], a=1 <- w[2].  In the dtype of `weight` (the
    device routine sums in fp32 and rounds to bf16 once); the reference the kernels' fold is checked against."""
    rows = (((0,), (1, 2)), ((0, 1), (2,)))
    cout, cin = weight.shape[:2]
    wf = weight.new_zeros(2, 2, 2, 2, cout, cin)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    for ky in rows[py][a]:
                        for kx in rows[px][b]:
                            wf[py, px, a, b] += weight[:, :, ky, kx]
    return wf


def conv3x3_upfold_reference(x_nchw: torch.Tensor, wf: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The phase decomposition itself in plain tensor ops (any device / dtype): `x [N, Cin, Hs, Ws]`, `wf` from `upsample_fold_weights` ->
    `[N, Cout, 2 Hs, 2 Ws]`."""
    import torch.nn.functional as F
    n, _, hs, ws = x_nchw.shape
    cout = wf.shape[4]
    xp = F.pad(x_nchw, (1, 1, 1, 1))
    out = x_nchw.new_zeros(n, cout, 2 * hs, 2 * ws)
    for py in range(2):
        for px in range(2):
            k = wf[py, px].permute(2, 3, 0, 1)                # [Cout, Cin, 2, 2]
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + hs + 1, px:px + ws + 1], k)
    return out if bias is None else out + bias[None, :, None, None]


def _upfold_route(n: int, hs: int, ws: int, cin: int, cout: int) -> Optional[HaloRoute]:
    """The phase-mode launch that takes the upsample convolution of `n` source images `hs x ws`, or None (the 9-tap path keeps the shape): the whole-tile
    launches of sources at least `UPS_FOLD_MIN_WS` wide first, then, with `PARTIAL_TILES` on, the partial ones where `partial_conv_routed` says so."""
    for kernel, partial in (("halo", False), ("halo4", False), ("halo", True), ("halo4", True)) if UPS_FOLD and CONV_HALO else ():
        if (kernel == "halo4" and not CONV_HALO4) or (not partial and ws < UPS_FOLD_MIN_WS) or (
                partial and not (PARTIAL_TILES and partial_conv_routed("upfold_" + kernel, n, hs, ws, cin, cout) and ws % (32 if kernel == "halo" else 8))):
            continue
        route = HaloRoute(kernel, partial, bn=160 if kernel == "halo" else 80)
        if kernel == "halo4" and not partial and UPS_FOLD_WIDE and HaloRoute("halo4w").entry("_fold", "supported")[1](n, hs, ws, cin, cout, 1):
            route = HaloRoute("halo4w")
        if not route.entry("_fold", "supported")[1](n, hs, ws, cin, cout, *route.tail[:1]):
            continue
        if kernel == "halo4" and partial:
            route = route._replace(tw=_halo4_tw(hs, ws, False))
        if _halo_tiles(route, n, hs, ws, cout, phases=4)[0] >= CONV_HALO_MIN_TILES:
            return route
    return None


def conv3x3_upfold_arm(n: int, hs: int, ws: int, cin: int, cout: int) -> Optional[str]:
    """Which phase-mode launch takes the upsample convolution of `n` source images `hs x ws`: "halo" (10 x 32 source tiles, csrc/conv_halo.hip),
    "halo4" / "halo4w" (320 source pixels of whole row blocks, csrc/conv_halo4.hip), or None (the 9-tap path keeps the shape).  With `PARTIAL_TILES`
    on, a source width none of them takes can go to "halo_partial" / "halo4_partial", the same launches with a partly filled last column tile, where
    `partial_conv_routed` says so."""
    route = _upfold_route(n, hs, ws, cin, cout)
    return None if route is None else route.arm


def _w_upfold_packed(weight_cl: torch.Tensor, tile_channels: int) -> torch.Tensor:
    """Channels-last 3x3 filter -> the folded 4 x 2x2-tap filter in the phase-mode kernels' sub-tile order (16 / 9 of the filter's bytes), cached on
    the weight per version like the other packs."""
    return _w_packed(weight_cl, "upfold%d" % tile_channels, 16, "fmc_conv3x3_upfold_pack_weight", tile_channels)


def conv3x3_upfold(x_nhwc: torch.Tensor, weight_cl: torch.Tensor, bias=None, emit_gn: bool = False, arm: Optional[str] = None,
                   partial_tiles: bool = False, tw: Optional[int] = None):
    """`conv3x3(nearest2x(x)) + bias` in phase mode: x `[N, Hs, Ws, Cin]` channels-last bf16, the RAW filter `[Cout, Cin, 3, 3]` channels-last (folded
    and packed once per weight version) -> out `[N, 2 Hs, 2 Ws, Cout]`, or `(out, partials [N, splits, 32, 2])` with `emit_gn`.  Inference only:
    the fold is not the filter the weight gradient belongs to.  A shape no phase-mode launch takes is an error (ask `conv3x3_upfold_arm`).
    `partial_tiles` (or an arm "halo_partial" / "halo4_partial"): any source width, partly filled last column tile; `tw`: conv_halo4's row blocks."""
    _dev(x_nhwc, weight_cl, bias)
    n, hs, ws, cin = x_nhwc.shape
    cout = weight_cl.shape[0]
    assert x_nhwc.is_contiguous() and x_nhwc.dtype == torch.bfloat16 and weight_cl.dtype == torch.bfloat16 and weight_cl.shape[1] == cin
    assert not (torch.is_grad_enabled() and (x_nhwc.requires_grad or weight_cl.requires_grad)), "conv3x3_upfold: inference only"
    if arm is None:
        arm = conv3x3_upfold_arm(n, hs, ws, cin, cout)
    if arm in ("halo_partial", "halo4_partial", "halo4w_partial"):
        arm, partial_tiles = arm[:-len("_partial")], True
    if arm not in ("halo", "halo4", "halo4w"):
        raise ValueError(f"conv3x3_upfold: no phase-mode launch for n={n} {hs}x{ws} {cin}->{cout} (arm {arm})")
    tw = _halo4_tw(hs, ws, arm == "halo4w", tw) if partial_tiles and arm != "halo" else None      # (conv_halo4's partial launches alone take one)
    route = HaloRoute(arm, bool(partial_tiles), tw, bn=80 if arm == "halo4" else 160)
    wp = _w_upfold_packed(weight_cl, route.bn)
    out = torch.empty(n, 2 * hs, 2 * ws, cout, dtype=x_nhwc.dtype, device=x_nhwc.device)
    shape, flops = (n, 2 * hs, 2 * ws, cin, cout, True), 2.0 * n * 4 * hs * ws * cout * 9 * cin      # (the algorithmic, 9-tap flops: useful-work rates)
    part = torch.empty(n, _halo_tiles(route, n, hs, ws, cout, phases=4)[1], 32, 2, dtype=torch.float32, device=x_nhwc.device) if emit_gn else None
    family = "conv" if arm == "halo" else "conv4"
    conv_halo_calls["upfold"] = conv_halo_calls.get("upfold", 0) + 1
    conv_halo_calls[family] = conv_halo_calls.get(family, 0) + 1
    if call_log is not None:
        call_log.append(("conv_halo" if arm == "halo" else "conv_halo4", shape + route.mark, flops))
    name, fn = route.entry("_fold", "bf16")
    _lib.check(fn(x_nhwc.data_ptr(), wp.data_ptr(), _p(bias), out.data_ptr(), n, hs, ws, cin, cout, _p(part), *route.tail, _stream()), name)
    return (out, part) if emit_gn else out


# --------------------------------------------------------------------------------------------
# fp32-storage ("parity") mode of the two GEMMs: split-bf16 x3 operands on the same gfx950 kernels, fp32 epilogue
# (include/fmc_hip.h: fmc_split_bf16x3 / fmc_linear_x3_f32 / fmc_conv3x3_x3_f32).  FMC_F32_GEMM=0 sends fp32 projections /
# convolutions back to the vendor libraries (A/B: which part of a parity figure is the product path's own indexing).
# --------------------------------------------------------------------------------------------
F32_GEMM = os.environ.get("FMC_F32_GEMM", "1") != "0"
f32_gemm_calls = {"linear": 0, "geglu": 0, "conv3x3": 0}      # launches through the split-bf16 x3 entry points (tests assert on these)


def split_bf16x3(src: torch.Tensor, role: int, dst: Optional[torch.Tensor] = None, col0: int = 0, K: Optional[int] = None) -> torch.Tensor:
    """fp32 `[..., C]` (dense last dim, uniformly strided rows) -> bf16 `[rows, 3 K]`: activation (role 0) `[hi | hi | lo]`, weight
    (role 1) `[hi | lo | hi]`; `dst` / `col0` / `K` place a second source into the same buffer (two-source operands)."""
    _dev(src)
    assert src.dtype == torch.float32
    C = src.shape[-1]
    rows, ld = _rows2d(src)
    K = C if K is None else K
    if dst is None:
        dst = torch.empty(rows, 3 * K, dtype=torch.bfloat16, device=src.device)
    assert dst.shape == (rows, 3 * K) and dst.is_contiguous()
    _lib.check(_lib.load().fmc_split_bf16x3(src.data_ptr(), dst.data_ptr(), rows, C, ld, 3 * K, col0, K, role, _stream()),
               "fmc_split_bf16x3")
    return dst


def _split_weight_cached(weight: torch.Tensor, rows: int, C: int) -> torch.Tensor:
    """`[hi | lo | hi]` form of a frozen fp32 weight viewed as `[rows, C]`, cached per version on the tensor that owns the storage (fresh views of
    one weight share the entry)."""
    def build():
        w2 = weight.detach()
        w2 = w2.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1).reshape(rows, C) if weight.ndim == 4 else w2.reshape(rows, C)
        return split_bf16x3(w2.contiguous(), 1)
    return derived_on_owner(weight, "_fmc_w3", (rows, C), build)


def _f32_arm(key_bf16, tile: int) -> int:
    """Parity mode runs the arm the bf16 product path chose for the same problem when that is a plain-grid arm (so the checked
    code is the timed code); stream-K forms map to their plain geometry, the vendor arm / arm 15 to the kernel's own rule."""
    if tile:
        return tile
    return _f32_arm_of(_choice.get(key_bf16, 0))


def _f32_arm_of(use: int) -> int:
    """bf16 autotune arm id -> the arm parity mode runs.  The 160 x 320 family (512.. / 544.., with or without split-K; 528 = its 256-row GEGLU
    form) maps to ARM_160 -- the same kernel on the row-major split-bf16 weight -- BEFORE the stream-K offsets are peeled (all of them are >= 256);
    128+ / 256+ / 384+ stream-K forms map to their plain geometry."""
    if ARM_160 <= use < ARM_160 + 5 or ARM_160B <= use < ARM_160B + 5 or use == ARM_256:
        return ARM_160
    if use >= 384:
        use -= 384
    elif use >= 256:
        use -= 256
    elif use >= 128:
        use -= 128
    if 16 <= use < 128:                                 # split-K ids (geometry + 16 log2(split)): the geometry
        use &= 15
    return use if 1 <= use <= 14 else 0


def linear_f32(x: torch.Tensor, weight: torch.Tensor, bias=None, residual=None, alpha: float = 1.0, geglu: bool = False,
               tile: int = 0, split_k: int = 1, x2=None, residual2=None) -> torch.Tensor:
    """`linear_bf16` for fp32 tensors: split-bf16 x3 operands, fp32 accumulate, fp32 epilogue (fmc_linear_x3_f32)."""
    tile, split_k = _decode_arm(tile, split_k)
    if split_k < 1:
        split_k = 1
    _dev(x, weight, bias, residual, x2)
    N, Kd = weight.shape
    M, _ = _rows2d(x)
    if x2 is None:
        x3 = split_bf16x3(x, 0)
    else:
        k1 = x.shape[-1]
        assert k1 + x2.shape[-1] == Kd and _rows2d(x2)[0] == M
        x3 = torch.empty(M, 3 * Kd, dtype=torch.bfloat16, device=x.device)
        split_bf16x3(x, 0, x3, 0, Kd)
        split_bf16x3(x2, 0, x3, k1, Kd)
    w3 = _split_weight_cached(weight, N, Kd)
    n_out = N // 2 if geglu else N
    out = torch.empty(*x.shape[:-1], n_out, dtype=torch.float32, device=x.device)
    ldres = 0
    if residual is not None:
        assert residual.shape == out.shape and residual.dtype == torch.float32
        _, ldres = _rows2d(residual)
    if residual2 is not None:
        assert residual is not None and residual2.shape == out.shape and _rows2d(residual2)[1] == ldres
    b = None if bias is None else bias.float()
    ws, ws_bytes = _splitk_workspace(x.device, split_k, M, N)
    f32_gemm_calls["geglu" if geglu else "linear"] += 1
    _lib.check(_lib.load().fmc_linear_x3_f32(x3.data_ptr(), w3.data_ptr(), _p(b), _p(residual), out.data_ptr(), M, N, 3 * Kd,
                                             3 * Kd, ldres, n_out, float(alpha), int(geglu), int(tile), int(split_k), ws, ws_bytes,
                                             _p(residual2), _stream()), "fmc_linear_x3_f32")
    return out


def conv3x3_f32(x_nhwc: torch.Tensor, weight: torch.Tensor, bias=None, temb=None, residual_nhwc=None, tile: int = 0,
                split_k: int = 1, temb_div: int = 1, upsample: bool = False, stride2: bool = False) -> torch.Tensor:
    """`conv3x3_bf16` for fp32 tensors (x `[N, H, W, Cin]` contiguous, weight logical `[Cout, Cin, 3, 3]`)."""
    tile, split_k = _decode_arm(tile, split_k)
    if split_k < 1:
        split_k = 1
    _dev(x_nhwc, weight, bias, temb, residual_nhwc)
    n, h, w, cin = x_nhwc.shape
    if upsample:
        h, w = 2 * h, 2 * w
    if stride2:
        assert not upsample and h % 2 == 0 and w % 2 == 0
        h, w = h // 2, w // 2
    cout = weight.shape[0]
    assert x_nhwc.is_contiguous() and x_nhwc.dtype == torch.float32
    assert temb is None or (temb.stride(1) == 1 and temb.shape == (n // temb_div, cout) and temb.dtype == torch.float32)
    assert residual_nhwc is None or (residual_nhwc.is_contiguous() and residual_nhwc.shape == (n, h, w, cout))
    x3 = split_bf16x3(x_nhwc.view(-1, cin), 0)
    w3 = _split_weight_cached(weight, cout * 9, cin)
    out = torch.empty(n, h, w, cout, dtype=torch.float32, device=x_nhwc.device)
    b = None if bias is None else bias.float()
    ws, ws_bytes = _splitk_workspace(x_nhwc.device, split_k, n * h * w, cout)
    f32_gemm_calls["conv3x3"] += 1
    _lib.check(_lib.load().fmc_conv3x3_x3_f32(x3.data_ptr(), w3.data_ptr(), _p(b), _p(temb), _p(residual_nhwc), out.data_ptr(),
                                              n, h, w, 3 * cin, cout, 0 if temb is None else temb.stride(0), int(temb_div),
                                              2 if stride2 else int(upsample), int(tile), int(split_k), ws, ws_bytes, _stream()),
               "fmc_conv3x3_x3_f32")
    return out


# --------------------------------------------------------------------------------------------
# projection / convolution front-ends: pick, per problem shape, between the fused gfx950 kernel and the vendor
# library call (+ separate epilogue passes).  The choice is measured once per shape on the first eager call (the
# pipelines run eager warm-up steps before capturing a HIP graph) and cached; while a graph is being captured an
# unseen shape falls back to a static rule.  Both arms compute the same function.
# --------------------------------------------------------------------------------------------
_choice = {}
_tune_log = {}      # key -> {arm: ms} measured when the choice was made
_calls = {}         # key -> eager calls seen (graph replays do not pass through Python)
# FMC_AUTOTUNE=0: never time anything -- unseen shapes take the static rule (reproducible arm choice for tests / goldens:
# split-K and stream-K arms change the summation order, so a timing-dependent choice changes low-order bits run to run)
AUTOTUNE = os.environ.get("FMC_AUTOTUNE", "1") != "0"
# FMC_DETERMINISTIC=1: the vendor convolution arm is never chosen (MIOpen's small-image 3x3 kernels accumulate with atomics:
# bit-different results run to run, measured on the 4x4 level of the camera encoder); every fmc_* kernel is deterministic
DETERMINISTIC = os.environ.get("FMC_DETERMINISTIC", "0") == "1"
# The measured table persists on disk, keyed by the sha256 of the library build and the device name: a second process
# (the next sampling run, every rank of a multi-GPU job) starts tuned and picks the SAME arms.  FMC_AUTOTUNE_CACHE=path
# moves the file, FMC_AUTOTUNE_CACHE=0 disables persistence.
_CACHE_ENV = os.environ.get("FMC_AUTOTUNE_CACHE", "")
_cache_state = {"loaded": False, "dirty": False, "meta": None}


def _cache_path():
    if _CACHE_ENV == "0":
        return None
    return _CACHE_ENV or os.path.join(os.path.dirname(_lib.LIB_PATH), "autotune_cache.json")


def _cache_meta():
    if _cache_state["meta"] is None:
        import hashlib
        with open(_lib.LIB_PATH, "rb") as f:
            sha = hashlib.sha256(f.read()).hexdigest()[:16]
        _cache_state["meta"] = {"lib_sha16": sha, "device": torch.cuda.get_device_name() if torch.cuda.is_available() else "cpu",
                                "arms": list(GEMM_TILES), "hipblaslt": vendor_version() if torch.cuda.is_available() else 0}
    return _cache_state["meta"]


DEFAULT_ARM_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "autotune_default_mi355x.json")
stale_table_entries = [0]                          # table entries dropped by `_pick` because their arm is disabled / ineligible in this process
autotune_sources = {"cache": 0, "defaults": 0}     # shapes taken from the per-build cache / from the tracked default table (bench.py reports them)


def _load_table_file(path: str, strict_meta: bool) -> int:
    import ast
    import json
    if not path or not os.path.isfile(path):
        return 0
    try:
        with open(path) as f:
            blob = json.load(f)
        meta, mine = blob.get("meta") or {}, _cache_meta()
        if strict_meta and meta != mine:
            return 0
        if not strict_meta:                        # the tracked defaults: made for this ARCHITECTURE (device names differ from box to box)
            arch = torch.cuda.get_device_properties(torch.cuda.current_device()).gcnArchName.split(":")[0]
            if meta.get("arch") != arch:
                return 0
        n = 0
        for k, v in blob["choices"].items():
            key = ast.literal_eval(k)
            if key[0] == "valgo" and meta.get("hipblaslt") != mine["hipblaslt"]:
                continue                           # an index into ANOTHER hipBLASLt version's candidate list names other kernels: re-time on this one
            if key not in _choice:
                _choice[key] = int(v["arm"])
                _tune_log[key] = {int(a): ms for a, ms in v.get("ms", {}).items()}
                n += 1
        return n
    except Exception:                              # a corrupt table must never take the run down: re-tune
        return 0


def load_autotune_table(path: Optional[str] = None) -> int:
    """Read the persisted arm tables.  First the per-build cache next to the library (ignored unless it was made by THIS library build on this
    device type and with this arm list); then, for shapes it does not hold, the TRACKED default table `autotune_default_mi355x.json` (made on an
    MI355X by `tools/make_default_arm_table.py` from a bench run; device type must match): a fresh box then runs the arms the table was
    measured with instead of letting timing noise pick them anew (arm tables differed box to box).  `FMC_AUTOTUNE_DEFAULTS=0`
    ignores the tracked table.  Returns the number of shapes loaded.  Called lazily by the first front-end call."""
    _cache_state["loaded"] = True
    n = _load_table_file(path or _cache_path(), True)
    autotune_sources["cache"] += n
    if os.environ.get("FMC_AUTOTUNE_DEFAULTS", "1") != "0" and torch.cuda.is_available():
        d = _load_table_file(DEFAULT_ARM_TABLE, False)
        autotune_sources["defaults"] += d
        n += d
    return n


def save_autotune_table(path: Optional[str] = None) -> Optional[str]:
    """Write the arm table next to the library (atomic rename); rank 0 / single process only is the caller's business."""
    import json
    path = path or _cache_path()
    if not path or not _choice:
        return None
    blob = {"meta": _cache_meta(),
            "choices": {repr(k): {"arm": v, "ms": _tune_log.get(k, {})} for k, v in _choice.items()}}
    tmp = f"{path}.{os.getpid()}.tmp"
    try:
        with open(tmp, "w") as f:
            json.dump(blob, f)
        os.replace(tmp, path)
    except OSError:
        return None
    _cache_state["dirty"] = False
    return path


def _save_at_exit():
    if _cache_state["dirty"] and os.environ.get("RANK", "0") == "0":
        save_autotune_table()


atexit.register(_save_at_exit)
GEMM_TILES = (1, 2, 3, 4, 5, 6, 7, 11,     # 8..10, 12 (4-stage rings) exist but never won on the FMC shapes
              13,                            # the 8-phase 256x256 kernel (staggered wave rows, half-tile DMA, counted vmcnt)
              15,                            # K = 320 token projections: persistent, weights resident in registers (falls back to 5 elsewhere)
              ARM_160B if W_TILEMAJOR else ARM_160,   # 160 x 320 tiles (whole rounds / no padded columns for N = 320 k; falls back to 13 elsewhere), reading the weight
                                             # pre-packed tile-major (bit-identical to ARM_160, -1 .. -5 % per launch: tools/scratch/probe_wtm.py)
              128 + 2, 128 + 3,              # stream-K (persistent workgroups) on the two 1-per-CU geometries
              128 + 13,                      # stream-K on the 8-phase kernel: persistent partial pass + one finishing workgroup per tile
              256 + 13,                      # the same for the LAST PARTIAL ROUND of tiles only, the whole rounds on the plain grid
              384 + 13)                      # k-lockstep split on the 8-phase kernel (round 4): the filter is read once per XCD, lean finishing pass
if os.environ.get("FMC_GEMM_ARMS"):              # A/B switch: the arm list the autotuner may choose from, e.g. "1,2,3,11"
    GEMM_TILES = tuple(int(a) for a in os.environ["FMC_GEMM_ARMS"].split(","))
# fmc_linear_bf16 / fmc_conv3x3_bf16 `tile` arms tried per shape (14 = arm 13 with a deeper prefetch measured no better anywhere,
# tools/scratch/probe_g8.py)


def autotune_report():
    """[(key, chosen arm, {arm: ms}, eager calls)] for every shape tuned so far (arm 0 = vendor library)."""
    return [(k, _choice[k], _tune_log.get(k, {}), _calls.get(k, 0)) for k in _choice]


_tune_stream = None
def _graph_ms(body, reps):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=_tune_stream):
        for _ in range(reps):
            body()
    g.replay()
    _tune_stream.synchronize()
    ms = float("inf")
    for _ in range(3):                              # min of 3: one noisy sample must not pick the arm
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        _tune_stream.synchronize()
        ms = min(ms, e0.elapsed_time(e1) / reps)
    del g
    return ms


def _time_ms(fn, reps=8):
    """GPU time of one `fn()` call, measured on a captured HIP graph of `reps` calls so that the Python / launch
    overhead of the 10-30 us kernels does not decide the arm (in the pipelines they replay from a graph as well)."""
    global _tune_stream
    if _tune_stream is None:
        _tune_stream = torch.cuda.Stream()
    cur = torch.cuda.current_stream()
    _tune_stream.wait_stream(cur)
    with torch.cuda.stream(_tune_stream):
        fn()                                            # lazy initialisation (workspaces, library heuristics) outside capture
        _tune_stream.synchronize()
        ms = _graph_ms(fn, reps)
    cur.wait_stream(_tune_stream)
    return ms


NO_VENDOR = os.environ.get("FMC_NO_VENDOR", "0") == "1"      # A/B switch: the vendor library (hipBLASLt / MIOpen) is never a candidate arm
# where the calls of the three GEMM-shaped front-ends went (bench.py counts one eager step): "own" = a kernel of this library, "vendor" = the
# autotuner chose the vendor arm, "ineligible" = the shape / dtype / layout is outside the own kernels and the call fell through to the library
dispatch_calls = {k: {"own": 0, "vendor": 0, "ineligible": 0} for k in ("linear", "geglu", "conv3x3")}
call_log = None                     # a list while bench.py records one eager step: (front-end, shape tuple, algorithmic flops) per launch


def _log_call(family: str, shape: tuple, flops: float) -> None:
    """One launch of a GEMM-shaped front-end into `call_log` (bench.py: flops per kernel family of the step, and -- by launch order within a
    family -- the in-step duration of one SHAPE of a kernel that serves several).  Families: "own_linear" (one gemm* launch of this library),
    "vendor" (one hipBLASLt launch), "geglu_direct", "fused_block" (temporal / text cross-attention block), "conv_halo", "conv_halo4", "mxfp8" (one launch
    of the MXFP8 feed-forward chain: ("ln" | "geglu" | "linear", M, ...))."""
    if call_log is not None:
        call_log.append((family, tuple(shape), float(flops)))


def _pick(key, hip_fn, lib_fn, static_hip: bool, extra_arms=(), k320: bool = False, own_only: bool = False) -> int:
    """0 = vendor library arm, 1..6 = fused gfx950 kernel with that tile geometry (`hip_fn(tile)`)."""
    if not _cache_state["loaded"]:
        load_autotune_table()
    no_lib = (DETERMINISTIC and key[0] == "conv") or own_only or NO_VENDOR
    if no_lib:
        key = key + ("det",)
    use = _choice.get(key)
    _calls[key] = _calls.get(key, 0) + 1
    n320 = (key[5] if key[0] == "conv" else key[2]) % 320 == 0
    # the arms THIS call may run: the enabled tile list (FMC_GEMM_ARMS / W_TILEMAJOR) + the caller's gated extras (split arms, small-M tiles, arm 700 only
    # where LINEAR4 and its shape gate hold), minus the forms that exist for some shapes only
    cands = tuple(t for t in GEMM_TILES + tuple(extra_arms)
                  if (t != 15 or k320)    # (arm 15 exists for the K = 320 token projections only,
                  and (not (ARM_160 <= t < ARM_160 + 5 or ARM_160B <= t < ARM_160B + 5 or t == ARM_256) or n320))  #  arm 16 for outputs whose width is a multiple of 320)
    if use is not None and not (use in cands or (use == 0 and not no_lib) or (use == -1 and key not in _tune_log)):
        # a table entry (tracked defaults, an older cache) naming an arm that is switched off or not eligible here: an A/B run must measure the arms it
        # asked for, and a gated arm (700 on a strided x, 15 off its shape) must not be reached through the table -- drop the entry, re-tune below
        _choice.pop(key, None)
        _tune_log.pop(key, None)
        stale_table_entries[0] += 1
        use = None
    if use is None:
        if not AUTOTUNE or torch.cuda.is_current_stream_capturing():
            return 0 if not (static_hip or no_lib) else -1          # -1: kernel's own geometry heuristic
        times = ([] if no_lib else [(_time_ms(lib_fn), 0)]) + [(_time_ms(lambda t=t: hip_fn(t)), t) for t in cands]
        use = min(times)[1]
        _choice[key] = use
        _tune_log[key] = {arm: round(ms, 4) for ms, arm in times}
        _cache_state["dirty"] = True
    return use


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
           residual: Optional[torch.Tensor] = None, alpha: float = 1.0, x2: Optional[torch.Tensor] = None,
           residual2: Optional[torch.Tensor] = None, gn_hw: int = 0, ln: Optional["LnSpec"] = None,
           lazy_residual: bool = False) -> torch.Tensor:
    """`alpha * (x @ weight^T + bias) + residual [+ residual2]` for bf16 device tensors (see `linear_bf16`).  With `x2`
    the input is the concat `[x, x2]` along the last dim; the fused kernel reads the two tensors in place."""
    import torch.nn.functional as F
    pend = getattr(x, "_fmc_pending_ln", None)
    if pend is not None:                                # x's LayerNorm is still to be applied (LayerNorm.forward(defer=True))
        if (x2 is None and residual is None and residual2 is None and alpha == 1.0 and not gn_hw and ln is None and weight.is_contiguous()
                and lnc_ok(x, weight)):
            dispatch_calls["linear"]["own"] += 1
            return linear_lnc(x, weight, bias, pend)
        x = resolve_pending_ln(x)

    def lib():
        xin = x if x2 is None else torch.cat([x, x2], dim=-1)
        if alpha == 1.0 and vendor_linear_ok(xin, weight, bias, residual):
            y = vendor_linear(xin, weight, bias, residual)         # bias + residual inside the library's epilogue: no elementwise pass behind the GEMM
            return y if residual2 is None else y + residual2
        y = F.linear(xin, weight, bias)
        _log_call("vendor", (xin.numel() // xin.shape[-1], weight.shape[0], weight.shape[1], bias is not None, False), 2.0 * xin.numel() * weight.shape[0])
        if residual is not None:
            y = torch.add(residual, y, alpha=alpha)
            return y if residual2 is None else y + residual2
        return y if alpha == 1.0 else y * alpha

    N, Kd = weight.shape
    if (F32_GEMM and x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and Kd % 64 == 0 and N % 8 == 0
            and x.shape[-1] % 8 == 0 and (x.is_contiguous() or x.ndim == 2) and (x2 is None or x2.is_contiguous())
            and (residual is None or residual.dtype == torch.float32)):
        M = x.numel() // x.shape[-1]
        key = ("lin", M, N, Kd, bias is not None, (residual is not None) + (residual2 is not None), 0 if x2 is None else x.shape[-1])
        return linear_f32(x, weight, bias, residual, alpha, tile=_f32_arm(key, 0), x2=x2, residual2=residual2)
    ok = x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and Kd % 64 == 0 and N % 8 == 0
    if x2 is None:
        ok = ok and linear_supported(x, weight)
    else:
        ok = ok and x.shape[-1] % 64 == 0 and x2.dtype == x.dtype and x2.is_contiguous()
    if not ok or (x.ndim > 2 and not x.is_contiguous()):
        dispatch_calls["linear"]["ineligible"] += 1
        return lib()
    M = x.numel() // x.shape[-1]
    if ln is not None and x2 is None and not gn_hw and ln_emit_ok(x, weight, residual, residual2, ln):
        # the consumer is a LayerNorm and the 160 x 320 tile holds whole rows (N == 320): it leaves the epilogue too, x is not read again
        dispatch_calls["linear"]["own"] += 1
        return linear_ln(x, weight, bias, residual, alpha, residual2, ln)
    if (gn_hw and x2 is None and x.is_contiguous() and gn_emit_ok(M, N, Kd, gn_hw, x.dtype)
            and (residual is None or (residual.is_contiguous() and residual.dtype == x.dtype))
            and (residual2 is None or residual2.is_contiguous())):
        # the consumer is a GroupNorm at a level where it would read x twice: the 160 x 320 kernel emits the statistics from its epilogue
        dispatch_calls["linear"]["own"] += 1
        return linear_gn(x, weight, bias, residual, alpha, residual2, gn_hw)
    key = ("lin", M, N, Kd, bias is not None, (residual is not None) + (residual2 is not None),
           0 if x2 is None else x.shape[-1])
    hip = lambda tile: (linear4_bf16(x, weight, bias, residual, alpha, residual2) if tile == ARM_G4
                        else linear_bf16(x, weight, bias, residual, alpha, tile=tile, x2=x2, residual2=residual2))
    small = (ARM_SMALLM, ARM_SMALLM + 2) if (M <= 2560 and x2 is None and residual2 is None) else ()      # 64 x 128 tiles: 200-400 workgroups where 128 x 128 gives 100-200
    # the software-pipelined 160 x 160 kernel: a candidate wherever its tiles are at most two rounds of the chip (the inner levels' projections)
    t160 = ((M + 159) // 160) * ((N + 159) // 160)
    if (LINEAR4 and x2 is None and weight.is_contiguous() and 48 <= t160 <= 640 and Kd >= 320
            and _lib.load().fmc_linear4_supported(M, N, Kd, _rows2d(x)[1])                       # (a strided x with ldx % 8 != 0 must not reach the tuner's timing loop)
            and (residual is None or _rows2d(residual)[1] % 8 == 0)
            and (residual2 is None or (residual is not None and _rows2d(residual2)[1] == _rows2d(residual)[1]))):
        small = small + (ARM_G4,)
    use = _pick(key, hip, lib, Kd <= 640 and N <= 1024 and M >= 16384, split_arms(M, N, Kd) + small,
                k320=(Kd == 320 and N % 320 == 0 and M % 64 == 0 and x2 is None and residual2 is None))
    if (use == 0 and lazy_residual and LAZY_RESIDUAL and residual is not None and residual2 is None and alpha == 1.0 and x2 is None
            and N in (320, 640, 1280) and residual.is_contiguous() and not torch.is_grad_enabled()
            and not vendor_linear_ok(x, weight, bias, residual)):
        # vendor arm through torch (FMC_VENDOR_DIRECT=0): the caller's next op is a LayerNorm of `y + residual` (LayerNorm.skip): it does the add in its
        # own pass.  With the direct hipBLASLt call the residual rides in the GEMM's epilogue instead and the LayerNorm reads one tensor (-0.08 ms, same-box A/B)
        dispatch_calls["linear"]["vendor"] += 1
        y = F.linear(x, weight, bias)
        y._fmc_pending_add = residual
        return y
    dispatch_calls["linear"]["vendor" if use == 0 else "own"] += 1
    return lib() if use == 0 else hip(max(use, 0))


def geglu_linear(x: torch.Tensor, weight: torch.Tensor, bias, weight_il: torch.Tensor, bias_il, weight_il160=None,
                 bias_il160=None) -> torch.Tensor:
    """GEGLU feed-forward input projection: `a * gelu(g)`, `a, g = (x @ weight^T + bias).chunk(2)`.  `weight_il` /
    `bias_il` are the tile-interleaved copies the fused kernel wants (`models.layers.interleave_geglu`); `weight_il160` /
    `bias_il160` the [8 value | 8 gate]-per-16 order of the 160 x 320 arm (without them arm 16 is not a candidate)."""
    import torch.nn.functional as F
    pend = getattr(x, "_fmc_pending_ln", None)
    if pend is not None:
        if weight_il160 is not None and weight_il160.is_contiguous() and lnc_ok(x, weight_il160):
            return linear_lnc(x, weight_il160, bias_il160, pend, geglu=True)
        x = resolve_pending_ln(x)
    lib = lambda: geglu(F.linear(x, weight, bias))
    if (F32_GEMM and x.is_cuda and x.dtype == torch.float32 and weight_il.dtype == torch.float32 and weight_il.shape[0] % 64 == 0
            and weight_il.shape[1] % 64 == 0 and x.is_contiguous()):
        N, Kd = weight.shape
        arm = _f32_arm(("geglu", x.numel() // Kd, N, Kd), 0)
        if arm in (ARM_160, ARM_160B) and weight_il160 is not None:
            return linear_f32(x, weight_il160, bias_il160, geglu=True, tile=ARM_160)
        return linear_f32(x, weight_il, bias_il, geglu=True, tile=0 if arm in (ARM_160, ARM_160B) else arm)
    if not linear_supported(x, weight_il) or weight_il.shape[0] % 64 or (x.ndim > 2 and not x.is_contiguous()):
        dispatch_calls["geglu"]["ineligible"] += 1
        return lib()
    N, Kd = weight.shape
    M = x.numel() // Kd
    has160 = weight_il160 is not None and N % 320 == 0

    def hip(tile):
        if tile in (ARM_160, ARM_256, ARM_160B):        # (without the 160-block order these arms would silently pair wrong rows: route them to 13)
            return linear_bf16(x, weight_il160, bias_il160, geglu=True, tile=tile) if has160 else linear_bf16(x, weight_il, bias_il, geglu=True, tile=13)
        return linear_bf16(x, weight_il, bias_il, geglu=True, tile=tile)
    # (ARM_256, the persistent 256 x 320 form, is selectable but not a candidate: measured 235 / 153 / 134 us against ARM_160's 203 / 153 / 130 us on
    #  the three U-Net levels, tools/scratch/probe_g256.py -- DESIGN.md section 6, round 3.  FMC_GEMM_ARMS=...,528 offers it.)
    use = _pick(("geglu", M, N, Kd), hip, lib, M >= 65536)
    dispatch_calls["geglu"]["vendor" if use == 0 else "own"] += 1
    return lib() if use == 0 else hip(max(use, 0))


def conv3x3(x_nchw: torch.Tensor, weight_cl: torch.Tensor, bias, temb=None, residual_nchw=None, stride=(1, 1),
            padding=(1, 1), temb_div: int = 1, upsample: bool = False, emit_gn: bool = False, own_only: bool = False, shortcut=None) -> torch.Tensor:
    """3x3 conv on a logical NCHW / physical channels-last tensor with `+ temb[:, :, None, None]` and `+ residual`.
    Returns a logical NCHW view over channels-last storage.  `own_only`: the vendor library is not a candidate arm.
    `shortcut = (xs, xs2 | None, w_sc [Cout, Cin_sc], b_sc | None)` (NCHW views like x): the block's 1x1 shortcut in the same reduction; the caller
    has asked `shortcut_fold_ok` -- there is no other route for it."""
    import torch.nn.functional as F

    if shortcut is not None:
        cout = weight_cl.shape[0]
        xs, xs2, w_sc, b_sc = shortcut
        assert temb is None and residual_nchw is None and not upsample and tuple(stride) == (1, 1) and tuple(padding) == (1, 1)
        route = _shortcut_fold_route(x_nchw, weight_cl, xs, xs2)
        if route is None:
            raise RuntimeError("conv3x3: no kernel takes this shape with the shortcut in the reduction")
        want = _halo_emit_gn(route, emit_gn, x_nchw.shape[2], x_nchw.shape[3], cout)
        dispatch_calls["conv3x3"]["own"] += 1
        y = conv3x3_halo(x_nchw.permute(0, 2, 3, 1), weight_cl, bias, emit_gn=want,
                         shortcut=(xs.permute(0, 2, 3, 1), None if xs2 is None else xs2.permute(0, 2, 3, 1), w_sc, b_sc), partial_tiles=route.partial)
        return _gn_tagged(y, want, cout)

    def lib():
        xin = F.interpolate(x_nchw, scale_factor=2.0, mode="nearest") if upsample else x_nchw
        y = F.conv2d(xin, weight_cl, bias, stride, padding)
        if temb is not None:
            y = y + (temb if temb_div == 1 else temb.repeat_interleave(temb_div, dim=0))[:, :, None, None]
        if residual_nchw is not None:
            y = y + residual_nchw
        return y

    if (F32_GEMM and x_nchw.is_cuda and x_nchw.dtype == torch.float32 and weight_cl.dtype == torch.float32
            and tuple(weight_cl.shape[2:]) == (3, 3) and tuple(padding) == (1, 1) and weight_cl.shape[1] % 64 == 0
            and weight_cl.shape[0] % 8 == 0 and (tuple(stride) == (1, 1) or (tuple(stride) == (2, 2) and not upsample
                                                                           and x_nchw.shape[-1] % 2 == 0 and x_nchw.shape[-2] % 2 == 0))):
        n, cin, h, w = x_nchw.shape
        x = x_nchw.permute(0, 2, 3, 1)
        r = None if residual_nchw is None else residual_nchw.permute(0, 2, 3, 1)
        if x.is_contiguous() and (r is None or r.is_contiguous()) and (temb is None or temb.stride(1) == 1):
            s2 = tuple(stride) == (2, 2)
            ho, wo = (2 * h, 2 * w) if upsample else ((h // 2, w // 2) if s2 else (h, w))
            key = ("conv", n, ho, wo, cin, weight_cl.shape[0], temb is not None, r is not None, upsample, s2)
            return conv3x3_f32(x, weight_cl, bias, temb, r, tile=_f32_arm(key, 0), temb_div=temb_div, upsample=upsample,
                               stride2=s2).permute(0, 3, 1, 2)
    if not conv3x3_supported(x_nchw, weight_cl, stride, padding):
        dispatch_calls["conv3x3"]["ineligible"] += 1
        return lib()
    n, cin, h, w = x_nchw.shape
    cout = weight_cl.shape[0]
    x = x_nchw.permute(0, 2, 3, 1)
    r = None if residual_nchw is None else residual_nchw.permute(0, 2, 3, 1)
    if not x.is_contiguous() or (r is not None and not r.is_contiguous()):
        dispatch_calls["conv3x3"]["ineligible"] += 1
        return lib()
    if upsample:
        h, w = 2 * h, 2 * w
    stride2 = tuple(stride) == (2, 2)
    if stride2:
        h, w = h // 2, w // 2
    # the upsample convolutions at inference: four 2x2-tap convolutions of the source on the folded filter (4 taps per output instead of 9)
    if upsample and temb is None and r is None and not torch.is_grad_enabled() and x.dtype == torch.bfloat16 and weight_cl.dtype == torch.bfloat16:
        route = _upfold_route(n, h // 2, w // 2, cin, cout)
        if route is not None:
            want = _halo_emit_gn(route, emit_gn, h, w, cout)
            dispatch_calls["conv3x3"]["own"] += 1
            y = conv3x3_upfold(x, weight_cl, bias, emit_gn=want, arm=route.arm)
            return _gn_tagged(y, want, cout)
    # the halo-resident kernels (`_halo_route`); every such convolution can also leave the statistics of the GroupNorm that consumes its output
    route = _halo_route(n, h, w, cin, cout, upsample) if not stride2 and (temb is None or temb.stride(1) == 1) else None
    if route is not None:
        want = _halo_emit_gn(route, emit_gn, h, w, cout)
        dispatch_calls["conv3x3"]["own"] += 1
        if route.kernel == "halo":
            y = conv3x3_halo(x, weight_cl, bias, temb, r, temb_div, upsample, emit_gn=want, partial_tiles=route.partial)
        else:
            y = conv3x3_halo4(x, weight_cl, bias, temb, r, temb_div, upsample, emit_gn=want, partial_tiles=route.partial, tw=route.tw)
        return _gn_tagged(y, want, cout)
    if emit_gn and gn_emit_ok(n * h * w, cout, 9 * cin, h * w, x.dtype):
        dispatch_calls["conv3x3"]["own"] += 1
        y, tag = conv3x3_gn(x, weight_cl, bias, temb, r, temb_div, upsample, stride2)
        y = y.permute(0, 3, 1, 2)
        y._fmc_gn = tag
        return y
    key = ("conv", n, h, w, cin, cout, temb is not None, r is not None, upsample, stride2)
    hip = lambda tile: conv3x3_bf16(x, weight_cl, bias, temb, r, tile=tile, temb_div=temb_div,
                                    upsample=upsample, stride2=stride2).permute(0, 3, 1, 2)
    tiles = ((n * h * w + 127) // 128) * ((cout + 127) // 128)
    use = _pick(key, hip, lib, tiles >= 256, split_arms(n * h * w, cout, 9 * cin), own_only=own_only)
    dispatch_calls["conv3x3"]["vendor" if use == 0 else "own"] += 1
    return lib() if use == 0 else hip(max(use, 0))


# --------------------------------------------------------------------------------------------
# frozen-weight autograd wrappers (training stages 2-3: the U-Net is frozen, only the activation gradient flows through
# it, train_cam_obj_ctrl.py:242).  Forward = the fused front-ends above; backward-data = the same kernels:
#   conv3x3:  dX = conv3x3(dY, W') with W'[ci, ky, kx, co] = W[co, 2-ky, 2-kx, ci]   (pad 1, stride 1)
#   linear:   dX = alpha * dY @ W,  d(residual) = dY
# --------------------------------------------------------------------------------------------
def _flipped_filter(weight_cl: torch.Tensor) -> torch.Tensor:
    """`[Cin, Cout, 3, 3]` filter of the backward-data convolution, channels-last memory format.  Cached on the tensor that
    owns the weight's storage, per version: a global dict keyed by `data_ptr()` hands out stale filters when a freed
    weight's address is reused by another model."""
    return derived_on_owner(weight_cl, "_fmc_flipped", None,
                            lambda: weight_cl.detach().flip(2, 3).permute(1, 0, 2, 3).contiguous(memory_format=torch.channels_last))


class _Conv3x3Frozen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight_cl, bias, temb, residual, temb_div):
        ctx.save_for_backward(weight_cl)
        ctx.has_res = residual is not None and residual.requires_grad
        with torch.no_grad():
            return conv3x3(x, weight_cl, bias, temb, residual, (1, 1), (1, 1), temb_div)

    @staticmethod
    def backward(ctx, dy):
        (weight_cl,) = ctx.saved_tensors
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = None
        if ctx.needs_input_grad[0]:
            with torch.no_grad():
                dx = conv3x3(dy, _flipped_filter(weight_cl), None)
        return dx, None, None, None, (dy if ctx.has_res else None), None


def conv3x3_frozen(x, weight_cl, bias, temb=None, residual=None, temb_div: int = 1):
    """3x3 / stride 1 / pad 1 conv with frozen filter, differentiable w.r.t. x (and the residual)."""
    return _Conv3x3Frozen.apply(x, weight_cl, bias, temb, residual, temb_div)


# the resampling convolutions and conv_out under a gradient (frozen filter): forward = the no-grad front-end, backward-data = csrc/conv_resample_bwd.hip
# (stride 2: 1 / 2 / 2 / 4 taps per output parity; upsample: 16 taps of the transposed fold) resp. the stride-1 kernel on zero-padded channels
RESAMPLE_BWD = os.environ.get("FMC_RESAMPLE_BWD", "1") != "0"     # A/B switch: 0 = F.interpolate / F.conv2d and torch's autograd, as before
resample_bwd_calls = {"down": 0, "up": 0, "edge": 0}               # backward launches (tests assert on these)


def conv3x3_down_bwd_supported(n: int, h: int, w: int, cin: int, cout: int) -> bool:
    """`h x w`: the forward's input (= dX)."""
    return bool(_lib.load().fmc_conv3x3_down_bwd_supported(n, h, w, cin, cout))


def conv3x3_up_bwd_supported(n: int, hs: int, ws: int, cin: int, cout: int) -> bool:
    return bool(_lib.load().fmc_conv3x3_up_bwd_supported(n, hs, ws, cin, cout))


def _w_resample_bwd_packed(weight_cl: torch.Tensor, up: bool) -> torch.Tensor:
    """Channels-last 3x3 filter -> the fragment order of the backward-data kernels (stride 2: the 9 taps; upsample: the 16 taps of G, folded in fp32
    and rounded once), cached on the weight per version like the other packs: a captured step never packs."""
    return _w_packed(weight_cl, "up_bwd" if up else "down_bwd", 16 if up else 9,
                     "fmc_conv3x3_up_bwd_pack_weight" if up else "fmc_conv3x3_down_bwd_pack_weight")


def conv3x3_down_bwd(dy_nhwc: torch.Tensor, w_packed: torch.Tensor, cin: int, out: Optional[torch.Tensor] = None, tile: int = 0) -> torch.Tensor:
    """dX `[N, 2 Ho, 2 Wo, Cin]` of the 3x3 / stride-2 / pad-1 convolution from dY `[N, Ho, Wo, Cout]` (contiguous bf16) and the packed filter.
    `tile`: 0 = the launcher's choice (`fmc_conv3x3_down_bwd_tile`), 1 / 2 / 3 = that tile whatever the shape (tests, A/B)."""
    _dev(dy_nhwc, w_packed, out)
    n, ho, wo, cout = dy_nhwc.shape
    assert dy_nhwc.is_contiguous() and dy_nhwc.dtype == torch.bfloat16 and w_packed.dtype == torch.bfloat16 and w_packed.numel() == 9 * cin * cout
    if out is None:
        out = torch.empty(n, 2 * ho, 2 * wo, cin, dtype=dy_nhwc.dtype, device=dy_nhwc.device)
    assert out.is_contiguous() and out.shape == (n, 2 * ho, 2 * wo, cin) and out.dtype == dy_nhwc.dtype
    resample_bwd_calls["down"] += 1
    if call_log is not None:
        call_log.append(("conv_down_bwd", (n, 2 * ho, 2 * wo, cin, cout), 2.0 * n * ho * wo * 9 * cin * cout))
    _lib.check(_lib.load().fmc_conv3x3_down_bwd_bf16(dy_nhwc.data_ptr(), w_packed.data_ptr(), out.data_ptr(), n, 2 * ho, 2 * wo, cin, cout, tile,
                                                     _stream()),
               "fmc_conv3x3_down_bwd_bf16")
    return out


def conv3x3_up_bwd(dy_nhwc: torch.Tensor, w_packed: torch.Tensor, cin: int, out: Optional[torch.Tensor] = None, tile: int = 0) -> torch.Tensor:
    """dX `[N, Hs, Ws, Cin]` of conv3x3(nearest2x(x)) from dY `[N, 2 Hs, 2 Ws, Cout]` (contiguous bf16) and the packed folded filter.
    `tile`: 0 = the launcher's choice (`fmc_conv3x3_up_bwd_tile`), 1 = unsplit, 2 = split over the rows of G."""
    _dev(dy_nhwc, w_packed, out)
    n, hd, wd, cout = dy_nhwc.shape
    assert hd % 2 == 0 and wd % 2 == 0
    hs, ws = hd // 2, wd // 2
    assert dy_nhwc.is_contiguous() and dy_nhwc.dtype == torch.bfloat16 and w_packed.dtype == torch.bfloat16 and w_packed.numel() == 16 * cin * cout
    if out is None:
        out = torch.empty(n, hs, ws, cin, dtype=dy_nhwc.dtype, device=dy_nhwc.device)
    assert out.is_contiguous() and out.shape == (n, hs, ws, cin) and out.dtype == dy_nhwc.dtype
    resample_bwd_calls["up"] += 1
    if call_log is not None:
        call_log.append(("conv_up_bwd", (n, hs, ws, cin, cout), 2.0 * n * hs * ws * 16 * cin * cout))
    _lib.check(_lib.load().fmc_conv3x3_up_bwd_bf16(dy_nhwc.data_ptr(), w_packed.data_ptr(), out.data_ptr(), n, hs, ws, cin, cout, tile, _stream()),
               "fmc_conv3x3_up_bwd_bf16")
    return out


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """Logical NCHW -> a contiguous `[N, H, W, C]` tensor (a view when the storage is channels-last already)."""
    return t.permute(0, 2, 3, 1).contiguous()


class _Conv3x3DownFrozen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight_cl, bias):
        ctx.save_for_backward(weight_cl)
        with torch.no_grad():
            return conv3x3(x, weight_cl, bias, None, None, (2, 2), (1, 1))

    @staticmethod
    def backward(ctx, dy):
        (weight_cl,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        with torch.no_grad():
            dx = conv3x3_down_bwd(_nhwc(dy), _w_resample_bwd_packed(weight_cl, False), weight_cl.shape[1])
        return dx.permute(0, 3, 1, 2), None, None


class _Conv3x3UpFrozen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight_cl, bias):
        ctx.save_for_backward(weight_cl)
        with torch.no_grad():
            return conv3x3(x, weight_cl, bias, None, None, (1, 1), (1, 1), 1, True)

    @staticmethod
    def backward(ctx, dy):
        (weight_cl,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        with torch.no_grad():
            dx = conv3x3_up_bwd(_nhwc(dy), _w_resample_bwd_packed(weight_cl, True), weight_cl.shape[1])
        return dx.permute(0, 3, 1, 2), None, None


def conv3x3_down_frozen(x, weight_cl, bias):
    """3x3 / stride 2 / pad 1 conv (even H, W) with frozen filter, differentiable w.r.t. x: nothing is saved but the weight."""
    return _Conv3x3DownFrozen.apply(x, weight_cl, bias)


def conv3x3_up_frozen(x, weight_cl, bias):
    """conv3x3(nearest2x(x)) with frozen filter, differentiable w.r.t. x.  The forward may take the folded arms: they are the exact adjoint
    partner of the backward's G (the same fp32 sums, rounded once)."""
    return _Conv3x3UpFrozen.apply(x, weight_cl, bias)


def _edge_flipped_filter(weight: torch.Tensor) -> torch.Tensor:
    """Backward-data filter of a thin convolution (`Cout % 64 != 0`, conv_out 320 -> 4): `[Cin, Cout padded to 64, 3, 3]` with
    `W'[ci, co, ky, kx] = W[co, ci, 2-ky, 2-kx]` and zero filters for the pad, channels-last; cached on the weight like `_flipped_filter`."""
    def build():
        cout, cin = weight.shape[:2]
        wf = torch.zeros(cin, (cout + 63) // 64 * 64, 3, 3, dtype=weight.dtype, device=weight.device)
        wf[:, :cout] = weight.detach().flip(2, 3).permute(1, 0, 2, 3)
        return wf.contiguous(memory_format=torch.channels_last)
    return derived_on_owner(weight, "_fmc_flipped", "edge", build)


class _Conv3x3EdgeFrozen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, fwd):
        ctx.save_for_backward(weight)
        with torch.no_grad():
            return fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (weight,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        with torch.no_grad():
            wf = _edge_flipped_filter(weight)
            n, cout, h, w = dy.shape
            # (the zero fill and the scatter of a 64-channel dY, 16 x conv_out's real gradient, are what this route costs: forward + backward of
            #  conv_out comes out level with F.conv2d under autograd at 32 x 48, profiles/resample_backward.md)
            dyp = torch.zeros(n, h, w, wf.shape[1], dtype=dy.dtype, device=dy.device)
            dyp[..., :cout] = dy.permute(0, 2, 3, 1)
            resample_bwd_calls["edge"] += 1
            dx = conv3x3(dyp.permute(0, 3, 1, 2), wf, None, own_only=True)
        return dx, None, None


def conv3x3_edge_frozen(x, weight, fwd):
    """A thin 3x3 / stride 1 / pad 1 conv (conv_out) with frozen filter, differentiable w.r.t. x.  `fwd(x)`: the no-grad forward, whatever
    `Conv2d.forward` takes for the shape without a gradient (`Conv2d.padded_conv3x3` where Cout is no multiple of 8); backward-data = the stride-1 kernel on dY zero-padded to 64 channels with the flipped padded filter."""
    return _Conv3x3EdgeFrozen.apply(x, weight, fwd)


def _transposed_weight(weight: torch.Tensor) -> torch.Tensor:
    """`W^T [K, N]` contiguous: the backward-data GEMM `dX = dY @ W` is `fmc_linear_bf16(dY, W^T)` -- both operands
    reduction-contiguous.  Cached on the tensor that owns the storage (`derived_on_owner`): frozen weights reached through a fresh view
    every call (`weight.view(out, in)` of a 1x1 conv) hit the cache, and the entry dies with its owner.  (A module-level dict keyed by
    the storage pointer -- the first form of this cache -- handed a freed weight's W^T to the next model whose weight landed on the
    same address with the same shape: wrong gradients, silently.)"""
    return derived_on_owner(weight, "_fmc_wt", None, lambda: weight.detach().t().contiguous())


def linear_backward_data(dy: torch.Tensor, weight: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
    """`alpha * dY @ W` for a frozen `W [N, K]` on the fused gfx950 GEMM (autotuned like every projection)."""
    if dy.is_cuda and dy.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and weight.shape[0] % 64 == 0 \
            and weight.shape[1] % 8 == 0:
        with torch.no_grad():
            return linear(dy if dy.is_contiguous() else dy.contiguous(), _transposed_weight(weight), None, None, alpha)
    dx = torch.matmul(dy, weight)
    return dx if alpha == 1.0 else dx * alpha


class _LinearFrozen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, alpha):
        ctx.save_for_backward(weight)
        ctx.alpha = alpha
        ctx.has_res = residual is not None and residual.requires_grad
        with torch.no_grad():
            return linear(x, weight, bias, residual, alpha)

    @staticmethod
    def backward(ctx, dy):
        (weight,) = ctx.saved_tensors
        dx = linear_backward_data(dy, weight, ctx.alpha) if ctx.needs_input_grad[0] else None
        return dx, None, None, (dy if ctx.has_res else None), None


def linear_frozen(x, weight, bias=None, residual=None, alpha: float = 1.0):
    """`alpha * (x @ W^T + b) + residual` with frozen W, b; differentiable w.r.t. x and the residual."""
    return _LinearFrozen.apply(x, weight, bias, residual, alpha)


def column_sum(x: torch.Tensor, alpha: float = 1.0, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """`alpha * x.sum(rows)` (+ out) in fp32 `[N]` for a bf16 / fp32 token matrix `[..., N]` (contiguous, or a 2-D row-strided view):
    `fmc_column_sum`, bit-reproducible.  The bias gradient of a trainable projection."""
    _dev(x, out)
    M, ld = _rows2d(x)
    N = x.shape[-1]
    if out is None:
        out, accumulate = torch.empty(N, dtype=torch.float32, device=x.device), False
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == N
    lib = _lib.load()
    ws = _workspace(x.device, lib.fmc_column_sum_workspace_bytes(M, N))
    _lib.check(lib.fmc_column_sum(x.data_ptr(), out.data_ptr(), M, N, ld, float(alpha), int(accumulate), ws.data_ptr(), _dt(x), _stream()),
               "fmc_column_sum")
    return out


class _LinearTrainable(torch.autograd.Function):
    """`x W^T + b + residual` whose W and b train (the motion modules' proj_in / proj_out under `train_mm`).  `w_run` / `b_run` are what
    the kernels read: for fp32 masters under bf16 activations their bf16 shadows (`layers.bf16_param`), else the parameters themselves.
        forward   y = linear(x, w_run, b_run, residual)                     (the projection GEMMs of `linear`)
        backward  dX = dY W (`linear_backward_data`);  dW = dY^T X (`linear_wgrad`, straight into fp32);  db = colsum(dY) (`column_sum`)
    Gradients come back in each parameter's dtype; the residual's is dY."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, w_run, b_run, alpha=1.0):
        with torch.no_grad():
            y = linear(x, w_run, b_run, residual, alpha)
        ctx.save_for_backward(x, w_run)
        ctx.has_res = residual is not None and residual.requires_grad
        ctx.dtypes = (weight.dtype, None if bias is None else bias.dtype)
        ctx.alpha = float(alpha)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_run = ctx.saved_tensors
        dy = dy if dy.dtype == x.dtype else dy.to(x.dtype)
        dy = dy if dy.is_contiguous() else dy.contiguous()
        N, Kd = w_run.shape
        dy2 = dy.view(-1, N)
        x2 = x if (x.ndim == 2 and not x.is_contiguous()) else x.reshape(-1, Kd)
        dx = dw = db = None
        with torch.no_grad():
            if ctx.needs_input_grad[0]:
                dx = linear_backward_data(dy, w_run, ctx.alpha).view(x.shape)
            if ctx.needs_input_grad[1]:
                dw = linear_wgrad(dy2, x2, ctx.alpha).to(ctx.dtypes[0])
            if ctx.needs_input_grad[2]:
                db = column_sum(dy2, ctx.alpha).to(ctx.dtypes[1])
        return dx, dw, db, (dy if ctx.has_res else None), None, None, None


def linear_trainable(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                     w_run: Optional[torch.Tensor] = None, b_run: Optional[torch.Tensor] = None, alpha: float = 1.0) -> torch.Tensor:
    """`alpha * (x @ weight^T + bias) + residual`, differentiable in x, weight, bias and the residual, on this library's kernels (see
    `_LinearTrainable`).  `w_run` / `b_run`: the weight / bias in x's dtype (cached bf16 shadows of fp32 masters); default: a cast per call.
    `alpha` (the Camera-Adapter merge's scale) multiplies dX, dW and db; the residual's gradient is dY."""
    if w_run is None:
        w_run = weight.detach() if weight.dtype == x.dtype else weight.detach().to(x.dtype)
    if b_run is None and bias is not None:
        b_run = bias.detach() if bias.dtype == x.dtype else bias.detach().to(x.dtype)
    return _LinearTrainable.apply(x, weight, bias, residual, w_run, b_run, float(alpha))


def conv3x3_weight_grad(x_nhwc: torch.Tensor, dy_nhwc: torch.Tensor) -> torch.Tensor:
    """dW `[Cout, Cin, 3, 3]` (bf16, a permuted view) of a 3x3 / stride 1 / pad 1 convolution from its NHWC input and output
    gradient: two `fmc_nhwc_to_cmajor_padded` layout passes + one split-K `fmc_linear_bf16` per kernel row (see fmc_hip.h)."""
    _dev(x_nhwc, dy_nhwc)
    n, H, W, cin = x_nhwc.shape
    cout = dy_nhwc.shape[-1]
    assert dy_nhwc.shape[:3] == x_nhwc.shape[:3] and x_nhwc.is_contiguous() and dy_nhwc.is_contiguous()
    assert x_nhwc.dtype == torch.bfloat16 and dy_nhwc.dtype == torch.bfloat16 and cin % 8 == 0 and cout % 8 == 0
    Hp, Wp = H + 2, (W + 2 + 7) // 8 * 8
    Lk = (n * Hp * Wp + 63) // 64 * 64                 # reduction length (padded pixels), a multiple of the k-tile
    G = Wp + 8                                          # guard in front of / behind every X^T row: a tap reaches +-Wp
    Lg = Lk + 2 * G
    lib = _lib.load()
    xt = torch.empty(3, cin, Lg, dtype=torch.bfloat16, device=x_nhwc.device)
    dyt = torch.empty(cout, Lk, dtype=torch.bfloat16, device=x_nhwc.device)
    _lib.check(lib.fmc_nhwc_to_cmajor_padded(x_nhwc.data_ptr(), xt.data_ptr(), n, H, W, cin, Lg, G, 3, _stream()),
               "fmc_nhwc_to_cmajor_padded")
    _lib.check(lib.fmc_nhwc_to_cmajor_padded(dy_nhwc.data_ptr(), dyt.data_ptr(), n, H, W, cout, Lk, 0, 1, _stream()),
               "fmc_nhwc_to_cmajor_padded")
    rows = xt.view(3 * cin, Lg)
    tiles = ((3 * cin + 127) // 128) * ((cout + 127) // 128)
    split = 1
    while split < 16 and tiles * split * 2 <= 512 and Lk // 64 >= split * 4:
        split *= 2
    out = []
    for dy in range(3):
        xs = rows[:, G + (dy - 1) * Wp: G + (dy - 1) * Wp + Lk]          # [3 Cin, Lk] view, row stride Lg
        out.append(linear_bf16(xs, dyt, None, None, 1.0, tile=1, split_k=split))      # [dx * Cin + ci][co]
    dwt = torch.stack(out)                                                # [dy][dx * Cin + ci][co]
    return dwt.view(3, 3, cin, cout).permute(3, 2, 0, 1)                  # logical [Cout, Cin, ky, kx]


CONV_WGRAD = os.environ.get("FMC_CONV_WGRAD", "1") != "0"        # A/B switch: 0 = the fp32 masters' 3x3 dW through `conv3x3_weight_grad` (bf16), as before
_conv_wgrad_ws = {}


def conv3x3_wgrad_ok(n: int, h: int, w: int, cin: int, cout: int, stride: int = 1) -> bool:
    """The domain of `fmc_conv3x3_wgrad_bf16`: any n, H, W >= 1, stride 1 or 2, Cin % 16 == Cout % 16 == 0 (and 32-bit pixel / filter counts)."""
    return (min(n, h, w) >= 1 and stride in (1, 2) and cin >= 16 and cout >= 16 and cin % 16 == 0 and cout % 16 == 0
            and n * ((h - 1) // stride + 1) * ((w - 1) // stride + 1) < 2 ** 31 and 9 * cin * cout < 2 ** 31)


CONV_WGRAD_MAX_FLOPS = 80e9      # stride 1: above this the old chain's 128 x 128-tile GEMMs win (profiles/conv_wgrad.md: 832 -> 320 at 16 x 32 x 48, 118 GFLOP)


def conv3x3_wgrad_routed(n: int, h: int, w: int, cin: int, cout: int, stride: int = 1) -> bool:
    """Whether `_Conv3x3Trainable` sends an fp32 master's dW to `conv3x3_wgrad`: inside the kernel's domain and, where the old chain exists
    (stride 1), not in the shape class in which that chain measured faster by more than its own spread."""
    return conv3x3_wgrad_ok(n, h, w, cin, cout, stride) and (stride == 2 or 2.0 * n * h * w * 9 * cin * cout <= CONV_WGRAD_MAX_FLOPS)


def conv3x3_wgrad(x_nhwc: torch.Tensor, dy_nhwc: torch.Tensor, stride: int = 1, alpha: float = 1.0, out: Optional[torch.Tensor] = None,
                  accumulate: bool = False) -> torch.Tensor:
    """`alpha * dW` (+ out) of a 3x3 / pad 1 / stride 1 or 2 convolution, fp32 `[Cout, Cin, 3, 3]`, from its contiguous bf16 NHWC input
    `[N, H, W, Cin]` and output gradient `[N, Ho, Wo, Cout]`: one `fmc_conv3x3_wgrad_bf16` launch (csrc/conv_wgrad.hip), plus its combine
    when the pixel reduction is split.  `out` may be contiguous or channels-last; `out=None` allocates a contiguous one."""
    _dev(x_nhwc, dy_nhwc, out)
    n, H, W, cin = x_nhwc.shape
    cout = dy_nhwc.shape[-1]
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert x_nhwc.dtype == torch.bfloat16 and dy_nhwc.dtype == torch.bfloat16 and x_nhwc.is_contiguous() and dy_nhwc.is_contiguous()
    assert tuple(dy_nhwc.shape) == (n, ho, wo, cout), "conv3x3_wgrad: dy must be [N, (H - 1) // stride + 1, (W - 1) // stride + 1, Cout]"
    if not conv3x3_wgrad_ok(n, H, W, cin, cout, stride):
        raise RuntimeError(f"conv3x3_wgrad: no kernel for n={n} H={H} W={W} Cin={cin} Cout={cout} stride={stride}")
    if out is None:
        out = torch.empty(cout, cin, 3, 3, dtype=torch.float32, device=x_nhwc.device)
        accumulate = False
    assert out.dtype == torch.float32 and tuple(out.shape) == (cout, cin, 3, 3)
    layout = 0 if out.is_contiguous() else 1
    assert layout == 0 or out.is_contiguous(memory_format=torch.channels_last), "conv3x3_wgrad: out must be contiguous or channels-last"
    lib = _lib.load()
    need = lib.fmc_conv3x3_wgrad_workspace_bytes(n, H, W, cin, cout, stride)
    if need < 0:
        _lib.check(-1, "fmc_conv3x3_wgrad_bf16")
    ws, ws_bytes = None, 0
    if need > 0:
        dev = out.device
        key = (dev.index, torch.cuda.current_stream().cuda_stream)
        buf = _conv_wgrad_ws.get(key)
        if buf is None or buf.numel() * 4 < need:
            if buf is not None:
                _ws_retired.append(buf)        # a captured HIP graph may have baked its address
            buf = torch.empty(need // 4 + 1024, dtype=torch.float32, device=dev)
            _conv_wgrad_ws[key] = buf
        ws, ws_bytes = buf.data_ptr(), buf.numel() * 4
    _log_call("conv_wgrad", (n, H, W, cin, cout, stride), 2.0 * n * ho * wo * 9 * cin * cout)
    _lib.check(lib.fmc_conv3x3_wgrad_bf16(x_nhwc.data_ptr(), dy_nhwc.data_ptr(), out.data_ptr(), n, H, W, cin, cout, stride, layout, float(alpha),
                                          int(bool(accumulate)), ws, ws_bytes, _stream()), "fmc_conv3x3_wgrad_bf16")
    return out


def conv3x3_trainable_ok(n: int, h: int, w: int, cin: int, cout: int, stride: int = 1) -> bool:
    """Whether `conv3x3_trainable` has all three kernels for a bf16 `[n, cin, h, w]` input.  Stride 1: the forward needs Cin % 64 == 0 and the
    flipped-filter dX, whose input channels are Cout, needs Cout % 64 == 0 (`conv3x3_supported` on either filter); dW would take any multiple
    of 16.  Stride 2: even h, w, the same forward rule and `conv3x3_down_bwd_supported` for dX."""
    if cin % 64 or cout % 64 or not conv3x3_wgrad_ok(n, h, w, cin, cout, stride):
        return False
    return stride == 1 or (h % 2 == 0 and w % 2 == 0 and conv3x3_down_bwd_supported(n, h, w, cin, cout))


class _Conv3x3Trainable(torch.autograd.Function):
    """3x3 / pad 1 conv whose FILTER trains (OMC Adapter, camera encoder): forward, backward-data AND the weight gradient on the gfx950
    kernels.  Stride 1: forward / dX on the implicit-GEMM kernel (the filter is re-laid-out / flipped per step: it changes every step and
    is small next to the activations).  Stride 2 (even H, W; shadows only): the stride-2 forward, dX on `conv3x3_down_bwd`.  dW of an fp32
    master: one `conv3x3_wgrad` launch straight into fp32; of a bf16 parameter (autocast) or with FMC_CONV_WGRAD=0: pixel-reduction GEMMs
    rounded to bf16 (`conv3x3_weight_grad`, stride 1 only)."""

    @staticmethod
    def forward(ctx, x, weight, bias, w_run=None, b_run=None, stride=1):
        ctx.has_bias = bias is not None
        ctx.shadow = w_run is not None
        ctx.stride = stride
        assert stride == 1 or (stride == 2 and ctx.shadow and CONV_WGRAD and weight.dtype == torch.float32), \
            "conv3x3_trainable: stride 2 needs the bf16 shadows of an fp32 master and the direct weight gradient"
        with torch.no_grad():
            if w_run is None:
                w_run = weight.detach().to(x.dtype)
                b_run = None if bias is None else bias.detach().to(x.dtype)
                w_cl = w_run.contiguous(memory_format=torch.channels_last)
            else:       # the cached bf16 shadow of an fp32 master: its channels-last form is derived once per version
                w_cl = derived_on_owner(w_run, "_fmc_w_cl", None, lambda: w_run.contiguous(memory_format=torch.channels_last))
            ctx.save_for_backward(x, weight if not ctx.shadow else w_run)
            ctx.dtypes = (weight.dtype, None if bias is None else bias.dtype)
            if stride == 2:
                ctx.w_cl = w_cl
                return conv3x3(x, w_cl, b_run, None, None, (2, 2), (1, 1))
            return conv3x3(x, w_cl, b_run)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = dw = db = None
        with torch.no_grad():
            if ctx.needs_input_grad[0] and ctx.stride == 2:
                dx = conv3x3_down_bwd(_nhwc(dy), _w_resample_bwd_packed(ctx.w_cl, False), x.shape[1]).permute(0, 3, 1, 2)
            elif ctx.needs_input_grad[0]:
                flip = lambda: weight.detach().to(dy.dtype).flip(2, 3).permute(1, 0, 2, 3).contiguous(memory_format=torch.channels_last)
                dx = conv3x3(dy, derived_on_owner(weight, "_fmc_w_flip", None, flip) if ctx.shadow else flip(), None)
            if ctx.needs_input_grad[1]:
                n, cin, h, w = x.shape
                if (CONV_WGRAD and ctx.dtypes[0] == torch.float32 and x.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16
                        and conv3x3_wgrad_routed(n, h, w, cin, dy.shape[1], ctx.stride)):
                    dw = conv3x3_wgrad(_nhwc(x), _nhwc(dy), ctx.stride)       # (views: both are channels-last)
                else:
                    assert ctx.stride == 1
                    dw = conv3x3_weight_grad(x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)).to(ctx.dtypes[0])
            if ctx.has_bias and ctx.needs_input_grad[2]:
                if ctx.shadow and dy.dtype == torch.bfloat16:
                    db = column_sum(dy.permute(0, 2, 3, 1).reshape(-1, dy.shape[1])).to(ctx.dtypes[1])
                else:
                    db = dy.sum(dim=(0, 2, 3), dtype=torch.float32).to(ctx.dtypes[1])
        return dx, dw, (db if ctx.has_bias else None), None, None, None


def conv3x3_trainable(x, weight, bias=None, w_run=None, b_run=None, stride: int = 1):
    """3x3 / pad 1 convolution whose filter trains (see `_Conv3x3Trainable`).  `w_run` / `b_run`: the filter / bias in x's dtype
    (cached bf16 shadows of fp32 masters, `layers.bf16_param`): their channels-last, flipped and packed forms are then derived once per
    version and the bias gradient is `column_sum`; default: a cast per call.  `stride=2` (even H, W) needs the shadows of an fp32 master;
    ask `conv3x3_trainable_ok`."""
    return _Conv3x3Trainable.apply(x, weight, bias, w_run, b_run, stride)


# --------------------------------------------------------------------------------------------
# the small passes of a Camera-Encoder / OMC-Adapter training step (csrc/train_elementwise.hip)
# --------------------------------------------------------------------------------------------
def _avgpool2x2_raw(x_nhwc: torch.Tensor) -> torch.Tensor:
    n, h, w, c = x_nhwc.shape
    y = torch.empty(n, h // 2, w // 2, c, dtype=x_nhwc.dtype, device=x_nhwc.device)
    _lib.check(_lib.load().fmc_avgpool2x2_fwd(x_nhwc.data_ptr(), y.data_ptr(), n, h, w, c, _stream()), "fmc_avgpool2x2_fwd")
    return y


class _AvgPool2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_nhwc):
        ctx.shape = tuple(x_nhwc.shape)
        return _avgpool2x2_raw(x_nhwc)

    @staticmethod
    def backward(ctx, dy):
        n, h, w, c = ctx.shape
        dy = dy.contiguous()
        dx = torch.empty(ctx.shape, dtype=dy.dtype, device=dy.device)
        _lib.check(_lib.load().fmc_avgpool2x2_bwd(dy.data_ptr(), dx.data_ptr(), n, h, w, c, _stream()), "fmc_avgpool2x2_bwd")
        return dx


def avg_pool2x2(x: torch.Tensor) -> torch.Tensor:
    """`AvgPool2d(kernel_size=2, stride=2)` of a logical NCHW / physical channels-last bf16 tensor (C % 8 == 0; odd sizes floor), with its
    backward, on `fmc_avgpool2x2_fwd / _bwd`.  Returns a logical NCHW view over channels-last storage."""
    _dev(x)
    assert x.dtype == torch.bfloat16 and x.ndim == 4 and x.shape[1] % 8 == 0, "avg_pool2x2: bf16 [N, C, H, W] with C % 8 == 0"
    t = x.permute(0, 2, 3, 1)
    if not t.is_contiguous():
        t = t.contiguous()
    y = _AvgPool2x2.apply(t) if (torch.is_grad_enabled() and t.requires_grad) else _avgpool2x2_raw(t)
    return y.permute(0, 3, 1, 2)


def _dense(t: torch.Tensor) -> torch.Tensor:
    """t itself when its elements fill one block of memory in some order (contiguous or channels-last), else a contiguous copy."""
    return t if (t.is_contiguous() or (t.ndim == 4 and t.is_contiguous(memory_format=torch.channels_last))) else t.contiguous()


def _relu_raw(x: torch.Tensor) -> torch.Tensor:
    y = torch.empty_like(x)              # (preserve_format: the strides of a dense x)
    _lib.check(_lib.load().fmc_relu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "fmc_relu_fwd")
    return y


class _Relu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = _relu_raw(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        if dy.stride() != y.stride():
            dy = torch.empty_like(y).copy_(dy)
        dx = torch.empty_like(y)
        _lib.check(_lib.load().fmc_relu_bwd(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), y.numel(), _stream()), "fmc_relu_bwd")
        return dx


def relu(x: torch.Tensor) -> torch.Tensor:
    """ReLU of a bf16 device tensor (contiguous or channels-last: the output keeps the layout) with `dx = dy * (y > 0)`, on
    `fmc_relu_fwd / _bwd`."""
    _dev(x)
    assert x.dtype == torch.bfloat16, "relu: bf16 only"
    x = _dense(x)
    if x.numel() == 0:
        return x
    return _Relu.apply(x) if (torch.is_grad_enabled() and x.requires_grad) else _relu_raw(x)


def _add_raw(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(a)
    _lib.check(_lib.load().fmc_add_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "fmc_add_bf16")
    return out


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        return _add_raw(a, b)

    @staticmethod
    def backward(ctx, dy):
        return (dy if ctx.needs_input_grad[0] else None), (dy if ctx.needs_input_grad[1] else None)


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """`a + b` for two bf16 device tensors of one shape (the fp32 sum rounded once) on `fmc_add_bf16`; both gradients are dY."""
    _dev(a, b)
    assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.shape == b.shape, "add: two bf16 tensors of one shape"
    a = _dense(a)
    if b.stride() != a.stride():
        b = torch.empty_like(a).copy_(b)
    if a.numel() == 0:
        return a
    if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
        return _Add.apply(a, b)
    return _add_raw(a, b)


# --------------------------------------------------------------------------------------------
# trainable LoRA on frozen projections (FMC stage 1; stage 3 with `train_image_lora`)
# --------------------------------------------------------------------------------------------
import ctypes as _ct


class WgradProblem(_ct.Structure):
    """`fmc_wgrad_problem` of include/fmc_hip.h."""
    _fields_ = [("a", _ct.c_void_p), ("b", _ct.c_void_p), ("out", _ct.c_void_p), ("M", _ct.c_int64), ("lda", _ct.c_int64),
                ("ldb", _ct.c_int64), ("ldo", _ct.c_int64), ("N", _ct.c_int), ("K", _ct.c_int), ("alpha", _ct.c_float), ("accumulate", _ct.c_int)]


_wgrad_ws = {}


def linear_wgrad_group(problems):
    """One `fmc_linear_wgrad_bf16` launch for up to 8 problems `(a [M, N], b [M, K], alpha, out, accumulate)`:
    `out [N, K] (fp32) = alpha * a^T b (+ out)`.  a / b are bf16 device tensors, contiguous or 2-D row-strided views (column
    slices of a fused tensor); `out=None` allocates.  Returns the list of outputs.  fp32 operands (the parity mode) take an fp32
    matmul instead; CPU tensors raise."""
    outs, descs = [], []
    for a, b, alpha, out, acc in problems:
        _dev(a, b, out)
        (M, lda), (Mb, ldb) = _rows2d(a), _rows2d(b)
        N, Kd = a.shape[-1], b.shape[-1]
        assert M == Mb, "linear_wgrad: a and b must have the same rows"
        if out is None:
            out = torch.empty(N, Kd, dtype=torch.float32, device=a.device)
            acc = False
        assert out.dtype == torch.float32 and out.ndim == 2 and out.shape == (N, Kd) and out.stride(1) == 1
        outs.append(out)
        if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
            g = torch.matmul(a.reshape(M, N).t().float(), b.reshape(M, Kd).float())
            out.add_(g, alpha=alpha) if acc else torch.mul(g, alpha, out=out)
            continue
        descs.append(WgradProblem(a.data_ptr(), b.data_ptr(), out.data_ptr(), M, lda, ldb, out.stride(0), N, Kd, float(alpha), int(bool(acc))))
    if not descs:
        return outs
    lib = _lib.load()
    arr = (WgradProblem * len(descs))(*descs)
    need = lib.fmc_linear_wgrad_workspace_bytes(arr, len(descs))
    if need < 0:
        _lib.check(-1, "fmc_linear_wgrad_bf16")
    ws, ws_bytes = None, 0
    if need > 0:
        dev = outs[0].device
        key = (dev.index, torch.cuda.current_stream().cuda_stream)
        buf = _wgrad_ws.get(key)
        if buf is None or buf.numel() * 4 < need:
            if buf is not None:
                _ws_retired.append(buf)        # a captured HIP graph may have baked its address
            buf = torch.empty(need // 4 + 1024, dtype=torch.float32, device=dev)
            _wgrad_ws[key] = buf
        ws, ws_bytes = buf.data_ptr(), buf.numel() * 4
    _log_call("lora_wgrad", tuple((d.M, d.N, d.K) for d in descs), sum(2.0 * d.M * d.N * d.K for d in descs))
    _lib.check(lib.fmc_linear_wgrad_bf16(arr, len(descs), ws, ws_bytes, _stream()), "fmc_linear_wgrad_bf16")
    return outs


def linear_wgrad(a: torch.Tensor, b: torch.Tensor, alpha: float = 1.0, out: Optional[torch.Tensor] = None,
                 accumulate: bool = False) -> torch.Tensor:
    """`alpha * a^T b` (+ out), fp32 `[N, K]`, for token matrices a `[M, N]`, b `[M, K]` (see `linear_wgrad_group`)."""
    return linear_wgrad_group([(a, b, alpha, out, accumulate)])[0]


def _lora_gemm(x, weight, bias=None, residual=None, x2=None, out=None):
    """`[x | x2] @ weight^T + bias + residual` for the LoRA projections: the bf16 GEMM of this library (kernel-chosen tile; `out` may be a
    column slice of a fused output), fp32 storage (parity mode, host tests) in plain torch ops."""
    if x.dtype == torch.bfloat16 and x.is_cuda:
        return linear_bf16(x, weight, bias, residual, x2=x2, out=out)
    xin = x if x2 is None else torch.cat([x, x2], dim=-1)
    y = torch.nn.functional.linear(xin, weight, bias)
    if residual is not None:
        y = y + residual
    if out is None:
        return y
    out.copy_(y)
    return out


def lora_pad_rank(r: int, dtype) -> int:
    """Width of P = x D^T inside the fused GEMMs: the bf16 kernel's reduction comes in 64-wide k-tiles, so the rank is zero-padded to
    the next multiple of 64 (exact: padded columns of P and of U are zero).  fp32 storage keeps the rank."""
    return (r + 63) // 64 * 64 if dtype == torch.bfloat16 else r


def lora_group_weights(weights, downs, ups, scales, dtype, cache: Optional[dict] = None):
    """The derived weights of one group of LoRA projections that share an input (q | k | v of self attention, k | v of the text, or one
    projection): with r' = `lora_pad_rank(r)`,
        d_stack [G r', Cin]       = [D_1; ...; D_G] (each padded to r' rows)             -> P = x d_stack^T
        w_fwd_i [N_i, Cin + r']   = [W_i | s_i U_i]                                       -> y_i = [x | P_i] w_fwd_i^T
        u_t_i   [r', N_i]         = U_i^T                                                 -> Q_i = dY_i U_i
        w_bwd   [Cin, sum N + G r'] = [W_1^T ... W_G^T | s_1 D_1^T ... s_G D_G^T]        -> dX = [dY | Q] w_bwd^T
    in `dtype`, rebuilt only when a source changes (`_version`): once per optimizer step."""
    key = tuple((t.data_ptr(), t._version) for t in list(weights) + list(downs) + list(ups)) + tuple(float(s) for s in scales) + (dtype,)
    if cache is not None and cache.get("key") == key:
        return cache["w"]
    r = downs[0].shape[0]
    rp = lora_pad_rank(r, dtype)
    cin = weights[0].shape[1]
    dev = weights[0].device
    with torch.no_grad():
        d_stack = torch.zeros(len(downs) * rp, cin, dtype=dtype, device=dev)
        w_fwd, u_t, d_scaled = [], [], torch.zeros(len(downs) * rp, cin, dtype=torch.float32, device=dev)
        for i, (w, d, u, s) in enumerate(zip(weights, downs, ups, scales)):
            d_stack[i * rp: i * rp + r] = d
            d_scaled[i * rp: i * rp + r] = d.float() * s
            wf = torch.zeros(w.shape[0], cin + rp, dtype=dtype, device=dev)
            wf[:, :cin] = w
            wf[:, cin: cin + r] = u.float() * s
            w_fwd.append(wf)
            ut = torch.zeros(rp, w.shape[0], dtype=dtype, device=dev)
            ut[:r] = u.t()
            u_t.append(ut)
        w_bwd = torch.cat([torch.cat([w.to(dtype) for w in weights], dim=0), d_scaled.to(dtype)], dim=0).t().contiguous()
    out = dict(d_stack=d_stack, w_fwd=w_fwd, u_t=u_t, w_bwd=w_bwd, r=r, rp=rp)
    if cache is not None:
        cache["key"], cache["w"] = key, out
    return out


class _LoRALinear(torch.autograd.Function):
    """`y = [x W_i^T + s_i U_i D_i x]_i + b + residual` for a group of frozen projections W_i sharing the input x, with trainable LoRA
    factors D_i [r, Cin] / U_i [N_i, r] (fp32 masters).  The LoRA branch stays inside the fp32 accumulation of the projection GEMM:
        forward   P = x D_stack^T;  y_i = [x | P_i] [W_i | s_i U_i]^T  (+ bias, residual in the epilogue)
        backward  Q_i = dY_i U_i;   dX = [dY | Q] [W^T | s D^T]^T;   dU_i = s_i dY_i^T P_i;   dD_i = s_i Q_i^T X
    (a merged bf16 weight W + s U D would lose every update below half an ulp of W).  The two weight-gradient reductions of the group
    are ONE `fmc_linear_wgrad_bf16` launch."""

    @staticmethod
    def forward(ctx, x, bias, residual, spec, *factors):
        G = len(spec["weights"])
        downs, ups = factors[:G], factors[G:]
        w = lora_group_weights(spec["weights"], downs, ups, spec["scales"], x.dtype, spec.get("cache"))
        cin = x.shape[-1]
        x2d = x if (x.ndim == 2 and not x.is_contiguous()) else x.reshape(-1, cin)     # (a 2-D row-strided view is read in place)
        M = x2d.shape[0]
        rp = w["rp"]
        with torch.no_grad():
            P = _lora_gemm(x2d, w["d_stack"])                                          # [M, G r']
            ns = [wi.shape[0] for wi in spec["weights"]]
            res2d = None if residual is None else residual.reshape(M, sum(ns))
            if G == 1:
                y = _lora_gemm(x2d, w["w_fwd"][0], bias, res2d, x2=P)
            else:
                assert bias is None and residual is None
                y = torch.empty(M, sum(ns), dtype=x.dtype, device=x.device)
                off = 0
                for i in range(G):
                    _lora_gemm(x2d, w["w_fwd"][i], x2=P[:, i * rp:(i + 1) * rp], out=y[:, off: off + ns[i]])
                    off += ns[i]
        ctx.save_for_backward(x2d, P)
        ctx.spec, ctx.w, ctx.ns, ctx.x_shape = spec, w, ns, x.shape
        ctx.has_res = residual is not None and residual.requires_grad
        ctx.factor_dtypes = [f.dtype for f in factors]
        return y.view(*x.shape[:-1], sum(ns))

    @staticmethod
    def backward(ctx, dy):
        x2d, P = ctx.saved_tensors
        w, ns, spec = ctx.w, ctx.ns, ctx.spec
        G, r, rp = len(ns), w["r"], w["rp"]
        M = x2d.shape[0]
        dy2 = dy.reshape(M, sum(ns)) if dy.is_contiguous() else dy.contiguous().view(M, sum(ns))
        if dy2.dtype != x2d.dtype:
            dy2 = dy2.to(x2d.dtype)
        with torch.no_grad():
            Q = torch.empty(M, G * rp, dtype=x2d.dtype, device=x2d.device)
            off = 0
            for i in range(G):
                _lora_gemm(dy2[:, off: off + ns[i]], w["u_t"][i], out=Q[:, i * rp:(i + 1) * rp])
                off += ns[i]
            dx = None
            if ctx.needs_input_grad[0]:
                dx = _lora_gemm(dy2, w["w_bwd"], x2=Q).view(ctx.x_shape)
            scales = spec["scales"]
            probs, off = [], 0
            for i in range(G):                                                  # dU_i = s_i dY_i^T P_i
                probs.append((dy2[:, off: off + ns[i]], P[:, i * rp: i * rp + r], scales[i], None, False))
                off += ns[i]
            if all(s == scales[0] for s in scales):                             # dD = s Q^T X, one problem for the stacked factors
                probs.append((Q, x2d, scales[0], None, False))
            else:
                probs += [(Q[:, i * rp:(i + 1) * rp], x2d, scales[i], None, False) for i in range(G)]
            g = linear_wgrad_group(probs)
            dus = g[:G]
            if len(g) == G + 1:
                dds = [g[G][i * rp: i * rp + r] for i in range(G)]
            else:
                dds = [t[:r] for t in g[G:]]
        grads = [t.to(dt) for t, dt in zip(dds + dus, ctx.factor_dtypes)]
        return (dx, None, dy if ctx.has_res else None, None, *grads)


def lora_linear(x: torch.Tensor, weights, downs, ups, scales, bias: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None, cache: Optional[dict] = None) -> torch.Tensor:
    """The group of LoRA projections `[x W_i^T + s_i up_i(down_i(x))]_i` (concatenated along the last dim) + bias + residual, trainable
    in `downs` / `ups`, differentiable in x and the residual; `weights` are the frozen base weights (see `_LoRALinear`).  `cache`: a dict
    the caller keeps, for the derived bf16 weights of this group."""
    spec = dict(weights=list(weights), scales=[float(s) for s in scales], cache=cache)
    return _LoRALinear.apply(x, bias, residual, spec, *downs, *ups)


# --------------------------------------------------------------------------------------------
# The parameter update: clip per group + AdamW + bf16 shadows + gradient zeroing (csrc/optim.hip)
# --------------------------------------------------------------------------------------------
OPTIM_CHUNK = 8192                  # elements per workgroup; checked against fmc_optim_chunk_elems() when a device plan is built
OPTIM_ZERO_GRAD = 1
OPTIM_HYPER = 8                     # floats per record: lr, beta1, beta2, eps, weight_decay, max_grad_norm, 1 - beta1, 1 - beta2


class OptimTensor(_ct.Structure):
    """`fmc_optim_tensor` of include/fmc_hip.h."""
    _fields_ = [("p", _ct.c_void_p), ("g", _ct.c_void_p), ("m", _ct.c_void_p), ("v", _ct.c_void_p), ("shadow_bf16", _ct.c_void_p),
                ("shadow_f32", _ct.c_void_p), ("step", _ct.c_void_p), ("n", _ct.c_int64), ("clip_group", _ct.c_int32),
                ("hyper_group", _ct.c_int32), ("flags", _ct.c_int32), ("reserved", _ct.c_int32)]


def _round4(n: int) -> int:
    return (n + 3) // 4 * 4


def optim_check_tables(table, chunks, n_hyper: int, n_clip_groups: int) -> None:
    """`fmc_optim_check_tables` on HOST copies of the two tables (int64 `[n, 10]`, int32 `[n_chunks, 2]` CPU tensors): raises what the
    ABI reports -- a NULL or misaligned pointer, a group index out of range, a chunk map that does not cover its tensors."""
    assert table.dtype == torch.int64 and chunks.dtype == torch.int32 and not table.is_cuda and not chunks.is_cuda
    table, chunks = table.contiguous(), chunks.contiguous()
    rc = _lib.load().fmc_optim_check_tables(table.data_ptr(), table.shape[0], chunks.data_ptr(), chunks.shape[0], n_hyper, n_clip_groups)
    _lib.check(rc, "fmc_optim_check_tables")


class OptimPlan:
    """What one fused update works on: the torch tensors (so that they stay alive), the two device tables built from them, the
    hyper-parameter records and the workspace.  `entries`: dicts with `p, g, m, v, step` (fp32 tensors; `step` 0-d), `shadow_bf16`,
    `shadow_f32` (tensors or None), `clip_group` (-1: not clipped), `hyper_group`, `zero` (bool).  `hyper`: the fp32 `[n_hyper, 8]` records
    on the tensors' device, refreshed by the owner.  On a device the tables pass `fmc_optim_check_tables` before they are uploaded."""

    def __init__(self, entries, n_clip_groups: int, hyper: torch.Tensor):
        assert entries, "OptimPlan: no tensors"
        self.entries, self.n_clip_groups, self.hyper = list(entries), int(n_clip_groups), hyper
        dev = self.entries[0]["p"].device
        assert hyper.dtype == torch.float32 and hyper.ndim == 2 and hyper.shape[1] == OPTIM_HYPER and hyper.is_contiguous() and hyper.device == dev
        rows, cmap = [], []
        for i, e in enumerate(self.entries):
            for k in ("p", "g", "m", "v", "step"):
                t = e[k]
                if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
                    raise TypeError(f"OptimPlan: {k} of tensor {i} must be a contiguous fp32 tensor on {dev} (got {t.dtype}, {t.device})")
            n = e["p"].numel()
            if not (e["g"].numel() == e["m"].numel() == e["v"].numel() == n) or e["step"].numel() != 1:
                raise ValueError(f"OptimPlan: p, g, m, v of tensor {i} differ in size, or step is not one element")
            sb, sf = e.get("shadow_bf16"), e.get("shadow_f32")
            if sb is not None and (sb.dtype != torch.bfloat16 or sb.numel() != n or not sb.is_contiguous() or sb.device != dev):
                raise TypeError(f"OptimPlan: shadow_bf16 of tensor {i} must be a contiguous bf16 tensor of p's size")
            if sf is not None and (sf.dtype != torch.float32 or sf.numel() != n or not sf.is_contiguous() or sf.device != dev):
                raise TypeError(f"OptimPlan: shadow_f32 of tensor {i} must be a contiguous fp32 tensor of p's size")
            flags_groups = (int(e["clip_group"]) & 0xffffffff) | (int(e["hyper_group"]) << 32)
            rows.append([e["p"].data_ptr(), e["g"].data_ptr(), e["m"].data_ptr(), e["v"].data_ptr(), sb.data_ptr() if sb is not None else 0,
                         sf.data_ptr() if sf is not None else 0, e["step"].data_ptr(), n, flags_groups, OPTIM_ZERO_GRAD if e.get("zero") else 0])
            cmap += [(i, c) for c in range((n + OPTIM_CHUNK - 1) // OPTIM_CHUNK)]
        table = torch.tensor(rows, dtype=torch.int64)
        chunks = torch.tensor(cmap, dtype=torch.int32)
        assert table.shape[1] * 8 == _ct.sizeof(OptimTensor)
        self.n_tensors, self.n_chunks, self.n_hyper = len(rows), len(cmap), hyper.shape[0]
        G = self.n_clip_groups
        self.coef_off = _round4(G)
        self.bc_off = self.coef_off + _round4(G)
        self.partials_off = self.bc_off + _round4(2 * self.n_tensors)
        ws_floats = self.partials_off + _round4(self.n_chunks)
        if dev.type == "cuda":
            lib = _lib.load()
            assert lib.fmc_optim_chunk_elems() == OPTIM_CHUNK
            assert lib.fmc_optim_workspace_bytes(self.n_tensors, self.n_chunks, G) == ws_floats * 4
            optim_check_tables(table, chunks, self.n_hyper, G)
        self.table, self.chunks = table.to(dev), chunks.to(dev)
        self.workspace = torch.zeros(ws_floats, dtype=torch.float32, device=dev)
        self.norms = self.workspace[:G]                                       # per clip group, valid after optim_grad_norm
        self.coefs = self.workspace[self.coef_off: self.coef_off + G]
        self.bias_corrections = self.workspace[self.bc_off: self.bc_off + 2 * self.n_tensors].view(self.n_tensors, 2)
        self.elements = sum(e["p"].numel() for e in self.entries)

    def _args(self):
        return (self.table.data_ptr(), self.n_tensors, self.chunks.data_ptr(), self.n_chunks, self.hyper.data_ptr(), self.n_hyper,
                self.n_clip_groups, self.workspace.data_ptr(), self.workspace.numel() * 4, _stream())


def optim_grad_norm(plan: OptimPlan) -> torch.Tensor:
    """Pass 1 of the fused update (`fmc_optim_grad_norm`): per clip group the gradient norm and the clip coefficient into the plan's
    workspace, every tensor's step counter advanced and its bias corrections written.  Returns `plan.norms` (a device tensor; nothing
    synchronises).  CPU tensors raise."""
    _dev(plan.table, plan.hyper, plan.workspace)
    _lib.check(_lib.load().fmc_optim_grad_norm(*plan._args()), "fmc_optim_grad_norm")
    return plan.norms


def optim_adamw_step(plan: OptimPlan) -> None:
    """Pass 2 (`fmc_optim_adamw_step`), after `optim_grad_norm` on the same plan: AdamW on the clipped gradients, the bf16 shadows, the
    zeroing -- one launch for every tensor.  The kernel writes through raw pointers: bumping the tensors' version counters is the
    caller's job (`training.FusedAdamW` does it).  CPU tensors raise."""
    _dev(plan.table, plan.hyper, plan.workspace)
    _lib.check(_lib.load().fmc_optim_adamw_step(*plan._args()), "fmc_optim_adamw_step")

"""Reference, bound and inputs of the spatial-attention backward tests (pure torch, runs on the CPU).

With `P = softmax(scale Q K^T)`, `O = P V`, `D = rowsum(dO * O)` and `dP = dO V^T`, per (batch entry, head):

    dV = P^T dO                      mag_dV = P^T |dO|
    dS = P * (dP - D)                A      = P * (|dP| + rowsum(|dO| * |O|))
    dQ = scale dS K                  mag_dQ = scale A |K|
    dK = scale dS^T Q                mag_dK = scale A^T |Q|

`mag` is the sum of the absolute terms behind every output element.  Frames that share one text (`B // Bkv > 1`) add their
dK, dV and magnitudes.  Everything is float64 on the rounded inputs cast up.  Used by test_attn_bwd_reference_host.py (CPU),
test_gpu_attn_backward.py and its worker attn_bwd_child.py.
"""
import torch

C_BF16 = 2.0 ** -7
C_F32 = 1e-4
BOUND = {torch.bfloat16: C_BF16, torch.float32: C_F32}

# name -> (B, Bkv, H, Sq, Skv, D).  Self attention reads one fused [B, S, 3C] projection, cross attention a dense q [B, Sq, C] and a
# fused kv [Bkv, Skv, 2C]; batch entry b reads K / V entry b // (B // Bkv).
SELF_CASES = {
    "self_b8_s129_d40": (8, 8, 2, 129, 129, 40),       # both kernels in the remapped block order; one row over every 128-row block
    "self_b16_s257_d80": (16, 16, 1, 257, 257, 80),    # the second group of eight batch entries; three blocks
    "self_b8_s65_d160": (8, 8, 2, 65, 65, 160),        # ten k-steps, two waves, 64 keys per workgroup, one row over
    "self_b8_s33_d64": (8, 8, 1, 33, 33, 64),          # head width 64; one over the fp32 kernels' 32-row blocks
    "self_b3_s96_d8": (3, 3, 2, 96, 96, 8),            # the plain block order; the smallest head width
}
CROSS_CASES = {
    "cross_c8_f2": (16, 8, 2, 70, 77, 40),             # dK/dV kernel remapped, two frames summed inside the workgroup
    "cross_c1_f8": (8, 1, 2, 70, 77, 40),              # one text for eight frames: per-frame partial dK | dV, summed afterwards
    "cross_c16_f1_skv1": (16, 16, 2, 70, 1, 40),       # one key: dQ and dK are exactly zero
}
CASES = {**SELF_CASES, **CROSS_CASES}
CHILD_CASES = ("self_b8_s129_d40", "self_b16_s257_d80", "cross_c8_f2")     # what the block-order worker runs


def _seed(name):
    return 4000 + 10 * sorted(CASES).index(name)


def rnd_cpu(shape, seed, dtype, scale=1.0):
    """Seeded values rounded to `dtype`, as fp32 on the CPU (exact: the device tensor is `.to(dtype)` of it)."""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale
    return x.to(dtype).float()


def make_inputs(name, dtype, logit_scale=1.0):
    """`(q, k, v, dO)` of a case as fp32 CPU tensors holding values of `dtype`: k and v are the column blocks of one fused
    tensor, and so is q for self attention.  `logit_scale` multiplies q (sharper softmax)."""
    B, Bkv, H, Sq, Skv, D = CASES[name]
    C, s = H * D, _seed(name)
    if name in SELF_CASES:
        qkv = rnd_cpu((B, Sq, 3 * C), s, dtype)
        if logit_scale != 1.0:
            qkv[..., :C] = (qkv[..., :C] * logit_scale).to(dtype).float()
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    else:
        q = rnd_cpu((B, Sq, C), s, dtype, logit_scale)
        kv = rnd_cpu((Bkv, Skv, 2 * C), s + 1, dtype)
        k, v = kv[..., :C], kv[..., C:]
    return q, k, v, rnd_cpu((B, Sq, C), s + 2, dtype)


def run_fused(K, name, dtype, kv_grad=True):
    """A case through the fused entry points of `hip_ops` (`K`) on the device: `self_attention_qkv` on the `[B, S, 3C]` projection,
    `cross_attention_q_kv` on q and the `[Bkv, Skv, 2C]` projection.  Returns dq, dk, dv as views of the fused gradients
    (dk = dv = None for a frozen kv)."""
    B, Bkv, H, Sq, Skv, D = CASES[name]
    C = H * D
    q, k, v, g = (t.to(dtype).cuda() for t in make_inputs(name, dtype))
    if name in SELF_CASES:
        qkv = torch.cat([q, k, v], -1).requires_grad_(True)
        K.self_attention_qkv(qkv, H, D ** -0.5, False).backward(g)
        return dict(dq=qkv.grad[..., :C], dk=qkv.grad[..., C:2 * C], dv=qkv.grad[..., 2 * C:])
    q.requires_grad_(True)
    kv = torch.cat([k, v], -1).requires_grad_(kv_grad)
    K.cross_attention_q_kv(q, kv, H, D ** -0.5).backward(g)
    if not kv_grad:
        assert kv.grad is None
        return dict(dq=q.grad, dk=None, dv=None)
    return dict(dq=q.grad, dk=kv.grad[..., :C], dv=kv.grad[..., C:])


def _heads(t, H, rep=1):
    B, S, C = t.shape
    t = t.double().reshape(B, S, H, C // H).permute(0, 2, 1, 3)
    return t.repeat_interleave(rep, dim=0) if rep > 1 else t


def _merge(t):
    B, H, S, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, S, H * D)


def _fold(t, Bkv):
    """[B, S, C] -> [Bkv, S, C]: sum over the frames that share a K / V entry."""
    return t.reshape(Bkv, t.shape[0] // Bkv, *t.shape[1:]).sum(1)


def terms(q, k, v, d_o, heads, scale):
    """The float64 pieces of the closed form, per head: dict of q, k, v, g (= dO) `[B, H, S, D]` and P, O, dP, D, dS, A."""
    rep = q.shape[0] // k.shape[0]
    qh, gh = _heads(q, heads), _heads(d_o, heads)
    kh, vh = _heads(k, heads, rep), _heads(v, heads, rep)
    P = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    O = P @ vh
    dP = gh @ vh.transpose(-1, -2)
    Dv = (gh * O).sum(-1, keepdim=True)
    dS = P * (dP - Dv)
    A = P * (dP.abs() + (gh.abs() * O.abs()).sum(-1, keepdim=True))
    return dict(q=qh, k=kh, v=vh, g=gh, P=P, O=O, dP=dP, D=Dv, dS=dS, A=A)


def reference_backward(q, k, v, d_o, heads, scale):
    """Closed-form gradients and magnitudes in float64: dict of dq, dk, dv, mag_dq, mag_dk, mag_dv (`[B, Sq, C]` / `[Bkv, Skv, C]`)."""
    Bkv = k.shape[0]
    t = terms(q, k, v, d_o, heads, scale)
    PT, dST, AT = t["P"].transpose(-1, -2), t["dS"].transpose(-1, -2), t["A"].transpose(-1, -2)
    return dict(dq=_merge(scale * t["dS"] @ t["k"]), mag_dq=_merge(scale * t["A"] @ t["k"].abs()),
                dk=_fold(_merge(scale * dST @ t["q"]), Bkv), mag_dk=_fold(_merge(scale * AT @ t["q"].abs()), Bkv),
                dv=_fold(_merge(PT @ t["g"]), Bkv), mag_dv=_fold(_merge(PT @ t["g"].abs()), Bkv))


def _bf(t):
    return t.to(torch.bfloat16).double()


def emulate_bf16_backward(q, k, v, d_o, heads, scale, per_frame_partials=False):
    """The bf16 kernels' rounding chain in plain torch, everything else exact (float64): the forward saves `O = bf16(bf16(P) V)`,
    the backward rounds P (dV), dS (dQ, dK) and its outputs.  `per_frame_partials`: dK | dV of every frame rounded to bf16, then
    summed and rounded again -- the one-text path of `cross_attention_q_kv`.  Returns dq, dk, dv."""
    Bkv = k.shape[0]
    t = terms(q, k, v, d_o, heads, scale)
    Pb = _bf(t["P"])
    O = _bf(Pb @ t["v"])
    dS = _bf(scale * t["P"] * (t["dP"] - (t["g"] * O).sum(-1, keepdim=True)))
    dq = _bf(_merge(dS @ t["k"]))
    dk, dv = _merge(dS.transpose(-1, -2) @ t["q"]), _merge(Pb.transpose(-1, -2) @ t["g"])
    if per_frame_partials:
        dk, dv = _bf(dk), _bf(dv)
    return dict(dq=dq, dk=_bf(_fold(dk, Bkv)), dv=_bf(_fold(dv, Bkv)))


def grad_ratio(got, ref, mag):
    """Worst `|got - ref| / mag` over the elements (0 where `mag` and the error are both zero)."""
    got, ref, mag = got.detach().double().cpu(), ref.detach().double().cpu(), mag.detach().double().cpu()
    err = (got - ref).abs()
    return float(torch.where(mag > 0, err / mag.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0)).max())


def assert_grad_close(got, ref, mag, c, what=""):
    """Element-wise bound of a gradient of the attention backward: `|got - ref| <= c mag + 1e-5 mag` for every element, `ref` the
    float64 closed form on the same rounded inputs and `mag` the sum of |terms| behind the element (`reference_backward`).  The
    form of `assert_bf16_close`, but relative to `mag` throughout: the bound still means something where `ref` is exactly zero
    (one key: dQ = dK = 0).  Returns the worst `err / mag` in units of `c`.

    `c = 2^-7` in bf16: a rounding is at most 2^-9 relative to the terms behind it, and the kernels of
    csrc/spatial_attn_bwd.hip (with the forward kernel that saves O and the log-sum-exp) round, counted in the source:

        dV   2   P (`p_frag(p8, pf)`), the output (`store4`)
        dQ   4   the saved O inside D -- itself two: the forward's bf16 P and the stored O --, dS (`p_frag(d8, df)`), the output;
                 P itself stays fp32 in front of dS
        dK   4   the same chain in the dK/dV kernel
        one text for all frames (`Bkv == 1`, several frames): one more each (dV 3, dK 5) -- the per-frame partial is stored
        as bf16 before the fp32 sum over the frames is rounded again

    `c = 1e-4` in fp32 storage (split-bf16 x3 products, about 2^-16 each)."""
    got, ref, mag = got.detach().double().cpu(), ref.detach().double().cpu(), mag.detach().double().cpu()
    assert got.shape == ref.shape == mag.shape, f"{what}: shapes {tuple(got.shape)} / {tuple(ref.shape)} / {tuple(mag.shape)}"
    err = (got - ref).abs()
    bound = c * mag + 1e-5 * mag
    bad = ~(err <= bound)                                 # (a NaN is bad)
    if bool(bad.any()):
        over = torch.where(bad, (err - bound).nan_to_num(nan=float("inf")), torch.full_like(err, -1.0))
        worst = tuple(int(i) for i in torch.unravel_index(over.argmax(), over.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} elements beyond {c:.3e} * |terms|, worst at {worst}: "
                             f"got {float(got[worst]):.6e} ref {float(ref[worst]):.6e} |terms| {float(mag[worst]):.6e}")
    return grad_ratio(got, ref, mag) / c

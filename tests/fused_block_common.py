"""Exact integer runs for the fused transformer blocks (profiles/fused_block_bounds.md has the derivations and the source lines they rest on).

The fused temporal attention block (csrc/temporal_block.hip, temporal_block640.hip), the text cross-attention blocks on the same skeleton and the
LayerNorm + GEGLU kernels chain LayerNorm, projections, a softmax or a GELU, and bf16 roundings.  On the inputs built here every one of those
steps has an exactly representable result, so a kernel must return the float64 expectation bit for bit whatever its accumulation order:

  LayerNorm   a row of `c0 +- a` (half the entries `+a`) normalises to +-1 within 1e-5; with integer gamma and integer beta + pe the value before
              the bf16 rounding lies within 1e-5 |gamma| of an integer below 256, and the rounding returns that integer -- if it is not 0 (where
              gamma is not 0, `+-gamma + beta` never cancels: `_offsets`);
  softmax     `scale` is chosen so that `scale * log2(e)` is exactly 1 in fp32: a logit in log2 units is the integer q . k.  The keys a query
              selects score at least 160 above every other one: exp2 gives exactly 0 for the others, the sum is 1, 2 or 4, p is 1, 0.5 or 0.25;
  GELU        gates are 0 or an integer in [10, 16]: `fmc_gelu_fast` returns 0 and g;
  the rest    sparse integer weights, integer pose term, bias and residual, merge_scale 0.5 on even products: every rounded tensor is
              representable in bf16 and every fp32 accumulator stays below 2^24.

`assert_exact_conditions` asserts all of it on the reference.  `chain(.., Exact)` is the float64 expectation, `chain(.., Emulated)` the fp32
restatement of the documented chain (two-pass LayerNorm as the source computes it, exp2 softmax on scale_log2, bf16 rounding points,
fmc_gelu_fast); `chain(.., Exact, fault=..)` the wrong stand-ins of tests/test_fused_block_reference_host.py."""
import functools
import os
import re
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from tests.attn_fwd_common import exact_scale, scale_log2

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
HEADS, FRAMES = 8, 16
GAP = 160                       # fp32's smallest denormal is 2^-149: exp2f(x - max) == 0 for x - max <= -160 on any implementation
PERIOD = 37                     # pixels (rows of an image) after which the generators repeat: odd, no multiple of a tile, so tiles differ
SCALE = exact_scale(0)          # float32(SCALE) * float32(log2 e) == 1
LN_EPS = 1e-5

# ---- row statistics (csrc/temporal_block.hip:700-723), counted from the source; unit 2^-24 = half an fp32 ulp -----------------------------------
# mean: a lane adds 80 values as 40 x (`a + b`, then `s1 +=`) = 80 roundings, two shuffle additions, the rounded constant 1.f / 320.f and the
# product = 84, each at most 2^-24 of the sum of |values| of the row:  |mean - mean64| <= 84 * 2^-24 * mean|x|.
STATS_MEAN_CHAIN = 84
STATS_MEAN_REL = STATS_MEAN_CHAIN * 2.0 ** -24            # 5.0e-6, of the row's mean |x|
# rstd: relative error of var + eps (all addends positive): `x - mean` 1, squared 2 + 1, `a * a + b * b` 1, the 40 `s2 +=` of a lane 40, two
# shuffle additions 2, constant and product 2, `+ eps` 1, the fp32 eps against the float64 one 1 = 50; halved by the inverse square root = 25; rsqrtf
# within 2 ulp = 4.  29, taken as 32.  The kernel centres on ITS mean: var grows by (mean - mean64)^2, added per row from the bound above.
STATS_RSTD_CHAIN = 32
STATS_RSTD_REL = STATS_RSTD_CHAIN * 2.0 ** -24            # 1.9e-6, of rstd


def bf16r(t):
    return t.to(F32).to(BF16).to(t.dtype)


def is_bf16(t):
    return bool((t.to(F32).to(BF16).to(F64) == t.to(F64)).all())


# =====================================================================================================================================================
# the two arithmetics
# =====================================================================================================================================================
def _gelu_constants():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "synfmc_amd", "csrc", "common.h")).read()
    body = src[src.index("float fmc_gelu_fast(float g)"):]
    body = body[:body.index("}")]
    clamp = float(re.search(r"fminf\(g \* g, ([0-9.eE+-]+)f\)", body).group(1))
    c2, c1, c0 = (float(x) for x in re.search(r"fmaf\(fmaf\(([0-9.eE+-]+)f, g2, ([0-9.eE+-]+)f\), g2, ([0-9.eE+-]+)f\)", body).groups())
    return clamp, c0, c1, c2


def gelu_fast_f32(g):
    """`fmc_gelu_fast` (common.h:89) in float32, as tests/test_gelu_fast.py restates it."""
    clamp, c0, c1, c2 = (np.float32(v) for v in _gelu_constants())
    g = g.numpy().astype(np.float32)
    g2 = np.minimum(g * g, clamp)
    s = (c2 * g2 + c1) * g2 + c0
    return torch.from_numpy(g * (np.float32(1) / (np.float32(1) + np.exp2(g * s))))


class Exact:
    """float64; the only roundings are the two the instrument relies on: the LayerNorm output (asserted away from every tie) and p."""
    dtype = F64

    @staticmethod
    def ln(h, gamma, bpe, C, fault=None):
        mean = h.mean(-1, keepdim=True)
        var = ((h - mean) ** 2).mean(-1, keepdim=True)
        core = h if fault == "ln_no_mean" else h - mean
        return core * (var + LN_EPS).rsqrt() * gamma + bpe            # (before the rounding: `ln_tie_distance` looks at this)

    r = staticmethod(lambda t: t)
    round_x = staticmethod(bf16r)

    @staticmethod
    def softmax(logits):
        e = torch.exp2((logits - logits.amax(-1, keepdim=True)) * scale_log2(SCALE))
        return bf16r(e / e.sum(-1, keepdim=True))

    gelu = staticmethod(F.gelu)


class Emulated:
    """float32 with the kernels' documented operation order and bf16 rounding points."""
    dtype = F32

    @staticmethod
    def ln(h, gamma, bpe, C, fault=None):
        inv_c = torch.tensor(1.0, dtype=F32) / torch.tensor(float(C), dtype=F32)          # the rounded 1.f / C
        mean = h.sum(-1, keepdim=True) * inv_c
        dl = h - mean
        rstd = torch.rsqrt((dl * dl).sum(-1, keepdim=True) * inv_c + torch.tensor(LN_EPS, dtype=F32))
        return (h - mean) * rstd * gamma + bpe

    r = staticmethod(bf16r)
    round_x = staticmethod(bf16r)

    @staticmethod
    def softmax(logits):
        sl = logits * float(np.float32(SCALE) * np.float32(1.4426950408889634))          # scale_log2 as every entry point forms it
        e = torch.exp2(sl - sl.amax(-1, keepdim=True))
        return bf16r(e * (1.0 / e.sum(-1, keepdim=True)))

    gelu = staticmethod(gelu_fast_f32)


# =====================================================================================================================================================
# generators
# =====================================================================================================================================================
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _nonzero(g, mag, shape):
    """Integers in [-mag, mag] without 0."""
    return _randint(g, 1, mag, shape) * (2 * _randint(g, 0, 1, shape) - 1)


def _offsets(g, shape):
    """beta (+ pe) of a data channel: 0 or +-3.  With |gamma| in {1, 2} the sum +-gamma + offset is never 0: an exact cancellation would leave the
    LayerNorm's 1e-5 residue, which bf16 (whose spacing shrinks towards 0) keeps instead of rounding it to the integer 0."""
    return 3.0 * _randint(g, -1, 1, shape)


def balanced_rows(fixed, g):
    """`h` rows `c0 +- a` with exactly half the entries `+a`: `fixed` [.., C] holds +1 / -1 where the sign is prescribed and 0 where it is free.
    Returns (h, sign); c0 in +-{1, 2, 3} and a in {1, 2, 4} vary per row."""
    C = fixed.shape[-1]
    score = torch.rand(fixed.shape, generator=g, dtype=F64)
    score = torch.where(fixed > 0, torch.full_like(score, -1.0), torch.where(fixed < 0, torch.full_like(score, 2.0), score))
    rank = score.argsort(-1).argsort(-1)
    sign = torch.where(rank < C // 2, 1.0, -1.0).to(F64)
    assert bool((sign.sum(-1) == 0).all()) and bool(((fixed == 0) | (fixed == sign)).all())
    c0 = _nonzero(g, 3, fixed.shape[:-1] + (1,))
    a = 2.0 ** _randint(g, 0, 2, fixed.shape[:-1] + (1,))
    return c0 + a * sign, sign


def _sparse_rows(g, n_out, cols, entries, mags, C):
    """[n_out, C] with `entries` nonzeros per row at distinct columns out of `cols`, magnitudes from `mags` with random sign."""
    w = torch.zeros(n_out, C, dtype=F64)
    pick = torch.rand(n_out, len(cols), generator=g).argsort(-1)[:, :entries]
    m = torch.tensor(mags, dtype=F64)[torch.randint(0, len(mags), (n_out, entries), generator=g)]
    w.scatter_(1, cols[pick], m * (2 * _randint(g, 0, 1, (n_out, entries)) - 1))
    return w


def _code_positions(g, d, n):
    """`n` distinct channels of a head for the codes; codes 0, 2, 5 and 9 among the last fifth of the channels -- at d = 40 the tail channels 32..39
    with their own 16x16x16 MFMA (with 4-way ties only codes 0 .. 3 are in use: two of them sit in the tail)."""
    tail = torch.arange(d - d // 5, d)
    body = torch.arange(0, d - d // 5)
    pos = body[torch.randperm(len(body), generator=g)[:n]].clone()
    pos[torch.tensor([0, 2, 5, 9])] = tail[torch.randperm(len(tail), generator=g)[:4]]
    return pos


TemporalCase = namedtuple("TemporalCase", "C B hw merge stats partial ties persistent")
TextCase = namedtuple("TextCase", "C B ipt hw S stats partial ties")
GegluCase = namedtuple("GegluCase", "kernel C M cff bias variant partial")


def base_hw(hw):
    return min(hw, PERIOD)


def expand_pixels(t, hw, axis):
    """A tensor generated for `base_hw(hw)` pixels -> `hw` pixels (pixel p holds what pixel p % PERIOD held).  Every fused block is local to a pixel
    (temporal) or to a row (text), so the expectation of the expanded input is the expanded expectation."""
    if t is None or hw <= PERIOD:
        return t
    return t.index_select(axis, torch.arange(hw) % PERIOD)


@functools.lru_cache(maxsize=None)
def temporal_inputs(c):
    """The temporal block on `base_hw(c.hw)` pixels.  Channel roles of x (a random subset of the C channels each):
      key code   16 channels, gamma 0, beta + pe = 8 where channel j == frame // ties: W_k routes channel j to `pos_w[j]` of head w, k = 16 one-hot;
      query code 16 channels, gamma 2, beta + pe 3, h = +a at the row's target and -a elsewhere: x = 5 at the target and 1 elsewhere (never 0: see
                 `_offsets`); W_q routes channel i to `pos_w[sigma_w(i)]` with weight 4: head w's q is 20 at code sigma_w(target) and 4 at the other
                 codes, scoring 320 on the `ties` frames of that code and 64 on the others;
      data       the rest: gamma in +-{1, 2}, beta + pe in {0, +-3} per frame, free signs: x = +-gamma + bpe, dense, different in every row; v, the
                 merge and the pose term live here."""
    C, B, P, T = c.C, c.B, base_hw(c.hw), c.ties
    d, ncode = C // HEADS, FRAMES // T
    g = _gen("temporal", C, B, P, c.merge, T)
    perm = torch.randperm(C, generator=g)
    kc, qc, data = perm[:16], perm[16:32], perm[32:]
    gamma = torch.zeros(C, dtype=F64)
    gamma[qc] = 2.0
    gamma[data] = _nonzero(g, 2, (len(data),))
    bpe = torch.zeros(FRAMES, C, dtype=F64)
    bpe[:, data] = _offsets(g, (FRAMES, len(data)))
    bpe[:, qc] = 3.0
    for f in range(FRAMES):
        bpe[f, kc[f // T]] = 8.0
    target = torch.randint(0, ncode, (B, FRAMES, P), generator=g)
    fixed = torch.zeros(B, FRAMES, P, C, dtype=F64)
    fixed[..., qc] = -1.0
    fixed.scatter_(-1, qc[target][..., None], 1.0)
    h, _ = balanced_rows(fixed, g)
    wq, wk = torch.zeros(C, C, dtype=F64), torch.zeros(C, C, dtype=F64)
    for w in range(HEADS):
        pos = _code_positions(g, d, 16)
        mult = 2 * (w % 4) + 1
        for i in range(ncode):
            wq[w * d + pos[(i * mult + w) % ncode], qc[i]] = 4.0
            wk[w * d + pos[i], kc[i]] = 2.0
    wv = _sparse_rows(g, C, data, 2, [1.0], C)
    d_ = dict(case=c, h=h, gamma=gamma, bpe=bpe, w_qkv=torch.cat([wq, wk, wv]), w_out=_sparse_rows(g, C, torch.arange(C), 2, [1.0], C),
              b_out=_nonzero(g, 2, (C,)), w_merge=None, pose=None, merge_scale=0.5)
    if c.merge:
        wm = _sparse_rows(g, C, data, 2, [2.0], C)
        wm[kc] = 0.0
        wm[qc] = 0.0
        pose = torch.zeros(B, FRAMES, P, C, dtype=F64)
        pose[..., data] = _randint(g, -2, 2, (B, FRAMES, P, len(data)))
        d_.update(w_merge=wm, pose=pose)
    return d_


@functools.lru_cache(maxsize=None)
def text_inputs(c):
    """The text cross-attention block on `base_hw(c.hw)` rows per image.  Head w sees its d channels through a permutation rho_w that keeps the last
    fifth (d = 40: the tail channels 32..39) in place as a set; logical channels 0 .. d - 2 carry 2-hot codes (16 each; code c = the pair (tail channel
    c % 8, body channel c // 2 mod the body's size): codes 2 j and 2 j + 1 differ in the tail channel alone; code of key g = g // ties, rotated by 3 w keys per head),
    logical channel d - 1 is the masking channel z: k[z] = 16 on every real key.  x has d - 1 query-code channels (gamma 2, beta 3: x = 5 on the row's pair, 1 elsewhere; W_q
    weight 4 -> q = 20 on the pair, 4 elsewhere: the target scores 640, a key sharing one channel 384, the others 128) and one mask channel (gamma 2,
    beta -1: x = -3 on every fifth row and 1 on the others, W_q weight 32 -> q[z] = -96 | 32: the logits of a masked row are <= 640 - 1536, and a padded
    key's zero row would take the softmax; on the other rows z adds 512 to every real logit alike).  v is dense."""
    C, B, ipt, P, S, T = c.C, c.B, c.ipt, base_hw(c.hw), c.S, c.ties
    d, N, ncode = C // HEADS, c.B * c.ipt, -(-c.S // c.ties)
    g = _gen("text", C, B, ipt, P, S, T)
    perm = torch.randperm(C, generator=g)
    qc, zc, data = perm[:d - 1], perm[d - 1], perm[d:]
    nt = d // 5                                                                          # logical 0 .. nt - 1: tail, nt .. d - 2: body, d - 1: z
    pairs = torch.tensor([[code % 8, nt + (code // 2) % (d - 1 - nt)] for code in range(80)])      # code -> its two logical channels, all distinct
    gamma = torch.zeros(C, dtype=F64)
    gamma[qc], gamma[zc] = 2.0, 2.0
    gamma[data] = _nonzero(g, 2, (len(data),))
    beta = torch.zeros(C, dtype=F64)
    beta[qc], beta[zc] = 3.0, -1.0
    beta[data] = _offsets(g, (len(data),))
    rows = torch.arange(N * P).view(N, P)
    target = (rows * 7 + rows // P) % ncode                                              # every code, the last key's among them, is some row's target
    masked = rows % 5 == 3
    fixed = torch.zeros(N, P, C, dtype=F64)
    fixed[..., qc] = -1.0
    fixed.scatter_(-1, qc[pairs[target]], 1.0)
    fixed[..., zc] = torch.where(masked, -1.0, 1.0).to(F64)
    h, _ = balanced_rows(fixed, g)
    wq = torch.zeros(C, C, dtype=F64)
    k = torch.zeros(B, S, HEADS, d, dtype=F64)
    for w in range(HEADS):
        rho = torch.cat([d - nt + torch.randperm(nt, generator=g), torch.randperm(d - nt, generator=g)])
        wq[w * d + rho[:d - 1], qc] = 4.0
        wq[w * d + rho[d - 1], zc] = 32.0
        for key in range(S):
            code = ((key - 3 * w) % S) // T if T == 1 else key // T                     # (tied keys share a code: no rotation, the groups stay whole)
            k[:, key, w, rho[pairs[code]]] = 16.0
        k[:, :, w, rho[d - 1]] = 16.0
    v = _randint(g, -4, 4, (B, S, C))
    return dict(case=c, h=h, gamma=gamma, beta=beta, w_q=wq, kv=torch.cat([k.reshape(B, S, C), v], -1), w_out=_sparse_rows(g, C, torch.arange(C), 3, [1.0], C),
                b_out=_nonzero(g, 2, (C,)), masked=masked)


@functools.lru_cache(maxsize=None)
def geglu_inputs(c):
    """LayerNorm + GEGLU.  n has one constant channel (gamma 0, beta 1: n = 1), three bit channels (gamma 1, beta 2: n in {1, 3}) and data channels
    (gamma in +-{1, 2}, beta in {0, +-3}).  A quarter of the gate columns are 0 for every row; the others are 10 + sum (n_i - 1) over a subset of the
    bits (the constant channel carries 10 - the size of the subset), so 10, 12, 14 or 16, different from row to row.  With a bias, part of the constant
    moves into it (-3 + 3 on the zero columns).  Values are two data channels with weights +-1 plus the bias."""
    C, M, cff = c.C, c.M, c.cff
    g = _gen("geglu", C, M, cff, c.bias)
    perm = torch.randperm(C, generator=g)
    one, bits, data = perm[0], perm[1:4], perm[4:]
    gamma, beta = torch.zeros(C, dtype=F64), torch.zeros(C, dtype=F64)
    gamma[bits], beta[bits], beta[one] = 1.0, 2.0, 1.0
    gamma[data], beta[data] = _nonzero(g, 2, (len(data),)), _offsets(g, (len(data),))
    h, _ = balanced_rows(torch.zeros(M, C, dtype=F64), g)
    wv = _sparse_rows(g, cff, data, 2, [1.0], C)
    wg = torch.zeros(cff, C, dtype=F64)
    zero = torch.arange(cff) % 4 == 1
    wg[:, bits] = _randint(g, 0, 1, (cff, 3))
    wg[zero] = 0.0
    bias = None
    if c.bias:
        bias = torch.cat([_nonzero(g, 2, (cff,)), torch.where(zero, -3.0, 4.0).to(F64)])
        wg[:, one] = torch.where(zero, 3.0, 6.0 - wg[:, bits].sum(-1))
    else:
        wg[:, one] = torch.where(zero, 0.0, 10.0 - wg[:, bits].sum(-1))
    return dict(case=c, h=h, gamma=gamma, beta=beta, w=torch.cat([wv, wg]), bias=bias)


def inputs(c):
    return {TemporalCase: temporal_inputs, TextCase: text_inputs, GegluCase: geglu_inputs}[type(c)](c)


# =====================================================================================================================================================
# the chains (float64 expectation, fp32 emulation, wrong stand-ins)
# =====================================================================================================================================================
FAULTS = {
    "pe_next_frame": "pe row of frame f + 1",
    "next_head_k": "head w using head w + 1's k",
    "drop_tail": "head-tail channels 32..39 left out of the scores",
    "unmask_pad": "padded text keys unmasked, with zero rows",
    "mask_last_key": "key n_keys - 1 masked as well",
    "no_merge_scale": "merge_scale dropped",
    "pose_next_pixel": "pose term of the neighbouring pixel",
    "no_bias": "bias omitted",
    "no_residual": "residual omitted",
    "v_next_pixel": "a pixel's v taken from the next pixel of the tile",
    "next_batch_text": "text of the neighbouring batch entry for the image at a segment boundary",
    "stats_unrounded": "statistics of the un-rounded output",
    "swap_value_gate": "value and gate columns swapped within a 40-column group",
    "ln_no_mean": "LayerNorm without the mean subtraction",
}


def applies(fault, c):
    """The cases in which a stand-in computes something else than the block (profiles/fused_block_bounds.md says why the others are left out)."""
    if isinstance(c, TemporalCase):
        return {"pe_next_frame": True, "next_head_k": True, "drop_tail": c.C == 320, "no_merge_scale": c.merge, "pose_next_pixel": c.merge and c.hw > 1,
                "no_bias": True, "no_residual": True, "v_next_pixel": c.hw > 1, "ln_no_mean": True}.get(fault, False)
    if isinstance(c, TextCase):
        # (one key: p = 1 whatever k holds; fewer than two codes: no pair of keys that the tail channel alone tells apart)
        return {"next_head_k": c.S > 1, "drop_tail": c.C == 320 and c.S >= 2 * c.ties, "unmask_pad": c.S % 16 != 0, "mask_last_key": True, "no_bias": True, "no_residual": True,
                "next_batch_text": c.B > 1}.get(fault, False)
    return {"no_bias": c.bias, "swap_value_gate": True, "ln_no_mean": True}.get(fault, False)


def _heads(t, d):
    return t.reshape(*t.shape[:-1], HEADS, d)


def _attend(A, q, k, v, fault, d, trace):
    """q [.., Q, H, d], k / v [.., K, H, d] -> o [.., Q, H d]; logits in log2 units are q . k (scale_log2 == 1)."""
    if fault == "next_head_k":
        k = k.roll(-1, -2)
    qs = q
    if fault == "drop_tail":
        qs = q.clone()
        qs[..., 32:40] = 0
    logits = torch.einsum("...qhd,...khd->...hqk", qs, k)
    if trace is not None:
        trace["logits"] = logits
        trace["logit_terms"] = torch.einsum("...qhd,...khd->...hqk", q.abs(), k.abs())
    p = A.softmax(logits)
    o = A.r(torch.einsum("...hqk,...khd->...qhd", p, v))
    if trace is not None:
        trace.update(p=p, o=o, o_terms=torch.einsum("...hqk,...khd->...qhd", p, v.abs()))
    return o.reshape(*o.shape[:-2], HEADS * d)


def _linear(x, w, trace, name):
    if trace is not None:
        trace[name + "_terms"] = x.abs() @ w.abs().t()
    return x @ w.t()


def temporal_chain(dd, A, fault=None, trace=None):
    """`[B, F, P, C]` -> the block's output, as csrc/temporal_block.hip documents the chain (phases A, B, D, E)."""
    t = lambda x: None if x is None else x.to(A.dtype)
    h, gamma, bpe, C = t(dd["h"]), t(dd["gamma"]), t(dd["bpe"]), dd["case"].C
    d = C // HEADS
    if fault == "pe_next_frame":
        bpe = bpe.roll(-1, 0)
    pre = A.ln(h, gamma, bpe[:, None, :], C, fault)
    x = A.round_x(pre)
    m = x
    if dd["w_merge"] is not None:
        pose = t(dd["pose"]).roll(-1, 2) if fault == "pose_next_pixel" else t(dd["pose"])
        s = 1.0 if fault == "no_merge_scale" else dd["merge_scale"]
        m = A.r(_linear(x, t(dd["w_merge"]), trace, "merge") * s + pose + x)
    qkv = A.r(_linear(m, t(dd["w_qkv"]), trace, "qkv"))
    q, k, v = (_heads(u, d).permute(0, 2, 1, 3, 4) for u in qkv.chunk(3, -1))            # [B, P, F, H, d]
    if fault == "v_next_pixel":
        v = v.roll(-1, 1)
    o = _attend(A, q, k, v, fault, d, trace).permute(0, 2, 1, 3)                         # [B, F, P, C]
    out = _linear(o, t(dd["w_out"]), trace, "out")
    if fault != "no_bias":
        out = out + t(dd["b_out"])
    if fault != "no_residual":
        out = out + h
    if trace is not None:
        trace.update(pre=pre, x=x, m=m, q=q, k=k, v=v, out=out)
        trace["out_terms"] = trace["out_terms"] + dd["b_out"].abs() + h.abs()
    return A.r(out)


def text_chain(dd, A, fault=None, trace=None):
    """`[N, P, C]` tokens, `kv [B, S, 2 C]` -> the block's output (the XATT path of csrc/temporal_block.hip, temporal_block640.hip)."""
    t = lambda x: x.to(A.dtype)
    c = dd["case"]
    h, C, S, B = t(dd["h"]), c.C, c.S, c.B
    d, P = C // HEADS, h.shape[1]
    pre = A.ln(h, t(dd["gamma"]), t(dd["beta"]), C, fault)
    x = A.round_x(pre)
    q = _heads(A.r(_linear(x, t(dd["w_q"]), trace, "q")), d).reshape(B, c.ipt, P, HEADS, d)
    kv = t(dd["kv"])
    if fault == "mask_last_key":
        kv = kv[:, :S - 1]
    if fault == "unmask_pad":
        kv = torch.cat([kv, kv.new_zeros(B, -(-S // 16) * 16 - S, 2 * C)], 1)
    k, v = _heads(kv[..., :C], d), _heads(kv[..., C:], d)
    if kv.shape[1] == 0:                                                                 # (every key masked: no finite answer; any value differs)
        return torch.full_like(h, float("nan"))
    o = _attend(A, q.reshape(B, c.ipt * P, HEADS, d), k, v, fault, d, trace).reshape(B, c.ipt, P, C)
    if fault == "next_batch_text":                                                       # the last image of every text's segment reads the next text
        q_last = q[:, -1].reshape(B, P, HEADS, d)
        o = o.clone()
        o[:, -1] = _attend(A, q_last, k.roll(-1, 0), v.roll(-1, 0), None, d, None)
    o = o.reshape(B * c.ipt, P, C)
    out = _linear(o, t(dd["w_out"]), trace, "out")
    if fault != "no_bias":
        out = out + t(dd["b_out"])
    if fault != "no_residual":
        out = out + h
    if trace is not None:
        trace.update(pre=pre, x=x, q=q, k=k, v=v, out=out)
        trace["out_terms"] = trace["out_terms"] + dd["b_out"].abs() + h.abs()
    return A.r(out)


def geglu_chain(dd, A, fault=None, trace=None):
    """`[M, C]` -> `[M, cff]`: (n W_v^T + b_v) * gelu(n W_g^T + b_g), n = LayerNorm(h) rounded to bf16."""
    t = lambda x: x.to(A.dtype)
    c = dd["case"]
    pre = A.ln(t(dd["h"]), t(dd["gamma"]), t(dd["beta"]), c.C, fault)
    x = A.round_x(pre)
    y = _linear(x, t(dd["w"]), trace, "y")
    if dd["bias"] is not None and fault != "no_bias":
        y = y + t(dd["bias"])
    val, gate = y[:, :c.cff], y[:, c.cff:]
    if fault == "swap_value_gate":
        val, gate = gate, val
    out = val * A.gelu(gate)
    if trace is not None:
        trace.update(pre=pre, x=x, gate=gate, value=val, out=out)
        if dd["bias"] is not None:
            trace["y_terms"] = trace["y_terms"] + dd["bias"].abs()
    return A.r(out)


def chain(c, A, fault=None, trace=None):
    fn = {TemporalCase: temporal_chain, TextCase: text_chain, GegluCase: geglu_chain}[type(c)]
    return fn(inputs(c), A, fault, trace)


@functools.lru_cache(maxsize=None)
def expectation(c):
    """(float64 expectation on the base pixels, its trace) -- computed once per case and shared; callers do not modify it."""
    trace = {}
    return chain(c, Exact, None, trace), trace


def expected_full(c):
    """The expectation at the case's own size, in bf16 (it is representable)."""
    ref = expectation(c)[0]
    if isinstance(c, TemporalCase):
        ref = expand_pixels(ref, c.hw, 2)
    elif isinstance(c, TextCase):
        ref = expand_pixels(ref, c.hw, 1)
    return ref.to(BF16)


def row_stats(out, eps=LN_EPS):
    """float64 (mean, rstd, mean |x|) of the rows of `out`."""
    o = out.detach().cpu().to(F64).reshape(-1, out.shape[-1])
    mean = o.mean(-1)
    return mean, (((o - mean[:, None]) ** 2).mean(-1) + eps).rsqrt(), o.abs().mean(-1)


def stats_violations(stats, out, eps=LN_EPS):
    """Rows whose (mean, rstd) leave the counted bounds against the float64 statistics of `out` (the kernel's own, rounded output)."""
    mean, rstd, mabs = row_stats(out, eps)
    s = stats.to(F64).cpu().reshape(-1, 2)
    dm = STATS_MEAN_REL * mabs
    bad_mean = (s[:, 0] - mean).abs() > dm
    bad_rstd = (s[:, 1] - rstd).abs() > rstd * (STATS_RSTD_REL + 0.5 * dm * dm * rstd * rstd)
    return bad_mean, bad_rstd


def check_stats(stats, out, what=""):
    bad_mean, bad_rstd = stats_violations(stats, out)
    mean, rstd, mabs = row_stats(out)
    s = stats.to(F64).cpu().reshape(-1, 2)
    print(f"   {what}: worst mean error {float(((s[:, 0] - mean).abs() / (STATS_MEAN_REL * mabs)).max()):.3f} of its bound, "
          f"worst rstd error {float(((s[:, 1] - rstd).abs() / (rstd * STATS_RSTD_REL)).max()):.3f} of {STATS_RSTD_CHAIN} x 2^-24")
    assert not bool(bad_mean.any()), f"{what}: {int(bad_mean.sum())} row means beyond {STATS_MEAN_CHAIN} x 2^-24 mean|x|, the first at row {int(bad_mean.nonzero()[0])}"
    assert not bool(bad_rstd.any()), f"{what}: {int(bad_rstd.sum())} row rstd beyond the bound, the first at row {int(bad_rstd.nonzero()[0])}"


def check_exact(got, ref, what=""):
    """Zero tolerance, element by element; names the first wrong (row, channel)."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.dtype == ref.dtype and torch.equal(got.detach().cpu(), ref.detach().cpu()):
        return
    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    bad = ~(got == ref)
    if bool(bad.any()):
        g2, r2, b2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1]), bad.reshape(-1, bad.shape[-1])
        row, ch = (int(v) for v in b2.nonzero()[0])
        rows = b2.any(-1).nonzero().reshape(-1)
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} elements in {rows.numel()} rows differ from the exact expectation; first at (row {row}, "
                             f"channel {ch}) of the flattened [rows, C] output with index {tuple(int(v) for v in bad.nonzero()[0])}: got {float(g2[row, ch])}, "
                             f"expected {float(r2[row, ch])}; last wrong row {int(rows[-1])}")


def ln_tie_distance(pre):
    """Distance of the un-rounded LayerNorm value to the nearest bf16 rounding tie, in units of the bf16 spacing there (0.5 = on a representable
    value, 0 = on a tie)."""
    p = pre.to(F64)
    lo = (p.to(F32).view(torch.int32) & -65536).view(F32).to(F64)                        # truncation: the representable value towards zero
    spacing = torch.where(lo == 0, torch.full_like(lo, 2.0 ** -133), 2.0 ** (torch.floor(torch.log2(lo.abs().clamp_min(2.0 ** -126))) - 7))
    frac = (p - lo).abs() / spacing
    return (frac - 0.5).abs()


def assert_exact_conditions(c):
    """Everything the exact run rests on, asserted on the float64 expectation of case `c` (on its base pixels: the generators are periodic)."""
    ref, tr = expectation(c)
    what = str(c)
    # 1. LayerNorm: within 1e-5 |gamma| (+ fp32 slack) of an integer below 256, and far from every rounding tie
    pre, x = tr["pre"], tr["x"]
    assert bool((x == x.round()).all()) and float(x.abs().max()) < 256, what
    assert float((pre - x).abs().max()) < 1e-4, (what, float((pre - x).abs().max()))
    assert float(ln_tie_distance(pre).min()) > 0.49, (what, float(ln_tie_distance(pre).min()))
    # 3. every tensor a kernel rounds is representable in bf16; every fp32 accumulator below 2^24
    for name in ("x", "m", "q", "k", "v", "o", "p", "out", "gate", "value"):
        if name in tr:
            assert is_bf16(tr[name]), f"{what}: {name} is not representable in bf16"
    for name, val in tr.items():
        if name.endswith("_terms"):
            assert float(val.max()) < 2 ** 24, f"{what}: {name} reaches {float(val.max())}"
    assert is_bf16(ref) and is_bf16(inputs(c)["h"])
    if isinstance(c, GegluCase):
        # 4. gates: 0 or an integer in [10, 16]; both occur; the fp32 restatement of fmc_gelu_fast is exact on them
        gate = tr["gate"]
        assert bool(((gate == 0) | ((gate >= 10) & (gate <= 16) & (gate == gate.round()))).all()), what
        assert bool((gate == 0).any()) and len(gate[gate > 0].unique()) >= 2, what
        ints = torch.arange(10, 17, dtype=F32)
        assert torch.equal(gelu_fast_f32(ints), ints) and float(gelu_fast_f32(torch.zeros(1))) == 0.0
        return
    # 2. softmax: scale_log2 == 1; per (query, head) the selected keys tie exactly and lead every other key by >= GAP; p in {0, 1, 1/2, 1/4}
    assert scale_log2(SCALE) == 1.0
    logits, p = tr["logits"], tr["p"]
    assert bool((logits == logits.round()).all())
    top = logits.amax(-1, keepdim=True)
    sel = logits == top
    rest = torch.where(sel, torch.full_like(logits, -1e9), logits).amax(-1, keepdim=True)
    assert bool(((top - rest) >= GAP).all()), (what, float((top - rest).min()))
    n_sel = sel.sum(-1, keepdim=True)
    assert bool(((n_sel == 1) | (n_sel == 2) | (n_sel == 4)).all()), what
    assert bool((p == sel.to(F64) / n_sel).all()), what
    assert int(n_sel.max()) == c.ties, (what, int(n_sel.max()))
    d = c.C // HEADS
    if d == 40:                                                                          # the head tail carries part of the decision in every head
        k = tr["k"]
        assert bool((k[..., 32:40].abs().sum(-1).reshape(-1, HEADS) > 0).any(0).all()), what
    if isinstance(c, TextCase):
        masked = inputs(c)["masked"].reshape(c.B, 1, -1, 1)
        assert bool((top[masked.expand_as(top)] <= -GAP).all()), what                    # a zero pad key (logit 0) would take these rows
        assert bool(masked.any()) or masked.numel() < 4, what
        tgt = sel.any(-2)                                                                # [B, H, S]: every key is some row's target in some head
        assert bool(tgt[..., c.S - 1].any()), what


# =====================================================================================================================================================
# the case table
# =====================================================================================================================================================
def T(C, B, hw, merge, stats=False, partial=False, ties=1, persistent=False):
    return TemporalCase(C, B, hw, merge, stats, partial, ties, persistent)


def X(C, B, ipt, hw, S, stats=False, partial=False, ties=1):
    return TextCase(C, B, ipt, hw, S, stats, partial, ties)


def G(kernel, C, M, cff, bias, variant=0, partial=False):
    return GegluCase(kernel, C, M, cff, bias, variant, partial)


def persistent_hw(c, cus):
    """Pixels per clip for `2 * CUs + 3` tiles in all (c.B == 1)."""
    return (2 * cus + 3) * (10 if c.C == 320 else 5)


TEMPORAL = (
    [T(320, B, hw, merge, stats) for (B, hw) in [(1, 10), (2, 30), (3, 70)] for merge in (True, False) for stats in (True, False)]
    + [T(320, 2, hw, merge, stats, partial=True) for hw in (1, 9, 11) for merge in (True, False) for stats in (True, False)]
    + [T(320, 2, 30, True, True, ties=2), T(320, 1, 11, False, True, partial=True, ties=4)]
    + [T(320, 1, 0, True, True, persistent=True)]
    + [T(640, B, hw, merge) for (B, hw) in [(1, 5), (2, 15)] for merge in (True, False)]
    + [T(640, 2, hw, merge, partial=True) for hw in (1, 4, 6) for merge in (True, False)]
    + [T(640, 2, 15, False, ties=2), T(640, 1, 6, True, partial=True, ties=4)]
    + [T(640, 1, 0, True, persistent=True)])

TEXT = (
    # C = 320: one tile / several tiles, S = 77, 80, 5, 1, images per text 1 and 3, with and without statistics
    [X(320, 1, 1, 160, 77, True), X(320, 1, 1, 160, 77, False), X(320, 3, 2, 320, 80, True), X(320, 2, 3, 160, 5, False), X(320, 2, 1, 160, 1, True),
     # a tile that spans two images of one text (80-row images, 160-row tiles; partial entry point)
     X(320, 2, 3, 80, 77, True, partial=True),
     # the partial forms at the shapes of test_xattn_block_partial_320
     X(320, 2, 1, 24, 77, True, partial=True), X(320, 2, 3, 100, 5, False, partial=True), X(320, 3, 2, 161, 80, True, partial=True),
     X(320, 2, 1, 160, 77, True, ties=2), X(320, 2, 3, 100, 80, False, partial=True, ties=4)]
    + [X(640, 1, 1, 80, 77), X(640, 3, 2, 160, 80), X(640, 2, 3, 80, 5), X(640, 2, 1, 80, 1),
       X(640, 2, 3, 40, 77, partial=True),
       X(640, 2, 1, 24, 77, partial=True), X(640, 2, 3, 50, 5, partial=True), X(640, 3, 2, 81, 80, partial=True),
       X(640, 2, 1, 80, 77, ties=2), X(640, 2, 3, 50, 80, partial=True, ties=4)])

GEGLU = (
    [G("direct", C, M, cff, bias) for (M, cff, C) in [(80, 320, 640), (240, 640, 640), (80, 160, 320), (400, 480, 320), (320, 640, 320)] for bias in (True, False)]
    + [G("pipe", C, M, cff, bias, variant) for (M, cff, C, variant) in [(80, 128, 320, 0), (320, 384, 320, 1), (400, 256, 320, 0), (240, 640, 640, 0), (160, 128, 320, 1)]
       for bias in (True, False)]
    + [G("pipe", C, M, cff, bias, variant, partial=True) for (M, cff, C, variant) in [(1, 128, 320, 0), (177, 256, 640, 0), (239, 384, 320, 0), (1, 128, 320, 1),
                                                                                      (241, 256, 320, 1), (319, 384, 320, 1)] for bias in (True, False)])


def all_cases():
    return TEMPORAL + TEXT + GEGLU


def case_id(c):
    if isinstance(c, TemporalCase):
        return f"temporal{c.C}-B{c.B}-hw{'persistent' if c.persistent else c.hw}-{'merge' if c.merge else 'nomerge'}{'-stats' if c.stats else ''}" \
               f"{'-partial' if c.partial else ''}{f'-tie{c.ties}' if c.ties > 1 else ''}"
    if isinstance(c, TextCase):
        return f"text{c.C}-B{c.B}x{c.ipt}-hw{c.hw}-S{c.S}{'-stats' if c.stats else ''}{'-partial' if c.partial else ''}{f'-tie{c.ties}' if c.ties > 1 else ''}"
    return f"geglu-{c.kernel}{c.variant if c.kernel == 'pipe' else ''}-C{c.C}-M{c.M}-cff{c.cff}{'-bias' if c.bias else ''}{'-partial' if c.partial else ''}"


def host_case(c):
    """The case the host tests examine in place of a persistent-loop one: its generator is periodic in the pixel, so PERIOD pixels are all it holds."""
    return c._replace(hw=PERIOD) if isinstance(c, TemporalCase) and c.persistent else c

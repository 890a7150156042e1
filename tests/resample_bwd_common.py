"""Backward-data of the two resampling convolutions in closed form (pure torch, any device; float64 in the tests), as the kernels of
csrc/conv_resample_bwd.hip compute it, with the sum of |terms| per output element for the accumulation bound.

The filter is `W[co][ci][ky][kx]`; zero is read outside the gradient's extent.

  stride 2 (3x3, pad 1, even input H x W; dY at H/2 x W/2):
      dX[2i+py, 2j+px, ci] = sum_{(ky,di) in T[py]} sum_{(kx,dj) in T[px]} sum_co W[co][ci][ky][kx] dY[i+di, j+dj, co]
      T[0] = {(1, 0)}      T[1] = {(2, 0), (0, +1)}
  nearest-2x upsample + 3x3 convolution (source Hs x Ws; dY at 2 Hs x 2 Ws):
      dX[u, v, ci] = sum_{r,c=0..3} sum_co G[co][ci][r][c] dY[2u-1+r, 2v-1+c, co]
      rows of G from rows of W:  r0 = w[2], r1 = w[1] + w[2], r2 = w[0] + w[1], r3 = w[0]     (columns likewise)

Tensors are logical NCHW here.  The `wrong` argument of the two functions builds the stand-ins that the host test must see fail.

Used by test_resample_bwd_reference_host.py (CPU) and test_gpu_resample_backward.py."""
import torch
import torch.nn.functional as F

T = {0: ((1, 0),), 1: ((2, 0), (0, 1))}                 # output parity -> ((filter row, source offset), ...)
G_ROWS = ((2,), (1, 2), (0, 1), (0,))                   # row r of G <- these rows of W (fmc_conv3x3_upfold_pack_weight's order of summation)

C_ACC = 1e-5                     # fp32 accumulation, relative to the sum of |terms| (tests/norm_bwd_common.py)
C_ROUND = 2.0 ** -8              # one rounding to bf16, relative to the result
C_FOLD = 2.0 ** -9               # the one rounding of the folded filter: half an ulp of every folded weight, relative to the sum of |terms|

WRONG_DOWN = ("parity_swapped", "offset_dropped", "filter_not_transposed", "edge_not_zero", "image_bleed")
WRONG_UP = ("filter_not_transposed", "edge_not_zero", "image_bleed", "g_row_unfolded")


def _pad_after(dy, lo, hi, wrong):
    """dY with `lo` rows / columns in front and `hi` behind.  Zeros, as the formulas say; `edge_not_zero`: what lies past the edge in a
    row-major tensor without the check -- the neighbouring row's values (replicated here); `image_bleed`: below the last row comes the
    first row of image n + 1 (and above the first row the last row of image n - 1)."""
    p = F.pad(dy, (lo, hi, lo, hi))
    if wrong == "edge_not_zero":
        p = F.pad(dy, (lo, hi, lo, hi), mode="replicate")
    elif wrong == "image_bleed":
        n, h = dy.shape[0], dy.shape[2]
        if hi:
            p[:-1, :, lo + h:, lo:p.shape[3] - hi] = dy[1:, :, :hi, :]
        if lo:
            p[1:, :, :lo, lo:p.shape[3] - hi] = dy[:-1, :, h - lo:, :]
    return p


def fold_g(w):
    """`[Cout, Cin, 3, 3]` -> `G [Cout, Cin, 4, 4]`, summed in the dtype of `w` in the kernels' order (rows, then columns, ascending)."""
    g = w.new_zeros(*w.shape[:2], 4, 4)
    for r in range(4):
        for c in range(4):
            for ky in G_ROWS[r]:
                for kx in G_ROWS[c]:
                    g[:, :, r, c] = g[:, :, r, c] + w[:, :, ky, kx]
    return g


def down_bwd(dy, w, wrong=None):
    """dX `[N, Cin, 2 Ho, 2 Wo]` of `F.conv2d(x, w, stride=2, padding=1)` from dY `[N, Cout, Ho, Wo]`."""
    n, _, ho, wo = dy.shape
    dyp = _pad_after(dy, 0, 1, wrong)
    dx = dy.new_zeros(n, w.shape[1], 2 * ho, 2 * wo)
    for py in range(2):
        for px in range(2):
            for ky, di in T[py]:
                for kx, dj in T[px]:
                    if wrong == "offset_dropped":
                        di, dj = 0, 0
                    k = w[:, :, kx, ky] if wrong == "filter_not_transposed" else w[:, :, ky, kx]
                    term = torch.einsum("ncij,cd->ndij", dyp[:, :, di:di + ho, dj:dj + wo], k)
                    if wrong == "parity_swapped":
                        dx[:, :, 1 - py::2, 1 - px::2] += term
                    else:
                        dx[:, :, py::2, px::2] += term
    return dx


def up_bwd_g(dy, g, wrong=None):
    """dX `[N, Cin, Hs, Ws]` from dY `[N, Cout, 2 Hs, 2 Ws]` and a 4x4 filter `g [Cout, Cin, 4, 4]` (the stride-2 gather)."""
    n, _, hd, wd = dy.shape
    hs, ws = hd // 2, wd // 2
    dyp = _pad_after(dy, 1, 1, wrong)
    dx = dy.new_zeros(n, g.shape[1], hs, ws)
    for r in range(4):
        for c in range(4):
            k = g[:, :, c, r] if wrong == "filter_not_transposed" else g[:, :, r, c]
            dx += torch.einsum("ncij,cd->ndij", dyp[:, :, r:r + 2 * hs:2, c:c + 2 * ws:2], k)
    return dx


def up_bwd(dy, w, wrong=None):
    """dX of `F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)`."""
    g = fold_g(w)
    if wrong == "g_row_unfolded":
        g[:, :, 1, :] = torch.stack([sum(w[:, :, 1, kx] for kx in G_ROWS[c]) for c in range(4)], dim=-1)       # row 1 = w[1] alone, not w[1] + w[2]
    return up_bwd_g(dy, g, wrong)


def magnitude(dy, w, up):
    """Sum of |terms| per output element, over |W| |dY| of the UNFOLDED filter (the fold of |W| is the sum of the |w| it merges)."""
    return up_bwd(dy.abs(), w.abs()) if up else down_bwd(dy.abs(), w.abs())


def bound(ref, mag, up):
    """`2^-8 |ref|` (output rounding) `+ 1e-5 sum|terms|` (fp32 accumulation), and for the upsample `+ 2^-9 sum|terms|` (the folded
    filter's one rounding to bf16)."""
    b = C_ROUND * ref.double().abs() + C_ACC * mag.double()
    return b + C_FOLD * mag.double() if up else b


def emulate(dy_bf16, w_bf16, up):
    """The kernels' rounding chain in plain torch: bf16 operands, the fold summed in fp32 and rounded to bf16 once, products accumulated
    in fp32 (in another order than the kernels'), one rounding of the result to bf16."""
    dy, w = dy_bf16.float(), w_bf16.float()
    if up:
        return up_bwd_g(dy, fold_g(w).to(torch.bfloat16).float()).to(torch.bfloat16)
    return down_bwd(dy, w).to(torch.bfloat16)


def misses(got, ref, mag, up):
    """Number of elements outside the bound, and the largest share of its bound any element uses."""
    err = (got.double() - ref.double()).abs()
    b = bound(ref, mag, up)
    return int((err > b).sum()), float((err / b.clamp_min(1e-300)).max())

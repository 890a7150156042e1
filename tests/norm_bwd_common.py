"""References, bounds, shapes and inputs of the LayerNorm / GroupNorm(+SiLU) / GEGLU backward tests (pure torch, runs on the CPU).

Float64 closed forms on the rounded inputs, each with `mag`, the sum of |terms| behind every element:

    LayerNorm   xh = (x - mean) rstd,  dyh = dy gamma,  dX = rstd (dyh - mean(dyh) - xh mean(dyh xh)) (+ addend)
                mag = rstd (|dyh| + mean|dyh| + |xh| mean|dyh xh|) (+ |addend|)
                dgamma = sum_rows dy xh,  mag = sum |dy xh|;   dbeta = sum_rows dy,  mag = sum |dy|
    GroupNorm   the same over the (pixels x channels) of a group, with dz = dy silu'(z), z = xh gamma + beta, in the place of dy
    GEGLU       y = a g Phi(g),  da = dy g Phi(g),  dg = dy a (Phi(g) + g phi(g));  Phi = 0.5 (1 + erf): its two terms are taken in absolute
                value, `0.5 (1 + |erf|)` -- the kernel forms 1 + erf in fp32, and at a negative gate that sum cancels: relative to
                |Phi| alone the bound would ask for digits fp32 does not have

Bounds (the project's own, tests/test_gpu_kernels.py): bf16 storage `2^-8 |ref| + 1e-5 mag` (one rounding of an fp32 result), fp32
storage and the fp32 dgamma / dbeta `1e-5 mag`.

Used by test_norm_bwd_reference_host.py (CPU) and test_gpu_norm_backward.py.
"""
import math

import torch

from tests import attn_bwd_common as AB

EPS = 1e-5
GROUPS = 32
C_ACC = 1e-5                      # fp32 accumulation, relative to the sum of |terms|
C_ROUND = 2.0 ** -8               # one rounding to bf16, relative to the result

# LayerNorm (M, C).  The backward's grid is capped at 2048 workgroups of 4 waves, one row per wave and trip.
LN_SHAPES = [
    (8197, 64),        # five rows on the second trip
    (16389, 72),       # three trips, nine chunks of eight
    (8200, 320),
    (5, 2560),         # five chunks per lane
    (6, 2048),         # four chunks per lane, all lanes full
    (37, 640),
    (3, 1280),
    (1, 8),
]
# GEGLU (M, Cff).  The grid is capped at 4096 workgroups of 256 threads, one chunk of eight per thread and trip.
GEGLU_SHAPES = [
    (6560, 1280),      # 1 049 600 chunks: the first of these shapes with a second trip
    (33, 72),
    (1, 8),
    (5, 2560),
]
# GroupNorm (N, HW, C), 32 groups
GN_SHAPES = [
    (2, 97, 320),      # two splits of 49 rows, ragged two-row trips
    (1, 6150, 320),    # the split cap of 64
    (2, 13, 2560),     # one row per trip
    (2, 130, 32),      # one channel per group
    (2, 33, 64),       # 264 threads: no whole number of waves
    (1, 9, 4096),      # the widest tensor the kernels take
]


def shape_id(shape):
    return "x".join(str(s) for s in shape)


def _seed(shape):
    return 7000 + sum((i + 1) * s for i, s in enumerate(shape)) % 997


def affine(C, seed):
    """fp32 gamma (around one) and beta"""
    g = torch.Generator().manual_seed(seed)
    return 1.0 + 0.5 * torch.randn(C, generator=g), torch.randn(C, generator=g)


def ln_inputs(shape, dtype):
    """x, dy, addend `[M, C]` (fp32 holding values of `dtype`), gamma, beta (fp32)"""
    M, C = shape
    s = _seed(shape)
    x = (AB.rnd_cpu((M, C), s, dtype, 1.5) + 0.3).to(dtype).float()               # (a mean to subtract)
    return x, AB.rnd_cpu((M, C), s + 1, dtype), AB.rnd_cpu((M, C), s + 2, dtype), *affine(C, s + 3)


def gn_inputs(shape, dtype):
    N, HW, C = shape
    s = _seed(shape)
    x = (AB.rnd_cpu((N, HW, C), s, dtype, 1.2) - 0.3).to(dtype).float()
    return x, AB.rnd_cpu((N, HW, C), s + 1, dtype), AB.rnd_cpu((N, HW, C), s + 2, dtype), *affine(C, s + 3)


def geglu_inputs(shape, dtype):
    M, Cff = shape
    s = _seed(shape)
    return AB.rnd_cpu((M, 2 * Cff), s, dtype, 1.5), AB.rnd_cpu((M, Cff), s + 1, dtype)


def ln_reference(x, dy, gamma, addend=None, eps=EPS):
    """LayerNorm backward over the last axis in float64: dict of dx, dgamma, dbeta and their mag_*."""
    x, dy, gamma = x.double(), dy.double(), gamma.double()
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).square().mean(-1, keepdim=True) + eps).rsqrt()
    xh, dyh = (x - mean) * rstd, dy * gamma
    dx = rstd * (dyh - dyh.mean(-1, keepdim=True) - xh * (dyh * xh).mean(-1, keepdim=True))
    mag = rstd * (dyh.abs() + dyh.abs().mean(-1, keepdim=True) + xh.abs() * (dyh * xh).abs().mean(-1, keepdim=True))
    if addend is not None:
        dx, mag = dx + addend.double(), mag + addend.double().abs()
    rows = tuple(range(x.ndim - 1))
    return dict(dx=dx, mag_dx=mag, dgamma=(dy * xh).sum(rows), mag_dgamma=(dy * xh).abs().sum(rows), dbeta=dy.sum(rows), mag_dbeta=dy.abs().sum(rows))


def gn_reference(x, dy, gamma, beta, act, addend=None, groups=GROUPS, eps=EPS, group_m2=True):
    """GroupNorm(+SiLU) backward of `[N, HW, C]` tokens in float64: dict of dx, mag_dx.  `group_m2=False` is a FAULT for the CPU tests: the
    mean of `dxh xh` taken over all C channels instead of the group."""
    N, HW, C = x.shape
    cpg = C // groups
    x5, dy5 = x.double().reshape(N, HW, groups, cpg), dy.double().reshape(N, HW, groups, cpg)
    gm, bt = gamma.double().reshape(groups, cpg), beta.double().reshape(groups, cpg)
    mean = x5.mean((1, 3), keepdim=True)
    rstd = ((x5 - mean).square().mean((1, 3), keepdim=True) + eps).rsqrt()
    xh = (x5 - mean) * rstd
    dz = dy5
    if act:
        z = xh * gm + bt
        s = torch.sigmoid(z)
        dz = dy5 * s * (1 + z * (1 - s))
    dxh = dz * gm
    m2 = (dxh * xh).mean((1, 3), keepdim=True) if group_m2 else (dxh * xh).mean((1, 2, 3), keepdim=True)
    dx = rstd * (dxh - dxh.mean((1, 3), keepdim=True) - xh * m2)
    mag = rstd * (dxh.abs() + dxh.abs().mean((1, 3), keepdim=True) + xh.abs() * (dxh * xh).abs().mean((1, 3), keepdim=True))
    dx, mag = dx.reshape(N, HW, C), mag.reshape(N, HW, C)
    if addend is not None:
        dx, mag = dx + addend.double(), mag + addend.double().abs()
    return dict(dx=dx, mag_dx=mag)


def geglu_reference(x, dy):
    """GEGLU forward and backward in float64: dict of y, dx (`[.., 2 Cff]`: da | dg) and mag_y, mag_dx."""
    a, g = x.double().chunk(2, dim=-1)
    dy = dy.double()
    erf = torch.erf(g / math.sqrt(2.0))
    cdf, cdf_abs = 0.5 * (1 + erf), 0.5 * (1 + erf.abs())
    pdf = torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)
    return dict(y=a * g * cdf, mag_y=a.abs() * g.abs() * cdf_abs,
                dx=torch.cat([dy * g * cdf, dy * a * (cdf + g * pdf)], -1),
                mag_dx=torch.cat([dy.abs() * g.abs() * cdf_abs, (dy * a).abs() * (cdf_abs + g.abs() * pdf)], -1))


def bound(ref, mag, dtype):
    """bf16 storage: `2^-8 |ref| + 1e-5 mag`; fp32 (storage, or the fp32 affine gradients): `1e-5 mag`."""
    b = C_ACC * mag.double()
    return b + C_ROUND * ref.double().abs() if dtype == torch.bfloat16 else b


def bound_ratio(got, ref, mag, dtype):
    """Worst `|got - ref| / bound` over the elements (0 where both are zero)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err, b = (got - ref).abs(), bound(ref, mag.detach().cpu(), dtype)
    return float(torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0)).max())


def assert_close(got, ref, mag, dtype, what=""):
    """Element-wise `|got - ref| <= bound(ref, mag, dtype)`; returns the worst error in units of the bound."""
    got, ref, mag = got.detach().double().cpu(), ref.detach().double().cpu(), mag.detach().double().cpu()
    assert got.shape == ref.shape == mag.shape, f"{what}: shapes {tuple(got.shape)} / {tuple(ref.shape)} / {tuple(mag.shape)}"
    err, b = (got - ref).abs(), bound(ref, mag, dtype)
    bad = ~(err <= b)                                      # (a NaN is bad)
    if bool(bad.any()):
        over = torch.where(bad, (err - b).nan_to_num(nan=float("inf")), torch.full_like(err, -1.0))
        worst = tuple(int(i) for i in torch.unravel_index(over.argmax(), over.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} elements beyond the bound, worst at {worst}: "
                             f"got {float(got[worst]):.6e} ref {float(ref[worst]):.6e} |terms| {float(mag[worst]):.6e}")
    return float(torch.where(b > 0, err / b.clamp_min(1e-300), torch.zeros_like(err)).max())


# ---- plain-torch restatements of how the kernels walk their rows, for the fault tests -------------------------------------------------
LN_ROWS_PER_TRIP = 2048 * 4           # the LayerNorm backward's grid cap x waves per workgroup


def ln_backward_by_trips(x, dy, gamma, addend=None, drop_second_trip_from_dgamma=False, drop_addend_after_first_trip=False, dtype=torch.float32):
    """The LayerNorm backward in fp32, row r on trip `r // 8192` as the grid-stride loop has it; dX rounded to `dtype`.
    Faults: the rows of the later trips missing from dgamma / dbeta; the addend added on the first trip only."""
    ref = ln_reference(x, dy, gamma, None)
    later = torch.arange(x.shape[0]) >= LN_ROWS_PER_TRIP
    dx = ref["dx"].float()
    if addend is not None:
        add = addend.float().clone()
        if drop_addend_after_first_trip:
            add[later] = 0
        dx = dx + add
    keep = ~later if drop_second_trip_from_dgamma else torch.ones_like(later)
    part = ln_reference(x[keep], dy[keep], gamma, None)
    return dict(dx=dx.to(dtype).float(), dgamma=part["dgamma"].float(), dbeta=part["dbeta"].float())


def gn_split_rows(HW, C):
    """(rows per split, splits) of the two-pass GroupNorm kernels, restated: 512 threads = C / 8 threads per row x rows per trip, about
    eight trips per split, at most 64 splits."""
    rpi = max(1, min(512 // (C // 8), HW))
    split = max(1, min(64, -(-HW // (8 * rpi))))
    rows = -(-HW // split)
    return rows, -(-HW // rows)


def gn_backward_by_splits(x, dy, gamma, beta, act, addend=None, skip_last_row_of_split=False, dtype=torch.float32):
    """The GroupNorm backward with dX rounded to `dtype`.  Fault: the last row of every split is never stored (the buffer's zeros stay)."""
    dx = gn_reference(x, dy, gamma, beta, act, addend)["dx"].float()
    if skip_last_row_of_split:
        rows, split = gn_split_rows(x.shape[1], x.shape[2])
        for s in range(split):
            dx[:, min((s + 1) * rows, x.shape[1]) - 1] = 0
    return dx.to(dtype).float()

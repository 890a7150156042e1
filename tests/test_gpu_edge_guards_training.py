"""The training-side reductions at their ragged edges, with poison around their inputs and sentinels around their outputs.

The conventions of tests/test_gpu_edge_guards.py: raw C ABI, every operand in an arena of the test's own (tests/edge_guard_common.py), every case
under zeros, quiet NaN and +Inf around the inputs.  Asserted per case:

  1. every output is finite and BIT-IDENTICAL across the three runs (`torch.equal`).  ONE exemption: the `dgamma` / `dbeta` of `fmc_layernorm_bwd`
     / `_bwd_add` are summed by fp32 `atomicAdd` in arrival order; each of their three runs is finite and meets the kernel's own bound instead;
  2. the zeros run meets the reference and the gate of the kernel's existing test: `NB.assert_close` (tests/norm_bwd_common.py) for the LayerNorm,
     GroupNorm and GEGLU backward, the fp64 autograd reference and 1e-4 rel-inf of test_gn_param_backward_matches_fp64 for the affine gradients of
     GroupNorm, 1e-5 rel-inf for the column sum (test_column_sum_matches_fp64), 1e-4 rel-inf for the weight gradient
     (test_wgrad_kernel_matches_fp64); the layout pass of the convolution weight gradient is a copy and is compared exactly;
  3. every word outside an output view keeps the sentinel and every word inside was written; outputs the ABI accumulates into start as the ABI
     demands (`Guard.out(init=...)`) and only their outside is checked; the poison around every input is still in place.

Bands in ROWS of the guarded tensor, next to the case tables with the source line they come from.  One run is recorded in profiles/edge_guards.md."""
import functools

import pytest
import torch

from tests import edge_guard_common as EG
from tests import mm_common as MC
from tests import norm_bwd_common as NB
from tests.test_gpu_edge_guards import _call, _p, _rnd, _run, _vec_band
from tests.test_gpu_mm_training import _gn_ref as gn_autograd_fp64

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [BF16, F32]
TAG = {BF16: "bf16", F32: "fp32"}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _flat_f32(g, nbytes, name, band=4096, written=True):
    """A guarded fp32 buffer of EXACTLY `nbytes` (a multiple of 16), as rows of four floats."""
    assert nbytes > 0 and nbytes % 16 == 0, nbytes
    return g.out((nbytes // 16, 4), F32, band, 0, name, written=written)


# =====================================================================================================================================
# LayerNorm backward (norm_kernels.hip: layernorm_bwd_kernel, launch_ln_bwd).  One row per wave and trip, four waves per workgroup, at most 2048
# workgroups (norm_kernels.hip:1394-1396): a whole grid-stride trip is 8192 rows.  A wave that ran one trip too many would touch the rows right
# behind M, so the band need not be a trip long.
# =====================================================================================================================================
LN_BAND = 512                                   # rows of x / dy / addend / dx: 128 x the four rows a workgroup has in flight (norm_kernels.hip:910)
LN_M = (1, 7, NB.LN_ROWS_PER_TRIP + 1)          # one row on the second trip
LN_C = (64, 320, 1280)                          # one, one (40 of 64 lanes) and three chunks per lane


@functools.lru_cache(maxsize=None)
def _ln_case(M, C, dtype):
    x, dy, add, gamma, _ = NB.ln_inputs((M, C), dtype)
    return x, dy, add, gamma, NB.ln_reference(x, dy, gamma)


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("entry", ["bwd-frozen", "bwd-trainable", "bwd_add-frozen", "bwd_add-trainable"])
@pytest.mark.parametrize("C", LN_C)
@pytest.mark.parametrize("M", LN_M)
def test_layernorm_backward(K, M, C, entry, dtype):
    x, dy, add, gamma, ref = _ln_case(M, C, dtype)
    with_add, train = entry.startswith("bwd_add"), entry.endswith("trainable")
    atomics = []                                  # (dgamma, dbeta) of each run: not bit-compared (arrival order of the atomicAdd, norm_kernels.hip:976)

    def fn(g):
        xd, dyd = g.inp(x.to(dtype), LN_BAND, 0, "x"), g.inp(dy.to(dtype), LN_BAND, 0, "dy")
        gd = g.inp(gamma, _vec_band(C), 0, "gamma")
        ad = g.inp(add.to(dtype), LN_BAND, 0, "addend") if with_add else None
        dx = g.out((M, C), dtype, LN_BAND, 0, "dx")
        dg = g.out((C,), F32, _vec_band(C), 0, "dgamma", init=0.0) if train else None          # "ACCUMULATED into: zero them first"
        db = g.out((C,), F32, _vec_band(C), 0, "dbeta", init=0.0) if train else None
        if with_add:
            _call(K, "fmc_layernorm_bwd_add", dyd.data_ptr(), xd.data_ptr(), gd.data_ptr(), dx.data_ptr(), _p(dg), _p(db), ad.data_ptr(), M, C, NB.EPS,
                  K._dt(xd), K._stream())
        else:
            _call(K, "fmc_layernorm_bwd", dyd.data_ptr(), xd.data_ptr(), gd.data_ptr(), dx.data_ptr(), _p(dg), _p(db), M, C, NB.EPS, K._dt(xd), K._stream())
        if train:
            torch.cuda.synchronize()
            atomics.append((g.poison, dg.clone(), db.clone()))
        return {"dx": dx}

    what = f"layernorm_{entry} M {M} C {C} {TAG[dtype]}"
    got = _run(fn, what)
    want, mag = (ref["dx"] + add.double(), ref["mag_dx"] + add.double().abs()) if with_add else (ref["dx"], ref["mag_dx"])
    ratios = dict(dx=NB.assert_close(got["dx"], want, mag, dtype, "dx"))
    for poison, dg, db in atomics:
        assert bool(torch.isfinite(dg).all()) and bool(torch.isfinite(db).all()), f"{what}: dgamma / dbeta not finite with {poison} around the inputs"
        r = (NB.assert_close(dg, ref["dgamma"], ref["mag_dgamma"], F32, f"dgamma [{poison}]"), NB.assert_close(db, ref["dbeta"], ref["mag_dbeta"], F32, f"dbeta [{poison}]"))
        ratios[f"dgamma/dbeta[{poison}]"] = max(r)
    print(f"   {what}: worst error in units of NB.bound: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


# =====================================================================================================================================
# GEGLU backward (norm_kernels.hip: geglu_bwd_kernel).  One chunk of eight per thread and trip, at most 4096 workgroups of 256 threads
# (norm_kernels.hip:1435-1438): a whole trip is 1 048 576 chunks; M = 8193 at Cff = 1280 is 1 310 880, so the last rows are a second trip's.
# =====================================================================================================================================
GEGLU_BAND = 512                                # rows; a workgroup's 256 chunks are at most 13 rows of Cff = 160 (norm_kernels.hip:989-996)


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("Cff", [160, 1280])
@pytest.mark.parametrize("M", LN_M)
def test_geglu_backward(K, M, Cff, dtype):
    x, dy = NB.geglu_inputs((M, Cff), dtype)
    ref = NB.geglu_reference(x, dy)

    def fn(g):
        xd, dyd = g.inp(x.to(dtype), GEGLU_BAND, 0, "x"), g.inp(dy.to(dtype), GEGLU_BAND, 0, "dy")
        dx = g.out((M, 2 * Cff), dtype, GEGLU_BAND, 0, "dx")
        _call(K, "fmc_geglu_bwd", dyd.data_ptr(), xd.data_ptr(), dx.data_ptr(), M, Cff, K._dt(xd), K._stream())
        return {"dx": dx}

    what = f"geglu_bwd M {M} Cff {Cff} {TAG[dtype]}"
    got = _run(fn, what)
    print(f"   {what}: worst error in units of NB.bound: da | dg {NB.assert_close(got['dx'], ref['dx'], ref['mag_dx'], dtype, 'da | dg'):.3f}")


# =====================================================================================================================================
# GroupNorm (+ SiLU) backward (norm_kernels.hip: gn_partial_kernel<., 1 / 2>, gn_apply_bwd_kernel, gn_param_combine_kernel).  `gn_geom`
# (norm_kernels.hip:28-42): C / 8 threads across a row, rpi = min(512 / (C / 8), HW) rows per trip of a workgroup, GN_U = 4 trips' loads in flight.
# =====================================================================================================================================
GN_BAND = 512                                   # rows of x / dy / addend / dx: 4 x rpi <= 4 x 128 (C = 32) rows in flight (norm_kernels.hip:26, 31)
GN_WS_BAND = 4096                               # rows of four floats around the workspace: one sample's 64 splits x 32 groups x 2 floats, x 4
# the shapes of NB.GN_SHAPES whose HW is no multiple of rpi (12, 12, 128), then the two the issue names (33 = rpi, one trip; 7 rows of one row per trip)
GN_SHAPES = [(2, 97, 320), (1, 6150, 320), (2, 130, 32), (2, 33, 64), (2, 7, 2560)]


@functools.lru_cache(maxsize=None)
def _gn_case(shape, dtype, act):
    x, dy, add, gamma, beta = NB.gn_inputs(shape, dtype)
    return x, dy, add, gamma, beta, NB.gn_reference(x, dy, gamma, beta, act)


def _gn_stats(K, x, gamma, beta, dtype, act, eps):
    """`[N, G, 2]` statistics of the forward kernel on plain tensors: an INPUT of the backward, guarded as such."""
    _, stats = K.groupnorm_silu_raw(x.to(dtype).cuda(), gamma.cuda(), beta.cuda(), NB.GROUPS, eps, act)
    torch.cuda.synchronize()
    return stats.cpu().view(x.shape[0], NB.GROUPS * 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("act", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("entry", ["bwd", "bwd_add"])
@pytest.mark.parametrize("shape", GN_SHAPES, ids=NB.shape_id)
def test_groupnorm_backward(K, shape, entry, act, dtype):
    N, HW, C = shape
    G = NB.GROUPS
    x, dy, add, gamma, beta, ref = _gn_case(shape, dtype, act)
    stats = _gn_stats(K, x, gamma, beta, dtype, act, NB.EPS)
    ws_bytes = K._lib.load().fmc_groupnorm_workspace_bytes(N, C, G)

    def fn(g):
        xd, dyd = g.inp(x.to(dtype), GN_BAND, 0, "x"), g.inp(dy.to(dtype), GN_BAND, 0, "dy")
        gd, bd, sd = g.inp(gamma, _vec_band(C), 0, "gamma"), g.inp(beta, _vec_band(C), 0, "beta"), g.inp(stats, 8, 0, "stats")
        dx = g.out((N, HW, C), dtype, GN_BAND, 0, "dx")
        ws = _flat_f32(g, ws_bytes, "workspace", GN_WS_BAND, written=False)                    # sized for 64 splits; `gn_geom` uses fewer
        if entry == "bwd_add":
            ad = g.inp(add.to(dtype), GN_BAND, 0, "addend")
            _call(K, "fmc_groupnorm_silu_bwd_add", dyd.data_ptr(), xd.data_ptr(), dx.data_ptr(), gd.data_ptr(), bd.data_ptr(), sd.data_ptr(), ws.data_ptr(),
                  N, HW, C, G, int(act), ad.data_ptr(), K._dt(xd), K._stream())
        else:
            _call(K, "fmc_groupnorm_silu_bwd", dyd.data_ptr(), xd.data_ptr(), dx.data_ptr(), gd.data_ptr(), bd.data_ptr(), sd.data_ptr(), ws.data_ptr(),
                  N, HW, C, G, int(act), K._dt(xd), K._stream())
        return {"dx": dx}

    what = f"groupnorm_silu_{entry} {shape} {'silu' if act else 'plain'} {TAG[dtype]}"
    got = _run(fn, what)
    want, mag = (ref["dx"] + add.double(), ref["mag_dx"] + add.double().abs()) if entry == "bwd_add" else (ref["dx"], ref["mag_dx"])
    print(f"   {what}: worst error in units of NB.bound: dx {NB.assert_close(got['dx'], want, mag, dtype, 'dx'):.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("mode", ["dx", "dx+addend", "no-dx", "accumulate"])
@pytest.mark.parametrize("shape", GN_SHAPES, ids=NB.shape_id)
def test_groupnorm_backward_params(K, shape, mode, dtype):
    """`fmc_groupnorm_silu_bwd_params` (SiLU on; eps 1e-6 and the fp64 autograd reference of test_gn_param_backward_matches_fp64): dX with and without
    the addend, dx NULL, and dgamma / dbeta accumulated into what is there.  The workspace is exactly `*_params_workspace_bytes`."""
    N, HW, C = shape
    G, act, eps = NB.GROUPS, True, 1e-6
    x, dy, add, gamma, beta = NB.gn_inputs(shape, dtype)
    stats = _gn_stats(K, x, gamma, beta, dtype, act, eps)
    ws_bytes = K._lib.load().fmc_groupnorm_silu_bwd_params_workspace_bytes(N, HW, C, G)
    base_g, base_b = _rnd((C,), 31, F32), _rnd((C,), 32, F32)
    accumulate, want_dx, addend = mode == "accumulate", mode != "no-dx", (add if mode == "dx+addend" else None)
    dx_ref, dg_ref, db_ref = gn_autograd_fp64(x, gamma, beta, dy, act, addend)

    def fn(g):
        xd, dyd = g.inp(x.to(dtype), GN_BAND, 0, "x"), g.inp(dy.to(dtype), GN_BAND, 0, "dy")
        gd, bd, sd = g.inp(gamma, _vec_band(C), 0, "gamma"), g.inp(beta, _vec_band(C), 0, "beta"), g.inp(stats, 8, 0, "stats")
        ad = g.inp(add.to(dtype), GN_BAND, 0, "addend") if addend is not None else None
        dx = g.out((N, HW, C), dtype, GN_BAND, 0, "dx") if want_dx else None
        dg = g.out((C,), F32, _vec_band(C), 0, "dgamma", init=base_g if accumulate else None)
        db = g.out((C,), F32, _vec_band(C), 0, "dbeta", init=base_b if accumulate else None)
        ws = _flat_f32(g, ws_bytes, "workspace", GN_WS_BAND, written=False)
        _call(K, "fmc_groupnorm_silu_bwd_params", dyd.data_ptr(), xd.data_ptr(), _p(dx), dg.data_ptr(), db.data_ptr(), gd.data_ptr(), bd.data_ptr(),
              sd.data_ptr(), _p(ad), int(accumulate), ws.data_ptr(), N, HW, C, G, int(act), K._dt(xd), K._stream())
        res = {"dgamma": dg, "dbeta": db}
        if want_dx:
            res["dx"] = dx
        return res

    what = f"groupnorm_silu_bwd_params {shape} {mode} {TAG[dtype]}"
    got = _run(fn, what)
    if accumulate:
        dg_ref, db_ref = dg_ref + base_g.double(), db_ref + base_b.double()
    errs = [MC.rel_inf(got["dgamma"], dg_ref), MC.rel_inf(got["dbeta"], db_ref)]
    assert errs[0] < 1e-4 and errs[1] < 1e-4, errs
    if want_dx:
        errs.append(MC.rel_inf(got["dx"], dx_ref))
        assert errs[2] < (1e-2 if dtype == BF16 else 1e-4), errs
    print(f"   {what}: rel-inf dgamma {errs[0]:.2e} dbeta {errs[1]:.2e} (gate 1e-4)" + (f" dx {errs[2]:.2e} (gate {'1e-2' if dtype == BF16 else '1e-4'})" if want_dx else ""))


# =====================================================================================================================================
# fmc_column_sum (norm_kernels.hip: column_sum_partial_kernel / column_sum_combine_kernel).  A workgroup is 64 columns x 4 row lanes with
# CSUM_U = 4 rows per lane in flight: 16 rows per trip (norm_kernels.hip:205, 244-250), over one of `csum_geom`'s splits of the rows.
# =====================================================================================================================================
CSUM_BAND = 64                                  # rows of x: four 16-row trips (norm_kernels.hip:244)
CSUM_PAD = 64                                   # spare columns of x (ld = N + 64): one 64-column block past N (norm_kernels.hip:237)


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("N", [8, 320, 1288])
@pytest.mark.parametrize("M", [1, 77, 1000, 24577])
def test_column_sum(K, M, N, accumulate, dtype):
    x = _rnd((M, N), 500 + M + N, dtype)
    base = _rnd((N,), 501, F32)
    ref = x.double().sum(0)
    ws_bytes = K._lib.load().fmc_column_sum_workspace_bytes(M, N)
    assert ws_bytes > 0 and ws_bytes % (4 * N) == 0
    alpha = -1.0 if accumulate else 0.5

    def fn(g):
        xd = g.inp(x, CSUM_BAND, CSUM_PAD, "x")
        out = g.out((N,), F32, _vec_band(N), 0, "out", init=base if accumulate else None)
        ws = g.out((ws_bytes // (4 * N), N), F32, 16, 0, "workspace")                            # exact, and every partial written
        _call(K, "fmc_column_sum", xd.data_ptr(), out.data_ptr(), M, N, xd.stride(0), alpha, int(accumulate), ws.data_ptr(), K._dt(xd), K._stream())
        return {"out": out, "partials": ws}

    what = f"column_sum M {M} N {N} {'accumulate' if accumulate else 'write'} {TAG[dtype]}"
    got = _run(fn, what)
    err = MC.rel_inf(got["out"], base.double() - ref if accumulate else 0.5 * ref)
    print(f"   {what}: rel-inf {err:.2e} (gate 1e-5)")
    assert err < 1e-5


# =====================================================================================================================================
# fmc_linear_wgrad_bf16 (lora_wgrad.hip).  A workgroup stages slabs of WG_BT = 128 tokens x 64 columns of a and of b (lora_wgrad.hip:20-22, 45-52),
# the next slab into registers under the current one (lora_wgrad.hip:106-110), and writes a 64 x 64 tile of out or of its split's partials.
# =====================================================================================================================================
WGRAD_BAND = 256                                # rows (tokens) of a / b: the slab in flight and the one requested ahead (lora_wgrad.hip:106)
WGRAD_BAND_OUT = 64                             # rows of out: one WG_BN tile (lora_wgrad.hip:21)
WGRAD_PAD = 64                                  # columns each side of a column slice: one WG_BN / WG_BK block (lora_wgrad.hip:100-101)
WGRAD_SHAPES = [(1, 320, 160), (77, 640, 768), (1000, 480, 320), (1232, 1280, 768), (24577, 320, 160)]


@functools.lru_cache(maxsize=None)
def _wgrad_data(M, N, Kd):
    a, b = _rnd((M, N), 900 + M + N, BF16), _rnd((M, Kd), 901 + M + Kd, BF16)
    return a, b, a.double().t() @ b.double(), _rnd((N, Kd), 902, F32)


def _wgrad_operand(g, t, sliced, name):
    """Dense: rows `cols + 64` apart, the spare columns poison.  Slice: the middle columns of a wider tensor whose other columns hold the poison."""
    if not sliced:
        return g.inp(t, WGRAD_BAND, WGRAD_PAD, name)
    wide = torch.full((t.shape[0], t.shape[1] + 2 * WGRAD_PAD), EG.poison_value(g.poison, t.dtype), dtype=t.dtype)
    wide[:, WGRAD_PAD:WGRAD_PAD + t.shape[1]] = t
    return g.inp(wide, WGRAD_BAND, 0, name + " (slice)")[:, WGRAD_PAD:WGRAD_PAD + t.shape[1]]


def _wgrad_launch(K, g, problems):
    """`problems`: (a, b, sliced, alpha, base or None).  Each out in an arena of its own (ldo = K + 8), the workspace exact."""
    descs, outs = [], []
    for i, (a, b, sliced, alpha, base) in enumerate(problems):
        ad, bd = _wgrad_operand(g, a, sliced, f"a{i}"), _wgrad_operand(g, b, sliced, f"b{i}")
        out = g.out((a.shape[1], b.shape[1]), F32, WGRAD_BAND_OUT, 8, f"out{i}", init=base)
        descs.append(K.WgradProblem(ad.data_ptr(), bd.data_ptr(), out.data_ptr(), a.shape[0], ad.stride(0), bd.stride(0), out.stride(0), a.shape[1], b.shape[1],
                                    float(alpha), int(base is not None)))
        outs.append(out)
    arr = (K.WgradProblem * len(descs))(*descs)
    lib = K._lib.load()
    need = lib.fmc_linear_wgrad_workspace_bytes(arr, len(descs))
    assert need >= 0, "fmc_linear_wgrad_workspace_bytes refused the list"
    ws = _flat_f32(g, need, "workspace", 4096) if need else None
    K._lib.check(lib.fmc_linear_wgrad_bf16(arr, len(descs), _p(ws), need, K._stream()), "fmc_linear_wgrad_bf16")
    res = {f"out{i}": o for i, o in enumerate(outs)}
    if ws is not None:
        res["partials"] = ws
    return res


def _wgrad_check(got, ref, alpha, base, what):
    want = alpha * ref if base is None else base.double() + alpha * ref
    err = float((got.double().cpu() - want).abs().max() / (alpha * ref).abs().max())           # (normalised as test_wgrad_kernel_matches_fp64 does)
    print(f"   {what}: rel-inf {err:.2e} (gate 1e-4)")
    assert err <= 1e-4


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "slices"])
@pytest.mark.parametrize("M,N,Kd", WGRAD_SHAPES)
def test_linear_wgrad(K, M, N, Kd, sliced, accumulate):
    a, b, ref, base = _wgrad_data(M, N, Kd)
    alpha, base = (-1.0, base) if accumulate else (0.5, None)
    what = f"linear_wgrad {(M, N, Kd)} {'slices' if sliced else 'dense'} {'accumulate' if accumulate else 'write'}"
    got = _run(lambda g: _wgrad_launch(K, g, [(a, b, sliced, alpha, base)]), what)
    _wgrad_check(got["out0"], ref, alpha, base, what)


def test_linear_wgrad_grouped_launch(K):
    """Four problems in one launch (two of them split, so two regions of the workspace), dense and sliced, written and accumulated; the bits of each
    are those of its own launch on plain tensors ("a problem gives the same bits in any group")."""
    shapes = [WGRAD_SHAPES[0], WGRAD_SHAPES[1], WGRAD_SHAPES[2], WGRAD_SHAPES[4]]
    probs = []
    for i, s in enumerate(shapes):
        a, b, _, base = _wgrad_data(*s)
        probs.append((a, b, i % 2 == 1, 0.25 * (i + 1), base if i >= 2 else None))
    got = _run(lambda g: _wgrad_launch(K, g, probs), "linear_wgrad grouped launch of four")
    assert "partials" in got
    for i, (s, (a, b, _, alpha, base)) in enumerate(zip(shapes, probs)):
        _wgrad_check(got[f"out{i}"], _wgrad_data(*s)[2], alpha, base, f"grouped, problem {i} {s}")
        alone = K.linear_wgrad(a.cuda(), b.cuda(), alpha=alpha, out=None if base is None else base.cuda(), accumulate=base is not None)
        assert torch.equal(alone, got[f"out{i}"]), f"problem {i}: the grouped launch and its own launch differ"


# =====================================================================================================================================
# fmc_nhwc_to_cmajor_padded (cond_kernels.hip:401-451): tiles of 64 positions x 64 channels per shifted copy; a position past row_len is not
# stored (cond_kernels.hip:430), a pixel outside the image or past the last image is not loaded (cond_kernels.hip:418).
# =====================================================================================================================================
CM_BAND_SRC = 128                               # pixels around src: a 64-position tile is at most 64 pixels, +-1 for the shift (cond_kernels.hip:411-419)
CM_BAND_DST = 64                                # rows (channels) of dst: one 64-channel tile (cond_kernels.hip:405)


@pytest.mark.parametrize("shifts", [1, 3])
def test_nhwc_to_cmajor_padded(K, shifts):
    """W = 7 is odd, so Wp = round_up(9, 8) = 16 has seven padding columns; C = 72 leaves eight channels in a second tile; row_len is no multiple of
    64.  shifts 3: the product's X^T geometry (guard Wp + 8 each side); shifts 1: dY^T with no guard and eight spare positions."""
    n, H, W, C = 3, 5, 7, 72
    Hp, Wp = H + 2, 16
    guard = Wp + 8 if shifts == 3 else 0
    row_len = (n * Hp * Wp + 63) // 64 * 64 + 2 * guard if shifts == 3 else n * Hp * Wp + 8
    assert row_len % 64 and row_len >= guard + n * Hp * Wp
    src = _rnd((n, H, W, C), 77, BF16)
    src = torch.where(src == 0, torch.ones_like(src), src)                       # no zero among the values: a zero in dst is padding
    want = torch.zeros(shifts, C, row_len, dtype=BF16)
    for s in range(shifts):
        padded = torch.zeros(n, Hp, Wp, C, dtype=BF16)
        for xp in range(W + 2):
            xs = xp - 1 + s - shifts // 2
            if 0 <= xs < W:
                padded[:, 1:H + 1, xp] = src[:, :, xs]
        want[s, :, guard:guard + n * Hp * Wp] = padded.view(-1, C).t()

    def fn(g):
        sd = g.inp(src.view(-1, C), CM_BAND_SRC, 0, "src")
        dst = g.out((shifts * C, row_len), BF16, CM_BAND_DST, 0, "dst")
        _call(K, "fmc_nhwc_to_cmajor_padded", sd.data_ptr(), dst.data_ptr(), n, H, W, C, row_len, guard, shifts, K._stream())
        return {"dst": dst}

    got = _run(fn, f"nhwc_to_cmajor_padded shifts {shifts}")["dst"].cpu().view(shifts, C, row_len)
    pad = want == 0
    assert int(pad.sum()) > 0 and bool((got[pad] == 0).all()), "a padding position of dst is not zero"
    assert torch.equal(got, want)

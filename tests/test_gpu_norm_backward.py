"""The LayerNorm, GroupNorm(+SiLU) and GEGLU backward kernels (synfmc_amd/csrc/norm_kernels.hip) element by element.

Every gradient is compared with the float64 closed form on the same rounded inputs (tests/norm_bwd_common.py): `2^-8 |ref| + 1e-5 mag` in
bf16 storage, `1e-5 mag` in fp32 storage and for the fp32 dgamma / dbeta, `mag` the sum of |terms| behind the element.  The shapes are
the geometries the kernels had never run: the second and third trip of the LayerNorm and GEGLU grid-stride loops, the LayerNorm addend
together with trainable gamma / beta, four and five chunks per lane, GroupNorm's split cap, one row per trip, one channel per group,
the widest tensor and a workgroup that is no whole number of waves.  Every test prints its worst error in units of the bound; one run
is recorded in profiles/temporal_norm_backward_bounds.md."""
import functools

import pytest
import torch

from tests import norm_bwd_common as NB

pytestmark = pytest.mark.gpu

F32 = torch.float32
DTYPES = [torch.bfloat16, torch.float32]
TAG = {torch.bfloat16: "bf16", torch.float32: "fp32"}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _dev(t, dtype=None):
    return t.to(dtype).cuda() if dtype is not None else t.cuda()


def _report(what, ratios):
    print(f"{what}: worst error in units of the bound: " + " ".join(f"{k} {r:.3f}" for k, r in ratios.items()))


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------
def _with_addend(ref, add):
    return dict(ref, dx=ref["dx"] + add.double(), mag_dx=ref["mag_dx"] + add.double().abs())


@functools.lru_cache(maxsize=None)
def _ln_reference(shape, dtype):
    """Float64 closed form of a shape without the addend, computed once and shared by the three entries (read only)."""
    x, dy, add, gamma, beta = NB.ln_inputs(shape, dtype)
    return NB.ln_reference(x, dy, gamma)


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("entry", ["frozen", "trainable", "skip_trainable"])
@pytest.mark.parametrize("shape", NB.LN_SHAPES, ids=NB.shape_id)
def test_layernorm_backward_elementwise(K, shape, entry, dtype):
    """frozen: gamma / beta need no gradient, dgamma = NULL.  trainable: the per-wave register partials and the atomics.  skip_trainable:
    `layernorm_skip` with both outputs used -- `fmc_layernorm_bwd_add` with an addend AND trainable gamma / beta, as `train_mm` runs it."""
    x, dy, add, gamma, beta = NB.ln_inputs(shape, dtype)
    train = entry != "frozen"
    xd = _dev(x, dtype).requires_grad_(True)
    gd, bd = _dev(gamma).requires_grad_(train), _dev(beta).requires_grad_(train)
    if entry == "skip_trainable":
        skip, y = K.layernorm_skip(xd, gd, bd, NB.EPS)
        torch.autograd.backward([skip, y], [_dev(add, dtype), _dev(dy, dtype)])
    else:
        K.layernorm(xd, gd, bd, NB.EPS).backward(_dev(dy, dtype))
    torch.cuda.synchronize()
    ref = _ln_reference(shape, dtype)
    if entry == "skip_trainable":
        ref = _with_addend(ref, add)
    assert xd.grad.dtype == dtype
    ratios = dict(dx=NB.bound_ratio(xd.grad, ref["dx"], ref["mag_dx"], dtype))
    if train:
        assert gd.grad.dtype == F32 and bd.grad.dtype == F32
        ratios.update(dgamma=NB.bound_ratio(gd.grad, ref["dgamma"], ref["mag_dgamma"], F32), dbeta=NB.bound_ratio(bd.grad, ref["dbeta"], ref["mag_dbeta"], F32))
    else:
        assert gd.grad is None and bd.grad is None
    _report(f"layernorm-bwd {NB.shape_id(shape)} {entry} {TAG[dtype]}", ratios)
    NB.assert_close(xd.grad, ref["dx"], ref["mag_dx"], dtype, "dx")
    if train:
        NB.assert_close(gd.grad, ref["dgamma"], ref["mag_dgamma"], F32, "dgamma")
        NB.assert_close(bd.grad, ref["dbeta"], ref["mag_dbeta"], F32, "dbeta")


# ---- GEGLU -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("shape", NB.GEGLU_SHAPES, ids=NB.shape_id)
def test_geglu_forward_and_backward_elementwise(K, shape, dtype):
    x, dy = NB.geglu_inputs(shape, dtype)
    xd = _dev(x, dtype).requires_grad_(True)
    y = K.geglu(xd)
    y.backward(_dev(dy, dtype))
    torch.cuda.synchronize()
    ref = NB.geglu_reference(x, dy)
    assert y.dtype == dtype and xd.grad.dtype == dtype
    Cff = shape[1]
    _report(f"geglu {NB.shape_id(shape)} {TAG[dtype]}", dict(
        y=NB.bound_ratio(y, ref["y"], ref["mag_y"], dtype),
        da=NB.bound_ratio(xd.grad[..., :Cff], ref["dx"][..., :Cff], ref["mag_dx"][..., :Cff], dtype),
        dg=NB.bound_ratio(xd.grad[..., Cff:], ref["dx"][..., Cff:], ref["mag_dx"][..., Cff:], dtype)))
    NB.assert_close(y, ref["y"], ref["mag_y"], dtype, "y")
    NB.assert_close(xd.grad, ref["dx"], ref["mag_dx"], dtype, "da | dg")


# ---- GroupNorm (+ SiLU) ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gn_reference(shape, dtype, act):
    """... without the addend, shared by the two entries (read only)"""
    x, dy, add, gamma, beta = NB.gn_inputs(shape, dtype)
    return NB.gn_reference(x, dy, gamma, beta, act)


@pytest.mark.parametrize("dtype", DTYPES, ids=TAG.get)
@pytest.mark.parametrize("act", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("entry", ["frozen", "skip"])
@pytest.mark.parametrize("shape", NB.GN_SHAPES, ids=NB.shape_id)
def test_groupnorm_backward_elementwise(K, shape, entry, act, dtype):
    """frozen: `groupnorm_silu` with a frozen gamma, the dX-only kernel pair every LoRA stage takes.  skip: `groupnorm_silu_skip` with both
    outputs used, the gradient along the skip connection added in the dX pass."""
    x, dy, add, gamma, beta = NB.gn_inputs(shape, dtype)
    xd = _dev(x, dtype).requires_grad_(True)
    if entry == "skip":
        skip, y = K.groupnorm_silu_skip(xd, _dev(gamma), _dev(beta), NB.GROUPS, NB.EPS, act)
        torch.autograd.backward([skip, y], [_dev(add, dtype), _dev(dy, dtype)])
    else:
        K.groupnorm_silu(xd, _dev(gamma), _dev(beta), NB.GROUPS, NB.EPS, act).backward(_dev(dy, dtype))
    torch.cuda.synchronize()
    ref = _gn_reference(shape, dtype, act)
    if entry == "skip":
        ref = _with_addend(ref, add)
    assert xd.grad.dtype == dtype
    _report(f"groupnorm-bwd {NB.shape_id(shape)} {entry} {'silu' if act else 'plain'} {TAG[dtype]}",
            dict(dx=NB.bound_ratio(xd.grad, ref["dx"], ref["mag_dx"], dtype)))
    NB.assert_close(xd.grad, ref["dx"], ref["mag_dx"], dtype, "dx")

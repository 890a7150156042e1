"""The closed forms of tests/resample_bwd_common.py against float64 autograd, the tables behind them, and the bound of the GPU test against
an emulation of the kernels' rounding chain and against wrong stand-ins (CPU)."""
import pytest
import torch
import torch.nn.functional as F

from tests import resample_bwd_common as RC

# (n, H, W, Cin, Cout) of the forward's input: odd counts of images and channels, one pixel, non-square, more than one image
DOWN = [(1, 2, 2, 3, 5), (3, 6, 10, 8, 4), (2, 12, 8, 16, 24)]
UP = [(1, 1, 1, 3, 5), (3, 3, 5, 8, 4), (2, 4, 6, 16, 24)]


def _rnd(shape, seed, dtype=torch.float64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)


def _forward(x, w, up):
    return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1) if up else F.conv2d(x, w, stride=2, padding=1)


def _case(shape, up, dtype=torch.float64):
    n, h, w_, cin, cout = shape
    ho, wo = (2 * h, 2 * w_) if up else (h // 2, w_ // 2)
    return _rnd((n, cout, ho, wo), 1, dtype), _rnd((cout, cin, 3, 3), 2, dtype) * 0.1


@pytest.mark.parametrize("up,shape", [(False, s) for s in DOWN] + [(True, s) for s in UP])
def test_closed_forms_equal_float64_autograd(up, shape):
    dy, w = _case(shape, up)
    n, h, w_, cin, _ = shape
    x = _rnd((n, cin, h, w_), 3).requires_grad_(True)
    (want,) = torch.autograd.grad(_forward(x, w, up), x, dy)
    got = RC.up_bwd(dy, w) if up else RC.down_bwd(dy, w)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * float(RC.magnitude(dy, w, up).max())


def test_tables_are_what_the_formulas_say():
    assert RC.T == {0: ((1, 0),), 1: ((2, 0), (0, 1))}
    # T from the forward: output row i' reads input row 2 i' - 1 + ky, so input row 2 i + py is read with ky = 2 (i - i') + py + 1
    for py in range(2):
        want = tuple(sorted(((2 * (-di) + py + 1, di) for di in (-1, 0, 1) if 0 <= 2 * (-di) + py + 1 <= 2), key=lambda t: t[1]))
        assert tuple(sorted(RC.T[py], key=lambda t: t[1])) == want
    w = _rnd((2, 3, 3, 3), 4)
    g = RC.fold_g(w)
    rows = [w[:, :, 2], w[:, :, 1] + w[:, :, 2], w[:, :, 0] + w[:, :, 1], w[:, :, 0]]          # [co, ci, kx] per r
    for r in range(4):
        cols = [rows[r][:, :, 2], rows[r][:, :, 1] + rows[r][:, :, 2], rows[r][:, :, 0] + rows[r][:, :, 1], rows[r][:, :, 0]]
        for c in range(4):
            assert torch.allclose(g[:, :, r, c], cols[c], rtol=0, atol=1e-14)
    # G is the transpose of the forward's fold (hip_ops.upsample_fold_weights): output row 2 i + py reads source row u = i + py - 1 + a with tap a,
    # so source row u meets dY row 2 u - py + 2 - 2 a = 2 u - 1 + r with r = 3 - py - 2 a
    from synfmc_amd.hip_ops import upsample_fold_weights
    wf = upsample_fold_weights(w)                                   # [py, px, a, b, co, ci]
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    assert torch.allclose(wf[py, px, a, b], g[:, :, 3 - py - 2 * a, 3 - px - 2 * b], rtol=0, atol=1e-14)


@pytest.mark.parametrize("up,shape", [(False, s) for s in DOWN] + [(True, s) for s in UP])
def test_emulated_rounding_chain_meets_the_bounds(up, shape):
    dy, w = _case(shape, up, torch.bfloat16)
    ref = RC.up_bwd(dy.double(), w.double()) if up else RC.down_bwd(dy.double(), w.double())
    mag = RC.magnitude(dy.double(), w.double(), up)
    bad, share = RC.misses(RC.emulate(dy, w, up), ref, mag, up)
    print(f"emulation {'up' if up else 'down'} {shape}: {bad} outside, largest share of the bound {share:.2f}")
    assert bad == 0


@pytest.mark.parametrize("up,wrong", [(False, k) for k in RC.WRONG_DOWN] + [(True, k) for k in RC.WRONG_UP])
def test_wrong_stand_ins_do_not_meet_the_bounds(up, wrong):
    shape = (UP if up else DOWN)[1]                                  # three images, 6 x 10 resp. 3 x 5
    dy, w = _case(shape, up, torch.bfloat16)
    dy, w = dy.double(), w.double()
    ref = RC.up_bwd(dy, w) if up else RC.down_bwd(dy, w)
    mag = RC.magnitude(dy, w, up)
    got = (RC.up_bwd(dy, w, wrong) if up else RC.down_bwd(dy, w, wrong)).to(torch.bfloat16)
    bad, _ = RC.misses(got, ref, mag, up)
    assert bad > 0, f"{wrong}: a wrong gradient passes the bound"
    assert RC.misses(ref.to(torch.bfloat16), ref, mag, up)[0] == 0   # ... which the rounded right one meets

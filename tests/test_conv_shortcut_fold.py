"""The shortcut fold of ResnetBlock2D's second convolution (csrc/conv_halo.hip, shortcut mode) on the CPU: the algebra the kernel relies on, and
the order of the combined filter pack restated in Python against the pack kernel's own index map (`fmc_conv3x3_halo_sc_pack_source`, host code)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F


def _pack_order(cin, cout, cin_sc, bn):
    """The packed filter as a list of (from_shortcut, element index of the first of eight) per 16-byte chunk:
    [cout / bn channel tiles][sub-tiles: (cin / 64) x 9 taps x 2 halves, then (cin_sc / 64) x 2 halves][bn rows][4 chunks], chunk p of a row
    holding logical chunk p ^ (3 * ((row >> 3) & 1))."""
    order = []
    for nt in range(cout // bn):
        subs = [(False, ch, tap, hk) for ch in range(cin // 64) for tap in range(9) for hk in range(2)]
        subs += [(True, ch, 0, hk) for ch in range(cin_sc // 64) for hk in range(2)]
        for sc, ch, tap, hk in subs:
            for row in range(bn):
                co = nt * bn + row
                for p in range(4):
                    lc = p ^ (3 * ((row >> 3) & 1))
                    k = ch * 64 + hk * 32 + lc * 8
                    order.append((True, co * cin_sc + k) if sc else (False, (co * 9 + tap) * cin + k))
    return order


@pytest.mark.parametrize("cin,cout,cin_sc,bn", [(64, 160, 64, 160), (128, 320, 192, 160), (64, 160, 128, 80)])
def test_combined_pack_order_is_the_packers_index_map(cin, cout, cin_sc, bn):
    from synfmc_amd import _lib
    L = _lib.load()
    order = _pack_order(cin, cout, cin_sc, bn)
    assert len(order) == cout * (9 * cin + cin_sc) // 8 == L.fmc_conv3x3_halo_sc_packed_bytes(cin, cout, cin_sc) // 16
    flag = ctypes.c_int(-1)
    for chunk in list(range(0, len(order), 7)) + [len(order) - 1]:
        src = L.fmc_conv3x3_halo_sc_pack_source(chunk, cin, cin_sc, bn, ctypes.byref(flag))
        assert (bool(flag.value), src) == order[chunk], chunk
    # every element of both filters exactly once
    seen3 = sorted(s for sc, s in order if not sc)
    seen1 = sorted(s for sc, s in order if sc)
    assert seen3 == list(range(0, cout * 9 * cin, 8)) and seen1 == list(range(0, cout * cin_sc, 8))


@pytest.mark.parametrize("n,h,w,cin,cout,cs1,cs2", [(2, 5, 7, 8, 12, 6, 0), (1, 4, 4, 16, 8, 8, 24)])
def test_one_reduction_equals_conv_plus_shortcut_plus_biases(n, h, w, cin, cout, cs1, cs2):
    """conv3x3(a) + 1x1([xs | xs2]) + b2 + bs == one product over K = 9 cin + cin_sc: im2col of `a` with the shortcut input appended as channels
    that only the centre tap sees (fp64)."""
    g = torch.Generator().manual_seed(cin + cs2)
    a = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    xs = torch.randn(n, cs1 + cs2, h, w, generator=g, dtype=torch.float64)
    w3 = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    w1 = torch.randn(cout, cs1 + cs2, generator=g, dtype=torch.float64)
    b2, bs = torch.randn(cout, generator=g, dtype=torch.float64), torch.randn(cout, generator=g, dtype=torch.float64)
    want = F.conv2d(a, w3, b2, padding=1) + F.conv2d(xs, w1[:, :, None, None], bs)
    cols = F.unfold(a, 3, padding=1)                                        # [n, cin * 9, h * w], zero-padded taps
    A = torch.cat([cols, xs.reshape(n, cs1 + cs2, h * w)], 1)               # the centre tap of the appended channels = the pixel itself
    W = torch.cat([w3.reshape(cout, cin * 9), w1], 1)
    got = (W @ A + (b2 + bs)[None, :, None]).reshape(n, cout, h, w)
    assert (got - want).abs().max().item() < 1e-12 * want.abs().max().item()
    # the same with the two shortcut sources kept apart (read in place, never concatenated)
    if cs2:
        got2 = (W[:, : cin * 9] @ cols + w1[:, :cs1] @ xs[:, :cs1].reshape(n, cs1, -1) + w1[:, cs1:] @ xs[:, cs1:].reshape(n, cs2, -1)
                + (b2 + bs)[None, :, None]).reshape(n, cout, h, w)
        assert (got2 - want).abs().max().item() < 1e-12 * want.abs().max().item()

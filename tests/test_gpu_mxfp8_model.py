"""`hip_ops.FP8_FF`: the feed-forward on the MXFP8 GEMMs (csrc/gemm_mxfp8.hip) at module and model level.

One `FeedForward` (C = 320 and 640, M = 330 rows: two tiles and a ragged third): the switch-on output equals the composition of the three wrappers bit for
bit, and lies within the kernels' own bounds of the float64 chain on the module's quantised weights (LayerNorm bytes as the kernel emitted them, pinned by
test_gpu_mxfp8.py; the intermediate compared as MXFP8, the output with `assert_bf16_close`).

The reduced FMC stack of tests/test_gpu_model.py (widths 64 / 128 / 256 / 256: every feed-forward has K % 64 == 0 and N % 64 == 0): the route is taken
(call counter), eager and a captured graph replayed twice give identical bits, and the rel-inf against the fp32 CPU oracle is measured with the switch off
and on; the switch-on value must meet the 6e-2 that `test_unet_forward_cmc_omc` applies to bf16 storage."""
import pytest
import torch

from tests import common_models as CM
from tests import mxfp8_common as MX
from tests.conv_fwd_common import assert_bf16_close
from tests.test_gpu_model import W4, rel_inf, stack  # noqa: F401  (the module-scoped oracle fixture)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture()
def K(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _mx_calls(K, fn):
    log0, K.call_log = K.call_log, []
    try:
        out = fn()
        return out, [c for c in K.call_log if c[0] == "mxfp8"]
    finally:
        K.call_log = log0


@pytest.mark.parametrize("C", [320, 640])
def test_feedforward_under_fp8_ff(K, monkeypatch, C):
    from synfmc_amd.models import layers as L
    torch.manual_seed(C)
    M, inner = 330, 4 * C
    ff = L.FeedForward(C).eval().requires_grad_(False).to("cuda", BF16)
    norm = L.LayerNorm(C).eval().requires_grad_(False).to("cuda", BF16)
    with torch.no_grad():
        norm.weight.copy_(1.0 + 0.3 * torch.randn(C))
        norm.bias.copy_(0.2 * torch.randn(C))
    h = (torch.randn(M, C, generator=torch.Generator().manual_seed(1)) * 1.5 + 0.2).to("cuda", BF16)
    proj, out = ff.net[0].proj, ff.net[2]
    monkeypatch.setattr(K, "MXFP8_FF_SLOWER", ())      # (these widths are not routed by default -- measured slower, profiles/mxfp8_ff.md; the chain itself is what is checked)
    with torch.no_grad():
        _, calls = _mx_calls(K, lambda: ff.forward_ln(h, norm, h))
        assert calls == []                                                  # switch off
        monkeypatch.setattr(K, "FP8_FF", True)
        y, calls = _mx_calls(K, lambda: ff.forward_ln(h, norm, h))
        assert [c[1][0] for c in calls] == ["ln", "geglu", "linear"] and y.shape == h.shape and getattr(y, "_fmc_tail", None) is None
        # the composition of the three wrappers, bit for bit
        g32, b32 = norm.weight.float(), norm.bias.float()
        w1q, w1s = K.mxfp8_pack_weight(proj.weight, geglu=True)
        w2q, w2s = K.mxfp8_pack_weight(out.weight)
        xq, xs = K.layernorm_mxfp8(h, g32, b32, norm.eps)
        mq, ms = K.linear_mxfp8(xq, xs, w1q, w1s, proj.bias, geglu=True)
        y2 = K.linear_mxfp8(mq, ms, w2q, w2s, out.bias, h)
        assert torch.equal(y, y2)
    # the float64 chain on the module's own quantised weights
    MX.assert_ln_mx_close(xq, xs, h, g32, b32, norm.eps, f"C {C} layernorm")
    inv = torch.empty(2 * inner, dtype=torch.long)
    inv[MX.geglu_pack_rows(inner)] = torch.arange(2 * inner)
    w1q_m, w1s_m = w1q.cpu()[inv], w1s.cpu()[inv]                             # back in the module's row order
    ref_mid, F = MX.geglu_reference(xq.cpu(), xs.cpu(), w1q_m, w1s_m, proj.bias.cpu(), inner)
    MX.assert_mx_close(mq, ms, ref_mid, F, f"C {C} GEGLU intermediate")
    ref, mag = MX.linear_reference(mq.cpu(), ms.cpu(), w2q.cpu(), w2s.cpu(), out.bias.cpu(), h.cpu())
    print(f"   FeedForward C {C}: output worst err / bound {assert_bf16_close(y, ref, mag, f'C {C} output'):.3f}")


def test_reduced_stack_under_fp8_ff(K, monkeypatch, stack):
    pu, pe, pa = CM.build_product(stack["ou"], stack["oe"], stack["oa"], W4, dtype=BF16)
    clip = stack["clip"]
    dev = lambda x: x.to("cuda", BF16)
    pose, traj = [dev(x) for x in stack["pose_feats"]], [dev(x) for x in stack["traj"]]
    lat, t, text = dev(clip["latents"]), stack["t"].cuda(), dev(clip["text"])
    call = lambda: pu(lat, t, text, pose_embedding_features=pose, traj_features=traj).sample
    n_ff = sum(1 for m in pu.modules() if type(m).__name__ == "FeedForward")
    monkeypatch.setattr(K, "DETERMINISTIC", True)      # (as test_pipeline_graph_reuse_across_clips: no vendor convolution arm, whose atomics differ run to run)
    with torch.no_grad():
        call()                                                               # (the per-shape autotuner settles on its arms in the first call)
        off, calls = _mx_calls(K, call)
        assert calls == []
        monkeypatch.setattr(K, "FP8_FF", True)
        call()                                                               # (... and on those of the shapes that only this setting launches; the packs are cached)
        on, calls = _mx_calls(K, call)
        assert torch.equal(call(), on), "two eager calls differ"
        assert len(calls) % 3 == 0 and 0 < len(calls) // 3 <= n_ff, f"{len(calls)} launches of the family for {n_ff} feed-forwards"
        # a captured graph, replayed twice: the bits of the eager call
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()
        torch.cuda.current_stream().wait_stream(side)
        cap = torch.cuda.Stream()
        K.prepare_streamk_workspace(cap)
        graph = torch.cuda.CUDAGraph()
        cap.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(graph, stream=cap):
            static = call()
        torch.cuda.current_stream().wait_stream(cap)
        for _ in range(2):
            static.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static, on), "a replay of the captured graph differs from the eager call"
        del graph
        K.release_streamk_workspace(cap)
    r_off, r_on = rel_inf(off.float(), stack["ref"]), rel_inf(on.float(), stack["ref"])
    print(f"   reduced stack, rel-inf against the fp32 oracle: switch off {r_off:.4e}, FP8_FF {r_on:.4e} (gate 6e-2); {len(calls) // 3} of {n_ff} feed-forwards on the new chain")
    assert r_off < 6e-2
    assert r_on < 6e-2

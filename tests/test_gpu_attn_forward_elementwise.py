"""Every attention forward launch, element by element (tests/attn_fwd_common.py has the case table, references, generators and bounds;
profiles/attn_forward_bounds.md the rounding points, the derivations and the measured shares):

* exact runs -- integer data and a power-of-two `scale_log2` on which every probability is a power of two and every partial sum exact in fp32: output
  and LSE equal the float64 reference up to one division and one output rounding, whatever the tiling, the reference of the softmax or the wave split;
* rounded runs -- Gaussian data: every element within the worst-case bound composed from the kernel's rounding points.

Kernels: `fmc_spatial_attn_fwd` (xattn40_kernel, sa_big80_kernel_w10, sa_small160_kernel<3 | 5>, sa40d_kernel and all 50 instantiations of the tiled
kernel the default dispatch reaches; its A/B switch arms in fresh child processes), `fmc_temporal_attn_fwd`, `fmc_temporal_attn_fp8_fwd` and
`fmc_attention_fwd`, through the `hip_ops` wrappers.  Each case prints the share of its bound that the kernel used."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import attn_fwd_common as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTRUMENTS = ["exact", "rounded"]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from synfmc_amd import hip_ops
    return hip_ops


def _operands(c, instrument):
    d = A.inputs(c, instrument)
    return d, A.views(c, {n: t.cuda() for n, t in A.pack(c, d).items()})


def _report(c, instrument, shares):
    A.reference.cache_clear()
    A.inputs.cache_clear()
    lse = "" if shares[1] is None else f", LSE {shares[1]:.3f}"
    print(f"   {c.kernel} {A.case_id(c)} {instrument}: err / bound {shares[0]:.3f}{lse}")
    return shares


@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("c", A.SPATIAL, ids=A.case_id)
def test_spatial_attention_every_element(K, c, instrument):
    """`fmc_spatial_attn_fwd`: output and LSE of every kernel and tiled instantiation of the default dispatch -- one, two and more key tiles, ragged and
    whole, one and two query blocks per wave, fused and separate projections, shared text K/V, the three block orders, the redo pass (spike cases: one
    waived row, every other row exact)."""
    d, (q, k, v) = _operands(c, instrument)
    out, lse = K.spatial_attention(q, k, v, c.H, d["scale"], return_lse=True)
    torch.cuda.synchronize()
    _report(c, instrument, A.check(c, instrument, out, lse, A.case_id(c)))
    out2 = K.spatial_attention(q, k, v, c.H, d["scale"])                        # without the LSE pointer: the same bits
    assert torch.equal(out2, out)


@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("c", A.TEMPORAL, ids=A.case_id)
def test_temporal_attention_every_element(K, c, instrument):
    """`fmc_temporal_attn_fwd`: 1 to 32 frames (whole and partial tiles), heads split unevenly over the waves, native and `[N, F, C]` layouts.

    The kernels round p as it leaves the exp and apply 1 / l to the PV accumulator (temporal_attn.hip:253-258, :288): with the normalised p rounded
    instead, as they did before, 24 of these 48 bf16 runs lay beyond the bound, by up to 1.106 x (exact) and 1.264 x (rounded)."""
    d, (q, k, v) = _operands(c, instrument)
    out = K.temporal_attention(q, k, v, c.H, d["scale"])
    torch.cuda.synchronize()
    _report(c, instrument, A.check(c, instrument, out, None, A.case_id(c)))


@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("c", A.FP8, ids=A.case_id)
def test_temporal_attention_fp8_every_element(K, c, instrument):
    """`fmc_temporal_attn_fp8_fwd` on the raw ABI: e4m3 bytes (small integers are exact in e4m3) and power-of-two scales for q, k and v."""
    d = A.inputs(c, instrument)
    qkv8 = A.pack(c, d)["qkv"].cuda()
    scales = torch.tensor(A.FP8_SCALES, dtype=torch.float32, device="cuda")
    out = K._temporal_fp8_raw(qkv8, scales, c.H, d["scale"])
    torch.cuda.synchronize()
    _report(c, instrument, A.check(c, instrument, out, None, A.case_id(c)))


@pytest.mark.parametrize("instrument", INSTRUMENTS)
@pytest.mark.parametrize("c", A.GENERIC, ids=A.case_id)
def test_generic_attention_every_element(K, c, instrument):
    """`fmc_attention_fwd`: head widths 64, 128 and 512, `Sq != Skv`, the causal mask, `key_keep` with kept keys on both sides of a stage seam and the
    last key masked, both together."""
    d, (q, k, v) = _operands(c, instrument)
    keep = d["keep"].cuda() if c.keep else None
    out = K.attention(q, k, v, c.H, d["scale"], causal=c.causal, key_keep=keep)
    torch.cuda.synchronize()
    _report(c, instrument, A.check(c, instrument, out, None, A.case_id(c)))


def test_one_perturbed_key_index_fails_the_exact_instrument(K):
    """The instrument's own sanity check on the device: the kernel's result against a reference in which one key took its neighbour's place."""
    c = A.fault_case("drop_last_key")
    d, (q, k, v) = _operands(c, "exact")
    out = A.canonical(c, K.spatial_attention(q, k, v, c.H, d["scale"]))
    kk = d["k"].clone()
    kk[0, 1, 100] = d["k"][0, 1, 101]
    ref = torch.softmax(torch.einsum("ghid,ghjd->ghij", d["q"], kk) * (A.scale_log2(d["scale"]) * A.LN2), -1) @ d["v"]
    beyond = (out - ref).abs() > A.reference(c, "exact")["exact_out"]
    assert bool(beyond[0, 1].any()) and not bool(beyond[0, 0].any())


def test_switch_arms_every_element(K, tmp_path):
    """The A/B switches of csrc/spatial_attn.hip are read once per process: each arm runs its cases under the exact instrument in one fresh child
    process (tests/attn_fwd_child.py), one after another, each under its own time limit.  A child that ends by signal, abort or time limit fails the
    test and no further child is started."""
    for i, (env, cases) in enumerate(A.SWITCH_ARMS):
        if any(k in os.environ for k in env):
            pytest.skip(f"{env} is set in this process")
        dst = tmp_path / f"arm{i}.json"
        try:
            run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_fwd_child.py"), ROOT, str(i), str(dst)],
                                 env=dict(os.environ, **env), capture_output=True, text=True, timeout=180)
        except subprocess.TimeoutExpired:
            pytest.fail(f"{env}: the child ran into its time limit; no further child started")
        if run.returncode < 0 or run.returncode in (134, 139, 124, 137):
            pytest.fail(f"{env}: the child ended by signal or abort ({run.returncode}); no further child started\n{run.stderr[-2000:]}")
        assert run.returncode == 0, f"{env}: {run.stderr[-3000:]}"
        shares = json.loads(dst.read_text())
        assert len(shares) == len(cases)
        print(f"   {env}: {len(shares)} cases, largest err / bound {max(s[0] for s in shares.values()):.3f}, "
              f"LSE {max(s[1] for s in shares.values()):.3f}")

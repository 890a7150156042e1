"""The dispatch restatement of tests/attn_fwd_common.py (`expected_kernel`, `temporal_kernel`, the generic kernel's name) against
tests/golden/attn_routes.json: what the library launched for every forward case on the MI355X, traced by tools/record_attn_routes.py.  No GPU: the
file is the device's word, the restatement is what the element-wise tests pick their rounding tables by."""
import json
import os
import re

import pytest

from tests import attn_fwd_common as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_routes.json")
TYPES = {"unsigned short": "bf16", "float": "fp32", "true": "1", "false": "0"}


@pytest.fixture(scope="module")
def routes():
    with open(GOLDEN) as f:
        data = json.load(f)
    assert data["source"].startswith("rocprofv3"), "the routes are traced, not restated"
    return data["routes"]


def restated(launch):
    """A traced launch `[name, grid, workgroup, lds]` in the spelling of `attn_fwd_common`: `k<unsigned short, 3, false>` -> `k<bf16,3,0>`."""
    name, _, wg, _ = launch
    m = re.fullmatch(r"(\w+)(?:<(.*)>)?", name)
    base, args = m.group(1), [TYPES.get(a.strip(), a.strip()) for a in m.group(2).split(",")] if m.group(2) else []
    if base == "spatial_attn_kernel":
        args = args[:7]                              # (the eighth, PIPE, follows from PREFETCH and the storage type)
    if base == "temporal_attn_fp8_kernel":           # <FT, NK32, PART>: the restatement also names the storage type and the waves of the workgroup
        args = ["bf16", args[0], args[1], str(wg[0] // 64), args[2]]
    return base + ("<" + ",".join(args) + ">" if args else "")


def test_every_forward_case_launches_the_kernel_the_restatement_names(routes):
    default = routes["default"]
    for c in A.all_cases():
        launches = default["fwd " + A.case_id(c)]
        assert len(launches) == 1, (A.case_id(c), launches)
        assert restated(launches[0]) == c.kernel, (A.case_id(c), launches[0], c.kernel)


def test_temporal_workgroups_are_the_restated_waves(routes):
    for c in A.TEMPORAL + A.FP8:
        _, gh, nw = A.temporal_kernel(c.dtype, c.Sq, c.H, c.D, c.abi == "fp8")
        (name, grid, wg, _), = routes["default"]["fwd " + A.case_id(c)]
        assert wg[0] == 64 * nw and grid[0] == c.B * c.pix * (c.H // gh) * wg[0], (A.case_id(c), grid, wg)


def test_switch_arms_are_recorded_and_leave_the_default_kernel(routes):
    """Every arm of SWITCH_ARMS has its process; its cases launch one kernel each, and (the arms are A/B switches of the route) another one than the
    default, except FMC_SA_PIPE=4, which changes the grid of the same kernel."""
    for env, cases in A.SWITCH_ARMS:
        key = ",".join(f"{k}={v}" for k, v in sorted(env.items()))
        arm = routes[key]
        assert sorted(arm) == sorted("fwd " + A.case_id(c) for c in cases)
        for c in cases:
            (launch,), (dflt,) = arm["fwd " + A.case_id(c)], routes["default"]["fwd " + A.case_id(c)]
            if env == {"FMC_SA_PIPE": "4"}:
                assert launch[0] == dflt[0] and launch[1][0] <= dflt[1][0]
            else:
                assert launch[0] != dflt[0], (key, A.case_id(c), launch)

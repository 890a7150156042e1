"""The host side of the attention kernels against tests/golden/attn_host_surface.json, recorded by tools/record_attn_host_surface.py before the argument
checks, the head-group search, the tile rule and the dispatch ladders were each written once: the return code and message of every refused call of
the eight entry points, and every argument the wrappers of `hip_ops` hand to the library, forward and backward (tests/attn_host_surface_common.py).
No GPU: nothing is launched."""
import json
import os

import pytest

from tests import attn_host_surface_common as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_host_surface.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def K():
    from synfmc_amd import hip_ops
    return hip_ops


def test_refused_calls_keep_code_and_message(K, golden):
    want = golden["errors"]
    assert [[want["names"][r[0]], r[1]] for r in want["rows"]] == [list(c[:2]) for c in S.error_calls()]
    assert all(rc in S.ATTN_REFUSALS and msg for rc, msg in want["values"])    # (recorded: every row fails before the launch)
    assert S.lds_refusal_unreachable()
    S.same_table(S.errors(K._lib.load()), want, "refused calls (entry point by index in `names`)", lambda data, v: v)


def test_every_check_of_every_entry_point_is_recorded(golden):
    """Each entry point's refusals as recorded: NULL, shape, stride and alignment where it has the check, the dtype where it takes one."""
    want = golden["errors"]
    codes = {name: set() for name in want["names"]}
    for ni, _, vi in want["rows"]:
        codes[want["names"][ni]].add(want["values"][vi][0])
    for name, got in codes.items():
        expect = {-5} if "roll" in name else {-5, -1, -3} | ({-2} if "dtype" in S.SIGS[name] else set())
        assert got == expect, (name, got)


def test_wrapper_calls(K, golden, monkeypatch):
    flat = lambda data, v: [[name, i, a] for name, args in v for i, a in enumerate(args)]
    S.same_table(S.calls(K, monkeypatch), golden["calls"], "wrapper calls (element = [entry point, argument position, value])", flat)

"""The host side of the fused attention blocks and the feed-forward chain against tests/golden/fused_host_surface.json, recorded by
tools/record_fused_host_surface.py before each rule of these families was written once: every predicate and count over its grid (hook as it is, hook
patched, tensors that say they are on the GPU), the return code and message of every refused call, and the launches the two transformer blocks and
`FeedForward.forward_ln` make over the shipped and ragged sizes (tests/fused_host_surface_common.py).  No GPU: nothing is launched."""
import json
import os

import pytest

from tests import fused_host_surface_common as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_host_surface.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def K():
    from synfmc_amd import hip_ops
    return hip_ops


def test_predicates_and_counts(K, golden, monkeypatch):
    S.same_table(S.predicates(K, monkeypatch), golden["predicates"], "predicates (by index in `names`; element = index into HWS / MS)", lambda data, v: S.unrle(v))


def test_refused_calls_keep_code_and_message(K, golden):
    want = golden["errors"]
    assert [[want["names"][r[0]], r[1]] for r in want["rows"]] == [list(c[:2]) for c in S.error_calls()]
    assert all(rc in S.REFUSALS for rc, _ in want["values"])                 # (recorded: every row fails before the launch)
    S.same_table(S.errors(K._lib.load()), want, "refused calls (entry point by index in `names`)", lambda data, v: v)


def test_routes(K, golden, monkeypatch):
    launches = lambda data, runs: [data["launches"][i] for i in S.unrle(runs)]
    S.same_table(S.routes(K, monkeypatch), golden["routes"], "routes (switch set by index in `switches`; element = size and call in order)", launches)

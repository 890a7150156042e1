"""The host side of the halo convolutions against tests/golden/halo_host_surface.json, recorded by tools/record_halo_host_surface.py before the launch
forms and the routing were each written once: every predicate and count function over its grid, the return code and message of every refused call,
and the launch `hip_ops.conv3x3` makes over the shipped sizes (tests/halo_host_surface_common.py).  No GPU: nothing is launched."""
import json
import os

import pytest

from tests import halo_host_surface_common as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "halo_host_surface.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def K():
    from synfmc_amd import hip_ops
    return hip_ops


def test_predicates_and_counts(K, golden):
    S.same_table(S.predicates(K._lib.load()), golden["predicates"], "predicates (by index in `names`; element = (H - 1) * 70 + W - 1)", S.expand_plane)


def test_refused_calls_keep_code_and_message(K, golden):
    want = golden["errors"]
    assert [[want["names"][r[0]], r[1]] for r in want["rows"]] == [list(c[:2]) for c in S.error_calls()]
    assert all(rc in S.REFUSALS for rc, _ in want["values"])                 # (recorded: every row fails before the launch)
    S.same_table(S.errors(K._lib.load()), want, "refused calls (entry point by index in `names`)", lambda data, v: v)


def test_routes(K, golden, monkeypatch):
    launches = lambda data, runs: [data["launches"][i] for i in S.unrle(runs)]
    S.same_table(S.routes(K, monkeypatch), golden["routes"], "routes (switch set by index in `switches`; element = (size, channels) in order)", launches)
